"""The inputs of tests/test_gpu_attention_tokens_tiles.py can see the bug the entry exists for (CPU, fp64 only).

For every kernel-level case of tests/attention_tiles_common.py: what "the keys of all E images" gives -- the batched entry on the
tall K / V -- is at least 10 bounds from the per-image truth on EVERY image that has a tile, under the fp32 bound and under the
(wider) bound of the fp16-operand form.  The lists are what the docstring there says."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import attention_tiles_common as TC  # noqa: E402


def test_the_shapes_and_lists_are_what_the_docstring_says():
    keys = list(TC.CASES)
    assert {k[4] for k in keys} == {16, 40, 80, 160}
    assert {k[3] for k in keys} == {1, 4, 8}
    assert {(k[0], k[1]) for k in keys} >= {(2, 8), (3, 8), (2, 16)}
    assert {k[1] * k[2] for k in keys} == {48, 40, 128}
    for key, rows in TC.CASES.items():
        E, h = key[0], key[1]
        assert all(r % 4 == 0 and 0 <= r < E * h for r in rows) and rows == sorted(rows)
        per = TC.per_image(key)
        assert len(set(per)) > 1, "uneven lists"
        seam = any((e + 1) * h - 4 in rows and (e + 1) * h in rows for e in range(E - 1))
        assert seam or 0 in per, "tiles on the last tile row of an image and the first of the next"
    assert any(0 in TC.per_image(key) for key in keys), "one case has an image with no tile"


@pytest.mark.parametrize("key", list(TC.CASES), ids=TC.case_id)
def test_all_keys_is_ten_bounds_from_the_truth_on_every_image(key):
    c = TC.case(key)
    E = key[0]
    assert torch.isfinite(c["want"]).all() and c["bound"] > 0 and c["bound16"] >= c["bound"]
    for e in range(E):
        mine = [t for t in range(len(c["image"])) if int(c["image"][t]) == e]
        if not mine:
            continue
        sel = torch.cat([torch.arange(16 * t, 16 * t + 16) for t in mine])
        away = float((c["mixed"][:, sel] - c["want"][:, sel]).abs().max())
        print("%s image %d: mixed - truth %.3e, e32 %.3e bound %.3e, e16 %.3e bound16 %.3e"
              % (TC.case_id(key), e, away, c["e32"], c["bound"], c["e16"], c["bound16"]))
        assert away >= 10.0 * c["bound"], (e, away, c["bound"])
        assert away >= 10.0 * c["bound16"], (e, away, c["bound16"])
