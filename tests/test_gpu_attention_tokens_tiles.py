"""sige_hip_attention_tokens_tiles_f32 / _f16c (sige_amd.hip.attention_tokens(..., tiles=...)) alone: under stacked edits the
queries of a 4x4 tile attend to the keys of the tile's OWN image, in one launch for the tiles of every edit.

Cases, truths and bounds: tests/attention_tiles_common.py (fp64 per image; tests.attention_stress.bound for the fp32 form,
tests.attention_f16.bound16 for the fp16-operand form; tests/test_attention_tokens_tiles_inputs.py shows on the CPU that a key read
from a neighbouring image is at least 10 bounds away on every image).  Every destination is NaN before the launch (util.poisoned:
torch.empty hands out NaN).  Margins are recorded (util.record_margin; kept as profiles/sd_unet_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import attention_tiles_common as TC  # noqa: E402
from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


class _edits:
    def __init__(self, hip, E):
        self.hip, self.E = hip, E

    def __enter__(self):
        self.prev = self.hip.get_edit_batch()
        self.hip.set_edit_batch(self.E)

    def __exit__(self, *exc):
        self.hip.set_edit_batch(self.prev)
        return False


_on_gpu = {}


def _case(key):
    """The CPU case with q, k, v, idx, want on the GPU: moved once per process and left unchanged."""
    if key not in _on_gpu:
        c = TC.case(key)
        _on_gpu[key] = dict(c, **{n: c[n].to(DEV) for n in ("q", "k", "v", "idx", "want")})
    return _on_gpu[key]


def _run(hip, key, compute):
    c = _case(key)
    E, h, W, heads, d = key
    with _edits(hip, E), util.poisoned() as p:
        got = hip.attention_tokens(c["q"], c["k"], c["v"], heads, c["scale"], compute=compute, tiles=(c["idx"], E * h, W))
    assert p.n > 0, "the output was not allocated under the poison"
    return got


@pytest.mark.parametrize("compute", ["f32", "f16"])
@pytest.mark.parametrize("key", list(TC.CASES), ids=TC.case_id)
def test_tiles_attend_to_their_own_image_vs_fp64(hip, key, compute):
    c = _case(key)
    bound = c["bound"] if compute == "f32" else c["bound16"]
    before = hip.launch_count()
    got = _run(hip, key, compute)
    assert got is not None and hip.launch_count() == before + 1
    assert tuple(got.shape) == tuple(c["q"].shape)
    util.assert_finite(got, "attention_tokens(tiles=...) into a poisoned output")
    err = float((got.double() - c["want"]).abs().max())
    print("attention_tokens tiles %s %s: err %.3e, bound %.3e" % (TC.case_id(key), compute, err, bound))
    util.record_margin("test_gpu_attention_tokens_tiles vs fp64", "%s %s" % (TC.case_id(key), compute), err, bound)
    assert err <= bound, "max |diff| %.3e > bound %.3e" % (err, bound)
    assert hip.get_edit_batch() == 1


@pytest.mark.parametrize("compute", ["f32", "f16"])
@pytest.mark.parametrize("h,W,heads,d,T", [(8, 5, 4, 40, 3), (16, 8, 8, 80, 2), (8, 6, 1, 160, 4), (8, 6, 1, 16, 1)])
def test_one_edit_through_the_new_entry_equals_the_batched_entry_bit_for_bit(hip, h, W, heads, d, T, compute):
    g = torch.Generator().manual_seed(h + W + d + heads)
    C = heads * d
    q = (torch.randn(1, 16 * T, C, generator=g) * 2.0).to(DEV)
    k, v = (torch.randn(1, h * W, C, generator=g).to(DEV) for _ in range(2))
    idx = torch.tensor([(4 * (t % (h // 4)), 0) for t in range(T)], dtype=torch.int32, device=DEV)
    with util.poisoned():
        old = hip.attention_tokens(q, k, v, heads, d ** -0.5, compute=compute)
        new = hip.attention_tokens(q, k, v, heads, d ** -0.5, compute=compute, tiles=(idx, h, W))
    assert old is not None and new is not None
    util.assert_finite(new, "attention_tokens(tiles=...) at E = 1")
    assert torch.equal(old, new)


@pytest.mark.parametrize("key", [(3, 8, 5, 4, 40), (2, 16, 8, 8, 40), (3, 8, 5, 1, 160)], ids=TC.case_id)
def test_knobs_1_and_2_both_give_the_form_1_result(key, tuning):
    """Form 2 is two query tiles per workgroup, which may belong to two images: with `tiles` knob 2 is form 1 (the measurement build)."""
    hip = tuning
    c = _case(key)
    got = {}
    for knob in (1, 2):
        hip.tuning_set("attention_form", knob)
        try:
            got[knob] = _run(hip, key, "f32")
        finally:
            hip.tuning_set("attention_form", 0)
        assert got[knob] is not None
        util.assert_finite(got[knob], "attention_tokens(tiles=...) form knob %d" % knob)
    assert torch.equal(got[1], got[2])
    err = float((got[1].double() - c["want"]).abs().max())
    util.record_margin("test_gpu_attention_tokens_tiles form 1 vs fp64", TC.case_id(key), err, c["bound"])
    assert err <= c["bound"], "max |diff| %.3e > bound %.3e" % (err, c["bound"])


@pytest.mark.parametrize("compute", ["f32", "f16"])
@pytest.mark.parametrize("E,H", [(2, 12), (2, 4), (5, 24)])  # (6 rows per image, 2 rows, E does not divide H)
def test_heights_that_do_not_stack_are_refused_without_a_launch(hip, E, H, compute):
    W, heads, d = 8, 4, 40
    q = torch.randn(1, 16, heads * d, device=DEV)
    k, v = (torch.randn(1, H * W, heads * d, device=DEV) for _ in range(2))
    idx = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        assert hip.attention_tokens(q, k, v, heads, d ** -0.5, compute=compute, tiles=(idx, H, W)) is None
    assert hip.launch_count() == before


@pytest.mark.parametrize("compute", ["f32", "f16"])
def test_an_empty_list_is_ok_without_a_launch(hip, compute):
    E, h, W, heads, d = 2, 8, 8, 4, 40
    q = torch.empty(1, 0, heads * d, device=DEV)
    k, v = (torch.randn(1, E * h * W, heads * d, device=DEV) for _ in range(2))
    idx = torch.empty(0, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        out = hip.attention_tokens(q, k, v, heads, d ** -0.5, compute=compute, tiles=(idx, E * h, W))
    assert out is not None and tuple(out.shape) == (1, 0, heads * d)
    assert hip.launch_count() == before


def test_the_arguments_are_checked(hip):
    E, h, W, heads, d = 2, 8, 8, 4, 40
    q = torch.randn(1, 32, heads * d, device=DEV)
    k, v = (torch.randn(1, E * h * W, heads * d, device=DEV) for _ in range(2))
    idx = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    for bad in ((idx.long(), E * h, W), (idx[:1], E * h, W), (idx, E * h, W + 1), (idx.cpu(), E * h, W), (idx.t(), E * h, W)):
        with pytest.raises(ValueError, match="tiles"):
            hip.attention_tokens(q, k, v, heads, d ** -0.5, tiles=bad)
    with pytest.raises(ValueError, match="tiles"):
        hip.attention_tokens(q.expand(2, -1, -1), k.expand(2, -1, -1), v.expand(2, -1, -1), heads, d ** -0.5, tiles=(idx, E * h, W))
