"""sige_hip_attention_wide_tiles_f32 (sige_amd.hip.attention_wide(..., tiles=...)) alone: under stacked edits the queries of a 4x4
tile attend to the keys of the tile's OWN image, in one launch for the tiles of every edit.

Truth: softmax(scale * q k^T) v in fp64 PER IMAGE -- tile t's 16 queries against the h * W keys of the image its origin row lies in,
and no others.  Bound: the rule of tests/test_gpu_attention_wide.py, four times the error of the fp32 torch chain against that
truth on the same inputs.  Inputs: q * 2 as there; V of image e is randn + 10 e, so that a key read from a neighbouring image moves
the output by units -- a thousand bounds.  The tile lists are written by hand and uneven between the images; every one has a tile
in the first and in the last tile row of an image, one has an image without a tile, one has every tile in the last image.  Every
destination holds NaN before the call.  Margins are recorded (util.record_margin; kept as
profiles/sd_vae_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.attention_stress import chain as _chain  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (E, h, W, d) -> the (origin row in the TALL image, origin column) of every tile, in list order
CASES = {
    # 16 keys per image: fewer key blocks than waves; one tile position per image, and every tile is in the last image
    (2, 4, 4, 192): [(4, 0)],
    # image 1 has no tile; images 0, 2 and 3 have 2, 3 and 1
    (4, 8, 8, 512): [(0, 0), (4, 4), (16, 4), (20, 0), (20, 4), (28, 0)],
    # the small VAE's middle block: 3 and 5 tiles, 256 keys per image (split over 4 workgroups per tile)
    (2, 16, 16, 192): [(0, 0), (4, 8), (12, 12), (16, 4), (20, 8), (24, 12), (28, 0), (28, 12)],
    # drawn through the key split at d = 512: image 2 has no tile
    (4, 16, 16, 512): [(0, 0), (12, 4), (28, 12), (16, 0), (48, 0), (52, 8), (60, 12)],
}


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


_made = {}


def _case(E, h, W, d, halves=False):
    """(q [1,16T,d], k, v [1,E*h*W,d], idx int32 [T,2], want fp64, bound) on the GPU, made once per process and left unchanged.
    `halves`: k and v are the two halves of ONE [1,E*h*W,2d] tensor (same values)."""
    key = (E, h, W, d)
    if key not in _made:
        tiles = CASES[key]
        T, N = len(tiles), h * W
        g = torch.Generator().manual_seed(1000 * E + 10 * h + d)
        q = (torch.randn(1, 16 * T, d, generator=g) * 2.0).to(DEV)
        k = torch.randn(1, E * N, d, generator=g).to(DEV)
        v = torch.randn(E, N, d, generator=g) + 10.0 * torch.arange(E, dtype=torch.float32).reshape(E, 1, 1)
        v = v.reshape(1, E * N, d).to(DEV)
        idx = torch.tensor(tiles, dtype=torch.int32, device=DEV)
        want = torch.empty(1, 16 * T, d, dtype=torch.float64, device=DEV)
        ref32 = torch.empty(1, 16 * T, d, dtype=torch.float32, device=DEV)
        for t, (row, _) in enumerate(tiles):
            e = row // h
            qs, ks, vs = q[:, 16 * t:16 * t + 16], k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N]
            want[:, 16 * t:16 * t + 16] = _chain(qs, ks, vs, 1, d ** -0.5, torch.float64)
            ref32[:, 16 * t:16 * t + 16] = _chain(qs, ks, vs, 1, d ** -0.5, torch.float32)
        kv = torch.cat([k, v], dim=2).contiguous()
        _made[key] = (q, k, v, kv, idx, want, 4.0 * float((ref32.double() - want).abs().max()))
    q, k, v, kv, idx, want, bound = _made[key]
    if halves:
        k, v = kv[:, :, :d], kv[:, :, d:]
    return q, k, v, idx, want, bound


def _poisoned(q):
    return torch.full(tuple(q.shape), float("nan"), device=DEV)


def _run(hip, E, h, W, d, halves=False, out=None):
    q, k, v, idx, _, _ = _case(E, h, W, d, halves)
    out = _poisoned(q) if out is None else out
    with _edits(hip, E):
        return hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W))


def test_the_lists_are_what_the_docstring_says():
    for (E, h, W, d), tiles in CASES.items():
        rows = {r % h for r, _ in tiles}
        assert 0 in rows and h - 4 in rows, "a tile in the first and in the last tile row of an image"
        assert all(r % 4 == 0 and c % 4 == 0 and 0 <= r < E * h and 0 <= c < W for r, c in tiles)
    per = lambda key: [sum(1 for r, _ in CASES[key] if r // key[1] == e) for e in range(key[0])]  # noqa: E731
    assert per((2, 4, 4, 192)) == [0, 1]           # every tile in the last image
    assert per((4, 8, 8, 512)) == [2, 0, 3, 1]     # an image with no tile
    assert per((2, 16, 16, 192)) == [3, 5]
    assert per((4, 16, 16, 512)) == [2, 2, 0, 3]


@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("E,h,W,d", list(CASES))
def test_tiles_attend_to_their_own_image_vs_fp64(hip, E, h, W, d, halves):
    _, _, _, _, want, bound = _case(E, h, W, d, halves)
    before = hip.launch_count()
    got = _run(hip, E, h, W, d, halves)
    assert got is not None and hip.launch_count() == before + 1
    util.assert_finite(got, "attention_wide(tiles=...) into a poisoned output")
    err = float((got.double() - want).abs().max())
    print("attention_wide tiles E=%d h=%d W=%d d=%d halves=%d: err %.3e, bound %.3e" % (E, h, W, d, halves, err, bound))
    util.record_margin("test_gpu_attention_wide_stacked vs fp64", "E=%d h=%d W=%d d=%d halves=%d" % (E, h, W, d, halves), err, bound)
    assert err <= bound, "max |diff| %.3e > 4 x the fp32 chain's %.3e" % (err, bound / 4.0)


def test_the_inputs_see_a_neighbours_keys(hip):
    """What `keys of every image` -- the batched entry on the tall K | V, the bug this entry exists for -- gives on these inputs is
    more than a thousand bounds from the truth."""
    E, h, W, d = 2, 16, 16, 192
    q, k, v, _, want, bound = _case(E, h, W, d)
    mixed = _chain(q, k, v, 1, d ** -0.5, torch.float64)
    assert float((mixed - want).abs().max()) > 1000.0 * bound


@pytest.mark.parametrize("h,W,d,T", [(16, 16, 192, 3), (16, 16, 512, 2), (5, 7, 256, 4)])  # (key split, key split at 512, tail keys)
def test_one_edit_through_the_new_entry_equals_the_batched_entry_bit_for_bit(hip, h, W, d, T):
    g = torch.Generator().manual_seed(h + W + d)
    q = (torch.randn(1, 16 * T, d, generator=g) * 2.0).to(DEV)
    k, v = (torch.randn(1, h * W, d, generator=g).to(DEV) for _ in range(2))
    idx = torch.tensor([(0, 0)] * T, dtype=torch.int32, device=DEV)
    old = hip.attention_wide(q, k, v, 1, d ** -0.5, out=_poisoned(q))
    new = hip.attention_wide(q, k, v, 1, d ** -0.5, out=_poisoned(q), tiles=(idx, h, W))
    assert old is not None and new is not None
    util.assert_finite(new, "attention_wide(tiles=...) at E = 1")
    assert torch.equal(old, new)


@pytest.mark.parametrize("E,h,W,d", [(2, 16, 16, 192), (4, 8, 8, 512)])  # (with and without the key split)
def test_graph_replay_and_repeats_equal_eager_bit_for_bit(hip, E, h, W, d):
    q, k, v, idx, _, _ = _case(E, h, W, d)
    eager = _run(hip, E, h, W, d).clone()
    for _ in range(3):
        assert torch.equal(_run(hip, E, h, W, d), eager)
    out = _poisoned(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with _edits(hip, E), torch.cuda.stream(s):
        hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W))
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W))
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("h", [6, 2])
def test_heights_that_do_not_stack_are_refused_without_a_launch(hip, h):
    E, W, d = 2, 8, 192
    q = torch.randn(1, 16, d, device=DEV)
    k, v = (torch.randn(1, E * h * W, d, device=DEV) for _ in range(2))
    idx = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        assert hip.attention_wide(q, k, v, 1, d ** -0.5, tiles=(idx, E * h, W)) is None
    assert hip.launch_count() == before


def test_an_empty_list_is_ok_without_a_launch(hip):
    E, h, W, d = 2, 8, 8, 192
    q = torch.empty(1, 0, d, device=DEV)
    k, v = (torch.randn(1, E * h * W, d, device=DEV) for _ in range(2))
    idx = torch.empty(0, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        out = hip.attention_wide(q, k, v, 1, d ** -0.5, tiles=(idx, E * h, W))
    assert out is not None and tuple(out.shape) == (1, 0, d)
    assert hip.launch_count() == before
