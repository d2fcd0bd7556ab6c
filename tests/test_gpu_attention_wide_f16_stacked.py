"""sige_hip_attention_wide_tiles_f16c (sige_amd.hip.attention_wide(..., tiles=..., compute="f16")) alone, on the cases of
tests/test_gpu_attention_wide_stacked.py (imported, not copied): under stacked edits the queries of a 4x4 tile attend to the keys of
the tile's OWN image, in one launch for the tiles of every edit, with fp16 operands.

Truth: softmax(scale * q k^T) v in fp64 PER IMAGE.  Bound: bound16 = max(4 * e16, 2e-5 * (1 + max|want|)), e16 the error of
tests.attention_f16.emulate, per image, on the same inputs -- the rule of tests/attention_f16.py.  V of image e is randn + 10 e, so that a
key read from a neighbouring image moves the output by units.  Every destination holds NaN before the call.  Margins are recorded
(util.record_margin; kept as profiles/attention_wide_f16_test_margins.jsonl)."""
import pytest
import torch

from tests import attention_f16 as F
from tests import util
from tests.attention_stress import chain as _chain
from tests.test_gpu_attention_wide_stacked import CASES, _case, _edits, _poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


_bounds = {}


def _bound16(E, h, W, d):
    """(want fp64 on the CPU, e16, bound16) of a case: the emulation tile by tile against its own image's keys; once per process."""
    key = (E, h, W, d)
    if key not in _bounds:
        q, k, v, _, want, _ = _case(E, h, W, d)
        q, k, v, want = q.cpu(), k.cpu(), v.cpu(), want.cpu()
        N, e16 = h * W, 0.0
        for t, (row, _) in enumerate(CASES[key]):
            e = row // h
            em = F.emulate(q[:, 16 * t:16 * t + 16], k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N], 1, d ** -0.5)
            e16 = max(e16, float((em.double() - want[:, 16 * t:16 * t + 16]).abs().max()))
        _bounds[key] = (want, e16, F.bound16(want, e16))
    return _bounds[key]


def _run(hip, E, h, W, d, halves=False, out=None):
    q, k, v, idx, _, _ = _case(E, h, W, d, halves)
    out = _poisoned(q) if out is None else out
    with _edits(hip, E):
        return hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W), compute="f16")


@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("E,h,W,d", list(CASES))
def test_tiles_attend_to_their_own_image_vs_fp64(hip, E, h, W, d, halves):
    want, e16, tol = _bound16(E, h, W, d)
    before = hip.launch_count()
    got = _run(hip, E, h, W, d, halves)
    assert got is not None and hip.launch_count() == before + 1
    util.assert_finite(got, "attention_wide(tiles=..., f16) into a poisoned output")
    err = float((got.double().cpu() - want).abs().max())
    print("attention_wide f16 tiles E=%d h=%d W=%d d=%d halves=%d: err %.3e, emulation %.3e, bound %.3e" % (E, h, W, d, halves, err, e16, tol))
    util.record_margin("test_gpu_attention_wide_f16_stacked vs fp64", "E=%d h=%d W=%d d=%d halves=%d" % (E, h, W, d, halves), err, tol)
    assert err <= tol, "max |diff| %.3e > bound %.3e (emulation %.3e)" % (err, tol, e16)


def test_the_inputs_see_a_neighbours_keys(hip):
    """What `keys of every image` gives on these inputs is more than a thousand bounds from the truth."""
    E, h, W, d = 2, 16, 16, 192
    q, k, v, _, want, _ = _case(E, h, W, d)
    _, _, tol = _bound16(E, h, W, d)
    mixed = _chain(q, k, v, 1, d ** -0.5, torch.float64)
    assert float((mixed - want).abs().max()) > 1000.0 * tol


@pytest.mark.parametrize("h,W,d,T", [(16, 16, 192, 3), (16, 16, 512, 2), (5, 7, 256, 4)])  # (key split, key split at 512, tail keys)
def test_one_edit_through_the_tiles_entry_equals_the_batched_f16_entry_bit_for_bit(hip, h, W, d, T):
    g = torch.Generator().manual_seed(h + W + d)
    q = (torch.randn(1, 16 * T, d, generator=g) * 2.0).to(DEV)
    k, v = (torch.randn(1, h * W, d, generator=g).to(DEV) for _ in range(2))
    idx = torch.tensor([(0, 0)] * T, dtype=torch.int32, device=DEV)
    old = hip.attention_wide(q, k, v, 1, d ** -0.5, out=_poisoned(q), compute="f16")
    new = hip.attention_wide(q, k, v, 1, d ** -0.5, out=_poisoned(q), tiles=(idx, h, W), compute="f16")
    assert old is not None and new is not None
    util.assert_finite(new, "attention_wide(tiles=..., f16) at E = 1")
    assert torch.equal(old, new)
    assert not torch.equal(new, hip.attention_wide(q, k, v, 1, d ** -0.5, out=_poisoned(q), tiles=(idx, h, W)))


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
        hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W), compute="f16")
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, tiles=(idx, E * h, W), compute="f16")
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del g


@pytest.mark.parametrize("h", [6, 2])
def test_heights_that_do_not_stack_are_refused_without_a_launch(hip, h):
    E, W, d = 2, 8, 192
    q = torch.randn(1, 16, d, device=DEV)
    k, v = (torch.randn(1, E * h * W, d, device=DEV) for _ in range(2))
    idx = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        assert hip.attention_wide(q, k, v, 1, d ** -0.5, tiles=(idx, E * h, W), compute="f16") is None
    assert hip.launch_count() == before


def test_an_empty_list_is_ok_without_a_launch(hip):
    E, h, W, d = 2, 8, 8, 192
    q = torch.empty(1, 0, d, device=DEV)
    k, v = (torch.randn(1, E * h * W, d, device=DEV) for _ in range(2))
    idx = torch.empty(0, 2, dtype=torch.int32, device=DEV)
    before = hip.launch_count()
    with _edits(hip, E):
        out = hip.attention_wide(q, k, v, 1, d ** -0.5, tiles=(idx, E * h, W), compute="f16")
    assert out is not None and tuple(out.shape) == (1, 0, d)
    assert hip.launch_count() == before
