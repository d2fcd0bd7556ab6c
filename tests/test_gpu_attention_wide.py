"""sige_hip_attention_wide_f32 (sige_amd.hip.attention_wide) alone: softmax(scale * q k^T) v for head dimensions above 160, against
the same expression in fp64.

Bound: four times the error of the fp32 torch chain (bmm / softmax / bmm on the GPU) against that fp64 truth on the same inputs --
the rule of tests/test_gpu_resample_tiles.py: the kernel sums in another order than the GEMM library (key blocks dealt to four
waves and, with few query tiles, to several workgroups, merged by online-softmax weights), never a worse one by more than a small
factor.  Every margin is recorded (util.record_margin; kept as profiles/attention_wide_test_margins.jsonl)."""
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
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


def _inputs(B, Nq, Nk, heads, d, strided=False):
    """(q, k, v) on the GPU; `strided`: k and v are the two halves of ONE [B,Nk,2C] tensor, q a column slice of a wider matrix."""
    g = torch.Generator().manual_seed(Nq + Nk + d)
    C = heads * d
    if strided:
        kv = torch.randn(B, Nk, 2 * C, generator=g).to(DEV)
        wide = torch.randn(B, Nq, C + 64, generator=g).to(DEV)
        wide[:, :, :C] *= 2.0  # (scores with a spread: the softmax is not flat)
        return wide[:, :, :C], kv[:, :, :C], kv[:, :, C:]
    q, k, v = (torch.randn(B, n, C, generator=g).to(DEV) for n in (Nq, Nk, Nk))
    return q * 2.0, k, v


CASES = [
    (1, 16, 5, 1, 512, False),    # fewer key blocks than waves, tail keys
    (1, 48, 100, 1, 192, False),
    (1, 16, 16, 1, 176, False),   # the smallest d served: a 64-channel group with one 16-channel unit past d
    (2, 32, 256, 1, 512, False),  # key blocks split over workgroups
    (1, 64, 64, 2, 256, False),   # heads as strides
    (1, 32, 96, 1, 512, True),    # k | v the halves of one [B,Nk,2C] tensor, q a strided view
]


@pytest.mark.parametrize("B,Nq,Nk,heads,d,strided", CASES)
def test_attention_wide_vs_fp64(hip, B, Nq, Nk, heads, d, strided):
    q, k, v = _inputs(B, Nq, Nk, heads, d, strided)
    scale = d ** -0.5
    got = hip.attention_wide(q, k, v, heads, scale)
    assert got is not None and tuple(got.shape) == (B, Nq, heads * d)
    util.assert_finite(got, "attention_wide output")
    want = _chain(q, k, v, heads, scale, torch.float64)
    ref32 = _chain(q, k, v, heads, scale, torch.float32)
    bound = 4.0 * float((ref32.double() - want).abs().max())
    err = float((got.double() - want).abs().max())
    print("attention_wide B=%d Nq=%d Nk=%d heads=%d d=%d strided=%d: err %.3e, fp32 chain %.3e, bound %.3e"
          % (B, Nq, Nk, heads, d, strided, err, bound / 4.0, bound))
    util.record_margin("test_gpu_attention_wide vs fp64", "B=%d Nq=%d Nk=%d heads=%d d=%d strided=%d" % (B, Nq, Nk, heads, d, strided), err, bound)
    assert err <= bound, "max |diff| %.3e > 4 x the fp32 chain's %.3e" % (err, bound / 4.0)


def test_poisoned_output_comes_back_finite_and_nothing_else_is_written(hip):
    """`out` holds NaN before the call: every element of the [Nq, C] block is written; the rows past Nq and the columns past C of the
    over-allocated matrix it is a view of keep their NaN bit for bit."""
    B, Nq, Nk, heads, d = 1, 32, 100, 1, 192
    q, k, v = _inputs(B, Nq, Nk, heads, d)
    big = torch.full((B, Nq + 16, d + 32), float("nan"), device=DEV)
    out = big[:, :Nq, :d]
    got = hip.attention_wide(q, k, v, heads, d ** -0.5, out=out)
    assert got is out
    torch.cuda.synchronize()
    util.assert_finite(out, "attention_wide into a poisoned output")
    bits = big.view(torch.int32)
    assert bool((bits[:, Nq:] == NAN_BITS).all()), "a row past Nq was written"
    assert bool((bits[:, :, d:] == NAN_BITS).all()), "a column past C was written"
    fresh = hip.attention_wide(q, k, v, heads, d ** -0.5)
    assert torch.equal(fresh, out)


@pytest.mark.parametrize("Nq,Nk,d", [(32, 256, 512), (16, 40, 192)])  # (with and without the key split)
def test_graph_replay_equals_eager_bit_for_bit(hip, Nq, Nk, d):
    q, k, v = _inputs(1, Nq, Nk, 1, d)
    out = torch.empty(1, Nq, d, device=DEV)
    eager = hip.attention_wide(q, k, v, 1, d ** -0.5).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        hip.attention_wide(q, k, v, 1, d ** -0.5, out=out)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            hip.attention_wide(q, k, v, 1, d ** -0.5, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_release_graph_tickets_restarts_tickets_and_workspace(hip):
    """hip.release_graph_tickets() once every captured graph is gone: the graph regions of BOTH pools of the split finish (tickets and
    workspace) start over.  B = 1, heads = 1, Nq = 16, Nk = 128: ksplit = min(256 / 1, 8 / 4, 16) = 2, the smallest launch that draws
    on both.  A capture before and a capture after the release replay the eager bits, and so does an eager launch afterwards."""
    Nq, Nk, d = 16, 128, 192
    q, k, v = _inputs(1, Nq, Nk, 1, d)
    out = torch.empty(1, Nq, d, device=DEV)
    eager = hip.attention_wide(q, k, v, 1, d ** -0.5).clone()
    s = torch.cuda.Stream()

    def capture_and_replay():
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                hip.attention_wide(q, k, v, 1, d ** -0.5, out=out)
        torch.cuda.current_stream().wait_stream(s)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        return g

    g = capture_and_replay()
    del g
    hip.release_graph_tickets()
    g = capture_and_replay()
    out.fill_(float("nan"))
    assert hip.attention_wide(q, k, v, 1, d ** -0.5, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_head_dimensions_outside_the_range_are_refused(hip):
    for d in (160, 528, 200):
        q, k, v = (torch.randn(1, 16, d, device=DEV) for _ in range(3))
        assert hip.attention_wide(q, k, v, 1, d ** -0.5) is None
    q, k, v = (torch.randn(1, 24, 512, device=DEV) for _ in range(3))
    assert hip.attention_wide(q, k, v, 1, 512 ** -0.5) is None  # (Nq % 16)
    q, k, v = (torch.randn(1, 16, 160, device=DEV) for _ in range(3))
    assert hip.attention_tokens(q, k, v, 1, 160 ** -0.5) is not None  # (the existing entry serves d = 160)
