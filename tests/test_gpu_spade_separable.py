"""sige_hip_spade_separable_nhwc_f32 (sige_amd.hip.spade_separable_cl) alone: gamma | beta of a sub-mobile SPADE layer -- per branch
depthwise 3x3 + bias, a per-channel affine, pointwise 1x1 + bias -- against torch in fp64 on the CPU (F.conv2d(groups=Ch) -> affine
-> 1x1 conv -> cat), in the tiled form (slabs [T,Ch,6,6] that carry their halo) and the dense form (zero padding at the border).

Tolerance: util.CONV_ATOL absolute on O(1) outputs (a ~ N(0,1), depthwise weights ~ N(0,1)/3, pointwise weights ~ N(0,1)/sqrt(Ch)).
Exact fp32 products summed in fp32 need about 1e-6 (1e-5 in the case with scales ~ 10); the measured margins are in
profiles/spade_separable_test_margins.jsonl -- the bound is not to be tightened without that file."""
import os
import sys

import pytest
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

TILED = [(1, 8, 4), (1, 16, 8), (5, 24, 24), (7, 48, 96), (3, 96, 512), (2, 128, 48)]           # (T, Ch, oc)
DENSE = [(16, 8, 2, 4), (24, 192, 5, 7), (64, 512, 8, 16), (96, 32, 16, 33)]                    # (Ch, oc, H, W)


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


def _weights(Ch, oc, seed, big_scale=False):
    g = torch.Generator().manual_seed(seed)
    dw_w = torch.randn(2, Ch, 3, 3, generator=g) / 3
    dw_b = 0.1 * torch.randn(2, Ch, generator=g)
    sc = (10.0 if big_scale else 1.0) + 0.3 * torch.randn(2, Ch, generator=g)
    sh = 0.3 * torch.randn(2, Ch, generator=g)
    pw_w = torch.randn(2, oc, Ch, generator=g) / Ch ** 0.5
    pw_b = 0.1 * torch.randn(2, oc, generator=g)
    return dw_w, dw_b, sc, sh, pw_w, pw_b


def _reference(a, ws, padding):
    """fp64, CPU.  a [N,Ch,h,w]; padding 0: the slabs carry their halo; 1: zero padding."""
    dw_w, dw_b, sc, sh, pw_w, pw_b = (t.double() for t in ws)
    Ch = a.shape[1]
    parts = []
    for b in range(2):
        d = F.conv2d(a.double(), dw_w[b].unsqueeze(1), dw_b[b], padding=padding, groups=Ch)
        n = d * sc[b].view(1, -1, 1, 1) + sh[b].view(1, -1, 1, 1)
        parts.append(F.conv2d(n, pw_w[b].unsqueeze(-1).unsqueeze(-1), pw_b[b]))
    return torch.cat(parts, 1)


def _run(hip, a, ws, tiled):
    """The launch on a NaN-poisoned destination."""
    oc = ws[4].shape[1]
    shape = (a.shape[0], 2 * oc, 4, 4) if tiled else (1, 2 * oc, a.shape[2], a.shape[3])
    out = torch.full(shape, float("nan"), device=DEV).contiguous(memory_format=CL)
    got = hip.spade_separable_cl(a.to(DEV).contiguous(memory_format=CL), *(t.to(DEV) for t in ws), out=out, tiled=tiled)
    return out, got


def _check(hip, a, ws, tiled, what):
    out, got = _run(hip, a, ws, tiled)
    assert got is out
    util.assert_finite(out, "spade_separable output over a poisoned buffer")
    want = _reference(a, ws, 0 if tiled else 1)
    err = float((out.cpu().double() - want).abs().max())
    print("spade_separable %s: err %.3e (|want| max %.2f)" % (what, err, float(want.abs().max())))
    util.record_margin("test_gpu_spade_separable vs fp64", what, err, util.CONV_ATOL)
    assert float(want.abs().max()) > 0.5
    assert err <= util.CONV_ATOL
    return out, want


@pytest.mark.parametrize("T,Ch,oc", TILED)
def test_tiled_vs_fp64(hip, T, Ch, oc):
    g = torch.Generator().manual_seed(100 * Ch + oc)
    a = torch.randn(T, Ch, 6, 6, generator=g)
    _check(hip, a, _weights(Ch, oc, 7 * Ch + oc), True, "tiled T=%d Ch=%d oc=%d" % (T, Ch, oc))


@pytest.mark.parametrize("Ch,oc,H,W", DENSE)
def test_dense_vs_fp64(hip, Ch, oc, H, W):
    g = torch.Generator().manual_seed(100 * Ch + oc + H)
    a = torch.randn(1, Ch, H, W, generator=g)
    _check(hip, a, _weights(Ch, oc, 7 * Ch + oc), False, "dense Ch=%d oc=%d %dx%d" % (Ch, oc, H, W))


def test_scales_of_ten(hip):
    """The cached InstanceNorm scale is 1 / std of the depthwise output: ~10 for a quiet channel."""
    g = torch.Generator().manual_seed(5)
    a = 0.1 * torch.randn(5, 24, 6, 6, generator=g)
    _check(hip, a, _weights(24, 24, 11, big_scale=True), True, "tiled T=5 Ch=24 oc=24 scales~10")


def test_dense_padding_is_zero(hip):
    """a shifted by +3.0: a clamped (replicate) halo instead of zeros moves the border outputs by O(1)."""
    Ch, oc, H, W = 24, 192, 5, 7
    g = torch.Generator().manual_seed(9)
    a = torch.randn(1, Ch, H, W, generator=g) + 3.0
    ws = _weights(Ch, oc, 13)
    want = _reference(a, ws, 1)
    leak = _reference(F.pad(a, (1, 1, 1, 1), mode="replicate"), ws, 0)
    assert float((leak - want).abs().max()) > 100 * util.CONV_ATOL  # (the case can see a leak)
    out, _ = _run(hip, a, ws, False)
    util.assert_finite(out, "spade_separable output over a poisoned buffer")
    err = float((out.cpu().double() - want).abs().max())
    util.record_margin("test_gpu_spade_separable padding", "dense +3.0 Ch=24 oc=192 5x7", err, util.CONV_ATOL)
    assert err <= util.CONV_ATOL


def test_tiled_equals_dense_on_the_same_pixels(hip):
    """Slabs cut out of the zero-padded full tensor: both forms sum in the same order, so the results are bit-identical."""
    Ch, oc, H, W = 48, 96, 8, 12
    g = torch.Generator().manual_seed(21)
    a = torch.randn(1, Ch, H, W, generator=g)
    ws = _weights(Ch, oc, 17)
    dense, _ = _run(hip, a, ws, False)
    ap = F.pad(a, (1, 1, 1, 1))
    origins = [(y, x) for y in range(0, H, 4) for x in range(0, W, 4)]
    slabs = torch.cat([ap[:, :, y:y + 6, x:x + 6] for y, x in origins])
    tiles, _ = _run(hip, slabs, ws, True)
    util.assert_finite(tiles, "tiled output")
    cut = torch.cat([dense[:, :, y:y + 4, x:x + 4] for y, x in origins])
    diff = float((tiles - cut).abs().max())
    util.record_margin("test_gpu_spade_separable tiled vs dense", "Ch=48 oc=96 8x12", diff, util.CONV_ATOL)
    assert torch.equal(tiles, cut)


def test_refuses_unsupported_shapes_without_a_launch(hip):
    def call(Ch, oc, hw=(6, 6), tiled=True):
        a = torch.randn(2, Ch, *hw)
        return hip.spade_separable_cl(a.to(DEV).contiguous(memory_format=CL), *(t.to(DEV) for t in _weights(Ch, oc, 3)), tiled=tiled)

    assert call(16, 8) is not None
    torch.cuda.synchronize()
    before = hip.launch_count()
    assert call(6, 8) is None        # Ch % 4
    assert call(132, 8) is None      # Ch > 128
    assert call(16, 6) is None       # oc % 4
    assert call(16, 8, hw=(5, 5)) is None  # not a 6x6 slab
    empty = hip.spade_separable_cl(torch.empty(0, 16, 6, 6, device=DEV).contiguous(memory_format=CL),
                                   *(t.to(DEV) for t in _weights(16, 8, 3)), tiled=True)
    assert empty is not None and tuple(empty.shape) == (0, 16, 4, 4)  # (no tiles: OK without a launch)
    assert hip.launch_count() == before
    assert call(16, 8) is not None and hip.launch_count() == before + 1  # (ONE launch)


@pytest.mark.parametrize("tiled", [True, False])
def test_bit_identical_from_run_to_run(hip, tiled):
    g = torch.Generator().manual_seed(33)
    a = torch.randn(7, 48, 6, 6, generator=g) if tiled else torch.randn(1, 96, 16, 33, generator=g)
    ws = _weights(a.shape[1], 96, 19)
    first, _ = _run(hip, a, ws, tiled)
    for _ in range(3):
        again, _ = _run(hip, a, ws, tiled)
        assert torch.equal(first, again)
