"""The sub-mobile SPADE layer's dense form under stacked edits (csrc/spade_separable.hip), kernel level, on NaN-poisoned destinations:
  * sige_hip_spade_separable_stats_nhwc_f32 (hip.spade_separable_stats_cl): the InstanceNorm affine of the two depthwise convs per
    image of the edit batch, against var_mean of the fp64 depthwise output on the CPU;
  * sige_hip_spade_separable_images_nhwc_f32 (hip.spade_separable_cl with [E,2,Ch] affines): one affine per image and taps that
    stop at a pixel's own image, against the E single-image calls (bit for bit) and the fp64 chain.

Bounds.  Statistics: |scale / scale64 - 1| <= 1e-4 and |shift - shift64| <= 1e-4 (1 + |shift64|), also with dw_bias = 100 + randn
(mean / sigma of 100 - 130).  The fp32 two-pass form (mean, then sum (d - mean)^2) is within 1e-5 there; a one-pass E[d^2] - E[d]^2 is
off by 5e-3 .. 1.5e-2: the bound is 10x over the first and at least 50x under the second.  Outputs: util.CONV_ATOL against fp64.  The
measured margins go through util.record_margin (profiles/spade_separable_stacked_test_margins.jsonl)."""
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
EPS = 1e-5
STAT_TOL = 1e-4

STATS = [(1, 2, 4, 8), (1, 5, 7, 24), (2, 4, 8, 16), (4, 8, 16, 64), (8, 4, 8, 96), (2, 16, 32, 128)]  # (E, h, W, Ch)
SEAM = [(4, 8, 16, 8), (8, 16, 24, 192)]                                                               # (h, W, Ch, oc)


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


class batch:
    """hip.set_edit_batch(E) for the block, 1 afterwards."""

    def __init__(self, hip, E):
        self.hip, self.E = hip, E

    def __enter__(self):
        self.hip.set_edit_batch(self.E)

    def __exit__(self, *exc):
        self.hip.set_edit_batch(1)
        return False


def _tall(imgs):
    """[E,Ch,h,W] on the CPU -> the tall channels-last GPU tensor [1,Ch,E*h,W]."""
    E, Ch, h, W = imgs.shape
    return imgs.permute(1, 0, 2, 3).reshape(1, Ch, E * h, W).to(DEV).contiguous(memory_format=CL)


def _one(img):
    return img.unsqueeze(0).to(DEV).contiguous(memory_format=CL)


def _dw(Ch, seed, big_mean=False):
    g = torch.Generator().manual_seed(seed)
    dw_w = torch.randn(2, Ch, 3, 3, generator=g) / 3
    dw_b = torch.randn(2, Ch, generator=g) + 100.0 if big_mean else 0.1 * torch.randn(2, Ch, generator=g)
    return dw_w, dw_b


def _pw(Ch, oc, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, oc, Ch, generator=g) / Ch ** 0.5, 0.1 * torch.randn(2, oc, generator=g)


def _depthwise64(imgs, dw_w, dw_b):
    """[E,2,Ch,h,W] fp64: per image, zero padding at ITS border."""
    Ch = imgs.shape[1]
    return torch.stack([F.conv2d(imgs.double(), dw_w[b].double().unsqueeze(1), dw_b[b].double(), padding=1, groups=Ch) for b in range(2)], 1)


def _stats64(imgs, dw_w, dw_b):
    var, mean = torch.var_mean(_depthwise64(imgs, dw_w, dw_b), unbiased=False, dim=[3, 4])
    scale = 1 / torch.sqrt(var + EPS)
    return scale, -mean * scale  # [E,2,Ch]


def _stats(hip, a, dw_w, dw_b):
    with util.poisoned():
        got = hip.spade_separable_stats_cl(a, dw_w.to(DEV), dw_b.to(DEV), EPS)
    return got


@pytest.mark.parametrize("big_mean", [False, True])
@pytest.mark.parametrize("E,h,W,Ch", STATS)
def test_statistics_vs_fp64(hip, E, h, W, Ch, big_mean):
    g = torch.Generator().manual_seed(1000 * E + 10 * h + Ch)
    imgs = torch.randn(E, Ch, h, W, generator=g)
    dw_w, dw_b = _dw(Ch, 7 * Ch + h, big_mean)
    with batch(hip, E):
        got = _stats(hip, _tall(imgs), dw_w, dw_b)
    assert got is not None
    sc, sh = (t.cpu().double() for t in got)
    assert tuple(sc.shape) == tuple(sh.shape) == (E, 2, Ch)
    util.assert_finite(sc, "scale over a poisoned buffer")
    util.assert_finite(sh, "shift over a poisoned buffer")
    sc64, sh64 = _stats64(imgs, dw_w, dw_b)
    e_sc = float((sc / sc64 - 1).abs().max())
    e_sh = float(((sh - sh64).abs() / (1 + sh64.abs())).max())
    what = "E=%d %dx%d Ch=%d%s" % (E, h, W, Ch, " bias~100" if big_mean else "")
    print("spade_separable_stats %s: scale %.3e shift %.3e (|shift64| max %.1f)" % (what, e_sc, e_sh, float(sh64.abs().max())))
    util.record_margin("test_gpu_spade_separable_stacked stats scale vs fp64", what, e_sc, STAT_TOL)
    util.record_margin("test_gpu_spade_separable_stacked stats shift vs fp64", what, e_sh, STAT_TOL)
    if big_mean:
        assert float(sh64.abs().min()) > 20  # (mean / sigma is large: the case a one-pass variance loses)
    assert e_sc <= STAT_TOL and e_sh <= STAT_TOL


def test_every_image_has_its_own_statistics(hip):
    """Image e = noise_e + 2 e: its affine is the single-image call's bit for bit, and it is not image 0's."""
    E, h, W, Ch = 4, 8, 16, 24
    g = torch.Generator().manual_seed(41)
    imgs = torch.randn(E, Ch, h, W, generator=g) + 2.0 * torch.arange(E).view(E, 1, 1, 1)
    dw_w, dw_b = _dw(Ch, 43)
    with batch(hip, E):
        sc, sh = _stats(hip, _tall(imgs), dw_w, dw_b)
    moved = 0.0
    for e in range(E):
        sc1, sh1 = _stats(hip, _one(imgs[e]), dw_w, dw_b)
        assert tuple(sc1.shape) == (1, 2, Ch)
        assert torch.equal(sc[e], sc1[0]) and torch.equal(sh[e], sh1[0]), e
        moved = max(moved, float((sh[e] - sh[0]).abs().max()))
    assert moved > 0.1


def _affines(E, Ch, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.3 * torch.randn(E, 2, Ch, generator=g), 0.3 * torch.randn(E, 2, Ch, generator=g)


def _chain64(imgs, dw_w, dw_b, sc, sh, pw_w, pw_b):
    """[E,2 oc,h,W] fp64: depthwise per image, image e's affine, pointwise, gamma | beta."""
    d = _depthwise64(imgs, dw_w, dw_b)
    n = d * sc.double()[:, :, :, None, None] + sh.double()[:, :, :, None, None]
    parts = [F.conv2d(n[:, b], pw_w[b].double()[:, :, None, None], pw_b[b].double()) for b in range(2)]
    return torch.cat(parts, 1)


def _dense(hip, a, dw_w, dw_b, sc, sh, pw_w, pw_b):
    """hip.spade_separable_cl on a full tensor, NaN-poisoned destination."""
    out = torch.full((1, 2 * pw_w.shape[1], a.shape[2], a.shape[3]), float("nan"), device=DEV).contiguous(memory_format=CL)
    got = hip.spade_separable_cl(a, *(t.to(DEV) for t in (dw_w, dw_b, sc, sh, pw_w, pw_b)), out=out, tiled=False)
    return got


@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("h,W,Ch,oc", SEAM)
def test_taps_and_affines_stop_at_the_seam(hip, E, h, W, Ch, oc):
    """+50 on the last row of every image: a tap that crosses the seam moves the first row of the next image by more than 10."""
    g = torch.Generator().manual_seed(100 * E + Ch)
    imgs = torch.randn(E, Ch, h, W, generator=g)
    imgs[:, :, h - 1, :] += 50.0
    dw_w, dw_b = _dw(Ch, 3 * Ch + E)
    pw_w, pw_b = _pw(Ch, oc, 5 * Ch + E)
    sc, sh = _affines(E, Ch, 11 * Ch + E)
    want = _chain64(imgs, dw_w, dw_b, sc, sh, pw_w, pw_b)
    # (the case can see a leak: the same chain on the tall image, zero padding at the outer border only)
    tall_cpu = imgs.permute(1, 0, 2, 3).reshape(1, Ch, E * h, W)
    d_leak = torch.stack([F.conv2d(tall_cpu.double(), dw_w[b].double().unsqueeze(1), dw_b[b].double(), padding=1, groups=Ch)
                          for b in range(2)], 1).reshape(2, Ch, E, h, W).permute(2, 0, 1, 3, 4)
    n_leak = d_leak * sc.double()[:, :, :, None, None] + sh.double()[:, :, :, None, None]
    leak = torch.cat([F.conv2d(n_leak[:, b], pw_w[b].double()[:, :, None, None], pw_b[b].double()) for b in range(2)], 1)
    assert float((leak - want).abs().max()) > 10

    with batch(hip, E):
        stacked = _dense(hip, _tall(imgs), dw_w, dw_b, sc, sh, pw_w, pw_b)
    assert stacked is not None and tuple(stacked.shape) == (1, 2 * oc, E * h, W)
    util.assert_finite(stacked, "stacked spade_separable output over a poisoned buffer")
    singles = [_dense(hip, _one(imgs[e]), dw_w, dw_b, sc[e], sh[e], pw_w, pw_b) for e in range(E)]
    assert all(s is not None for s in singles)
    stitched = torch.cat(singles, dim=2)
    assert torch.equal(stacked, stitched)
    want_tall = want.permute(1, 0, 2, 3).reshape(1, 2 * oc, E * h, W)
    what = "E=%d %dx%d Ch=%d oc=%d" % (E, h, W, Ch, oc)
    for name, t in (("stacked", stacked), ("stitched", stitched)):
        err = float((t.cpu().double() - want_tall).abs().max())
        print("spade_separable_images %s %s: err %.3e (|want| max %.1f)" % (what, name, err, float(want.abs().max())))
        util.record_margin("test_gpu_spade_separable_stacked seam vs fp64", "%s %s" % (what, name), err, util.CONV_ATOL)
        assert err <= util.CONV_ATOL


def test_one_image_through_the_new_entry_equals_the_old_dense_call(hip):
    Ch, oc, H, W = 24, 192, 5, 7
    g = torch.Generator().manual_seed(77)
    a = _one(torch.randn(Ch, H, W, generator=g))
    dw_w, dw_b = _dw(Ch, 79)
    pw_w, pw_b = _pw(Ch, oc, 83)
    sc, sh = _affines(1, Ch, 89)
    old = _dense(hip, a, dw_w, dw_b, sc[0], sh[0], pw_w, pw_b)
    n0 = hip.launch_count()
    new = _dense(hip, a, dw_w, dw_b, sc, sh, pw_w, pw_b)
    assert hip.launch_count() == n0 + 1
    util.assert_finite(new, "output over a poisoned buffer")
    assert torch.equal(old, new)


def test_refusals_come_without_a_launch(hip):
    Ch, oc, W, E = 16, 8, 8, 2
    dw_w, dw_b = _dw(Ch, 5)
    pw_w, pw_b = _pw(Ch, oc, 6)
    sc, sh = _affines(E, Ch, 7)
    g = torch.Generator().manual_seed(8)
    with batch(hip, E):
        ok = _tall(torch.randn(E, Ch, 4, W, generator=g))
        assert _stats(hip, ok, dw_w, dw_b) is not None and _dense(hip, ok, dw_w, dw_b, sc, sh, pw_w, pw_b) is not None
        torch.cuda.synchronize()
        before = hip.launch_count()
        for h in (2, 6):  # (below four rows; no power of two)
            a = _tall(torch.randn(E, Ch, h, W, generator=g))
            assert _stats(hip, a, dw_w, dw_b) is None
            assert _dense(hip, a, dw_w, dw_b, sc, sh, pw_w, pw_b) is None
        assert _dense(hip, ok, dw_w, dw_b, sc[0], sh[0], pw_w, pw_b) is None  # (ONE affine for a tall tensor: the old entry refuses)
        assert hip.launch_count() == before
    assert hip.get_edit_batch() == 1


def test_bit_identical_from_run_to_run(hip):
    E, h, W, Ch, oc = 4, 8, 16, 64, 96
    g = torch.Generator().manual_seed(33)
    a = _tall(torch.randn(E, Ch, h, W, generator=g))
    dw_w, dw_b = _dw(Ch, 19)
    pw_w, pw_b = _pw(Ch, oc, 23)
    with batch(hip, E):
        sc, sh = _stats(hip, a, dw_w, dw_b)
        first = _dense(hip, a, dw_w, dw_b, sc, sh, pw_w, pw_b)
        for _ in range(3):
            sc2, sh2 = _stats(hip, a, dw_w, dw_b)
            assert torch.equal(sc, sc2) and torch.equal(sh, sh2)
            assert torch.equal(first, _dense(hip, a, dw_w, dw_b, sc2, sh2, pw_w, pw_b))
