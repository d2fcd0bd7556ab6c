"""sige_hip_resample_tiles_nhwc_f32 (sige_amd.hip.resample_tiles) alone: the activated, pooled conv-input tiles and the resampled
shortcut cells of a residual block that resamples inside the block, against fp64 on the CPU.

Truth: avg_pool2d(silu(x * s + t), 2) / avg_pool2d(x, 2) / nearest x2 in fp64, then a pixel walk over the zero-padded tensor (the
tiles) or over the cells the scatter of a 3x3 / stride-1 conv writes (the shortcut).  Bound for the averaged values: four times the
largest error of the reference's OWN fp32 arithmetic (the fp32 torch chain on the CPU) against that truth on the same inputs,
never below SWISH_ATOL -- the factor covers the library's v_exp / v_rcp SiLU (<= 1 ulp each) and another order of the three
additions.  Copies (UP) are bit-exact."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK, CELLS, OFFSET, STRIDE = (6, 6), (4, 4), (1, 1), (1, 1)  # a 3x3 / stride-1 conv over 6x6 tiles: 4x4 output cells
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(B, C, H, W, seed):
    """A large common offset and scales of both signs: s * x + t reaches both tails of SiLU (|z| up to ~30)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 3.0 + 5.0
    s = torch.randn(C, generator=g) * 1.5
    s[::2] = -s[::2].abs() - 0.25
    t = torch.randn(C, generator=g) * 2.0
    return x, s, t


def _index_lists(Ho, Wo, seed):
    from sige_amd.utils import reduce_mask

    full = reduce_mask(torch.ones(Ho, Wo, dtype=torch.bool), BLOCK, CELLS, OFFSET)  # every tile: origins 4 i - 1
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(full.shape[0], generator=g)[:max(2, full.shape[0] // 3)].sort().values
    return {
        "empty": torch.zeros((0, 2), dtype=torch.int32),
        "corner": torch.tensor([[-1, -1]], dtype=torch.int32),
        # three rows / columns of the window and two of its cells lie beyond the bottom-right border
        "overhang": torch.tensor([[Ho - 3, Wo - 3]], dtype=torch.int32),
        "full": full,
        "subset": full[pick].contiguous(),
    }


def _tiles_truth(P, idx):
    """P [B,C,Ho,Wo] -> [B*N,C,6,6] with zero padding: a pixel walk over the padded tensor."""
    pad = 8
    Pp = F.pad(P, (pad, pad, pad, pad))
    out = [Pp[b, :, h0 + pad:h0 + pad + BLOCK[0], w0 + pad:w0 + pad + BLOCK[1]] for b in range(P.shape[0]) for h0, w0 in idx.tolist()]
    return torch.stack(out) if out else P.new_zeros((0, P.shape[1]) + BLOCK)


def _cell_mask(idx, Ho, Wo):
    m = torch.zeros(Ho, Wo, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        hs, ws = (OFFSET[0] + h0) // STRIDE[0], (OFFSET[1] + w0) // STRIDE[1]
        m[max(hs, 0):max(min(hs + CELLS[0], Ho), 0), max(ws, 0):max(min(ws + CELLS[1], Wo), 0)] = True
    return m


def _nan_res(B, C, Ho, Wo):
    return _cl(torch.full((B, C, Ho, Wo), float("nan"), device="cuda"))


def _bound(ref32, truth):
    return max(4.0 * float((ref32.double() - truth).abs().max()), util.SWISH_ATOL)


def _check_res(res, truth, cells, bound, what):
    """`truth` on the active cells (bound None: bit-exact, truth fp32), the NaN it was filled with -- bit for bit -- elsewhere."""
    res = res.cpu()
    m = cells[None, None].expand_as(res)
    assert bool((res.view(torch.int32)[~m] == NAN_BITS).all()), "%s: a cell outside the active tiles was written" % what
    if not bool(m.any()):
        return 0.0
    got = res[m]
    util.assert_finite(got, what)
    if bound is None:
        assert torch.equal(got, truth[m]), what
        return 0.0
    err = float((got.double() - truth[m]).abs().max())
    assert err <= bound, "%s: max |diff| %.3e > %.3e" % (what, err, bound)
    return err


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(16, 16), (24, 40)])
@pytest.mark.parametrize("C", [4, 36, 64])
def test_resample_tiles_against_fp64(C, H, W, B):
    from sige_amd import hip

    x, s, t = _inputs(B, C, H, W, seed=C * 1000 + H * 10 + B)
    xd = x.double()
    act64 = F.avg_pool2d(F.silu(xd * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)), 2)
    act32 = F.avg_pool2d(F.silu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)), 2)
    raw64, raw32 = F.avg_pool2d(xd, 2), F.avg_pool2d(x, 2)
    up32 = F.interpolate(x, scale_factor=2)
    xg, sg, tg = _cl(x.cuda()), s.cuda(), t.cuda()
    tag = "C%d_%dx%d_B%d" % (C, H, W, B)

    # ---- DOWN: tiles (activated, then pooled; raw pooling without an affine) + pooled shortcut cells, one launch
    Ho, Wo = H // 2, W // 2
    lists = _index_lists(Ho, Wo, seed=C + H)
    for name, idx in lists.items():
        cells = _cell_mask(idx, Ho, Wo)
        for affine in (True, False):
            res = _nan_res(B, C, Ho, Wo)
            with util.poisoned():  # (the tile tensor the wrapper allocates starts as NaN)
                tiles = hip.resample_tiles(xg, "down", idx.cuda(), BLOCK, sg if affine else None, tg if affine else None,
                                           res=res, offset=OFFSET, stride=STRIDE, cells=CELLS)
            torch.cuda.synchronize()
            assert tuple(tiles.shape) == (B * idx.shape[0], C, *BLOCK) and (tiles.numel() == 0 or hip.is_cl(tiles) or C == 1)
            what = "%s down %s %s" % (tag, name, "affine" if affine else "raw")
            truth, ref32 = (act64, act32) if affine else (raw64, raw32)
            want = _tiles_truth(truth, idx)
            got = tiles.cpu()
            util.assert_finite(got, what + " tiles")
            inside = _tiles_truth(torch.ones_like(truth), idx) > 0
            assert bool((got[~inside] == 0).all()) and not bool(torch.signbit(got[~inside]).any()), what + ": padding is not exactly 0.0"
            bound = _bound(ref32, truth)
            err = float((got.double() - want).abs().max()) if got.numel() else 0.0
            util.record_margin("test_gpu_resample_tiles", what + " tiles", err, bound)
            assert err <= bound, "%s tiles: max |diff| %.3e > %.3e" % (what, err, bound)
            rb = _bound(raw32, raw64)
            util.record_margin("test_gpu_resample_tiles", what + " res", _check_res(res, raw64, cells, rb, what + " res"), rb)
        if name == "full":
            # the whole-tensor form = the tiled form over every tile, bit for bit
            whole = _nan_res(B, C, Ho, Wo)
            assert hip.resample_tiles(xg, "down", res=whole) is None
            assert torch.equal(whole, res)

    # ---- UP: shortcut cells are copies
    Ho, Wo = 2 * H, 2 * W
    for name, idx in _index_lists(Ho, Wo, seed=C + W).items():
        res = _nan_res(B, C, Ho, Wo)
        assert hip.resample_tiles(xg, "up", idx.cuda(), None, res=res, offset=OFFSET, stride=STRIDE, cells=CELLS) is None
        _check_res(res, up32, _cell_mask(idx, Ho, Wo), None, "%s up %s" % (tag, name))
        if name == "full":
            whole = _nan_res(B, C, Ho, Wo)
            hip.resample_tiles(xg, "up", res=whole)
            assert torch.equal(whole, res) and torch.equal(whole.cpu(), up32)


def test_resample_tiles_graph_replay_is_bit_identical():
    """One launch, no host synchronisation: a captured graph replays to the eager result, into the same buffers."""
    from sige_amd import hip

    B, C, H, W = 2, 36, 24, 40
    x, s, t = _inputs(B, C, H, W, seed=7)
    xg, sg, tg = _cl(x.cuda()), s.cuda(), t.cuda()
    idx = _index_lists(H // 2, W // 2, seed=3)["subset"].cuda()
    kw = dict(offset=OFFSET, stride=STRIDE, cells=CELLS)
    res_e = _nan_res(B, C, H // 2, W // 2)
    tiles_e = hip.resample_tiles(xg, "down", idx, BLOCK, sg, tg, res=res_e, **kw)
    torch.cuda.synchronize()
    res_g = _nan_res(B, C, H // 2, W // 2)
    before = hip.launch_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tiles_g = hip.resample_tiles(xg, "down", idx, BLOCK, sg, tg, res=res_g, **kw)
    assert hip.launch_count() - before == 1
    for _ in range(2):
        tiles_g.fill_(float("nan"))
        res_g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tiles_g, tiles_e)
        assert torch.equal(res_g.view(torch.int32), res_e.view(torch.int32))
