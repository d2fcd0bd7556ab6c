"""sige_hip_resample_tiles_nhwc_f32 (sige_amd.hip.resample_tiles) alone under stacked edits (hip.set_edit_batch(E)): the tensors
are the tall image [1,C,E*hp,W] of E = 3 images, the index list holds the tiles of all of them at the resampled resolution.

A tile belongs to the image its window's third row lies in.  A window row of conv1's tiles beyond that image is exactly +0.0 (never
the neighbour's pooled pixels, never passed through the affine or SiLU), and the rows of the shortcut cells are clipped to that
image.  Truth, bounds and inputs are those of tests/test_gpu_resample_tiles.py, PER IMAGE: avg_pool2d(silu(x * s + t), 2) /
avg_pool2d(x, 2) / nearest x2 in fp64 on each image alone, its pixel walk with zero padding, every tile of the concatenated list
from the image the rule gives it to (_by_rule: the candidates a full single-image list ends with, at origin row ho - 1, are in the
tall list the next image's origin -1); averaged values within
max(4 x the fp32 torch chain's own error against that truth, SWISH_ATOL), copies bit-exact, padding exactly +0.0, `res` keeps the NaN
it was filled with outside the active cells of each tile's own image.  The launch is also bit-identical to E separate launches on
the E images at edit batch 1.

Before any launch the test checks on the CPU that its inputs can see a missed seam: the fp64 result of reading the tall tensor as
ONE image differs from the per-image truth by more than 1e-2 in the seam tiles, and the shortcut cells of an overhanging tile differ.

Margins go through util.record_margin (kept as profiles/pd_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.test_gpu_resample_tiles import (BLOCK, CELLS, OFFSET, STRIDE, _bound, _cell_mask, _check_res, _cl, _index_lists,  # noqa: E402
                                           _inputs, _nan_res, _tiles_truth)

pytestmark = pytest.mark.gpu
E = 3  # (not a power of two: a shift / count mix-up shows)
KW = dict(offset=OFFSET, stride=STRIDE, cells=CELLS)
TEST = "test_gpu_resample_tiles_stacked"


def _tall(t):
    """[E,C,h,w] -> [1,C,E*h,w]: the images one below the other."""
    return torch.cat(list(t), dim=1)[None]


def _stacked_lists(ho, wo, seed):
    """{name: [per-image list of tile origins at the image's own rows]}; the launch gets them concatenated, each with its image's
    row offset."""
    per = [_index_lists(ho, wo, seed + 17 * e) for e in range(E)]  # (another random third per image)
    none = torch.zeros((0, 2), dtype=torch.int32)

    def only(e, idx):
        return [idx if k == e else none for k in range(E)]

    return {
        "empty": [none] * E,
        "full": [p["full"] for p in per],
        "subset": [p["subset"] for p in per],
        # the first window row is the previous image's last row
        "corner of image 1": only(1, per[0]["corner"]),
        "corner of image 2": only(2, per[0]["corner"]),
        # three window rows and two rows of cells lie in the next image
        "overhang of image 0": only(0, per[0]["overhang"]),
        "overhang of image 1": only(1, per[0]["overhang"]),
    }


def _concat(local, ho):
    return torch.cat([idx + torch.tensor([e * ho, 0], dtype=torch.int32) for e, idx in enumerate(local)]).contiguous()


def _by_rule(idx, ho):
    """[(image, origin at that image's own rows)] of the tall list: a tile belongs to the image its window's THIRD row lies in.  (A
    full single-image list ends with the candidates at origin row ho - 1, whose only row inside the image is its last one; in the
    tall list that origin is the next image's origin -1 -- the rule reads it so -- and behind the last image it belongs to none.)"""
    return [((h0 + 2) // ho, [h0 - ((h0 + 2) // ho) * ho, w0]) for h0, w0 in idx.tolist()]


def _one(origin):
    return torch.tensor([origin], dtype=torch.int32)


def _tiles_per_image(P, idx, ho):
    """P [E,C,ho,wo] -> every tile of the tall list from ITS image alone (zero padding around that image), in the list's order."""
    out = [_tiles_truth(P[e:e + 1], _one(o)) if 0 <= e < E else P.new_zeros((1, P.shape[1]) + BLOCK) for e, o in _by_rule(idx, ho)]
    return torch.cat(out) if out else P.new_zeros((0, P.shape[1]) + BLOCK)


def _cells_per_image(idx, ho, wo):
    m = torch.zeros(E, ho, wo, dtype=torch.bool)
    for e, o in _by_rule(idx, ho):
        if 0 <= e < E:
            m[e] |= _cell_mask(_one(o), ho, wo)
    return m.reshape(E * ho, wo)


def _seam_list(name):
    return "corner" in name or "overhang" in name


def _singles(x_imgs, mode, idx, ho, block, s, t):
    """E separate launches at edit batch 1, each image with the tiles the rule gives it: (tiles in the tall list's order or None,
    res [1,C,E*ho,wo]).  A tile behind the last image is all padding."""
    from sige_amd import hip

    assert hip.get_edit_batch() == 1
    rule = _by_rule(idx, ho)
    C = x_imgs.shape[1]
    tiles = torch.zeros((idx.shape[0], C) + BLOCK, device="cuda") if block is not None else None
    res = []
    for e in range(E):
        xe = _cl(x_imgs[e:e + 1].cuda())
        _, _, H, W = xe.shape
        r = _nan_res(1, C, H // 2, W // 2) if mode == "down" else _nan_res(1, C, 2 * H, 2 * W)
        at = [k for k, (img, _) in enumerate(rule) if img == e]
        mine = torch.tensor([rule[k][1] for k in at], dtype=torch.int32).reshape(-1, 2)
        te = hip.resample_tiles(xe, mode, mine.cuda(), block, s, t, res=r, **KW)
        if block is not None and at:
            tiles[at] = te
        res.append(r)
    torch.cuda.synchronize()
    return tiles, _cl(torch.cat(res, dim=2))


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("W", [16, 24])
@pytest.mark.parametrize("hp", [8, 16])
def test_stacked_down_against_fp64_per_image(hp, W, C):
    from sige_amd import hip

    x, s, t = _inputs(E, C, hp, W, seed=C * 1000 + hp * 10 + W)
    xd, s4, t4 = x.double(), s.view(1, -1, 1, 1), t.view(1, -1, 1, 1)
    act64 = F.avg_pool2d(F.silu(xd * s4.double() + t4.double()), 2)
    act32 = F.avg_pool2d(F.silu(x * s4 + t4), 2)
    raw64, raw32 = F.avg_pool2d(xd, 2), F.avg_pool2d(x, 2)
    ho, wo = hp // 2, W // 2
    lists = _stacked_lists(ho, wo, seed=C + hp)
    tag = "E%d_C%d_%dx%d" % (E, C, hp, W)

    # ---- the inputs can see a missed seam (CPU, before any launch)
    for name, local in lists.items():
        if not _seam_list(name):
            continue
        idx = _concat(local, ho)
        for truth in (act64, raw64):
            no_seam = _tiles_truth(_tall(truth), idx)
            assert float((no_seam - _tiles_per_image(truth, idx, ho)).abs().max()) > 1e-2, name
        if "overhang" in name:
            assert not torch.equal(_cell_mask(idx, E * ho, wo), _cells_per_image(idx, ho, wo)), name

    xg, sg, tg = _cl(_tall(x).cuda()), s.cuda(), t.cuda()
    for name, local in lists.items():
        idx = _concat(local, ho)
        cells = _cells_per_image(idx, ho, wo)
        for affine in (True, False):
            sa, ta = (sg, tg) if affine else (None, None)
            res = _nan_res(1, C, E * ho, wo)
            hip.set_edit_batch(E)
            try:
                with util.poisoned():  # (the tile tensor the wrapper allocates starts as NaN)
                    tiles = hip.resample_tiles(xg, "down", idx.cuda(), BLOCK, sa, ta, res=res, **KW)
                torch.cuda.synchronize()
            finally:
                hip.set_edit_batch(1)
            assert tuple(tiles.shape) == (idx.shape[0], C, *BLOCK)
            what = "%s down %s %s" % (tag, name, "affine" if affine else "raw")
            truth, ref32 = (act64, act32) if affine else (raw64, raw32)
            want = _tiles_per_image(truth, idx, ho)
            got = tiles.cpu()
            util.assert_finite(got, what + " tiles")
            inside = _tiles_per_image(torch.ones_like(truth), idx, ho) > 0
            assert bool((got[~inside] == 0).all()) and not bool(torch.signbit(got[~inside]).any()), what + ": padding is not exactly +0.0"
            bound = _bound(ref32, truth)
            err = float((got.double() - want).abs().max()) if got.numel() else 0.0
            print("%s tiles: %.3e (bound %.3e)" % (what, err, bound))
            util.record_margin(TEST, what + " tiles", err, bound)
            assert err <= bound, "%s tiles: max |diff| %.3e > %.3e" % (what, err, bound)
            rb = _bound(raw32, raw64)
            util.record_margin(TEST, what + " res", _check_res(res, _tall(raw64), cells, rb, what + " res"), rb)
            # the arithmetic per element is that of E single launches
            tiles_1, res_1 = _singles(x, "down", idx, ho, BLOCK, sa, ta)
            assert torch.equal(tiles.view(torch.int32), tiles_1.view(torch.int32)), what + ": tiles differ from E single launches"
            assert torch.equal(res.view(torch.int32), res_1.view(torch.int32)), what + ": res differs from E single launches"
        if name == "full":
            # the whole-tensor form stacks as it is (an even per-image height: no 2x2 window straddles a seam)
            whole = _nan_res(1, C, E * ho, wo)
            hip.set_edit_batch(E)
            try:
                assert hip.resample_tiles(xg, "down", res=whole) is None
            finally:
                hip.set_edit_batch(1)
            assert torch.equal(whole, res)


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("W", [16, 24])
@pytest.mark.parametrize("hp", [4, 8])
def test_stacked_up_cells_are_copies_of_the_tiles_own_image(hp, W, C):
    from sige_amd import hip

    x, _, _ = _inputs(E, C, hp, W, seed=C * 1000 + hp * 10 + W + 1)
    up32 = F.interpolate(x, scale_factor=2)
    ho, wo = 2 * hp, 2 * W
    lists = _stacked_lists(ho, wo, seed=C + W)
    for name, local in lists.items():  # (the inputs can see a missed seam)
        if "overhang" in name:
            assert not torch.equal(_cell_mask(_concat(local, ho), E * ho, wo), _cells_per_image(_concat(local, ho), ho, wo)), name
    xg = _cl(_tall(x).cuda())
    for name, local in lists.items():
        idx = _concat(local, ho)
        res = _nan_res(1, C, E * ho, wo)
        hip.set_edit_batch(E)
        try:
            assert hip.resample_tiles(xg, "up", idx.cuda(), None, res=res, **KW) is None
            torch.cuda.synchronize()
        finally:
            hip.set_edit_batch(1)
        what = "E%d_C%d_%dx%d up %s" % (E, C, hp, W, name)
        _check_res(res, _tall(up32), _cells_per_image(idx, ho, wo), None, what)
        _, res_1 = _singles(x, "up", idx, ho, None, None, None)
        assert torch.equal(res.view(torch.int32), res_1.view(torch.int32)), what + ": res differs from E single launches"
        if name == "full":
            whole = _nan_res(1, C, E * ho, wo)
            hip.set_edit_batch(E)
            try:
                hip.resample_tiles(xg, "up", res=whole)
            finally:
                hip.set_edit_batch(1)
            assert torch.equal(whole, res) and torch.equal(whole.cpu(), _tall(up32))


def test_stacked_down_graph_replay_is_bit_identical():
    """One launch, no host synchronisation: a captured graph replays to the eager result, into the same buffers."""
    from sige_amd import hip

    C, hp, W = 36, 16, 24
    x, s, t = _inputs(E, C, hp, W, seed=7)
    xg, sg, tg = _cl(_tall(x).cuda()), s.cuda(), t.cuda()
    ho, wo = hp // 2, W // 2
    idx = _concat(_stacked_lists(ho, wo, seed=3)["subset"], ho).cuda()
    hip.set_edit_batch(E)
    try:
        res_e = _nan_res(1, C, E * ho, wo)
        tiles_e = hip.resample_tiles(xg, "down", idx, BLOCK, sg, tg, res=res_e, **KW)
        torch.cuda.synchronize()
        res_g = _nan_res(1, C, E * ho, wo)
        before = hip.launch_count()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tiles_g = hip.resample_tiles(xg, "down", idx, BLOCK, sg, tg, res=res_g, **KW)
        assert hip.launch_count() - before == 1
    finally:
        hip.set_edit_batch(1)
    for _ in range(2):
        tiles_g.fill_(float("nan"))
        res_g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tiles_g, tiles_e)
        assert torch.equal(res_g.view(torch.int32), res_e.view(torch.int32))
