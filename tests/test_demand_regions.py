"""Demand regions of a dense level in front of a tiled Upsample, without a GPU.

The 32x32 up level of DDPM-256 (`up[3]`: three dense ResBlocks, no attention) feeds only `up[3].upsample`, whose gather reads the
half-resolution tensor through 6x6 windows of its x2 upsampling.  N0 = the 32x32 pixels under those windows; the conv k 3x3
layers before the level's output is needed on N0 (+) k (k one-pixel 3x3 dilations, clamped to the image).

  * sige_amd.utils.demand_tiles -- the host restatement of the device kernel -- against a brute-force pixel walk, for the nine
    masks of tests/mask_zoo.py, bench.py's squares (counts pinned) and a hand-made list over an odd-sized level;
  * the premise itself on the CPU oracle: garbling the three block outputs outside N0 (+) 4, 2, 0 does not move one bit of the
    network's output."""
import pytest
import torch

from tests import mask_zoo, util

DEPTH = 6


def _level_indices(mask, res=64):
    """The index list of a 3x3 gather (6x6 blocks, stride 4, offset 1) over the `res` level of bench.py's mask recipe."""
    from oracle import oracle

    pyramid = oracle.downsample_mask(oracle.dilate_mask(mask, 5), 8)
    return oracle.reduce_mask(pyramid[(res, res)], (6, 6), (4, 4), (1, 1))


def _brute(idx, block, in_res, up, prod_res, tile, pad, depth):
    """Pixel by pixel: (need sets per depth as sets of (y, x), main lists, flat lists)."""
    hp, wp = prod_res
    need = set()
    for y0, x0 in idx.tolist():
        for dy in range(block):
            for dx in range(block):
                y, x = y0 + dy, x0 + dx
                if 0 <= y < in_res[0] and 0 <= x < in_res[1]:
                    need.add((y >> up, x >> up))
    needs, mains, flats = [], [], []
    for k in range(depth):
        needs.append(set(need))
        cells = sorted({(y // tile, x // tile) for y, x in need})
        flats.append(torch.tensor([(cy * tile, cx * tile) for cy, cx in cells], dtype=torch.int32).reshape(-1, 2))
        mains.append(torch.tensor([(cy * tile - pad, cx * tile - pad) for cy, cx in cells], dtype=torch.int32).reshape(-1, 2))
        grown = set()
        for y, x in need:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < hp and 0 <= x + dx < wp:
                        grown.add((y + dy, x + dx))
        need = grown
    return needs, mains, flats


def _host(idx, depth=DEPTH):
    from sige_amd.utils import demand_tiles

    return demand_tiles(idx, (6, 6), (64, 64), True, (32, 32), (4, 4), (1, 1), depth)


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == torch.int32 and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(mask_zoo.COUNTS))
def test_host_lists_equal_the_pixel_walk_on_the_zoo(name):
    idx = _level_indices(mask_zoo.zoo()[name])
    _, mains, flats = _brute(idx, 6, (64, 64), 1, (32, 32), 4, 1, DEPTH)
    got_main, got_flat = _host(idx)
    assert _same(got_main, mains) and _same(got_flat, flats), name
    for k in range(DEPTH):  # (reduce_mask form: row-major sorted, inside the grid, one geometry = the other shifted by the offset)
        flat = got_flat[k]
        assert int(flat.min()) >= 0 and int(flat.max()) <= 28 and bool((flat % 4 == 0).all())
        keys = (flat[:, 0].long() * 64 + flat[:, 1].long()).tolist()
        assert keys == sorted(set(keys))
        assert torch.equal(got_main[k], flat - 1)
        if k:
            assert set(map(tuple, got_flat[k - 1].tolist())) <= set(map(tuple, flat.tolist()))
    if name == "full_grid":
        every = torch.stack(torch.meshgrid(torch.arange(8) * 4, torch.arange(8) * 4, indexing="ij"), -1).reshape(-1, 2).int()
        assert all(torch.equal(f, every) for f in got_flat)


@pytest.mark.parametrize("ratio,cells,n0", [(0.012, (12, 12, 24, 24, 30, 30), (18, 112, (9, 18), (7, 18))),
                                            (0.05, (20, 20, 30, 30, 42, 42), None)])
def test_counts_of_the_benchmark_squares(ratio, cells, n0):
    """bench.py's masks: 132 of 384 cells at a 1.2 % edit, 184 at 5 % (last conv first)."""
    import bench

    idx = _level_indices(bench.edit_mask(ratio))
    needs, mains, _ = _brute(idx, 6, (64, 64), 1, (32, 32), 4, 1, DEPTH)
    got_main, _ = _host(idx)
    assert _same(got_main, mains)
    assert tuple(int(m.shape[0]) for m in got_main) == cells
    if n0 is not None:
        tiles, pixels, rows, cols = n0
        ys, xs = [p[0] for p in needs[0]], [p[1] for p in needs[0]]
        assert (idx.shape[0], len(needs[0]), (min(ys), max(ys)), (min(xs), max(xs))) == (tiles, pixels, rows, cols)


def test_borders_are_clamped_and_do_not_wrap():
    """Need sets that touch row 0, column 0, row 31 and column 31 (the corners and frame masks), one that touches the last corner
    only, and an odd-sized level (14 x 14: the last cell row / column is partial) under a list with windows over every border."""
    zoo = mask_zoo.zoo()
    needs, _, flats = _brute(_level_indices(zoo["corners"]), 6, (64, 64), 1, (32, 32), 4, 1, DEPTH)
    assert {(0, 0), (0, 31), (31, 0), (31, 31)} <= needs[0]
    assert all(0 <= y < 32 and 0 <= x < 32 for n in needs for y, x in n)
    needs, _, flats = _brute(_level_indices(zoo["last_pixel"]), 6, (64, 64), 1, (32, 32), 4, 1, DEPTH)
    got_main, got_flat = _host(_level_indices(zoo["last_pixel"]))
    assert _same(got_flat, flats)
    # one pixel in the last corner: nothing near row 0 / column 0 at any depth (a wrapped index would land there)
    assert all(int(f.min()) >= 16 for f in got_flat) and (31, 31) in needs[0]
    from sige_amd.utils import demand_tiles

    idx = torch.tensor([[-1, -1], [-1, 23], [11, 7], [23, -1], [23, 23]], dtype=torch.int32)
    for up, in_res, prod in ((1, (28, 28), (14, 14)), (0, (28, 28), (28, 28)), (1, (26, 30), (13, 15))):
        _, mains, flats = _brute(idx, 6, in_res, up, prod, 4, 1, 5)
        got_main, got_flat = demand_tiles(idx, 6, in_res, bool(up), prod, 4, 1, 5)
        assert _same(got_main, mains) and _same(got_flat, flats), (up, in_res, prod)
    assert all(t.shape == (0, 2) for lists in demand_tiles(idx[:0], 6, (28, 28), True, (14, 14), 4, 1, 3) for t in lists)
    with pytest.raises(ValueError):
        demand_tiles(idx, 6, (28, 28), True, (15, 14), 4, 1, 1)


# ---- the premise, on the CPU oracle ---------------------------------------------------------------------------------------------
_net = {}


def _cpu_net():
    """bench.py's network on the CPU after ONE full pass (shared by the cases below), with the oracle as native backend."""
    if not _net:
        import bench
        from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

        torch.manual_seed(0)
        model = DDPMSparseUNet(DDPMConfig()).eval()
        x0, noise = bench.make_inputs()
        _net.update(model=model, x0=x0, noise=noise, t=torch.zeros(1), full=False)
    return _net


def _dead_masks():
    import bench

    zoo = mask_zoo.zoo()
    return {"square_1p2": bench.edit_mask(0.012), "frame": zoo["frame"], "corners": zoo["corners"], "last_pixel": zoo["last_pixel"]}


@pytest.mark.parametrize("name", ["square_1p2", "frame", "corners", "last_pixel"])
def test_outputs_outside_the_need_sets_are_dead(name):
    """One sparse forward as it is and one with the outputs of up[3].block[0], [1], [2] overwritten with 1e4 outside N0 (+) 4,
    N0 (+) 2 and N0: the network's output is the same bits."""
    from oracle import oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask

    net = _cpu_net()
    model, x0, noise, t = net["model"], net["x0"], net["noise"], net["t"]
    mask = _dead_masks()[name]
    n_thr = min(32, torch.get_num_threads())
    oracle.set_num_threads(n_thr)
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    hooks = []
    try:
        with torch.no_grad():
            if not net["full"]:
                model.set_mode("full")
                model(x0, t)
                net["full"] = True
            model.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
            model.set_mode("sparse")
            x1 = x0 + noise * mask
            clean = model(x1, t).clone()
            g = model.up[3].upsample.gather
            assert tuple(g.input_res) == (64, 64) and tuple(g.block_size) == (6, 6) and tuple(g.offset) == (1, 1)
            needs, _, _ = _brute(g.active_indices, 6, (64, 64), 1, (32, 32), 4, 1, DEPTH)
            garbled = []
            for i, block in enumerate(model.up[3].block):
                keep = torch.zeros(32, 32, dtype=torch.bool)
                for y, x in needs[2 * (2 - i)]:
                    keep[y, x] = True
                garbled.append(int((~keep).sum()))

                def hook(_m, _inp, out, keep=keep):
                    assert tuple(out.shape[2:]) == (32, 32)
                    return torch.where(keep, out, torch.full_like(out, 1e4))

                hooks.append(block.register_forward_hook(hook))
            dirty = model(x1, t)
            assert sum(garbled) > 0 or name == "frame", garbled  # (something was overwritten, or the set is everything)
            assert torch.equal(dirty, clean), (name, float((dirty - clean).abs().max()), garbled)
    finally:
        for h in hooks:
            h.remove()
        runtime.unregister_backend("cpu")
