"""Change regions of a dense level behind a tiled Downsample, without a GPU.

The 32x32 down level of DDPM-256 (`down[3]`: two dense ResBlocks, no attention, no shortcut) reads the persistent output of the
tiled `down[2].downsample`, which equals the original's cache outside S0 = the 2x2 output tiles its Scatter writes.  On the cached
GroupNorm affines every conv of the level is local, so its k-th 3x3 conv can differ from the original's values only on S_k = S0
grown k times by one pixel (clamped to the image).

  * sige_amd.utils.change_tiles -- the host restatement of the device kernel -- against a brute-force pixel walk, for the nine
    masks of tests/mask_zoo.py, bench.py's squares (counts pinned), empty lists, borders and geometries that do not fit;
  * the premise itself on the CPU oracle, on the smallest network with such a level: in a sparse forward the outputs of the
    level's four convs equal the full pass's outside S_k, and differ from them inside."""
import pytest
import torch

from tests import mask_zoo, util
from tests.change_regions_common import brute, downsample_indices, same, small_cfg, small_inputs, small_masks

DEPTH = 4


def _host(idx, depth=DEPTH, res=(32, 32)):
    from sige_amd.utils import change_tiles

    return change_tiles(idx, (5, 5), (2, 2), (0, 0), (2, 2), res, (4, 4), (1, 1), depth)


@pytest.mark.parametrize("name", list(mask_zoo.COUNTS))
def test_host_lists_equal_the_pixel_walk_on_the_zoo(name):
    idx = downsample_indices(mask_zoo.zoo()[name])
    _, mains, flats = brute(idx, 2, 0, 2, (32, 32), 4, 1, DEPTH)
    got_main, got_flat = _host(idx)
    assert same(got_main, mains) and same(got_flat, flats), name
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


@pytest.mark.parametrize("ratio,tiles,cells", [(0.012, 14, (12, 12, 20, 20)), (0.05, 34, (20, 20, 30, 30)),
                                               (0.15, 71, (30, 30, 49, 49))])
def test_counts_of_the_benchmark_squares(ratio, tiles, cells):
    """bench.py's masks: active tiles of down[2].downsample and the cells of 64 that S_1 .. S_4 touch."""
    import bench

    idx = downsample_indices(bench.edit_mask(ratio))
    _, mains, _ = brute(idx, 2, 0, 2, (32, 32), 4, 1, DEPTH)
    got_main, _ = _host(idx)
    assert same(got_main, mains)
    assert (idx.shape[0], tuple(int(m.shape[0]) for m in mains)) == (tiles, cells)


def test_borders_empty_lists_and_geometries_that_do_not_fit():
    from sige_amd.utils import change_tiles

    zoo = mask_zoo.zoo()
    sets, _, flats = brute(downsample_indices(zoo["corners"]), 2, 0, 2, (32, 32), 4, 1, DEPTH)
    assert {(0, 0), (0, 31), (31, 0), (31, 31)} <= sets[0]
    assert all(0 <= y < 32 and 0 <= x < 32 for s in sets for y, x in s)
    # one pixel in the last corner: nothing near row 0 / column 0 at any depth (a wrapped index would land there)
    _, got_flat = _host(downsample_indices(zoo["last_pixel"]))
    assert all(int(f.min()) >= 16 for f in got_flat)
    # an odd-sized level (the last cell row / column is partial, the last tiles hang over the border), both geometries of a tile
    idx = torch.tensor([[0, 0], [0, 24], [12, 8], [24, 0], [24, 24]], dtype=torch.int32)
    for res in ((14, 14), (13, 15)):
        _, mains, flats = brute(idx, 2, 0, 2, res, 4, 1, 5)
        got_main, got_flat = change_tiles(idx, 5, 2, 0, 2, res, 4, 1, 5)
        assert same(got_main, mains) and same(got_flat, flats), res
    idx1 = torch.tensor([[-1, -1], [3, 7], [11, 11]], dtype=torch.int32)  # (a stride-1 producer: 6x6 blocks, offset 1, 4x4 tiles)
    _, mains, flats = brute(idx1, 1, 1, 4, (14, 14), 4, 1, 3)
    got_main, got_flat = change_tiles(idx1, 6, 1, 1, 4, (14, 14), 4, 1, 3)
    assert same(got_main, mains) and same(got_flat, flats)
    assert all(t.shape == (0, 2) and t.dtype == torch.int32 for lists in change_tiles(idx[:0], 5, 2, 0, 2, (14, 14), 4, 1, 3) for t in lists)
    with pytest.raises(ValueError):
        change_tiles(idx, 5, 2, 0, 4, (14, 14), 4, 1, 1)  # (four outputs at stride 2 need a 7-wide block)
    with pytest.raises(ValueError):
        change_tiles(idx, 5, 2, 0, 2, (14, 14), 4, 1, 0)


# ---- the premise, on the CPU oracle ---------------------------------------------------------------------------------------------
_net = {}


def _small_net():
    """The small network on the CPU after ONE full pass (shared by the cases below) with the outputs of the dense level's four
    convs in that pass: [block[0].conv1, block[0], block[1].conv1, block[1]]."""
    if not _net:
        from sige_amd import runtime
        from sige_amd.workloads import ddpm_unet
        from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

        torch.manual_seed(0)
        model = DDPMSparseUNet(small_cfg()).eval()
        x0, noise = small_inputs()
        stage = model.down[2]
        conv1s = [b.conv1 for b in stage.block]
        seen = {}
        real = ddpm_unet.full_conv2d

        def spy(conv, *args, **kwargs):  # (the full pass calls nn.Conv2d.forward directly: no module hook fires)
            out = real(conv, *args, **kwargs)
            if any(conv is c for c in conv1s):
                seen[id(conv)] = out.clone()
            return out

        hooks = [b.register_forward_hook(lambda m, i, o: seen.__setitem__(id(m), o.clone())) for b in stage.block]
        backend, _ = util.cpu_backend()
        runtime.register_backend("cpu", backend)
        ddpm_unet.full_conv2d = spy
        try:
            with torch.no_grad():
                model.set_mode("full")
                model(x0, torch.zeros(1))
        finally:
            ddpm_unet.full_conv2d = real
            runtime.unregister_backend("cpu")
            for h in hooks:
                h.remove()
        assert [(lvl, len(s.block)) for lvl, s, _ in model._change_stages()] == [(2, 2)]
        original = [seen[id(m)] for b in stage.block for m in (b.conv1, b)]
        _net.update(model=model, x0=x0, noise=noise, original=original)
    return _net


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_convs_equal_the_original_outside_their_change_region(name):
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask

    net = _small_net()
    model, x0, noise, original = net["model"], net["x0"], net["noise"], net["original"]
    mask = small_masks()[name]
    stage = model.down[2]
    seen = {}
    hooks = [m.register_forward_hook(lambda m, i, o: seen.__setitem__(id(m), o.clone())) for b in stage.block for m in (b.conv1, b)]
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            model.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
            model.set_mode("sparse")
            model(x0 + noise * mask, torch.zeros(1))
    finally:
        runtime.unregister_backend("cpu")
        for h in hooks:
            h.remove()
    g = model.down[1].downsample.gather
    assert (tuple(g.input_res), tuple(g.block_size), tuple(g.model_stride), tuple(g.out_tile), tuple(g.offset)) == \
        ((32, 32), (5, 5), (2, 2), (2, 2), (0, 0))
    sets, _, _ = brute(g.active_indices, 2, 0, 2, (16, 16), 4, 1, DEPTH)
    got = [seen[id(m)] for b in stage.block for m in (b.conv1, b)]
    for k, (new, ref) in enumerate(zip(got, original)):
        assert tuple(new.shape) == tuple(ref.shape) == (1, 256, 16, 16)
        inside = torch.zeros(16, 16, dtype=torch.bool)
        for y, x in sets[k]:
            inside[y, x] = True
        bound = 2e-5 * (1.0 + float(ref.abs().max()))  # (the project's fp32-chain bound)
        diff = (new - ref).abs().amax(dim=(0, 1))
        out_err = float(diff[~inside].max()) if bool((~inside).any()) else 0.0
        in_err = float(diff[inside].max())
        print("change_regions %s conv %d: |S| = %d, outside %.3e, inside %.3e, bound %.3e" % (name, k + 1, len(sets[k]), out_err, in_err, bound))
        assert out_err <= bound, (name, k, out_err, bound)
        assert in_err > bound, (name, k, in_err, bound)
    if name == "large":
        assert len(sets[-1]) == 256
    else:
        assert len(sets[0]) < len(sets[-1]) < 256
