"""On the MI355X: a dense up level in front of a tiled Upsample computed on its demand regions only (DESIGN.md 5.11;
DDPMSparseUNet.DENSE_ON_DEMAND).  The device lists against the host restatement; a small network and DDPM-256 against the CPU
oracle with the flag on and off; NaN / 1e30 in everything the level leaves unwritten; one model walking through masks of very
different footprints; graph replay, launch plan and launch count."""
import pytest
import torch

from tests import mask_zoo, util

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


def _err(got, want):
    return float((got.detach().float().cpu() - want.detach().float().cpu()).abs().max())


def _close(what, got, want, tol=util.CONV_ATOL):
    err = util.record_margin("dense_on_demand", what, _err(got, want), tol)
    print("dense_on_demand %-64s %.3e" % (what, err), flush=True)
    assert err <= tol, (what, err)


@pytest.fixture(scope="module")
def net(hip):
    """bench.py's network (seed-0 weights, channels-last, in-place scatter) after its full pass on the library's exact-fp32 kernels."""
    import bench
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0, noise = bench.make_inputs()
    t = torch.zeros(1, device=DEV)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        model(_cl(x0), t)
    assert model.DENSE_ON_DEMAND and [n for n, _ in model._demand_stages()] == ["up.3"]
    return model, _cl(x0), _cl(noise), t


def _sparse(model, x0, noise, t, mask, forwards=3):
    """set_masks + `forwards` sparse forwards under `mask` (CPU bool); returns (x1, the last output)."""
    mask = mask.to(DEV)
    x1 = _cl(x0 + noise * mask)
    model.set_masks(_build_masks(mask))
    model.set_mode("sparse")
    out = None
    for _ in range(forwards):
        out = model(x1, t)
    return x1, out.clone()


# ---- a. the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mask_zoo.COUNTS))
def test_device_lists_equal_the_host_restatement(hip, net, name):
    from oracle import oracle
    from sige_amd.utils import demand_tiles

    model = net[0]
    mask = mask_zoo.zoo()[name]
    model.set_masks(_build_masks(mask.to(DEV)))
    region = model._demand_lists["up.3"]
    g = model.up[3].upsample.gather
    level = oracle.downsample_mask(oracle.dilate_mask(mask, 5), 8)[(64, 64)]
    idx = oracle.reduce_mask(level, g.block_size, g.block_stride, g.offset)
    assert torch.equal(g.active_indices.cpu(), idx)
    main, flat = demand_tiles(idx, g.block_size, (64, 64), True, (32, 32), (4, 4), (1, 1), 6)
    assert region.cells == 64 and len(region.main) == len(region.flat) == 6
    for k in range(6):
        assert region.main[k].dtype == torch.int32 and torch.equal(region.main[k].cpu(), main[k]), (name, k)
        assert torch.equal(region.flat[k].cpu(), flat[k]), (name, k)
    assert region.counts == [int(m.shape[0]) for m in main]
    if name == "full_grid":
        assert region.counts == [64] * 6


# ---- b. the smallest network with a dense, attention-free up level under a tiled Upsample -------------------------------------------
def _small_cfg():
    from sige_amd.workloads.ddpm_unet import DDPMConfig

    # levels 64 / 32 (tiled) and 16 (dense: 16 cells, two ResBlocks on the way up); 128 channels: the two-pointer cat of the 1x1
    # shortcuts splits on the 128-channel chunks of the channels-last kernels
    return DDPMConfig(ch=128, ch_mult=(1, 1, 2), num_res_blocks=1, attn_resolutions=(), resolution=64, sparse_threshold=32)


def _small_masks():
    interior = torch.zeros(64, 64, dtype=torch.bool)
    interior[29:33, 30:35] = True
    corner = torch.zeros(64, 64, dtype=torch.bool)
    corner[:3, :4] = True
    large = torch.zeros(64, 64, dtype=torch.bool)
    large[3:61, 2:62] = True
    return {"interior": interior, "corner": corner, "large": large}


@pytest.fixture(scope="module")
def small(hip):
    """(GPU model after its full pass, x0, noise, t, {mask name: CPU-oracle sparse output})."""
    from oracle import oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    gen = torch.Generator().manual_seed(3)
    x0, noise = torch.randn(1, 3, 64, 64, generator=gen), torch.randn(1, 3, 64, 64, generator=gen)
    torch.manual_seed(0)
    cpu = DDPMSparseUNet(_small_cfg()).eval()
    wants = {}
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            cpu.set_mode("full")
            cpu(x0, torch.zeros(1))
            for name, m in _small_masks().items():
                cpu.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                cpu.set_mode("sparse")
                wants[name] = cpu(x0 + noise * m, torch.zeros(1)).clone()
    finally:
        runtime.unregister_backend("cpu")
    torch.manual_seed(0)
    model = DDPMSparseUNet(_small_cfg()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    t = torch.zeros(1, device=DEV)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        model(_cl(x0), t)
    assert [n for n, _ in model._demand_stages()] == ["up.2"]
    return model, _cl(x0), _cl(noise), t, wants


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_small_network_flag_on_and_off_vs_oracle(hip, small, name):
    model, x0, noise, t, wants = small
    mask = _small_masks()[name]
    outs = {}
    try:
        with torch.no_grad():
            for flag in (True, False):
                model.DENSE_ON_DEMAND = flag
                _, outs[flag] = _sparse(model, x0, noise, t, mask)
                if flag:
                    counts = model._demand_lists["up.2"].counts
                    assert model._demand_lists["up.2"].cells == 16 and len(counts) == 4
                else:
                    assert not model._demand_lists
                _close("small %s flag %s vs oracle" % (name, "on" if flag else "off"), outs[flag], wants[name])
    finally:
        del model.DENSE_ON_DEMAND
    _close("small %s flag on vs off" % name, outs[True], outs[False], util.SELF_ATOL)
    if name == "large":  # every list holds every cell: the launches of the flag-off forward exactly
        assert counts == [16] * 4 and torch.equal(outs[True], outs[False])
    else:            # proper sublists, growing with the depth
        assert 0 < counts[0] < 16 and counts == sorted(counts)


# ---- c. DDPM-256: what the level does not write is never read ---------------------------------------------------------------------
def _demand_buffers(model):
    """[(buffer, depth index of its list)]: every persistent output and twin of up[3]'s convs."""
    out = []
    blocks = model.up[3].block
    for i, b in enumerate(blocks):
        j2 = 2 * (len(blocks) - 1 - i)
        for conv, k in ((b.conv1, j2 + 1), (b.conv2, j2), (b.nin_shortcut, j2)):
            for buf in conv.__dict__.get("_sige_demand_bufs", {}).values():
                out.append((buf, k))
    return out


@pytest.mark.parametrize("fill", [NAN, 1e30], ids=["nan", "1e30"])
def test_ddpm_stale_buffers_are_unread(hip, net, fill):
    import bench

    model, x0, noise, t = net
    with torch.no_grad():
        x1, want = _sparse(model, x0, noise, t, bench.edit_mask(0.012))
        region = model._demand_lists["up.3"]
        assert region.counts == [12, 12, 24, 24, 30, 30]
        bufs = _demand_buffers(model)
        assert len(bufs) >= 9 + 2  # (three outputs per block, and the twins the next block's conv1 registered)
        for buf, k in bufs:
            inside = torch.zeros(32, 32, dtype=torch.bool, device=DEV)
            for y, x in region.flat[k].tolist():
                inside[y:y + 4, x:x + 4] = True
            buf.copy_(torch.where(inside, buf, torch.full_like(buf, fill)))
        got = model(x1, t).clone()
        util.assert_finite(got, "output after filling the stale cells")
        assert torch.equal(got, want)
        if fill != fill:  # (once: the same forward with every uninitialised allocation poisoned)
            with util.poisoned(NAN) as p:
                again = model(x1, t).clone()
            util.assert_finite(again, "poisoned forward")
            assert torch.equal(again, want) and p.n > 0
    full_c, (want_c,) = util.ddpm_cpu_oracle([bench.edit_mask(0.012)])
    _close("ddpm 1.2 %% square flag on, stale cells = %r" % fill, got, want_c)


# ---- d. one model through masks of very different footprints ------------------------------------------------------------------------
def test_ddpm_mask_walk_vs_oracle(hip, net):
    """small -> every tile -> small -> borders, no full pass in between: state of one mask must not survive into the next."""
    model, x0, noise, t = net
    zoo = mask_zoo.zoo()
    names = ["last_pixel", "full_grid", "corners", "frame"]
    _, wants = util.ddpm_cpu_oracle([zoo[n] for n in names])
    seen = []
    with torch.no_grad():
        for name, want in zip(names, wants):
            _, first = _sparse(model, x0, noise, t, zoo[name], forwards=1)
            _close("walk %s first forward" % name, first, want)
            x1 = _cl(x0 + noise * zoo[name].to(DEV))
            model(x1, t)
            third = model(x1, t).clone()
            _close("walk %s third forward" % name, third, want)
            seen.append(model._demand_lists["up.3"].counts)
    assert seen[1] == [64] * 6 and seen[0][0] < 8 and seen[2][0] < 32, seen


# ---- e. graph replay, launch plan, launch count ---------------------------------------------------------------------------------
def test_ddpm_graph_replay_equals_eager(hip, net):
    import bench

    model, x0, noise, t = net
    with torch.no_grad():
        x1, want = _sparse(model, x0, noise, t, bench.edit_mask(0.012))
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), _err(out, want)
        del g, out


def test_ddpm_launch_plan_equals_module_forward(hip, net):
    import bench
    from sige_amd.plan import LaunchPlan

    model, x0, noise, t = net
    zoo = mask_zoo.zoo()
    m0 = bench.edit_mask(0.012).to(DEV)
    xs = (x0 + noise * m0).clone()
    with torch.no_grad():
        plan = LaunchPlan(model)
        plan.record(m0, _build_masks, lambda: model(xs, t))
        assert not plan.shape_bound and plan.unbound_counts == 0
        for name, mask in (("square_5", bench.edit_mask(0.05)), ("full_grid", zoo["full_grid"]), ("corners", zoo["corners"])):
            mask = mask.to(DEV)
            xs.copy_(x0 + noise * mask)
            plan.bind_mask(mask)
            got = plan.run().clone()
            if name == "square_5":  # (bind_mask adopts: the model holds the plan's lists under the new mask, until its next set_masks)
                assert model._demand_lists["up.3"].counts == [20, 20, 30, 30, 42, 42]
            model.set_masks(_build_masks(mask))
            model.set_mode("sparse")
            for _ in range(3):
                want = model(xs, t)
            assert torch.equal(got, want), (name, _err(got, want))
        torch.cuda.synchronize()
        del plan


def test_ddpm_launch_count_is_unchanged(hip, net):
    import bench

    model, x0, noise, t = net
    counts = {}
    try:
        with torch.no_grad():
            for flag in (True, False):
                model.DENSE_ON_DEMAND = flag
                x1, _ = _sparse(model, x0, noise, t, bench.edit_mask(0.012))
                n0 = hip.launch_count()
                model(x1, t)
                counts[flag] = hip.launch_count() - n0
    finally:
        del model.DENSE_ON_DEMAND
    assert counts[True] == counts[False] > 0, counts
