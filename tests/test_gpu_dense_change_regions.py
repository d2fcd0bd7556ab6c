"""On the MI355X: a dense down level behind a tiled Downsample computed on the cells an edit can change (DESIGN.md 5.14;
DDPMSparseUNet.DENSE_ON_CHANGE).  The device lists against the host restatement; the smallest network with such a level against the
CPU oracle with the flag on and off, walking through masks, after a second full pass, after a cache rewritten in place and under
NaN-poisoned allocations; graph replay, launch plan, launch count and the guards."""
import pytest
import torch

from tests import mask_zoo, util
from tests.change_regions_common import small_cfg, small_inputs, small_masks

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
    err = util.record_margin("dense_change_regions", what, _err(got, want), tol)
    print("dense_change_regions %-64s %.3e" % (what, err), flush=True)
    assert err <= tol, (what, err)


class _flags:
    """Class flags of DDPMSparseUNet for the duration of a block (restored whatever happens)."""

    def __init__(self, **flags):
        self.flags = flags

    def __enter__(self):
        from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

        self.keep = {k: getattr(DDPMSparseUNet, k) for k in self.flags}
        for k, v in self.flags.items():
            setattr(DDPMSparseUNet, k, v)

    def __exit__(self, *exc):
        from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

        for k, v in self.keep.items():
            setattr(DDPMSparseUNet, k, v)
        return False


# ---- a. the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mask_zoo.COUNTS))
def test_device_lists_equal_the_host_restatement(hip, name):
    """The level-64 list of DDPM-256's down[2].downsample (5x5 blocks, stride 2, 2x2 tiles) and the four lists of the 32x32 level
    behind it, from one reduce_mask_batch call as set_masks makes it."""
    from oracle import oracle
    from sige_amd.utils import change_tiles

    mask = mask_zoo.zoo()[name]
    level = _build_masks(mask.to(DEV))[(64, 64)]
    lists, demands, regions = hip.reduce_mask_batch([(level, (5, 5), (4, 4), (0, 0))], [],
                                                    [(0, (2, 2), (2, 2), (0, 0), (32, 32), (4, 4), (1, 1), 4)])
    idx = oracle.reduce_mask(oracle.downsample_mask(oracle.dilate_mask(mask, 5), 8)[(64, 64)], (5, 5), (4, 4), (0, 0))
    assert demands == [] and torch.equal(lists[0].cpu(), idx)
    main, flat = change_tiles(idx, (5, 5), (2, 2), (0, 0), (2, 2), (32, 32), (4, 4), (1, 1), 4)
    region = regions[0]
    assert isinstance(region, hip.ChangeTiles) and region.cells == 64 and len(region.main) == len(region.flat) == 4
    for k in range(4):
        assert region.main[k].dtype == torch.int32 and torch.equal(region.main[k].cpu(), main[k]), (name, k)
        assert torch.equal(region.flat[k].cpu(), flat[k]), (name, k)
    assert region.counts == [int(m.shape[0]) for m in main]
    if name == "full_grid":
        assert region.counts == [64] * 4


# ---- b. the smallest network with a dense, attention-free down level behind a tiled Downsample ------------------------------------
def _new_model(x0):
    """The small network on the GPU (seed-0 weights) after its full pass on `x0`."""
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(small_cfg()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        model(_cl(x0), torch.zeros(1, device=DEV))
    return model


@pytest.fixture(scope="module")
def small(hip):
    """(GPU model after its full pass on image A, x0 of A and B, noise, t, {(image, mask name): CPU-oracle sparse output})."""
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    xa, noise = small_inputs()
    xb = xa.flip(-1).contiguous() * 0.75 + 0.1  # (a second original)
    torch.manual_seed(0)
    cpu = DDPMSparseUNet(small_cfg()).eval()
    wants = {}
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            for img, x0, names in (("A", xa, ("interior", "corner", "large")), ("B", xb, ("interior",))):
                cpu.set_mode("full")
                cpu(x0, torch.zeros(1))
                for name in names:
                    m = small_masks()[name]
                    cpu.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                    cpu.set_mode("sparse")
                    wants[(img, name)] = cpu(x0 + noise * m, torch.zeros(1)).clone()
    finally:
        runtime.unregister_backend("cpu")
    model = _new_model(xa)
    assert model.DENSE_ON_CHANGE and [lvl for lvl, _, _ in model._change_stages()] == [2]
    return model, {"A": _cl(xa), "B": _cl(xb)}, _cl(noise), torch.zeros(1, device=DEV), wants


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


class _StageLaunches:
    """Spy on hip.gather_conv_cl: the tile counts of the launches that write a persistent change-region buffer of `stage`."""

    def __init__(self, hip, stage):
        self.hip, self.stage, self.counts = hip, stage, []

    def __enter__(self):
        self.real = self.hip.gather_conv_cl
        bufs = {b.data_ptr() for blk in self.stage.block for c in (blk.conv1, blk.conv2, getattr(blk, "nin_shortcut", None)) if c is not None
                for n, b in c.__dict__.get("_sige_demand_bufs", {}).items() if isinstance(n, tuple) and n[0] == "out"}

        def spy(*args, **kwargs):
            out = kwargs.get("out")
            if out is not None and out.data_ptr() in bufs:
                self.counts.append(int(args[3].shape[0]))
            return self.real(*args, **kwargs)

        self.hip.gather_conv_cl = spy
        return self

    def __exit__(self, *exc):
        self.hip.gather_conv_cl = self.real
        return False


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_small_network_flag_on_and_off_vs_oracle(hip, small, name):
    model, x0s, noise, t, wants = small
    mask = small_masks()[name]
    outs = {}
    with torch.no_grad():
        for tag, flags in (("on", {}), ("off", dict(DENSE_ON_CHANGE=False)), ("on, demand off", dict(DENSE_ON_DEMAND=False))):
            with _flags(**flags):
                x1, outs[tag] = _sparse(model, x0s["A"], noise, t, mask)
                if tag == "off":
                    assert not model._change_lists
                else:
                    region = model._change_lists["down.2"]
                    counts = region.counts
                    assert region.cells == 16 and len(counts) == 4
                    if tag == "on" and name != "large":  # (the fourth forward is a steady one: each conv on its own list)
                        with _StageLaunches(hip, model.down[2]) as spy:
                            again = model(x1, t)
                        # (shortcut and conv2 of block 0 on S_2, its conv1 on S_1, block 1 on S_3 and S_4; a list that holds
                        #  every cell takes the all-tiles call into a fresh tensor)
                        want = [c for c in (counts[1], counts[0], counts[1], counts[2], counts[3]) if c < region.cells]
                        assert spy.counts == want, (spy.counts, counts)
                        assert torch.equal(again, outs[tag])
                _close("small %s flag %s vs oracle" % (name, tag), outs[tag], wants[("A", name)])
    _close("small %s flag on vs off" % name, outs["on"], outs["off"], util.SELF_ATOL)
    _close("small %s flag on, demand off vs off" % name, outs["on, demand off"], outs["off"], util.SELF_ATOL)
    if name == "large":  # every list holds every cell: the launches of the flag-off forward exactly
        assert counts == [16] * 4 and torch.equal(outs["on"], outs["off"])
    else:            # proper sublists, growing with k
        assert 0 < counts[0] < 16 and counts == sorted(counts)


def test_small_network_mask_walk_vs_oracle(hip, small):
    """corner -> interior -> large -> corner on one model, no full pass in between: what the previous mask left in the level's
    persistent buffers must not survive -- after one forward under the new mask and after three."""
    model, x0s, noise, t, wants = small
    with torch.no_grad():
        for step, name in enumerate(["corner", "interior", "large", "corner"]):
            mask = small_masks()[name]
            x1, first = _sparse(model, x0s["A"], noise, t, mask, forwards=1)
            _close("walk %d %s first forward" % (step, name), first, wants[("A", name)])
            model(x1, t)
            third = model(x1, t).clone()
            _close("walk %d %s third forward" % (step, name), third, wants[("A", name)])


def test_small_network_second_original(hip, small):
    """A new full pass on another image under the same mask: the level's buffers follow the new original."""
    model, x0s, noise, t, wants = small
    mask = small_masks()["interior"]
    try:
        with torch.no_grad():
            _, out_a = _sparse(model, x0s["A"], noise, t, mask)
            _close("second original: A", out_a, wants[("A", "interior")])
            with util.native_full_pass():
                model.set_mode("full")
                model(x0s["B"], t)
            model.set_mode("sparse")
            x1 = _cl(x0s["B"] + noise * mask.to(DEV))
            first = model(x1, t).clone()
            _close("second original: B first forward", first, wants[("B", "interior")])
            model(x1, t)
            _close("second original: B third forward", model(x1, t), wants[("B", "interior")])
    finally:
        with util.native_full_pass(), torch.no_grad():  # (the module-scoped model goes back to image A)
            model.set_mode("full")
            model(x0s["A"], t)


def test_small_network_cache_rewritten_in_place(hip, small):
    """full(A) -> sparse -> pack_caches -> sparse, graph captured -> flat <- cache of B -> refresh_derived -> sparse, eagerly and by
    replaying the graph captured under A: both give B's result (the level's buffers are rebuilt at their addresses)."""
    from sige_amd import parallel

    _, x0s, noise, t, wants = small
    mask = small_masks()["interior"]
    with torch.no_grad():
        flat_b = parallel.pack_caches(_new_model(x0s["B"])).clone()  # (what another rank would send)
        net = _new_model(x0s["A"])
        xs, _ = _sparse(net, x0s["A"], noise, t, mask, forwards=1)
        xs = xs.clone()
        flat = parallel.pack_caches(net)
        net(xs, t)
        net(xs, t)
        got_a = net(xs, t).clone()
        _close("rewritten in place: A after pack", got_a, wants[("A", "interior")])
        g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            net(xs, t)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                captured = net(xs, t)
        torch.cuda.current_stream().wait_stream(st)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, got_a)
        assert net._change_state, "the captured forward was not a steady one"

        flat.copy_(flat_b)  # (the broadcast)
        parallel.refresh_derived(net)
        xs.copy_(x0s["B"] + noise * mask.to(DEV))
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        _close("rewritten in place: B by the graph captured under A", captured, wants[("B", "interior")])
        net(xs, t)
        _close("rewritten in place: B eager", net(xs, t), wants[("B", "interior")])


def test_small_network_poisoned_allocations(hip, small):
    """Every uninitialised allocation of the sparse forwards -- the level's first, every-cell forward included -- filled with NaN:
    the same bits."""
    model, x0s, noise, t, wants = small
    mask = small_masks()["interior"]
    with torch.no_grad():
        _, want = _sparse(model, x0s["A"], noise, t, mask)
        net = _new_model(x0s["A"])
        with util.poisoned(NAN) as p:
            x1, got = _sparse(net, x0s["A"], noise, t, mask)
            again = net(x1, t).clone()
        util.assert_finite(got, "poisoned forwards")
        assert p.n > 0 and torch.equal(got, want) and torch.equal(again, want)


# ---- c. graph replay, launch plan, launch count, guards -------------------------------------------------------------------------
def test_small_network_graph_replay_equals_eager(hip, small):
    import bench

    model, x0s, noise, t, _ = small
    with torch.no_grad():
        x1, want = _sparse(model, x0s["A"], noise, t, small_masks()["interior"])
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), _err(out, want)
        del g, out


def test_small_network_launch_count_is_unchanged(hip, small):
    model, x0s, noise, t, _ = small
    counts = {}
    with torch.no_grad():
        for flag in (True, False):
            with _flags(DENSE_ON_CHANGE=flag):
                x1, _ = _sparse(model, x0s["A"], noise, t, small_masks()["interior"])
                n0 = hip.launch_count()
                model(x1, t)
                counts[flag] = hip.launch_count() - n0
    assert counts[True] == counts[False] > 0, counts


def test_small_network_guards(hip, small):
    """Stacked edits (E = 2) and fp16 operands: the flag changes nothing."""
    from sige_amd import stacked

    model, x0s, noise, t, _ = small
    masks = [small_masks()["interior"].to(DEV), small_masks()["corner"].to(DEV)]
    xe = _cl(torch.cat([x0s["A"] + noise * m for m in masks], 0))
    outs = {}
    with torch.no_grad():
        for flag in (True, False):
            with _flags(DENSE_ON_CHANGE=flag):
                stacked.stack_caches(model, 2)
                try:
                    stacked.set_masks(model, [_build_masks(m) for m in masks])
                    model.set_mode("sparse")
                    with stacked.edit_batch(model, 2):
                        for _ in range(3):
                            out = model(xe, t)
                    outs[("stacked", flag)] = out.clone()
                    assert not getattr(model, "_change_lists", {})
                finally:
                    stacked.unstack_caches(model)
                model.set_compute_dtype("f16", keep=())
                try:
                    _, outs[("f16", flag)] = _sparse(model, x0s["A"], noise, t, small_masks()["interior"])
                finally:
                    model.set_compute_dtype("f32")
    assert torch.equal(outs[("stacked", True)], outs[("stacked", False)])
    assert torch.equal(outs[("f16", True)], outs[("f16", False)])
    util.assert_finite(outs[("f16", True)], "f16 forward")


def test_ddpm_launch_plan_equals_module_forward(hip):
    """DDPM-256: a launch plan recorded at the 1.2 % square and bound to three further masks gives the bits of the module forward;
    bind_mask replays, behind the restore of the Scatter outputs, the every-cell run of down[3]."""
    import bench
    from sige_amd.plan import LaunchPlan
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0, noise = (_cl(v) for v in bench.make_inputs())
    t = torch.zeros(1, device=DEV)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        model(x0, t)
    assert [lvl for lvl, _, _ in model._change_stages()] == [3]
    zoo = mask_zoo.zoo()
    m0 = bench.edit_mask(0.012).to(DEV)
    xs = (x0 + noise * m0).clone()
    with torch.no_grad():
        plan = LaunchPlan(model)
        plan.record(m0, _build_masks, lambda: model(xs, t))
        assert model._change_lists["down.3"].counts == [12, 12, 20, 20]
        assert not plan.shape_bound and plan.unbound_counts == 0
        for name, mask in (("square_5", bench.edit_mask(0.05)), ("full_grid", zoo["full_grid"]), ("corners", zoo["corners"])):
            mask = mask.to(DEV)
            xs.copy_(x0 + noise * mask)
            plan.bind_mask(mask)
            got = plan.run().clone()
            if name == "square_5":  # (bind_mask adopts: the model holds the plan's lists under the new mask, until its next set_masks)
                assert model._change_lists["down.3"].counts == [20, 20, 30, 30]
            model.set_masks(_build_masks(mask))
            model.set_mode("sparse")
            for _ in range(3):
                want = model(xs, t)
            assert torch.equal(got, want), (name, _err(got, want))
        torch.cuda.synchronize()
        del plan
