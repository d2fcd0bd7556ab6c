"""On the MI355X: the sparse forward of the DDPM-256 U-Net against the CPU oracle under masks that are NOT an interior square
(tests/mask_zoo.py: the reference's brush mask, a frame along the four borders, isolated pixels, alternating tile rows and columns,
the four corners, one pixel in the last corner, a diagonal, every tile of every level) -- in every form the forward has: the
benchmarked one (channels-last, persistent in-place outputs, twins, graph replay) as ONE model walks through the whole set, a
launch plan that follows the masks, fp16 compute and fp16 caches, eight edits stacked into one forward, the reference-layout module
path.  Reference everywhere: util.ddpm_cpu_oracle over the nine masks (memoised: one full pass, nine sparse forwards per process).
Tolerances are the project's own: util.CONV_ATOL for fp32 forms, tolerance.f16_check for fp16 forms.  Every assertion that is not
against the oracle is a bit equality riding on one that is; nothing here is a self-check."""
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


def _ddpm():
    """bench.py's network (seed-0 weights, ch 128, channels-last, in-place scatter) after its cache-producing full pass on the
    library's exact-fp32 kernels (fixed kernels: the same caches on every box)."""
    import bench
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0, noise = bench.make_inputs()
    t = torch.zeros(1, device=DEV)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        full = model(_cl(x0), t).clone()
    return model, _cl(x0), _cl(noise), t, full


@pytest.fixture(scope="module")
def net(hip):
    return _ddpm()


def _err(got, want):
    return float((got.detach().float().cpu() - want).abs().max())


def _fp32(what, got, want):
    """max |got - oracle| <= CONV_ATOL, recorded (a NaN fails: it is not <= anything)."""
    err = util.record_margin("masks", what, _err(got, want), util.CONV_ATOL)
    print("masks %-60s %.3e" % (what, err), flush=True)
    assert err <= util.CONV_ATOL, (what, err)


def _f16(what, got, want):
    from sige_amd import tolerance

    util.assert_finite(got, what)
    r = tolerance.f16_check(got, want)
    util.record_margin("masks", what, r["worst_over_allowed"], 1.0)
    print("masks %-60s %.4f of the f16 allowance (max |delta| %.3e)" % (what, r["worst_over_allowed"], r["max_abs"]), flush=True)
    assert r["ok"], (what, r)


# ---- a. the index lists of every Gather, per mask -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mask_zoo.COUNTS))
def test_index_lists_under_every_mask(hip, net, name):
    """SIGEModel.set_masks on the device pyramid of each zoo mask: every Gather of the network holds exactly the list the oracle
    builds from the CPU pyramid (as test_set_masks_builds_every_index_list_with_one_sync does for one interior square), and the
    lists have the sizes tests/mask_zoo.py states."""
    from oracle import oracle
    from sige_amd.nn import Gather

    model = net[0]
    mask = mask_zoo.zoo()[name]
    model.set_masks(_build_masks(mask.to(DEV)))
    cpu_masks = oracle.downsample_mask(oracle.dilate_mask(mask, 5), 8)
    seen, sizes = 0, {}
    for m in model.modules():
        if isinstance(m, Gather):
            want = oracle.reduce_mask(cpu_masks[tuple(m.input_res)], m.block_size, m.block_stride, m.offset)
            assert torch.equal(m.active_indices.cpu(), want), (name, tuple(m.input_res), tuple(m.block_size))
            sizes[(int(m.input_res[0]), int(m.block_size[0]), int(m.block_stride[0]), int(m.offset[0]))] = int(want.shape[0])
            seen += 1
    assert seen > 30
    n6, n4 = mask_zoo.COUNTS[name]
    table = {(res, 6, 4, 1): n6[k] for k, res in enumerate(mask_zoo.LEVELS)}
    table.update({(res, 4, 4, 0): n4[k] for k, res in enumerate(mask_zoo.LEVELS)})
    hits = [key for key in sizes if key in table]
    assert len(hits) >= 6 and all(sizes[key] == table[key] for key in hits), (name, sizes)


# ---- b. the benchmarked form: one model through the whole set -----------------------------------------------------------------
def _walk(tag, model, x0, noise, t, wants):
    import bench

    zoo = mask_zoo.zoo()
    for name in mask_zoo.SEQUENCE:
        mask = zoo[name].to(DEV)
        x1 = _cl(x0 + noise * mask)
        model.set_masks(_build_masks(mask))
        model.set_mode("sparse")
        first = model(x1, t).clone()  # (the path a mask change takes: twins and persistent outputs rebuilt from the cache)
        model(x1, t)
        third = model(x1, t).clone()
        _fp32("%s %s first forward after set_masks" % (tag, name), first, wants[name])
        _fp32("%s %s third forward" % (tag, name), third, wants[name])
        assert model._h0_buf is not None
        model._h0_buf.fill_(NAN)  # (conv_in's window buffer: stale, and by design unread, outside the active windows)
        fourth = model(x1, t).clone()
        util.assert_finite(fourth, "%s %s after NaN _h0_buf" % (tag, name))
        assert torch.equal(fourth, third), (tag, name, "NaN in _h0_buf moved the output")
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, third), (tag, name, "graph replay != eager forward", _err(out, third.cpu()))
        del g, out


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_one_model_through_every_mask_vs_oracle(hip, net, poison):
    """The benchmarked configuration, ONE model, the nine masks in an order that alternates large and small footprints (the first
    step shrinks 4225 tiles to 8: in-place buffers and twins must come back from the cache).  Per mask: the first forward after
    set_masks and the third against that mask's CPU-oracle output; NaN in `_h0_buf` does not move a bit; a captured graph
    replays the eager forward bit for bit.  Once plainly, once with every uninitialised allocation poisoned with NaN (model
    built inside)."""
    zoo = mask_zoo.zoo()
    full_c, outs = util.ddpm_cpu_oracle(list(zoo.values()))
    wants = dict(zip(zoo, outs))
    if not poison:
        model, x0, noise, t, full = net
        _fp32("plain full pass", full, full_c)
        with torch.no_grad():
            _walk("plain", model, x0, noise, t, wants)
        return
    with util.poisoned() as p, torch.no_grad():
        model, x0, noise, t, full = _ddpm()
        util.assert_finite(full, "poisoned full pass")
        _fp32("poisoned full pass", full, full_c)
        _walk("poisoned", model, x0, noise, t, wants)
    assert p.n > 100


# ---- c. a launch plan against the oracle --------------------------------------------------------------------------------------
def test_launch_plan_follows_every_mask_vs_oracle(hip, net):
    """ONE recording under the benchmark's interior square, then bind_mask of each zoo mask: the forward issued from C against the
    CPU oracle, its hipGraph replay bit-equal to it; `full_grid` fills the plan's buffers to their capacity (65 x 65 tiles)."""
    import bench
    from sige_amd.plan import LaunchPlan

    model, x0, noise, t, _ = net
    zoo = mask_zoo.zoo()
    _, outs = util.ddpm_cpu_oracle(list(zoo.values()))
    wants = dict(zip(zoo, outs))
    m0 = bench.edit_mask(0.012).to(DEV)
    xs = (x0 + noise * m0).clone()
    seen = {}
    with torch.no_grad():
        plan = LaunchPlan(model)
        plan.record(m0, _build_masks, lambda: model(xs, t))
        assert not plan.shape_bound
        for name in mask_zoo.SEQUENCE:
            mask = zoo[name].to(DEV)
            xs.copy_(x0 + noise * mask)
            plan.bind_mask(mask)
            got = plan.run().clone()
            _fp32("plan.run %s" % name, got, wants[name])
            rep = plan.replay().clone()
            assert torch.equal(rep, got), (name, "plan.replay != plan.run", _err(rep, got.cpu()))
            seen[name] = tuple(plan.counts)
        torch.cuda.synchronize()
        del plan
    assert len(set(seen.values())) >= 8, seen
    assert max(seen["full_grid"]) == 65 * 65 and all(c > 0 for c in seen["full_grid"])


# ---- e. eight edits stacked into one forward ----------------------------------------------------------------------------------
def test_stacked_zoo_vs_cpu_oracle(hip, net):
    """E = 8 edits of the one original, each its own zoo mask, through ONE stacked forward (sige_amd/stacked.py); every edit's
    slice against THAT mask's CPU-oracle output (the reference's semantics: one forward per mask).  The order puts masks whose last
    rows are active directly above masks whose first rows are: at least three of the seven seams have active tiles on both sides,
    whose halos would read the neighbouring image without the seam rule."""
    from oracle import oracle
    from sige_amd import stacked

    model, x0, noise, t, _ = net
    zoo = mask_zoo.zoo()
    _, outs = util.ddpm_cpu_oracle(list(zoo.values()))
    wants = dict(zip(zoo, outs))
    names = list(mask_zoo.STACK)
    E = len(names)
    assert E == 8 and "diagonal" not in names
    # (the first and last rows of the DILATED masks, i.e. of the pyramid's 256 x 256 level: what makes a tile active)
    dil = {n: oracle.dilate_mask(zoo[n], 5) for n in names}
    both = [(a, b) for a, b in zip(names[:-1], names[1:]) if dil[a][255].any() and dil[b][0].any()]
    assert len(both) >= 3 and set(mask_zoo.SEAMS_ACTIVE_ON_BOTH_SIDES) <= set(both), both
    gm = [zoo[n].to(DEV) for n in names]
    with torch.no_grad():
        xe = _cl(torch.cat([x0 + noise * m for m in gm], 0))
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, [_build_masks(m) for m in gm])
            model.set_mode("sparse")
            with stacked.edit_batch(model, E):
                model(xe, t)  # (registers the activated twins; from the next forward on they are read)
                out = model(xe, t).clone()
        finally:
            stacked.unstack_caches(model)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (E, 3, 256, 256)
    for e, n in enumerate(names):
        _fp32("stacked edit %d %s" % (e, n), out[e], wants[n][0])


# ---- f. the reference-layout module path --------------------------------------------------------------------------------------
def test_reference_layout_module_path_vs_oracle(hip):
    """The same network on contiguous NCHW tensors, fresh outputs instead of persistent ones (no set_scatter_inplace), full pass
    through torch's convs and the sparse forward through the NCHW kernels, as test_ddpm_unet_gpu_vs_oracle_backend runs them --
    here at the benchmark's width, so that the memoised oracle outputs serve -- under the brush mask, the frame and the specks."""
    import bench
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    zoo = mask_zoo.zoo()
    full_c, outs = util.ddpm_cpu_oracle(list(zoo.values()))
    wants = dict(zip(zoo, outs))
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV)
    x0, noise = bench.make_inputs()
    x0, noise, t = x0.to(DEV), noise.to(DEV), torch.zeros(1, device=DEV)
    with torch.no_grad():
        model.set_mode("full")
        full = model(x0, t)
        _fp32("NCHW module path full pass", full, full_c)
        for name in ("assets_mask", "frame", "specks"):
            mask = zoo[name].to(DEV)
            model.set_masks(_build_masks(mask))
            model.set_mode("sparse")
            got = model((x0 + noise * mask).contiguous(), t)
            _fp32("NCHW module path %s" % name, got, wants[name])


# ---- d. fp16 forms (last: they re-make the shared model's caches) -------------------------------------------------------------
@pytest.mark.parametrize("form", ["f16_compute", "f16_cache"])
def test_f16_forms_under_every_mask_vs_oracle(hip, net, form):
    """set_compute_dtype("f16") with the model's keep policy on (no edit_ratio), and the same with the cache STORED as fp16
    (set_cache_dtype("f16"), full pass repeated): all nine masks, the second forward, finite and inside the f16 criterion
    (sige_amd.tolerance) against the fp32 CPU oracle."""
    model, x0, noise, t, _ = net
    zoo = mask_zoo.zoo()
    _, outs = util.ddpm_cpu_oracle(list(zoo.values()))
    wants = dict(zip(zoo, outs))

    def full_pass():
        with util.native_full_pass():
            model.set_mode("full")
            model(x0, t)

    try:
        with torch.no_grad():
            if form == "f16_cache":
                model.set_compute_dtype("f32")
                model.set_cache_dtype("f16")
                full_pass()
            model.set_compute_dtype("f16")
            assert model.compute_policy["keep"] == tuple(model.F16_KEEP)
            for name in mask_zoo.SEQUENCE:
                mask = zoo[name].to(DEV)
                x1 = _cl(x0 + noise * mask)
                model.set_masks(_build_masks(mask))
                model.set_mode("sparse")
                model(x1, t)  # (consumers register their activated twins on the first forward)
                _f16("%s %s" % (form, name), model(x1, t).clone(), wants[name])
    finally:
        with torch.no_grad():
            model.set_compute_dtype("f32")
            if form == "f16_cache":
                model.set_cache_dtype("f32")
                full_pass()  # (the shared model's fp32 caches back)
