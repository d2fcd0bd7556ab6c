"""On the MI355X: the skip half of a dense up level's conv1 computed as side convs behind the launches of the level below
(DDPMSparseUNet.SIDE_SKIP_PRODUCTS).  tests/test_gpu_dense_change_regions.py's small network has no qualifying
level (its only dense level is the lowest one: nothing below it could host), so this is the smallest that has one: 32 x 32 input,
levels 32 (tiled) / 16 (dense, 256 channels: the qualifying level; four blocks, so it is no demand stage) / 8 (dense, 512
channels: its single 3x3 launches are 128 workgroups of 16 x 16 blocks, the hosts).  Against the CPU oracle with the flag on and
off, first forward, graph replay, launch plan, counters, a second original, pack_caches and cache id 1; DDPM-256 once."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cfg():
    from sige_amd.workloads.ddpm_unet import DDPMConfig

    return DDPMConfig(ch=128, ch_mult=(1, 2, 4), num_res_blocks=3, attn_resolutions=(), resolution=32, sparse_threshold=32)


def _masks():
    interior = torch.zeros(32, 32, dtype=torch.bool)
    interior[13:17, 14:19] = True
    corner = torch.zeros(32, 32, dtype=torch.bool)
    corner[:3, :4] = True
    large = torch.zeros(32, 32, dtype=torch.bool)
    large[2:30, 1:31] = True
    edge = torch.zeros(32, 32, dtype=torch.bool)
    edge[20:27, 28:] = True
    return {"interior": interior, "corner": corner, "large": large, "edge": edge}


def _inputs():
    gen = torch.Generator().manual_seed(5)
    return torch.randn(1, 3, 32, 32, generator=gen), torch.randn(1, 3, 32, 32, generator=gen)


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


def _err(got, want):
    return float((got.detach().float().cpu() - want.detach().float().cpu()).abs().max())


def _close(what, got, want, tol=util.CONV_ATOL):
    err = util.record_margin("side_products", what, _err(got, want), tol)
    print("side_products %-64s %.3e" % (what, err), flush=True)
    assert err <= tol, (what, err)


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

        self.keep, DDPMSparseUNet.SIDE_SKIP_PRODUCTS = DDPMSparseUNet.SIDE_SKIP_PRODUCTS, self.on

    def __exit__(self, *exc):
        from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

        DDPMSparseUNet.SIDE_SKIP_PRODUCTS = self.keep
        return False


def _new_model(x0, cache_id=0):
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(_cfg()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    _full(model, x0, cache_id)
    return model


def _full(model, x0, cache_id=0):
    with util.native_full_pass(), torch.no_grad():
        model.set_cache_id(cache_id)
        model.set_mode("full")
        model(_cl(x0), torch.zeros(1, device=DEV))


def _sparse(model, x0, noise, t, mask, forwards=3):
    mask = mask.to(DEV)
    x1 = _cl(x0.to(DEV) + noise.to(DEV) * mask)
    model.set_masks(_build_masks(mask))
    model.set_mode("sparse")
    out = None
    with torch.no_grad():
        for _ in range(forwards):
            out = model(x1, t)
    return x1, out.clone()


@pytest.fixture(scope="module")
def net(hip):
    """(GPU model after its full pass on A, {A, B} originals, noise, t, {(image, mask): the CPU oracle's sparse output})."""
    from sige_amd import runtime
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    xa, noise = _inputs()
    xb = xa.flip(-1).contiguous() * 0.75 + 0.1
    torch.manual_seed(0)
    cpu = DDPMSparseUNet(_cfg()).eval()
    wants = {}
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            for img, x0, names in (("A", xa, ("interior", "corner", "large", "edge")), ("B", xb, ("interior",))):
                cpu.set_mode("full")
                cpu(x0, torch.zeros(1))
                for name in names:
                    m = _masks()[name]
                    cpu.set_masks(_build_masks(m))
                    cpu.set_mode("sparse")
                    wants[(img, name)] = cpu(x0 + noise * m, torch.zeros(1)).clone()
    finally:
        runtime.unregister_backend("cpu")
    del cpu
    model = _new_model(xa)
    assert model.SIDE_SKIP_PRODUCTS in (True, False) and model._side_levels() == [1]
    return model, {"A": xa, "B": xb}, noise, torch.zeros(1, device=DEV), wants


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_flag_on_and_off_vs_oracle(hip, net, name):
    model, x0s, noise, t, wants = net
    outs, hosted = {}, {}
    for on in (True, False):
        with _flag(on), util.poisoned(NAN):
            h0 = hip.conv_side_workgroups()[0]
            _, outs[on] = _sparse(model, x0s["A"], noise, t, _masks()[name])
            hosted[on] = hip.conv_side_workgroups()[0] - h0
        util.assert_finite(outs[on], "flag %s" % on)
        _close("%s flag %s vs oracle" % (name, "on" if on else "off"), outs[on], wants[("A", name)])
    _close("%s flag on vs off" % name, outs[True], outs[False], util.SELF_ATOL)
    assert hosted[True] > 0 and hosted[False] == 0, hosted


def test_first_forward_after_a_full_pass_has_the_flag_off_bits(hip, net):
    """No twins yet: conv1 runs unsplit, nothing is queued."""
    _, x0s, noise, t, _ = net
    outs = {}
    for on in (True, False):
        with _flag(on):
            model = _new_model(x0s["A"])
            w0 = hip.conv_side_workgroups()
            _, outs[on] = _sparse(model, x0s["A"], noise, t, _masks()["interior"], forwards=1)
            assert hip.conv_side_workgroups() == w0
    assert torch.equal(outs[True], outs[False])


def test_counters_and_launch_count(hip, net):
    """A steady forward: every product fully hosted (four products of 128 blocks behind thirteen hosts), as many launches as with
    the flag off."""
    model, x0s, noise, t, _ = net
    counts = {}
    for on in (True, False):
        with _flag(on), torch.no_grad():
            x1, _ = _sparse(model, x0s["A"], noise, t, _masks()["interior"])
            w0, n0 = hip.conv_side_workgroups(), hip.launch_count()
            model(x1, t)
            w1 = hip.conv_side_workgroups()
            counts[on] = (hip.launch_count() - n0, w1[0] - w0[0], w1[1] - w0[1])
    assert counts[False][1:] == (0, 0) and counts[True][1] > 0 and counts[True][2] == 0, counts
    assert counts[True][0] == counts[False][0] > 0, counts


def test_graph_replay_and_launch_plan_equal_the_module_forward(hip, net):
    import bench
    from sige_amd.plan import LaunchPlan

    model, x0s, noise, t, _ = net
    with _flag(True), torch.no_grad():
        x1, want = _sparse(model, x0s["A"], noise, t, _masks()["interior"])
        h0 = hip.conv_side_workgroups()[0]
        g, out = bench.capture(model, x1, t)
        assert hip.conv_side_workgroups()[0] > h0
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), _err(out, want)
        del g, out

        m0 = _masks()["interior"].to(DEV)
        xs = x1.clone()
        plan = LaunchPlan(model)
        plan.record(m0, _build_masks, lambda: model(xs, t))
        assert not plan.shape_bound and plan.unbound_counts == 0
        for name in ("corner", "edge"):
            mask = _masks()[name].to(DEV)
            xs.copy_(_cl(x0s["A"]) + _cl(noise) * mask)
            plan.bind_mask(mask)
            got = plan.run().clone()
            model.set_masks(_build_masks(mask))
            model.set_mode("sparse")
            for _ in range(3):
                ref = model(xs, t)
            assert torch.equal(got, ref), (name, _err(got, ref))
        torch.cuda.synchronize()
        del plan


def test_second_original_pack_caches_and_cache_id_1(hip, net):
    from sige_amd import parallel

    _, x0s, noise, t, wants = net
    mask = _masks()["interior"]
    with _flag(True):
        model = _new_model(x0s["A"])
        _, out = _sparse(model, x0s["A"], noise, t, mask)
        _close("A before pack_caches", out, wants[("A", "interior")])
        parallel.pack_caches(model)
        _, out = _sparse(model, x0s["A"], noise, t, mask)
        _close("A after pack_caches", out, wants[("A", "interior")])
        _full(model, x0s["B"])
        h0 = hip.conv_side_workgroups()[0]
        _, out = _sparse(model, x0s["B"], noise, t, mask)
        _close("B after a second full pass", out, wants[("B", "interior")])
        assert hip.conv_side_workgroups()[0] > h0
        # cache id 1 holds A next to B under id 0; both keep working, one after the other
        _full(model, x0s["A"], cache_id=1)
        _, out = _sparse(model, x0s["A"], noise, t, mask)
        _close("A under cache id 1", out, wants[("A", "interior")])
        model.set_cache_id(0)
        _, out = _sparse(model, x0s["B"], noise, t, mask)
        _close("B under cache id 0 again", out, wants[("B", "interior")])


def test_ddpm_256_headline(hip):
    """The benchmarked forward at 1.2 % with the flag on: against the CPU oracle, 96 launches, every product hosted."""
    import bench
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    m0 = bench.edit_mask(0.012)
    _, (want,) = util.ddpm_cpu_oracle([m0])
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0, noise = bench.make_inputs()
    t = torch.zeros(1, device=DEV)
    with _flag(True), torch.no_grad():
        _full(model, x0)
        x1, out = _sparse(model, x0, noise, t, m0)
        assert model._side_levels() == [4]  # (up[3] runs on demand lists, up[5] has no level below it)
        _close("ddpm-256 1.2 % flag on vs oracle", out, want)
        w0, n0 = hip.conv_side_workgroups(), hip.launch_count()
        model(x1, t)
        w1 = hip.conv_side_workgroups()
        assert hip.launch_count() - n0 == 96, hip.launch_count() - n0
        assert w1[0] - w0[0] == 1280 and w1[1] == w0[1], (w0, w1)
