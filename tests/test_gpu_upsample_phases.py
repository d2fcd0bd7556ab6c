"""On the MI355X: the Upsample conv (nearest x2, then a tiled 3x3 conv) as four 2x2 phase convs on the half-resolution tensor
(Gather.PHASE_UPSAMPLE, sige_hip_gather_conv_nhwc with upsample2x = 2).  The kernel against fp64 of the 9-tap
definition with the ORIGINAL weights, what it leaves alone, the epilogue's twins and out-affine, what the library refuses, and the
smallest network with two Upsamples against the CPU oracle, its graph, its launch plan and its launch count.

Shapes.  Low-res 6x5 -> 12x10: 3 x 3 hi-res tiles whose last row and column hang over the image.  One tile gives each phase 4 pixels, so
an M block of the 16-pixel kernel holds 4 tiles: the 9 (batch 1) or 18 (batch 2) tiles are 3 or 5 M blocks, the last one ragged, the
batch boundary inside a block.  The output block is the one the 9-tap form picks for the call (plan_conv, csrc/block_conv.hip): 16 x 16
here; low-res 16x16 (64 tiles) is the smallest square at which 128 output channels take 16 x 32 blocks (64 * 4 >= 224) and 256 output
channels take the 32-pixel block (32 * 8 >= 224), the other two kernels built.
Bound: the suite's convention for exact-fp32 convs against fp64, 2e-5 * (1 + max |ref|)."""
import pytest
import torch
import torch.nn.functional as F

from tests import util
from tests.change_regions_common import small_cfg, small_inputs, small_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
UP_ARG = 37  # position of `upsample2x` in sige_hip_gather_conv_nhwc (include/sige_hip.h)


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bound(ref):
    return 2e-5 * (1.0 + float(ref.abs().max()))


def _err(got, want):
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max())


class _calls:
    """Spy on the entry point: (upsample2x, status) of every sige_hip_gather_conv_nhwc call inside the block."""

    def __init__(self, hip):
        self.lib, self.seen = hip.lib(), []

    def __enter__(self):
        self.real = self.lib.sige_hip_gather_conv_nhwc

        def spy(*args):
            status = self.real(*args)
            self.seen.append((int(args[UP_ARG]), int(status)))
            return status

        self.lib.sige_hip_gather_conv_nhwc = spy
        return self

    def __exit__(self, *exc):
        self.lib.sige_hip_gather_conv_nhwc = self.real
        return False


class _phase_flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.nn import Gather

        self.keep, Gather.PHASE_UPSAMPLE = Gather.PHASE_UPSAMPLE, self.on

    def __exit__(self, *exc):
        from sige_amd.nn import Gather

        Gather.PHASE_UPSAMPLE = self.keep
        return False


# ---- a. the kernel ----------------------------------------------------------------------------------------------------------------
def _tile_lists(H, W):
    """Named tile lists over the hi-res [H,W] image: origins (4i - 1, 4j - 1) of the 6x6 windows (padding 1)."""
    gh, gw = (H + 3) // 4, (W + 3) // 4
    every = [(i, j) for i in range(gh) for j in range(gw)]
    lists = {
        "every": every,
        "corners": [(0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1)],
        "interior": [(gh // 2, gw // 2)],
        "holes": [c for k, c in enumerate(every) if k % 2 == 0 and k != 4],
        "empty": [],
    }
    return {n: torch.tensor([(4 * i - 1, 4 * j - 1) for i, j in c], dtype=torch.int32).reshape(-1, 2) for n, c in lists.items()}


_CASES = {}


def _case(cin, cout, batch, res, with_bias=True):
    """Inputs and the fp64 reference of one shape, computed once: conv2d(interpolate(x, 2, nearest), w, b, padding=1)."""
    key = (cin, cout, batch, res, with_bias)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * cin + cout + batch)
        x = torch.randn(batch, cin, *res, generator=gen)
        w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
        b = torch.randn(cout, generator=gen) if with_bias else None
        ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), None if b is None else b.double(), padding=1)
        _CASES[key] = (x, w, b, ref)
    return _CASES[key]


def _covered(idx, H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[max(h0 + 1, 0):h0 + 5, max(w0 + 1, 0):w0 + 5] = True
    return m


def _launch(hip, x, w, b, idx, form, before, residual=None, out_affine=None, twins=None):
    """One call in `form` (2: phase, 1: 9-tap) into a copy of `before`; returns (out, [(upsample2x, status)])."""
    cout = w.shape[0]
    H, W = 2 * x.shape[2], 2 * x.shape[3]
    wd = w.to(DEV)
    packed = hip.conv_pack_weights(wd, 6, 6, (1, 1), "f32")
    phase = hip.upsample_phase_pack(wd) if form == 2 else None
    out = before.clone(memory_format=torch.channels_last)
    with _calls(hip) as spy:
        got = hip.gather_conv_cl(_cl(x), None, (6, 6), idx.to(DEV), None, None, "identity", packed, None if b is None else b.to(DEV), cout,
                                 (3, 3), (1, 1), full=dict(offset=(1, 1), out_res=(H, W), residual=residual), out_affine=out_affine,
                                 upsample2x=True, out=out, twins=twins, phase=phase)
    torch.cuda.synchronize()
    assert got is out
    return out, spy.seen


@pytest.mark.parametrize("cin,cout,res,batch", [(64, 64, (6, 5), 1), (64, 64, (6, 5), 2), (96, 48, (6, 5), 1), (96, 48, (6, 5), 2),
                                                (128, 128, (6, 5), 1), (128, 128, (6, 5), 2),
                                                (128, 128, (16, 16), 1), (64, 256, (16, 16), 1)])  # (the last two: NB 2, 32-pixel block)
def test_phase_kernel_vs_fp64_of_the_nine_tap_definition(hip, cin, cout, res, batch):
    x, w, b, ref = _case(cin, cout, batch, res)
    H, W = 2 * res[0], 2 * res[1]
    tol = _bound(ref)
    for name, idx in _tile_lists(H, W).items():
        if res == (16, 16) and name != "every":
            continue
        with util.poisoned(NAN):
            before = torch.empty(batch, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen = _launch(hip, x, w, b, idx, 2, before)
            old, seen_old = _launch(hip, x, w, b, idx, 1, before)
        assert seen == [(2, 0)] and seen_old == [(1, 0)], (name, seen, seen_old)
        inside = _covered(idx, H, W)
        g, o = got.cpu().double(), old.cpu().double()
        assert bool(torch.isnan(g[:, :, ~inside]).all()) and bool(torch.isnan(o[:, :, ~inside]).all()), name  # untouched cells
        if not bool(inside.any()):
            continue
        err = util.record_margin("upsample_phases", "phase %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name),
                                 float((g - ref)[:, :, inside].abs().max()), tol)
        err_old = util.record_margin("upsample_phases", "9-tap %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name),
                                     float((o - ref)[:, :, inside].abs().max()), tol)
        print("upsample_phases %3d/%3d %s B%d %-8s phase %.3e  9-tap %.3e  bound %.3e" % (cin, cout, res, batch, name, err, err_old, tol), flush=True)
        assert err <= tol and err_old <= tol, (name, err, err_old, tol)


@pytest.mark.parametrize("with_bias", [True, False])
def test_cells_outside_the_list_keep_their_bits(hip, with_bias):
    x, w, b, ref = _case(64, 64, 2, (6, 5), with_bias)
    idx = _tile_lists(12, 10)["holes"]
    before = _cl(torch.randn(2, 64, 12, 10, generator=torch.Generator().manual_seed(7)))
    got, seen = _launch(hip, x, w, b, idx, 2, before)
    assert seen == [(2, 0)]
    inside = _covered(idx, 12, 10)
    assert torch.equal(got[:, :, ~inside.to(DEV)], before[:, :, ~inside.to(DEV)])
    err = util.record_margin("upsample_phases", "holes, bias %s" % with_bias, float((got.cpu().double() - ref)[:, :, inside].abs().max()), _bound(ref))
    assert err <= _bound(ref), err


def test_twins_out_affine_and_residual_as_the_nine_tap_form(hip):
    """Both twins, the out-affine with SiLU and a residual in one launch: each output against fp64 and against the 9-tap launch."""
    x, w, b, ref = _case(96, 48, 2, (6, 5))
    gen = torch.Generator().manual_seed(9)
    idx = _tile_lists(12, 10)["every"]
    res = torch.randn(2, 48, 12, 10, generator=gen)
    vec = lambda: (0.5 + torch.rand(48, generator=gen), torch.randn(48, generator=gen))  # noqa: E731
    (os_, oh_), (s0, t0), (s1, t1) = vec(), vec(), vec()
    v = ref + res.double()
    bc = lambda t: t.double().reshape(1, -1, 1, 1)  # noqa: E731
    wants = {"out": F.silu(bc(os_) * v + bc(oh_)), "twin0": F.silu(bc(s0) * v + bc(t0)), "twin1": F.silu(bc(s1) * v + bc(t1))}
    outs = {}
    for form in (2, 1):
        with util.poisoned(NAN):
            tw = [torch.empty(2, 48, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last) for _ in range(2)]
            before = torch.empty(2, 48, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last)
            out, seen = _launch(hip, x, w, b, idx, form, before, residual=_cl(res), out_affine=(os_.to(DEV), oh_.to(DEV), "swish"),
                                twins=[(tw[0], s0.to(DEV), t0.to(DEV)), (tw[1], s1.to(DEV), t1.to(DEV))])
        assert seen == [(form, 0)]
        outs[form] = {"out": out, "twin0": tw[0], "twin1": tw[1]}
    inside = _covered(idx, 12, 10)
    assert bool(inside.all())
    for name, want in wants.items():
        tol = _bound(v)  # (SiLU and a scale of at most 1.5 on v: the conv's bound on the pre-activation carries over)
        for form in (2, 1):
            err = util.record_margin("upsample_phases", "%s form %d" % (name, form), _err(outs[form][name], want), tol)
            assert err <= tol, (name, form, err)
        assert _err(outs[2][name], outs[1][name]) <= tol


def test_what_the_phase_form_does_not_cover_is_refused(hip):
    """A gather affine, fp16 operands and a tile destination: SIGE_HIP_EUNSUPPORTED from the entry point; through the binding the
    call then runs in the 9-tap form with the bits of a call that never asked for the phase form."""
    x, w, b, ref = _case(64, 64, 1, (6, 5))
    idx = _tile_lists(12, 10)["every"].to(DEV)
    wd, bd, xd = w.to(DEV), b.to(DEV), _cl(x)
    packed, phase = hip.conv_pack_weights(wd, 6, 6, (1, 1), "f32"), hip.upsample_phase_pack(wd)
    sc, sh = (0.5 + torch.rand(1, 64, 1, 1)).to(DEV), torch.randn(1, 64, 1, 1).to(DEV)
    full = dict(offset=(1, 1), out_res=(12, 10), residual=None)
    outs = {}
    for ph in (phase, None):
        with _calls(hip) as spy:
            outs[ph is None] = hip.gather_conv_cl(xd, None, (6, 6), idx, sc, sh, "swish", packed, bd, 64, (3, 3), (1, 1), full=full,
                                                  upsample2x=True, phase=ph)
        assert spy.seen == ([(2, hip.UNSUPPORTED), (1, 0)] if ph is not None else [(1, 0)]), spy.seen
    assert torch.equal(outs[False], outs[True])
    # a tile destination never asks; fp16 operands are refused
    with _calls(hip) as spy:
        hip.gather_conv_cl(xd, None, (6, 6), idx, None, None, "identity", packed, bd, 64, (3, 3), (1, 1), upsample2x=True, phase=phase)
    assert spy.seen == [(1, 0)]
    packed_h = hip.conv_pack_weights(wd, 6, 6, (1, 1), "f16")
    L = hip.lib()
    out = torch.empty(1, 64, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last)
    args = [0, xd.data_ptr(), None, 1, 64, 0, 12, 10, 6, 6, idx.data_ptr(), idx.shape[0], None, 0, 0, None, 0, 0, 0, phase.data_ptr(), bd.data_ptr(), 64,
            3, 3, 1, 1, 1, 1, 1, None, 12, 10, None, 0, None, None, 0, 2, None, None, None, None, None, None, None, 0, out.data_ptr(), None]
    assert L.sige_hip_gather_conv_nhwc(*args) == 0
    bad = list(args)
    bad[0], bad[19] = 1, packed_h.data_ptr()
    assert L.sige_hip_gather_conv_nhwc(*bad) == hip.UNSUPPORTED
    bad = list(args)
    bad[26] = 0  # tile destination
    assert L.sige_hip_gather_conv_nhwc(*bad) == hip.UNSUPPORTED
    bad = list(args)
    bad[UP_ARG] = 3
    assert L.sige_hip_gather_conv_nhwc(*bad) != 0
    torch.cuda.synchronize()


# ---- b. the small network: two Upsamples (256 ch 16 -> 32, 128 ch 32 -> 64) ---------------------------------------------------------
def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


def _new_model(x0):
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
    """(GPU model after its full pass, x0, noise, t, {mask name: CPU-oracle sparse output})."""
    from sige_amd import runtime
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    x0, noise = small_inputs()
    torch.manual_seed(0)
    cpu = DDPMSparseUNet(small_cfg()).eval()
    wants = {}
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            cpu.set_mode("full")
            cpu(x0, torch.zeros(1))
            for name, m in small_masks().items():
                cpu.set_masks(_build_masks(m))
                cpu.set_mode("sparse")
                wants[name] = cpu(x0 + noise * m, torch.zeros(1)).clone()
    finally:
        runtime.unregister_backend("cpu")
    return _new_model(x0), _cl(x0), _cl(noise), torch.zeros(1, device=DEV), wants


def _sparse(model, x0, noise, t, mask, forwards=3):
    mask = mask.to(DEV)
    x1 = _cl(x0 + noise * mask)
    model.set_masks(_build_masks(mask))
    model.set_mode("sparse")
    out = None
    for _ in range(forwards):
        out = model(x1, t)
    return x1, out.clone()


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_small_network_flag_on_vs_oracle_and_flag_off_takes_the_old_launches(hip, small, name):
    model, x0, noise, t, wants = small
    mask = small_masks()[name]
    with torch.no_grad():
        with _phase_flag(True), _calls(hip) as on:
            x1, got = _sparse(model, x0, noise, t, mask, forwards=1)
        with _phase_flag(False), _calls(hip) as off:
            _, old = _sparse(model, x0, noise, t, mask, forwards=1)
        # the parent's forward: the same module code with the phase pack never handed to the binding
        real = hip.gather_conv_cl
        hip.gather_conv_cl = lambda *a, **k: real(*a, **{kk: v for kk, v in k.items() if kk != "phase"})
        try:
            with _phase_flag(True):
                _, parent = _sparse(model, x0, noise, t, mask, forwards=1)
        finally:
            hip.gather_conv_cl = real
    assert [c for c in on.seen if c[0] == 2] == [(2, 0), (2, 0)], on.seen      # both Upsamples, neither refused
    assert not [c for c in off.seen if c[0] == 2] and len([c for c in off.seen if c[0] == 1]) == 2, off.seen
    assert torch.equal(old, parent)
    err = util.record_margin("upsample_phases", "small %s flag on vs oracle" % name, _err(got, wants[name]), util.CONV_ATOL)
    err_off = util.record_margin("upsample_phases", "small %s flag off vs oracle" % name, _err(old, wants[name]), util.CONV_ATOL)
    print("upsample_phases small %-8s on %.3e off %.3e on-off %.3e" % (name, err, err_off, _err(got, old)), flush=True)
    assert err <= util.CONV_ATOL and err_off <= util.CONV_ATOL, (err, err_off)


def test_small_network_graph_replay_equals_eager(hip, small):
    import bench

    model, x0, noise, t, _ = small
    with torch.no_grad(), _phase_flag(True):
        x1, want = _sparse(model, x0, noise, t, small_masks()["interior"])
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), _err(out, want)
        del g, out


def test_small_network_launch_plan_follows_a_second_mask(hip, small):
    from sige_amd.plan import LaunchPlan

    _, x0, noise, t, _ = small
    masks = small_masks()
    with torch.no_grad(), _phase_flag(True):
        model = _new_model(x0.cpu())
        m0 = masks["interior"].to(DEV)
        xs = (x0 + noise * m0).clone(memory_format=torch.channels_last)
        plan = LaunchPlan(model)
        plan.record(m0, _build_masks, lambda: model(xs, t))
        assert not plan.shape_bound and plan.unbound_counts == 0
        for name in ("corner", "large"):
            mask = masks[name].to(DEV)
            xs.copy_(x0 + noise * mask)
            plan.bind_mask(mask)
            got = plan.run().clone()
            model.set_masks(_build_masks(mask))
            model.set_mode("sparse")
            with _calls(hip) as spy:
                for _ in range(3):
                    want = model(xs, t)
            assert len([c for c in spy.seen if c == (2, 0)]) == 6, spy.seen
            assert torch.equal(got, want), (name, _err(got, want))
        torch.cuda.synchronize()
        del plan


def test_small_network_launch_count_is_unchanged(hip, small):
    model, x0, noise, t, _ = small
    counts = {}
    with torch.no_grad():
        for flag in (True, False):
            with _phase_flag(flag):
                x1, _ = _sparse(model, x0, noise, t, small_masks()["interior"])
                n0 = hip.launch_count()
                model(x1, t)
                counts[flag] = hip.launch_count() - n0
    assert counts[True] == counts[False] > 0, counts


def test_small_network_guards(hip, small):
    """Stacked edits (E = 2) and fp16 operands: the flag changes nothing, and no call asks for the phase form."""
    from sige_amd import stacked

    model, x0, noise, t, _ = small
    masks = [small_masks()["interior"].to(DEV), small_masks()["corner"].to(DEV)]
    xe = _cl(torch.cat([x0 + noise * m for m in masks], 0))
    outs = {}
    with torch.no_grad():
        for flag in (True, False):
            with _phase_flag(flag), _calls(hip) as spy:
                stacked.stack_caches(model, 2)
                try:
                    stacked.set_masks(model, [_build_masks(m) for m in masks])
                    model.set_mode("sparse")
                    with stacked.edit_batch(model, 2):
                        for _ in range(3):
                            out = model(xe, t)
                    outs[("stacked", flag)] = out.clone()
                finally:
                    stacked.unstack_caches(model)
                model.set_compute_dtype("f16", keep=())
                try:
                    _, outs[("f16", flag)] = _sparse(model, x0, noise, t, small_masks()["interior"])
                finally:
                    model.set_compute_dtype("f32")
            assert not [c for c in spy.seen if c[0] == 2], spy.seen
    assert torch.equal(outs[("stacked", True)], outs[("stacked", False)])
    assert torch.equal(outs[("f16", True)], outs[("f16", False)])
    util.assert_finite(outs[("f16", True)], "f16 forward")
