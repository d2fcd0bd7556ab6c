"""On the MI355X: the Upsample conv's four 2x2 phase convs on the tile conv v3 (Gather.PHASE_UPSAMPLE_TILE3,
sige_hip_upsample_phase_tile3_nhwc).  The kernel in exact fp32 against fp64 of the 9-tap definition with the ORIGINAL weights and on
fp16 operands against fp64 of the rounded operands, what it leaves alone, its epilogue, the rows of a tile's own image under stacked
edits, what the entry point refuses, and the smallest network with two Upsamples against the CPU oracle -- one edit and two stacked.

Shapes.  A workgroup is 8 tiles x one phase x 64 output channels.  Low-res 6x5 -> 12x10: 3 x 3 hi-res tiles whose last row and column
hang over the image: 9 tiles (batch 1) are one full and one ragged workgroup, 18 (batch 2) have the batch boundary inside the second
workgroup and a ragged third; low-res 16x16 (64 tiles) is eight full workgroups.  Channels 64 -> 64 is one chunk (the prologue's two
stages hold the same chunk), 128 -> 64 both stages, 192 -> 128 an odd chunk count (the ring position across chunks) and two
output-channel blocks.  Every call runs with `min_blocks` = 1.
Bounds: exact fp32 against fp64, and fp16 operands against fp64 of the SAME rounded operands (exact products, fp32 accumulation): the
suite's 2e-5 * (1 + max |ref|); fp16 operands against the unrounded definition: sige_amd.tolerance's f16 criterion per element."""
import pytest
import torch
import torch.nn.functional as F

from tests import util
from tests.change_regions_common import small_masks
from tests.test_gpu_upsample_phases import _bound, _build_masks, _case, _cl, _covered, _err, _sparse, _tile_lists, hip, small  # noqa: F401
from tests.test_upsample_phases import phase_conv

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TEST = "upsample_phase_tile3"
MIN_ARG = 25  # position of `min_blocks` in sige_hip_upsample_phase_tile3_nhwc (include/sige_hip.h)


@pytest.fixture(autouse=True)
def min_blocks_one(hip):  # noqa: F811
    keep, hip.PHASE_TILE3_MIN_BLOCKS = hip.PHASE_TILE3_MIN_BLOCKS, 1
    yield
    hip.PHASE_TILE3_MIN_BLOCKS = keep


class _calls:
    """Spy on the new entry point: the status of every call inside the block."""

    def __init__(self, hip):  # noqa: F811
        self.lib, self.seen = hip.lib(), []

    def __enter__(self):
        self.real = self.lib.sige_hip_upsample_phase_tile3_nhwc

        def spy(*args):
            status = self.real(*args)
            self.seen.append(int(status))
            return status

        self.lib.sige_hip_upsample_phase_tile3_nhwc = spy
        return self

    def __exit__(self, *exc):
        self.lib.sige_hip_upsample_phase_tile3_nhwc = self.real
        return False


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.nn import Gather

        self.keep, Gather.PHASE_UPSAMPLE_TILE3 = Gather.PHASE_UPSAMPLE_TILE3, self.on

    def __exit__(self, *exc):
        from sige_amd.nn import Gather

        Gather.PHASE_UPSAMPLE_TILE3 = self.keep
        return False


def _launch(hip, x, w, b, idx, new, before, compute="f32", residual=None, out_affine=None, twins=None):  # noqa: F811
    """One call into a copy of `before`: the new form (`new`) or the 9-tap launch of the same call; returns (out, statuses seen).
    `_launch.kernels`: the library launches of that call (the weight packs come before it)."""
    cout = w.shape[0]
    H, W = 2 * x.shape[2], 2 * x.shape[3]
    wd = w.to(DEV)
    packed = hip.conv_pack_weights(wd, 6, 6, (1, 1), compute)
    assert packed.compute == compute
    p3 = hip.upsample_phase_tile3_pack(wd, compute) if new else None
    assert p3 is None or p3.compute == compute
    out = before.clone(memory_format=torch.channels_last)
    xd, idxd, bd = _cl(x), idx.to(DEV), None if b is None else b.to(DEV)
    n0 = hip.launch_count()
    with _calls(hip) as spy:
        got = hip.gather_conv_cl(xd, None, (6, 6), idxd, None, None, "identity", packed, bd, cout,
                                 (3, 3), (1, 1), full=dict(offset=(1, 1), out_res=(H, W), residual=residual), out_affine=out_affine,
                                 upsample2x=True, out=out, twins=twins, phase3=p3)
    _launch.kernels = hip.launch_count() - n0
    torch.cuda.synchronize()
    assert got is out
    return out, spy.seen


_SHAPES = [(64, 64, (6, 5), 1), (64, 64, (6, 5), 2), (128, 64, (6, 5), 1), (128, 64, (6, 5), 2), (192, 128, (6, 5), 1), (192, 128, (6, 5), 2),
           (64, 64, (16, 16), 1), (192, 128, (16, 16), 1)]
_RQ = {}


def _rounded_ref(cin, cout, batch, res):
    """fp64 of the four phase convs over x.half() and the phase kernels rounded to fp16: what the fp16 form computes, exactly."""
    from sige_amd import hip as h

    key = (cin, cout, batch, res)
    if key not in _RQ:
        x, w, b, _ = _case(cin, cout, batch, res)
        _RQ[key] = phase_conv(x.half().double(), h.upsample_phase_kernels(w).half().double(), b.double())
    return _RQ[key]


# ---- a. / d. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,res,batch", _SHAPES)
def test_fp32_kernel_vs_fp64_of_the_nine_tap_definition(hip, cin, cout, res, batch):  # noqa: F811
    x, w, b, ref = _case(cin, cout, batch, res)
    H, W = 2 * res[0], 2 * res[1]
    tol = _bound(ref)
    for name, idx in _tile_lists(H, W).items():
        if res == (16, 16) and name != "every":
            continue
        with util.poisoned(NAN):
            before = torch.empty(batch, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen = _launch(hip, x, w, b, idx, True, before)
            kernels = _launch.kernels
            old, seen_old = _launch(hip, x, w, b, idx, False, before)
        assert seen == [0] and seen_old == [], (name, seen, seen_old)
        inside = _covered(idx, H, W)
        g, o = got.cpu().double(), old.cpu().double()
        assert bool(torch.isnan(g[:, :, ~inside]).all()) and bool(torch.isnan(o[:, :, ~inside]).all()), name  # untouched cells
        if not bool(inside.any()):
            assert kernels == 0, (name, kernels)  # ("empty" launches nothing)
            continue
        assert kernels == 1, (name, kernels)
        err = util.record_margin(TEST, "f32 phase3 %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name), float((g - ref)[:, :, inside].abs().max()), tol)
        err_old = util.record_margin(TEST, "f32 9-tap %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name), float((o - ref)[:, :, inside].abs().max()), tol)
        print("%s f32 %3d/%3d %s B%d %-8s phase3 %.3e  9-tap %.3e  bound %.3e" % (TEST, cin, cout, res, batch, name, err, err_old, tol), flush=True)
        assert err <= tol and err_old <= tol, (name, err, err_old, tol)


@pytest.mark.parametrize("cin,cout,res,batch", _SHAPES)
def test_fp16_operands_vs_fp64_of_the_rounded_operands_and_the_f16_criterion(hip, cin, cout, res, batch):  # noqa: F811
    from sige_amd.tolerance import f16_check

    x, w, b, ref = _case(cin, cout, batch, res)
    refq = _rounded_ref(cin, cout, batch, res)
    H, W = 2 * res[0], 2 * res[1]
    tol = _bound(refq)
    for name, idx in _tile_lists(H, W).items():
        if res == (16, 16) and name != "every":
            continue
        with util.poisoned(NAN):
            before = torch.empty(batch, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen = _launch(hip, x, w, b, idx, True, before, compute="f16")
        assert seen == [0], (name, seen)
        inside = _covered(idx, H, W)
        g = got.cpu().double()
        assert bool(torch.isnan(g[:, :, ~inside]).all()), name
        if not bool(inside.any()):
            continue
        err = util.record_margin(TEST, "f16 phase3 vs rounded operands %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name),
                                 float((g - refq)[:, :, inside].abs().max()), tol)
        chk = f16_check(got.cpu()[:, :, inside], ref[:, :, inside])
        util.record_margin(TEST, "f16 phase3 worst / allowed %d/%d %dx%d B%d %s" % (cin, cout, *res, batch, name), chk["worst_over_allowed"], 1.0)
        print("%s f16 %3d/%3d %s B%d %-8s vs rounded %.3e bound %.3e  criterion %s" % (TEST, cin, cout, res, batch, name, err, tol, chk), flush=True)
        assert err <= tol, (name, err, tol)
        assert chk["ok"], (name, chk)


# ---- b. what the launch leaves alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
def test_cells_outside_the_list_keep_their_bits(hip, with_bias):  # noqa: F811
    x, w, b, ref = _case(64, 64, 2, (6, 5), with_bias)
    idx = _tile_lists(12, 10)["holes"]
    before = _cl(torch.randn(2, 64, 12, 10, generator=torch.Generator().manual_seed(7)))
    got, seen = _launch(hip, x, w, b, idx, True, before)
    assert seen == [0]
    inside = _covered(idx, 12, 10)
    assert torch.equal(got[:, :, ~inside.to(DEV)], before[:, :, ~inside.to(DEV)])
    err = util.record_margin(TEST, "holes, bias %s" % with_bias, float((got.cpu().double() - ref)[:, :, inside].abs().max()), _bound(ref))
    assert err <= _bound(ref), err


# ---- c. the epilogue ---------------------------------------------------------------------------------------------------------------
def test_twins_out_affine_and_residual_as_the_nine_tap_form(hip):  # noqa: F811
    """Both twins, the out-affine with SiLU and a residual in one launch: each output against fp64 and against the 9-tap launch."""
    x, w, b, ref = _case(128, 64, 2, (6, 5))
    gen = torch.Generator().manual_seed(9)
    idx = _tile_lists(12, 10)["every"]
    res = torch.randn(2, 64, 12, 10, generator=gen)
    vec = lambda: (0.5 + torch.rand(64, generator=gen), torch.randn(64, generator=gen))  # noqa: E731
    (os_, oh_), (s0, t0), (s1, t1) = vec(), vec(), vec()
    v = ref + res.double()
    bc = lambda t: t.double().reshape(1, -1, 1, 1)  # noqa: E731
    wants = {"out": F.silu(bc(os_) * v + bc(oh_)), "twin0": F.silu(bc(s0) * v + bc(t0)), "twin1": F.silu(bc(s1) * v + bc(t1))}
    outs = {}
    for new in (True, False):
        with util.poisoned(NAN):
            tw = [torch.empty(2, 64, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last) for _ in range(2)]
            before = torch.empty(2, 64, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last)
            out, seen = _launch(hip, x, w, b, idx, new, before, residual=_cl(res), out_affine=(os_.to(DEV), oh_.to(DEV), "swish"),
                                twins=[(tw[0], s0.to(DEV), t0.to(DEV)), (tw[1], s1.to(DEV), t1.to(DEV))])
        assert seen == ([0] if new else [])
        outs[new] = {"out": out, "twin0": tw[0], "twin1": tw[1]}
    for name, want in wants.items():
        tol = _bound(v)  # (SiLU and a scale of at most 1.5 on v: the conv's bound on the pre-activation carries over)
        for new in (True, False):
            err = util.record_margin(TEST, "%s %s" % (name, "phase3" if new else "9-tap"), _err(outs[new][name], want), tol)
            assert err <= tol, (name, new, err)
        assert _err(outs[True][name], outs[False][name]) <= tol


# ---- e. stacked edits: a tile reads the rows of its own image ---------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "f16"])
def test_seam_rows_of_another_image_are_padding(hip, compute):  # noqa: F811
    from sige_amd.tolerance import f16_check

    gen = torch.Generator().manual_seed(21)
    cin, cout = 128, 64
    xs = [c + 0.25 * torch.randn(1, cin, 8, 5, generator=gen) for c in (1.5, -2.0)]  # (different constants: a row read across the seam shows)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=gen)
    nine = lambda t: F.conv2d(F.interpolate(t.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)  # noqa: E731
    ref = torch.cat([nine(t) for t in xs], 2)  # [1,cout,32,10]: the per-image conv, stacked
    if compute == "f16":
        wq = hip.upsample_phase_kernels(w).half().double()
        want = torch.cat([phase_conv(t.half().double(), wq, b.double()) for t in xs], 2)
    else:
        want = ref
    x = torch.cat(xs, 2)
    idx = _tile_lists(32, 10)["every"]
    rows = set(idx[:, 0].tolist())
    assert 11 in rows and 15 in rows  # the last tile row of image 0 and the first of image 1
    hip.set_edit_batch(2)
    try:
        with util.poisoned(NAN):
            before = torch.empty(1, cout, 32, 10, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen = _launch(hip, x, w, b, idx, True, before, compute=compute)
    finally:
        hip.set_edit_batch(1)
    assert seen == [0]
    tol = _bound(want)
    err = util.record_margin(TEST, "seam %s" % compute, _err(got, want), tol)
    print("%s seam %s err %.3e bound %.3e" % (TEST, compute, err, tol), flush=True)
    assert err <= tol, (err, tol)
    if compute == "f16":
        chk = f16_check(got, ref)
        assert chk["ok"], chk


# ---- f. refusals --------------------------------------------------------------------------------------------------------------------
def test_what_the_entry_point_does_not_cover_is_refused_and_touches_nothing(hip):  # noqa: F811
    x, w, b, ref = _case(64, 64, 1, (6, 5))
    idx = _tile_lists(12, 10)["every"].to(DEV)
    wd, bd = w.to(DEV), b.to(DEV)
    xd = _cl(torch.randn(1, 128, 6, 5, generator=torch.Generator().manual_seed(4)))  # (128 channels: every refused C fits inside)
    p3 = hip.upsample_phase_tile3_pack(wd, "f32")
    assert hip.upsample_phase_tile3_pack(torch.zeros(48, 64, 3, 3, device=DEV)) is None
    assert hip.upsample_phase_tile3_pack(torch.zeros(64, 96, 3, 3, device=DEV)) is None
    before = _cl(torch.randn(1, 64, 12, 10, generator=torch.Generator().manual_seed(5)))
    out = before.clone(memory_format=torch.channels_last)
    L = hip.lib()
    grid = 2 * 1 * 4  # ceil(9 / 8) x (64 / 64) x 4 phases
    args = [0, xd.data_ptr(), 1, 64, 12, 10, idx.data_ptr(), idx.shape[0], p3.data_ptr(), bd.data_ptr(), 64, 1, 1, None, 12, 10,
            None, None, 0, None, None, None, None, None, None, grid, out.data_ptr(), None]
    assert len(args) == 28 and args[MIN_ARG] == grid

    def refused(**change):
        bad = list(args)
        for k, v in change.items():
            bad[int(k[1:])] = v
        status = L.sige_hip_upsample_phase_tile3_nhwc(*bad)
        torch.cuda.synchronize()
        return status == hip.UNSUPPORTED and torch.equal(out, before)

    assert refused(a3=96)             # C
    assert refused(a10=48)            # Cout
    assert refused(a0=2)              # compute
    assert refused(a4=11)             # odd H
    assert refused(a11=0)             # an even offset: the output blocks would not start on even pixels
    assert refused(a25=grid + 1)      # one above the call's grid
    assert refused(a25=0)
    n0 = hip.launch_count()
    assert L.sige_hip_upsample_phase_tile3_nhwc(*args) == 0   # (the grid itself runs)
    torch.cuda.synchronize()
    assert hip.launch_count() - n0 == 1 and not torch.equal(out, before)
    empty = list(args)
    empty[7] = 0
    assert L.sige_hip_upsample_phase_tile3_nhwc(*empty) == 0 and hip.launch_count() - n0 == 1  # N = 0: success, no launch

    # through the binding: a refused call is the call that never had the pack, bit for bit
    packed = hip.conv_pack_weights(wd, 6, 6, (1, 1), "f32")
    x64 = _cl(x)
    full = dict(offset=(1, 1), out_res=(12, 10), residual=None)
    hip.PHASE_TILE3_MIN_BLOCKS = grid + 1
    outs = {}
    for pk in (p3, None):
        with _calls(hip) as spy:
            outs[pk is None] = hip.gather_conv_cl(x64, None, (6, 6), idx, None, None, "identity", packed, bd, 64, (3, 3), (1, 1), full=full,
                                                  upsample2x=True, phase3=pk)
        assert spy.seen == ([hip.UNSUPPORTED] if pk is not None else []), spy.seen
    assert torch.equal(outs[False], outs[True])
    # a gather affine and a tile destination never reach the entry point
    hip.PHASE_TILE3_MIN_BLOCKS = 1
    sc, sh = (0.5 + torch.rand(1, 64, 1, 1)).to(DEV), torch.randn(1, 64, 1, 1).to(DEV)
    with _calls(hip) as spy:
        hip.gather_conv_cl(x64, None, (6, 6), idx, sc, sh, "swish", packed, bd, 64, (3, 3), (1, 1), full=full, upsample2x=True, phase3=p3)
        hip.gather_conv_cl(x64, None, (6, 6), idx, None, None, "identity", packed, bd, 64, (3, 3), (1, 1), upsample2x=True, phase3=p3)
    assert spy.seen == []
    torch.cuda.synchronize()


def test_the_derived_pack_of_a_conv_on_the_gpu(hip):  # noqa: F811
    from sige_amd.nn.base import SIGEConv2d

    for conv in (SIGEConv2d(64, 64, 1), SIGEConv2d(64, 64, 3, stride=2, padding=1), SIGEConv2d(64, 64, 3, padding=0),
                 SIGEConv2d(64, 64, 3, padding=1, groups=2), SIGEConv2d(48, 64, 3, padding=1)):
        assert conv.to(DEV).phase_tile3_packed() is None
    conv = SIGEConv2d(64, 128, 3, padding=1).to(DEV)
    keys = set(conv.state_dict())
    p = conv.phase_tile3_packed()
    assert p is not None and p.compute == "f32" and conv.phase_tile3_packed() is p and conv._phase is None
    assert torch.equal(p, hip.upsample_phase_tile3_pack(conv.weight, "f32"))
    with torch.no_grad():
        conv.weight.mul_(2.0)
    conv.rebuild_derived_caches()  # rewritten in place: a captured graph keeps reading the same address
    p2 = conv.phase_tile3_packed()
    assert p2 is p and torch.equal(p2, hip.upsample_phase_tile3_pack(conv.weight, "f32"))
    conv.compute_dtype = "f16"
    ph = conv.phase_tile3_packed()
    assert ph is not p and ph.compute == "f16" and ph.numel() * 2 < p.numel() + 9 * 4096
    conv.compute_dtype = "f16x3"
    assert conv.phase_tile3_packed() is None
    conv.clear_cache()
    assert conv._phase3 is None and set(conv.state_dict()) == keys
    torch.cuda.synchronize()


# ---- g. the small network: two Upsamples (256 ch 16 -> 32, 128 ch 32 -> 64) ---------------------------------------------------------
@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_small_network_switch_on_vs_oracle_and_switch_off_is_todays_forward(hip, small, name):  # noqa: F811
    model, x0, noise, t, wants = small
    mask = small_masks()[name]
    with torch.no_grad():
        with _flag(True), _calls(hip) as on:
            _, got = _sparse(model, x0, noise, t, mask, forwards=1)
        with _flag(False), _calls(hip) as off:
            _, old = _sparse(model, x0, noise, t, mask, forwards=1)
        real = hip.gather_conv_cl
        hip.gather_conv_cl = lambda *a, **k: real(*a, **{kk: v for kk, v in k.items() if kk != "phase3"})
        try:
            with _flag(True), _calls(hip) as stripped:
                _, parent = _sparse(model, x0, noise, t, mask, forwards=1)
        finally:
            hip.gather_conv_cl = real
    assert on.seen == [0, 0], on.seen           # both Upsamples, neither refused
    assert off.seen == [] and stripped.seen == []
    assert torch.equal(old, parent)
    err = util.record_margin(TEST, "small %s switch on vs oracle" % name, _err(got, wants[name]), util.CONV_ATOL)
    print("%s small %-8s on %.3e on-off %.3e" % (TEST, name, err, _err(got, old)), flush=True)
    assert err <= util.CONV_ATOL, err


def test_small_network_launch_count_and_graph_replay(hip, small):  # noqa: F811
    import bench

    model, x0, noise, t, _ = small
    counts = {}
    with torch.no_grad():
        for on in (True, False):
            with _flag(on):
                x1, _ = _sparse(model, x0, noise, t, small_masks()["interior"])
                n0 = hip.launch_count()
                model(x1, t)
                counts[on] = hip.launch_count() - n0
        assert counts[True] == counts[False] > 0, counts
        with _flag(True):
            x1, want = _sparse(model, x0, noise, t, small_masks()["interior"])
            g, out = bench.capture(model, x1, t)
            for _ in range(2):
                g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), _err(out, want)
            del g, out


def test_small_network_f16_compute(hip, small):  # noqa: F811
    from sige_amd.tolerance import f16_check

    model, x0, noise, t, wants = small
    with torch.no_grad():
        model.set_compute_dtype("f16", keep=())
        try:
            with _flag(True), _calls(hip) as on:
                _, got = _sparse(model, x0, noise, t, small_masks()["interior"], forwards=1)
        finally:
            model.set_compute_dtype("f32")
    assert on.seen == [0, 0], on.seen
    chk = f16_check(got, wants["interior"])
    util.record_margin(TEST, "small interior f16 worst / allowed", chk["worst_over_allowed"], 1.0)
    assert chk["ok"], chk


# ---- h. the small network, two stacked edits ---------------------------------------------------------------------------------------
def test_small_network_stacked_edits(hip, small):  # noqa: F811
    from sige_amd import stacked

    model, x0, noise, t, wants = small
    names = ["interior", "corner"]
    masks = [small_masks()[n].to(DEV) for n in names]
    xe = _cl(torch.cat([x0 + noise * m for m in masks], 0))
    outs, seen = {}, {}
    with torch.no_grad():
        for on in (True, False):
            with _flag(on), _calls(hip) as spy:
                stacked.stack_caches(model, 2)
                try:
                    stacked.set_masks(model, [_build_masks(m) for m in masks])
                    model.set_mode("sparse")
                    with stacked.edit_batch(model, 2):
                        out = model(xe, t)
                    outs[on] = out.clone()
                finally:
                    stacked.unstack_caches(model)
            seen[on] = spy.seen
        # today's stacked forward: the same module code with the pack never handed to the binding
        real = hip.gather_conv_cl
        hip.gather_conv_cl = lambda *a, **k: real(*a, **{kk: v for kk, v in k.items() if kk != "phase3"})
        try:
            with _flag(True):
                stacked.stack_caches(model, 2)
                try:
                    stacked.set_masks(model, [_build_masks(m) for m in masks])
                    model.set_mode("sparse")
                    with stacked.edit_batch(model, 2):
                        parent = model(xe, t).clone()
                finally:
                    stacked.unstack_caches(model)
        finally:
            hip.gather_conv_cl = real
    assert seen[True] == [0, 0] and seen[False] == [], seen
    assert torch.equal(outs[False], parent)
    for e, n in enumerate(names):
        err = util.record_margin(TEST, "stacked E=2 edit %d (%s) vs its single-forward oracle" % (e, n), _err(outs[True][e], wants[n][0]), util.CONV_ATOL)
        print("%s stacked edit %d %-8s %.3e" % (TEST, e, n, err), flush=True)
        assert err <= util.CONV_ATOL, (n, err)
