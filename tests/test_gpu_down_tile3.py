"""On the MI355X: the 3x3 / stride-2 Downsample conv on the tile conv v3, fp16 operands (Gather.DOWNSAMPLE_TILE3,
sige_hip_down_tile3_nhwc).  The kernel against fp64 of the nine-tap definition -- of the operands rounded to fp16 at the exact-fp32
bound, of the unrounded operands at the f16 criterion --, what it leaves alone, its epilogue, the rows of a tile's own image under
stacked edits, what the entry point refuses, and the small SD VAE encoder in f16 mode against the CPU oracle.

Shapes.  A workgroup is 8 tiles x 64 output channels.  20x28 and 36x20 images: 5 x 7 and 9 x 5 windows of 5x5 whose last row and
column (offset 0: origins 4i, the (0,1,0,1) padding) or first row and column (offset -1: origins 4i - 1, padding 1) leave the image.
Lists of 1 tile, 11 tiles (one full and one ragged workgroup; batch 2: the batch boundary inside the third) and every tile.
64 -> 64 channels is one chunk and one output block, 128 -> 192 two chunks (the weight ring across chunks) and three output blocks."""
import pytest
import torch
import torch.nn.functional as F

from tests import util
from tests.test_gpu_upsample_phases import _bound, _cl, _err, hip  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TEST = "down_tile3"
MIN_ARG = 25  # position of `min_blocks` in sige_hip_down_tile3_nhwc (include/sige_hip.h)


@pytest.fixture(autouse=True)
def min_blocks_one(hip):  # noqa: F811
    keep, hip.DOWN_TILE3_MIN_BLOCKS_F16 = hip.DOWN_TILE3_MIN_BLOCKS_F16, 1
    yield
    hip.DOWN_TILE3_MIN_BLOCKS_F16 = keep


class _calls:
    """Spy on the new entry point: the status of every call inside the block."""

    def __init__(self, hip):  # noqa: F811
        self.lib, self.seen = hip.lib(), []

    def __enter__(self):
        self.real = self.lib.sige_hip_down_tile3_nhwc

        def spy(*args):
            status = self.real(*args)
            self.seen.append(int(status))
            return status

        self.lib.sige_hip_down_tile3_nhwc = spy
        return self

    def __exit__(self, *exc):
        self.lib.sige_hip_down_tile3_nhwc = self.real
        return False


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.nn import Gather

        self.keep, Gather.DOWNSAMPLE_TILE3 = Gather.DOWNSAMPLE_TILE3, self.on

    def __exit__(self, *exc):
        from sige_amd.nn import Gather

        Gather.DOWNSAMPLE_TILE3 = self.keep
        return False


def _nine_tap(x, w, b, off):
    """The definition in fp64: offset 0 = zero padding (0,1,0,1), offset -1 = padding 1; stride 2."""
    xp = F.pad(x.double(), (0, 1, 0, 1) if off == 0 else (1, 1, 1, 1))
    return F.conv2d(xp, w.double(), None if b is None else b.double(), stride=2)


_CASES = {}


def _case(cin, cout, batch, res, off, with_bias=True):
    """Inputs, the fp64 truth and the fp64 truth of the operands rounded to fp16 (RNE), computed once and left unchanged."""
    key = (cin, cout, batch, res, off, with_bias)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * cin + cout + 10 * batch - off)
        x = torch.randn(batch, cin, *res, generator=gen)
        w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
        b = torch.randn(cout, generator=gen) if with_bias else None
        _CASES[key] = (x, w, b, _nine_tap(x, w, b, off), _nine_tap(x.half(), w.half(), b, off))
    return _CASES[key]


def _tile_lists(H, W, off):
    gh, gw = (H + 3) // 4, (W + 3) // 4
    every = [(i, j) for i in range(gh) for j in range(gw)]
    lists = {"one": [(gh // 2, gw // 2)], "eleven": every[:5] + every[-6:], "every": every,
             "holes": [c for k, c in enumerate(every) if k % 2 == 0 and k != 4]}
    return {n: torch.tensor([(4 * i + off, 4 * j + off) for i, j in c], dtype=torch.int32).reshape(-1, 2) for n, c in lists.items()}


def _covered(idx, off, Ho, Wo):
    m = torch.zeros(Ho, Wo, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[(h0 - off) // 2:(h0 - off) // 2 + 2, (w0 - off) // 2:(w0 - off) // 2 + 2] = True
    return m


def _launch(hip, x, w, b, idx, off, before, residual=None, out_affine=None, twins=None):  # noqa: F811
    """One call with the pack into a copy of `before`; returns (out, statuses the new entry point gave, library launches)."""
    wd = w.to(DEV)
    packed = hip.conv_pack_weights(wd, 5, 5, (2, 2), "f16")
    assert packed.compute == "f32"  # (this geometry's tile pack stays exact fp32: the fallback of a refused call)
    d3 = hip.down_tile3_pack(wd)
    assert d3.compute == "f16"
    out = before.clone(memory_format=torch.channels_last)
    xd, idxd, bd = _cl(x), idx.to(DEV), None if b is None else b.to(DEV)
    n0 = hip.launch_count()
    with _calls(hip) as spy:
        got = hip.gather_conv_cl(xd, None, (5, 5), idxd, None, None, "identity", packed, bd, w.shape[0], (3, 3), (2, 2),
                                 full=dict(offset=(-off, -off), out_res=tuple(before.shape[2:]), residual=residual),
                                 out_affine=out_affine, out=out, twins=twins, down3=d3)
    n = hip.launch_count() - n0
    torch.cuda.synchronize()
    assert got is out
    return out, spy.seen, n


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, -1])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("res", [(20, 28), (36, 20)])
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 192)])
def test_kernel_vs_fp64_of_the_rounded_operands_and_the_f16_criterion(hip, cin, cout, res, batch, off):  # noqa: F811
    from sige_amd.tolerance import f16_check

    x, w, b, ref, refq = _case(cin, cout, batch, res, off)
    Ho, Wo = ref.shape[2:]
    assert (Ho, Wo) == (res[0] // 2, res[1] // 2)
    tol = _bound(refq)
    emu = f16_check(refq, ref)  # (the emulation itself against the unrounded truth, on the CPU)
    util.record_margin(TEST, "emulation worst / allowed %d/%d %dx%d B%d off %d" % (cin, cout, *res, batch, off), emu["worst_over_allowed"], 1.0)
    assert emu["ok"], emu
    for name in ("one", "eleven", "every"):
        idx = _tile_lists(*res, off)[name]
        with util.poisoned(NAN):
            before = torch.empty(batch, cout, Ho, Wo, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen, launches = _launch(hip, x, w, b, idx, off, before)
        assert seen == [0] and launches == 1, (name, seen, launches)
        inside = _covered(idx, off, Ho, Wo)
        g = got.cpu().double()
        assert bool(torch.isnan(g[:, :, ~inside]).all()), name  # untouched cells
        what = "%d/%d %dx%d B%d off %d %s" % (cin, cout, *res, batch, off, name)
        err = util.record_margin(TEST, "vs rounded operands " + what, float((g - refq)[:, :, inside].abs().max()), tol)
        chk = f16_check(got.cpu()[:, :, inside], ref[:, :, inside])
        util.record_margin(TEST, "worst / allowed " + what, chk["worst_over_allowed"], 1.0)
        print("%s %s vs rounded %.3e bound %.3e  criterion %s" % (TEST, what, err, tol, chk), flush=True)
        assert err <= tol, (name, err, tol)
        assert chk["ok"], (name, chk)


# ---- 2. what the launch leaves alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
def test_cells_outside_the_list_keep_their_bits(hip, with_bias):  # noqa: F811
    x, w, b, ref, refq = _case(64, 64, 2, (20, 28), 0, with_bias)
    idx = _tile_lists(20, 28, 0)["holes"]
    before = _cl(torch.randn(2, 64, 10, 14, generator=torch.Generator().manual_seed(7)))
    got, seen, _ = _launch(hip, x, w, b, idx, 0, before)
    assert seen == [0]
    inside = _covered(idx, 0, 10, 14)
    assert torch.equal(got[:, :, ~inside.to(DEV)], before[:, :, ~inside.to(DEV)])
    err = util.record_margin(TEST, "holes, bias %s" % with_bias, float((got.cpu().double() - refq)[:, :, inside].abs().max()), _bound(refq))
    assert err <= _bound(refq), err


# ---- 3. the epilogue ------------------------------------------------------------------------------------------------------------------
def test_residual_out_affine_and_both_twins(hip):  # noqa: F811
    x, w, b, _, refq = _case(128, 64, 2, (20, 28), -1)
    gen = torch.Generator().manual_seed(9)
    idx = _tile_lists(20, 28, -1)["every"]
    res = torch.randn(2, 64, 10, 14, generator=gen)
    vec = lambda: (0.5 + torch.rand(64, generator=gen), torch.randn(64, generator=gen))  # noqa: E731
    (os_, oh_), (s0, t0), (s1, t1) = vec(), vec(), vec()
    v = refq + res.double()
    bc = lambda t: t.double().reshape(1, -1, 1, 1)  # noqa: E731
    wants = {"out": F.silu(bc(os_) * v + bc(oh_)), "twin0": F.silu(bc(s0) * v + bc(t0)), "twin1": F.silu(bc(s1) * v + bc(t1))}
    with util.poisoned(NAN):
        tw = [torch.empty(2, 64, 10, 14, device=DEV).contiguous(memory_format=torch.channels_last) for _ in range(2)]
        before = torch.empty(2, 64, 10, 14, device=DEV).contiguous(memory_format=torch.channels_last)
        out, seen, _ = _launch(hip, x, w, b, idx, -1, before, residual=_cl(res), out_affine=(os_.to(DEV), oh_.to(DEV), "swish"),
                               twins=[(tw[0], s0.to(DEV), t0.to(DEV)), (tw[1], s1.to(DEV), t1.to(DEV))])
    assert seen == [0]
    tol = _bound(v)  # (SiLU and a scale of at most 1.5 on v: the conv's bound on the pre-activation carries over)
    for name, got in (("out", out), ("twin0", tw[0]), ("twin1", tw[1])):
        err = util.record_margin(TEST, "epilogue " + name, _err(got, wants[name]), tol)
        assert err <= tol, (name, err, tol)


# ---- 4. stacked edits: a tile reads the rows of its own image -------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, -1])
def test_seam_rows_of_another_image_are_padding(hip, off):  # noqa: F811
    from sige_amd.tolerance import f16_check

    gen = torch.Generator().manual_seed(21 - off)
    cin, cout = 128, 64
    xs = [c + 0.25 * torch.randn(1, cin, 16, 12, generator=gen) for c in (1.5, -2.0)]  # (different constants: a row read across the seam shows)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=gen)
    ref = torch.cat([_nine_tap(t, w, b, off) for t in xs], 2)  # [1,cout,16,6]: the per-image conv, stacked
    want = torch.cat([_nine_tap(t.half(), w.half(), b, off) for t in xs], 2)
    idx = _tile_lists(32, 12, off)["every"]
    rows = set(idx[:, 0].tolist())
    assert 12 + off in rows and 16 + off in rows  # the last tile row of image 0 and the first of image 1
    hip.set_edit_batch(2)
    try:
        with util.poisoned(NAN):
            before = torch.empty(1, cout, 16, 6, device=DEV).contiguous(memory_format=torch.channels_last)
            got, seen, _ = _launch(hip, torch.cat(xs, 2), w, b, idx, off, before)
    finally:
        hip.set_edit_batch(1)
    assert seen == [0]
    tol = _bound(want)
    err = util.record_margin(TEST, "seam off %d" % off, _err(got, want), tol)
    print("%s seam off %d err %.3e bound %.3e" % (TEST, off, err, tol), flush=True)
    assert err <= tol, (err, tol)
    chk = f16_check(got, ref)
    assert chk["ok"], chk


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_what_the_entry_point_does_not_cover_is_refused_and_touches_nothing(hip):  # noqa: F811
    x, w, b, _, _ = _case(64, 64, 1, (20, 28), 0)
    idx = _tile_lists(20, 28, 0)["every"].to(DEV)
    wd, bd = w.to(DEV), b.to(DEV)
    xd = _cl(torch.randn(1, 128, 20, 28, generator=torch.Generator().manual_seed(4)))  # (128 channels: every refused C fits inside)
    d3 = hip.down_tile3_pack(wd)
    assert hip.down_tile3_pack(torch.zeros(48, 64, 3, 3, device=DEV)) is None
    assert hip.down_tile3_pack(torch.zeros(64, 96, 3, 3, device=DEV)) is None
    sentinel = torch.full((1, 64, 10, 14), 0x7FC0DEAD, dtype=torch.int32, device=DEV).contiguous(memory_format=torch.channels_last)
    out = sentinel.clone(memory_format=torch.channels_last).view(torch.float32)
    L = hip.lib()
    grid = 5  # ceil(35 / 8) x (64 / 64)
    args = [1, xd.data_ptr(), 1, 64, 20, 28, idx.data_ptr(), idx.shape[0], d3.data_ptr(), bd.data_ptr(), 64, 0, 0, None, 10, 14,
            None, None, 0, None, None, None, None, None, None, grid, out.data_ptr(), None]
    assert len(args) == 28 and args[MIN_ARG] == grid

    def refused(**change):
        bad = list(args)
        for k, v in change.items():
            bad[int(k[1:])] = v
        status = L.sige_hip_down_tile3_nhwc(*bad)
        torch.cuda.synchronize()
        return status == hip.UNSUPPORTED and torch.equal(out.view(torch.int32), sentinel)

    assert refused(a0=0) and refused(a0=2)   # compute: exact fp32 and f16x3 stay on conv_mfma.hpp
    assert refused(a3=96)                    # C
    assert refused(a10=96)                   # Cout
    assert refused(a25=grid + 1)             # one above the call's grid
    assert refused(a25=0)
    assert refused(a1=xd.data_ptr() + 4)     # a pointer off 16 bytes
    assert refused(a26=out.data_ptr() + 8)
    hip.set_edit_batch(4)                    # a stacked height that does not stack: 20 rows are no four images of 2^k
    try:
        assert refused()
    finally:
        hip.set_edit_batch(1)
    n0 = hip.launch_count()
    assert L.sige_hip_down_tile3_nhwc(*args) == 0  # (the grid itself runs)
    torch.cuda.synchronize()
    assert hip.launch_count() - n0 == 1 and not torch.equal(out.view(torch.int32), sentinel)
    # through the binding: a refused call is the call that never had the pack, bit for bit
    packed = hip.conv_pack_weights(wd, 5, 5, (2, 2), "f16")
    full = dict(offset=(0, 0), out_res=(10, 14), residual=None)
    hip.DOWN_TILE3_MIN_BLOCKS_F16 = grid + 1
    outs = {}
    for pk in (d3, None):
        with _calls(hip) as spy:
            outs[pk is None] = hip.gather_conv_cl(_cl(x), None, (5, 5), idx, None, None, "identity", packed, bd, 64, (3, 3), (2, 2), full=full, down3=pk)
        assert spy.seen == ([hip.UNSUPPORTED] if pk is not None else []), spy.seen
    assert torch.equal(outs[False], outs[True])
    torch.cuda.synchronize()


# ---- 6. the small SD VAE encoder in f16 mode: its 64 -> 64 Downsample takes the new launch -------------------------------------------
def test_small_vae_encoder_switch_on_vs_oracle_launches_graph_and_switch_off(hip):  # noqa: F811
    from tests import test_gpu_sd_vae_f16 as V

    cfg, size = V.SMALL["encoder"]
    model, fns, x0, x1, masks = V._setup("encoder", cfg, size, "f16")
    V._forwards(model, fns, x0, x1, masks)  # (the one full pass, masks, a first sparse forward: packs and buffers)
    with torch.no_grad():
        off_before = V._sparse(model, fns, x1)
        n0 = hip.launch_count()
        model(x1)
        n_off = hip.launch_count() - n0
        with _flag(True):
            with _calls(hip) as on:
                got = V._sparse(model, fns, x1)
            n0 = hip.launch_count()
            model(x1)
            n_on = hip.launch_count() - n0
            eager = model(x1).clone()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model(x1)
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
            del graph
        with _calls(hip) as off:
            off_after = V._sparse(model, fns, x1)
    assert on.seen == [0, 0], on.seen  # (model and moments: the 64-channel Downsample each time; the 32-channel one has no pack)
    assert off.seen == []
    assert n_on == n_off > 0, (n_on, n_off)
    for name in sorted(got):
        util.assert_finite(got[name], name)
        assert not torch.equal(got[name], off_before[name]), "%s: the switch changed nothing" % name
        assert torch.equal(off_after[name], off_before[name]), "%s: switch off again is not the forward before the flip" % name
        V._inside_bound("down_tile3", "encoder", name, got[name])


def test_small_vae_encoder_stacked_edits(hip):  # noqa: F811
    from sige_amd import stacked
    from tests import test_gpu_sd_vae_f16 as V
    from tests import test_gpu_sd_vae_stacked as S
    from tests import vae_f16

    E = 2
    want = S.oracle_outputs("encoder")
    model, run = S.build("encoder", DEV, True, True)
    model.set_compute_dtype("f16")
    pyrs = S.pyramids("encoder", DEV)[:E]
    x0, edits, noise = S.edit_inputs("encoder", pyrs, DEV)
    x0, xs, ns = S._fmt(x0, True), S._fmt(torch.cat(edits[:E], 0), True), torch.cat(noise[:E], 0)
    with torch.no_grad(), _flag(True):
        model.set_mode("full")
        run(x0, noise[0])
        model.set_mode("sparse")
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                run(xs, ns)
                with _calls(hip) as spy, util.poisoned():
                    got = run(xs, ns).clone()
        finally:
            stacked.unstack_caches(model)
    assert spy.seen == [0], spy.seen
    ref, emu = V._oracle("encoder")
    e16 = vae_f16.err(emu["sparse_moments"], ref["sparse_moments"])
    for e in range(E):
        tol = vae_f16.bound(want[e], e16)
        err = util.record_margin(TEST, "stacked E=2 edit %d vs oracle" % e, float((got[e].cpu() - want[e]).abs().max()), tol)
        assert err <= tol, (e, err, tol)
