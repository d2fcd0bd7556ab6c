"""On the MI355X: the 6x6 form of the tile conv v3 (csrc/conv_tile3.hpp: Tile3Geo<2>, exact fp32 and fp16 operands) -- the kernel the
forward routes to from hip.TILE3_MIN_BLOCKS workgroups on -- against fp64 convs of the CPU oracle's tiles on a ragged image, as
tests/test_gpu_tile_conv_block10.py pins the 10x10 form.

Shapes (tests/tile3_common.py).  Image 18x26, neither a multiple of the 4-pixel stride: origins (4i - 1, 4j - 1) on a 5x7 grid, the
last row of windows writes rows 16..19 of 18, the last column 24..27 of 26.  Lists: `every` (35 tiles, odd: the last workgroup
holds ONE tile; at B = 2 one workgroup holds image 0's last tile and image 1's first), `corners`, `interior`, `holes` (23),
`empty`, and `every34` (even: a per-batch affine needs whole tile pairs per image; on `every` it is refused).  (C1, C2, Cout) =
(64, 0, 64): one chunk; (128, 0, 64): two chunks, both stages and ring parities; (64, 0, 128): two output blocks; 64 + 64: the
fused cat.  A launch is at most 36 workgroups.

Every positive case runs inside `_v3`: hip.TILE3 = True, and the block fails unless hip.tile_conv3_cl launched exactly once and
the library counted exactly one launch -- a refused call that falls back to conv_mfma.hpp cannot pass.

Bounds.  Exact fp32: the suite's 2e-5 * (1 + max |ref|) on every element, against an fp64 conv of the oracle's tiles.  fp16
operands with raw staging: the operand rounding is exactly .half(), the same bound against an fp64 conv of the fp16-rounded tiles
and weights.  fp16 operands behind an affine / SiLU: |d| <= 3e-4 (1 + |want|) for all but 1e-3 of the elements (a staged value
next to a rounding boundary may round the other way; tests/test_tile_conv3_block6_inputs.py holds the reference alone to 1e-4).
Outputs are allocated NaN-poisoned and checked finite; pixels no tile covers are compared bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from tests import tile3_common as T
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = T.H, T.W


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _d(t):
    return None if t is None else t.to(DEV)


def _no_tiles(C):
    return torch.zeros((0, C, 4, 4), device=DEV).contiguous(memory_format=torch.channels_last)


_WORST = {}


@pytest.fixture(autouse=True)
def _margins(request):
    """The worst err / bound of the test's checks goes to the margin file (util.record_margin)."""
    _WORST.clear()
    yield
    if _WORST:
        util.record_margin("tile_conv3_block6", "%s: %s" % (request.node.name, _WORST["what"]), _WORST["err"], _WORST["tol"])


def _note(what, err, tol):
    if tol > 0 and (not _WORST or err / tol > _WORST["err"] / _WORST["tol"]):
        _WORST.update(what=what, err=err, tol=tol)


def _check(got, want, what):
    util.assert_finite(got, what)
    err = float((got.detach().double().cpu() - want.double()).abs().max()) if got.numel() else 0.0
    tol = T.bound(want)
    print("tile3 b6 %-72s err %.3e bound %.3e" % (what, err, tol), flush=True)
    _note(what, err, tol)
    assert tuple(got.shape) == tuple(want.shape) and err <= tol, (what, err, tol)


def _check_f16_staged(got, want, what):
    """Staged fp16 operands: the share of elements outside 3e-4 (1 + |want|), NaN counting as outside, is at most 1e-3."""
    util.assert_finite(got, what)
    share = T.f16_outside(got, want)
    print("tile3 b6 %-72s err %.3e bound %.3e  (share outside)" % (what, share, T.F16_SHARE), flush=True)
    _note(what, share, T.F16_SHARE)
    assert tuple(got.shape) == tuple(want.shape) and share <= T.F16_SHARE, (what, share)


class _v3:
    """hip.TILE3 = True inside the block; unless `launches` is None the block must have launched the v3 kernel `launches` times
    through hip.tile_conv3_cl (a call it refuses returns None) and the library must have counted as many launches, no more."""

    def __init__(self, hip, launches=1):
        self.hip, self.launches, self.ran = hip, launches, 0

    def __enter__(self):
        h = self.hip
        self.keep = (h.TILE3, h.tile_conv3_cl)
        real = h.tile_conv3_cl

        def spy(*a, **k):
            out = real(*a, **k)
            self.ran += int(out is not None)
            return out

        h.TILE3, h.tile_conv3_cl = True, spy
        self.n0 = h.launch_count()
        return self

    def __exit__(self, et, ev, tb):
        h = self.hip
        counted = h.launch_count() - self.n0
        h.TILE3, h.tile_conv3_cl = self.keep
        if et is None and self.launches is not None:
            assert self.ran == self.launches and counted == self.launches, "v3 launches %d, library launches %d, expected %d" % (
                self.ran, counted, self.launches)
        return False


def _expect(N):
    return 1 if N else None  # (an empty list launches nothing on any kernel)


def _pack(hip, c, compute="f32"):
    packed = hip.conv_pack_weights(c["w"].to(DEV), 6, 6, (1, 1), compute)
    assert packed is not None and packed.compute == compute and hip._tile3_packed(packed) is not None
    return packed


def _direct(hip, source, x, x2, idx_d, sc, sh, act, packed, bias, cout, out, full=None, residual=None, smap=None, up=False):
    """hip.tile_conv3_cl itself (no fallback behind it): source 1 (x, x2 = the tensors) or 2 (x = conv-1 tiles, x2 = the cache)."""
    t3 = hip._tile3_packed(packed)
    assert t3 is not None
    if source == 1:
        B, C1, Hx, Wx = x.shape
        C2 = 0 if x2 is None else x2.shape[1]
        Hx, Wx = (2 * Hx, 2 * Wx) if up else (Hx, Wx)
    else:
        B, C1, Hx, Wx = x2.shape
        C2 = 0
    return hip.tile_conv3_cl(source, x, x2, B, C1, C2, Hx, Wx, up, idx_d, smap, (4, 4) if source == 2 else (0, 0), sc, sh, act, t3, bias,
                             cout, full, residual, hip._NO_BLOCK_RESIDUAL, None, hip._NO_TWINS, out, compute=hip._compute_id(packed))


def _gather_call(c, form, kind=None):
    """(x, x2, scale, shift, activation, upsample2x) on the device for one staging form of source 1."""
    aff, act, up = T.GATHER_FORMS[form]
    if kind is not None and aff != "none":
        aff = kind  # (the form's affine per batch instead of shared)
    sc, sh = T.affine_of(c, aff)
    x, x2 = (c["lo"], c["lo2"]) if up else (c["x"], c["x2"])
    return _cl(x), None if x2 is None else _cl(x2), _d(sc), _d(sh), act, up, aff


def _run_gather(hip, c, shape, B, name, form, packed, kind=None, exact=True, f16=False):
    """One staging form of source 1 over one list: into tiles, and into the full tensor (`prev` buffer, residual, offset (1,1))."""
    cout = shape[2]
    idx = T.LISTS[name]
    N = idx.shape[0]
    idx_d, bd = idx.to(DEV), c["bias"].to(DEV)
    x, x2, sc, sh, act, up, aff = _gather_call(c, form, kind)
    tiles = T.gather_tiles(c, idx, aff, act, up)
    want = T.conv64(tiles.half(), c["w"].half(), c["bias"]) if f16 else T.conv64(tiles, c["w"], c["bias"])
    check = _check if exact else _check_f16_staged
    tag = "gather %s %s%s B%d %s" % (shape, form, " per-batch" if aff == "batch" else "", B, name)
    args = (x, x2, (6, 6), idx_d, sc, sh, act, packed, bd, cout, (3, 3), (1, 1))
    with util.poisoned(), _v3(hip, _expect(N)):
        got = hip.gather_conv_cl(*args, upsample2x=up)
    assert got is not None and tuple(got.shape) == (B * N, cout, 4, 4)
    check(got, want, tag + " -> tiles")
    out = _cl(c["prev"])
    with util.poisoned(), _v3(hip, _expect(N)):
        got = hip.gather_conv_cl(*args, upsample2x=up, out=out, full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(c["residual"])))
    assert got is out
    ref = T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: t + c["residual"][b, :, hs, ws].double())
    cover = T.covered(idx)
    if exact:
        check(got, ref, tag + " -> full + residual")
    else:  # (the share is taken over the pixels the launch writes)
        check(got.cpu()[:, :, cover], ref[:, :, cover], tag + " -> full + residual")
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag


# ---- a. exact fp32: the gather source ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%d+%d_%d" % s)
def test_gather_forms_to_tiles_and_full(hip, shape, B):
    """T3_GATHER: raw, shared [1,C] affine + SiLU, affine alone, upsample2x addressing raw and with affine + SiLU; one tensor and the
    fused cat; into tiles and into the full tensor; every list.  `every` and `holes` are odd: the last workgroup is half filled, and
    at B = 2 one workgroup holds tiles of both images (a shared affine allows that)."""
    c = T.case(*shape, B)
    packed = _pack(hip, c)
    for name in T.NAMES:
        for form in T.GATHER_FORMS:
            _run_gather(hip, c, shape, B, name, form, packed)


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%d+%d_%d" % s)
def test_gather_per_batch_affine(hip, shape):
    """A [2,C,1,1] affine (aff_sb != 0, the workgroup's image b0): on the even lists it runs -- with SiLU, alone and under
    upsample2x --; on `every` (35 tiles: a workgroup would hold tiles of two images) the entry point refuses and writes nothing."""
    B = 2
    c = T.case(*shape, B)
    packed = _pack(hip, c)
    for name in ("corners", "every34"):
        for form in ("affine+silu", "affine", "up+affine+silu"):
            _run_gather(hip, c, shape, B, name, form, packed, kind="batch")
    cout = shape[2]
    idx_d = T.LISTS["every"].to(DEV)
    x, x2, sc, sh, act, up, _ = _gather_call(c, "affine+silu", "batch")
    assert tuple(sc.shape) == (2, shape[0] + shape[1], 1, 1)
    n0 = hip.launch_count()
    out = _cl(torch.full((B * 35, cout, 4, 4), float("nan")))
    assert _direct(hip, 1, x, x2, idx_d, sc, sh, act, packed, c["bias"].to(DEV), cout, out) is None
    full = _cl(c["prev"])
    assert _direct(hip, 1, x, x2, idx_d, sc, sh, act, packed, c["bias"].to(DEV), cout, full, full=(1, 1, H, W),
                   residual=_cl(c["residual"])) is None
    torch.cuda.synchronize()
    assert hip.launch_count() == n0 and bool(torch.isnan(out).all()) and torch.equal(full.cpu(), c["prev"])
    # the same two calls with the shared affine run (the refusal above is about the affine, nothing else)
    sc1, sh1 = c["scale1"].to(DEV), c["shift1"].to(DEV)
    got = _direct(hip, 1, x, x2, idx_d, sc1, sh1, act, packed, c["bias"].to(DEV), cout, out)
    assert got is out
    _check(got, T.conv64(T.gather_tiles(c, T.LISTS["every"], "shared", "swish", False), c["w"], c["bias"]),
           "gather %s direct call, shared affine B2 every -> tiles" % (shape,))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["every", "holes"])
def test_gather_full_with_twins_and_out_affine(hip, name, B):
    """The full destination against fp64: residual, both twins SiLU(ts * (conv + bias + residual) + tt) -- taken before the
    out-affine, as the epilogue does -- and the consumer's out-affine + SiLU; tiles with an out-affine."""
    shape = (64, 64, 128)
    c = T.case(*shape, B)
    cout = shape[2]
    packed = _pack(hip, c)
    idx = T.LISTS[name]
    want = T.conv64(T.gather_tiles(c, idx, "shared", "swish", False), c["w"], c["bias"])
    v = lambda t: t.double().view(-1, 1, 1)  # noqa: E731
    base = lambda t, b, hs, ws: t + c["residual"][b, :, hs, ws].double()  # noqa: E731
    args = (_cl(c["x"]), _cl(c["x2"]), (6, 6), idx.to(DEV), c["scale1"].to(DEV), c["shift1"].to(DEV), "swish", packed, c["bias"].to(DEV),
            cout, (3, 3), (1, 1))
    tw = [(_cl(c["prev"]), c["ts"][k].to(DEV), c["tt"][k].to(DEV)) for k in range(2)]
    out = _cl(c["prev"])
    with _v3(hip):
        got = hip.gather_conv_cl(*args, out=out, twins=tw, out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "swish"),
                                 full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(c["residual"])))
    assert got is out
    cover = T.covered(idx)
    _check(got, T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(v(c["os"]) * base(t, b, hs, ws) + v(c["oh"]))),
           "gather B%d %s twins + out-affine: out" % (B, name))
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover])
    for k in range(2):
        _check(tw[k][0], T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(v(c["ts"][k]) * base(t, b, hs, ws) + v(c["tt"][k]))),
               "gather B%d %s twins + out-affine: twin %d" % (B, name, k))
        assert torch.equal(tw[k][0].cpu()[:, :, ~cover], c["prev"][:, :, ~cover])
    # residual + twins without an out-affine: `out` is the plain sum
    tw = [(_cl(c["prev"]), c["ts"][0].to(DEV), c["tt"][0].to(DEV))]
    out = _cl(c["prev"])
    with _v3(hip):
        got = hip.gather_conv_cl(*args, out=out, twins=tw, full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(c["residual"])))
    _check(got, T.place(c["prev"], want, idx, B, base), "gather B%d %s one twin: out" % (B, name))
    _check(tw[0][0], T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(v(c["ts"][0]) * base(t, b, hs, ws) + v(c["tt"][0]))),
           "gather B%d %s one twin: twin" % (B, name))
    # tiles with the out-affine (what SIGEConv2d(out_affine=...) asks for), identity and SiLU
    for oact in ("identity", "swish"):
        with util.poisoned(), _v3(hip):
            got = hip.gather_conv_cl(*args, out_affine=(c["os"].to(DEV), c["oh"].to(DEV), oact))
        ref = v(c["os"]) * want + v(c["oh"])
        _check(got, F.silu(ref) if oact == "swish" else ref, "gather B%d %s tiles + out-affine %s" % (B, name, oact))


# ---- b. exact fp32: the scatter_gather source -------------------------------------------------------------------------------------
def _run_sg(hip, c, shape, B, name, kind, packed, y_cpu=None, f16=False, half_cache=False):
    """Source 2 over one list: conv-1 tiles + the cached tensor through the oracle's scatter map, raw (kind "none") or behind a
    cached affine + SiLU; into tiles (the entry point itself), into the full tensor with a plain residual and a twin (Scatter), and
    with the block residual over a 4x4 shortcut list (ScatterWithBlockResidual).  EVERY tile is compared."""
    cin, _, cout = shape
    idx = T.LISTS[name]
    N = idx.shape[0]
    act = "identity" if kind == "none" else "swish"
    exact = not f16 or kind == "none"
    check = _check if exact else _check_f16_staged
    y_ref = c["y"].half().float() if half_cache else c["y"]
    t4, tiles = T.sg_tiles(c, idx, B, kind, act, y=y_ref)
    want = T.conv64(tiles.half(), c["w"].half(), c["bias"]) if f16 else T.conv64(tiles, c["w"], c["bias"])
    smap = T.scatter_map(idx)
    idx_d, smap_d, bd = idx.to(DEV), smap.to(DEV), c["bias"].to(DEV)
    sc, sh = (_d(t) for t in T.affine_of(c, kind))
    t4d = _cl(t4) if N else _no_tiles(cin)
    yd = _cl(c["y"]).half() if half_cache else _cl(c["y"])
    tag = "scatter_gather %s %s%s B%d %s" % (shape, {"none": "raw", "shared": "affine+silu", "batch": "per-batch affine+silu"}[kind],
                                            " f16 cache" if half_cache else "", B, name)
    cover = T.covered(idx)
    pick = (lambda t: t) if exact else (lambda t: t.cpu()[:, :, cover])  # noqa: E731  (staged fp16: the share over the written pixels)
    if N:
        with util.poisoned():
            out = hip._empty_tiles_cl(B, idx_d, cout, 4, 4, DEV)
        n0 = hip.launch_count()
        got = _direct(hip, 2, t4d, yd, idx_d, sc, sh, act, packed, bd, cout, out, smap=smap_d)
        assert got is out and hip.launch_count() == n0 + 1
        check(got, want, tag + " -> tiles")
    y1 = c["residual"]
    args = (t4d, yd, (6, 6), idx_d, smap_d, sc, sh, act, packed, bd, cout, (3, 3), (1, 1))
    # Scatter: conv + bias + residual, and an activated twin
    out = _cl(c["prev"])
    tw = [(_cl(c["prev"]), c["ts"][0].to(DEV), c["tt"][0].to(DEV))]
    with _v3(hip, _expect(N)):
        got = hip.scatter_gather_conv_scatter_cl(*args, out, residual=_cl(y1), twins=tw)
    assert got is out
    plain = lambda t, b, hs, ws: t + y1[b, :, hs, ws].double()  # noqa: E731
    check(pick(got), pick(T.place(c["prev"], want, idx, B, plain)), tag + " -> full + residual")
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag
    ts, tt = c["ts"][0].double().view(-1, 1, 1), c["tt"][0].double().view(-1, 1, 1)
    check(pick(tw[0][0]), pick(T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(ts * plain(t, b, hs, ws) + tt))), tag + " -> twin")
    assert torch.equal(tw[0][0].cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag
    # ScatterWithBlockResidual: the shortcut tiles replace the cached shortcut tensor where they cover the cell
    idx1, table1 = T.shortcut(idx)
    N1 = idx1.shape[0]
    table1_d = hip.tile_table(idx1.to(DEV), (0, 0), (1, 1), (4, 4), (H, W)) if N1 else table1.to(DEV)
    assert torch.equal(table1_d.cpu(), table1)
    x1 = c["x1"][:, :N1].reshape(B * N1, cout, 4, 4).contiguous()
    x1d = _cl(x1) if N1 else _no_tiles(cout)
    r1 = y1.half().float() if half_cache else y1  # (an fp16-stored cache: the cached shortcut tensor holds halves too)

    def block(t, b, hs, ws):
        n1 = int(table1[hs.start // 4, ws.start // 4])
        if n1 < 0:
            return t + r1[b, :, hs, ws].double()
        return t + x1[b * N1 + n1][:, :hs.stop - hs.start, :ws.stop - ws.start].double()

    out = _cl(c["prev"])
    with _v3(hip, _expect(N)):
        got = hip.scatter_gather_conv_scatter_cl(*args, out, residual=_cl(y1).half() if half_cache else _cl(y1), x1=x1d, table1=table1_d)
    assert got is out
    check(pick(got), pick(T.place(c["prev"], want, idx, B, block)), tag + " -> full + block residual")
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", T.SHAPES[:3], ids=lambda s: "%d+%d_%d" % s)
def test_scatter_gather_source_to_tiles_and_full(hip, shape, B):
    """T3_SCATTER_GATHER, raw and with a shared cached affine + SiLU, every list (`every`: the ring comes from neighbouring tiles;
    the others read the cache too); at B = 2 the per-batch affine on the even list."""
    c = T.case(*shape, B)
    packed = _pack(hip, c)
    for name in T.NAMES:
        for kind in ("none", "shared"):
            _run_sg(hip, c, shape, B, name, kind, packed)
    if B == 2:
        _run_sg(hip, c, shape, B, "every34", "batch", packed)


# ---- c. exact fp32: stacked edits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%d+%d_%d" % s)
def test_stacked_edits_seam_rule(hip, shape):
    """hip.set_edit_batch(2): two different 16x26 images as one 32x26 tensor, each with its own list.  A window's rows beyond its own
    image are zero padding (conv_tile3.hpp: hp_shift), not the neighbour's pixels: image 0's windows at origin row 11 read zeros at
    row 16, image 1's at origin row 15 read zeros at row 15.  Reference: each image alone through the oracle and fp64."""
    c1, c2, cout = shape
    c = T.case(c1, c2, cout, 1)
    packed = _pack(hip, c)
    idx = T.stacked_list()
    idx_d, bd = idx.to(DEV), c["bias"].to(DEV)
    assert int(idx[T.NS - 1, 0]) == 11 and int(idx[T.NS, 0]) == 15
    prev, residual = T.stack(c["prevs"]), T.stack(c["residuals"])
    res = (2 * T.HS, W)
    plain = lambda t, b, hs, ws: t + residual[b, :, hs, ws].double()  # noqa: E731
    hip.set_edit_batch(2)
    try:
        for affine in (False, True):
            sc, sh = (c["scale1"].to(DEV), c["shift1"].to(DEV)) if affine else (None, None)
            act = "swish" if affine else "identity"
            for source in ((1, 2) if c2 == 0 else (1,)):
                want = T.conv64(T.stacked_tiles(c, source, affine), c["w"], c["bias"])
                tag = "stacked %s source %d %s" % (shape, source, "affine+silu" if affine else "raw")
                out = _cl(prev)
                if source == 1:
                    args = (_cl(T.stack(c["xs"])), None if c2 == 0 else _cl(T.stack(c["xs2"])), (6, 6), idx_d, sc, sh, act, packed, bd,
                            cout, (3, 3), (1, 1))
                    with util.poisoned(), _v3(hip):
                        got = hip.gather_conv_cl(*args)
                    with _v3(hip):
                        full = hip.gather_conv_cl(*args, out=out, full=dict(offset=(1, 1), out_res=res, residual=_cl(residual)))
                else:
                    t4d, yd, smap_d = _cl(c["t4s"].reshape(2 * T.NS, -1, 4, 4)), _cl(T.stack(c["ys"])), T.stacked_map().to(DEV)
                    with util.poisoned():
                        tiles = hip._empty_tiles_cl(1, idx_d, cout, 4, 4, DEV)
                    n0 = hip.launch_count()
                    got = _direct(hip, 2, t4d, yd, idx_d, sc, sh, act, packed, bd, cout, tiles, smap=smap_d)
                    assert got is tiles and hip.launch_count() == n0 + 1
                    with _v3(hip):
                        full = hip.scatter_gather_conv_scatter_cl(t4d, yd, (6, 6), idx_d, smap_d, sc, sh, act, packed, bd, cout, (3, 3), (1, 1),
                                                                  out, residual=_cl(residual))
                assert got is not None and tuple(got.shape) == (2 * T.NS, cout, 4, 4) and full is out
                _check(got, want, tag + " -> tiles")
                _check(full, T.place(prev, want, idx, 1, plain), tag + " -> full + residual")
                cover = T.covered(idx, res)
                assert torch.equal(full.cpu()[:, :, ~cover], prev[:, :, ~cover]), tag
    finally:
        hip.set_edit_batch(1)


# ---- d. fp16 operands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%d+%d_%d" % s)
def test_f16_gather_forms(hip, shape, B):
    """Tile3Geo<2, WIDE_F16>, source 1: the staging forms and lists of the fp32 test.  Raw staging (also under upsample2x) rounds the
    operand exactly like .half(): every element against fp64 of the rounded tiles and weights; behind an affine: the share
    criterion."""
    c = T.case(*shape, B)
    packed = _pack(hip, c, "f16")
    for name in T.NAMES:
        for form, (aff, _, _) in T.GATHER_FORMS.items():
            _run_gather(hip, c, shape, B, name, form, packed, exact=aff == "none", f16=True)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("half_cache", [False, True], ids=["cache_f32", "cache_f16"])
@pytest.mark.parametrize("shape", T.SHAPES[:3], ids=lambda s: "%d+%d_%d" % s)
def test_f16_scatter_gather_source(hip, shape, half_cache, B):
    """Tile3Geo<2, WIDE_F16>, source 2 over an fp32- and an fp16-stored cache (the cached tensor, and with the block residual the
    cached shortcut tensor, hold halves): raw -- exact operand rounding, every element -- and behind the cached affine + SiLU."""
    c = T.case(*shape, B)
    packed = _pack(hip, c, "f16")
    for name in T.NAMES:
        for kind in ("none", "shared"):
            _run_sg(hip, c, shape, B, name, kind, packed, f16=True, half_cache=half_cache)
