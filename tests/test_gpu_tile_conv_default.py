"""On the MI355X: the DEFAULT channels-last tile conv (csrc/conv_mfma.hpp: ConvGeo exact fp32, ConvGeoH fp16 operands, ConvGeoX split
fp16 operands; launched by csrc/block_conv.hip: plan_conv, launch_conv) -- the kernel family every forward below hip.TILE3_MIN_BLOCKS
workgroups runs on, and every 1x1 shortcut, stride-2 Downsample, pair launch and K-split dense level at any edit size -- against fp64
convs of the CPU ORACLE's tiles on a ragged image, as tests/test_gpu_tile_conv3_block6.py pins the v3 kernels.

Shapes (tests/tile_default_common.py, tests/tile3_common.py).  Image 18 x 26; K31 = 3x3 / s1 on 6x6 windows, K11 = 1x1 on 4x4
blocks, K32 = 3x3 / s2 on 5x5 blocks (output 9 x 13, row 9 and column 13 clipped); lists every (35: a ragged last M block, and at
B = 2 M blocks that hold tiles of both images), corners, interior, holes, empty, every34.  (C1, C2, Cout) from the chunk sizes.

Every positive case runs inside `_default`: hip.TILE3 = False, a spy on hip.tile_conv3_cl sees no call, hip.launch_count() rises by
exactly the expected number, the result is not None.  Once on the product build with the library's own block choice; on the
measurement build with the output block forced: K31 gather / epilogues / per-batch affine / scatter_gather and K11 under all four
(MT, NB) x 4 and 8 waves, fp16-stored caches and fp16 operands under the four (MT, NB) at 4 waves, split fp16 operands and K32 at
MT = 16 and 32, the K split under factor x finish x (automatic | four (MT, NB)); the pair on the product build only.  A case plan_conv's usable() leaves no block shape for (tile_default_common.refused,
held to usable()'s arithmetic without a GPU) must return None with the destination untouched and nothing launched.

Bounds.  Exact fp32 and split fp16 operands: 2e-5 * (1 + max |ref|) on every element (for f16x3 this IS tests/test_gpu_round3.py's
2e-5 * (wmag + max |ref|) at wmag = 1, the weights' scale here).  fp16 operands, raw staging: the same bound against the fp64 conv of
.half()-rounded tiles and weights; behind an affine: at most 1e-3 of the elements outside 3e-4 (1 + |want|).  Outputs and workspaces
are allocated NaN-poisoned and checked finite; pixels no tile covers are compared bit for bit with what the destination held."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import tile3_common as T
from tests import tile_default_common as D
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
DEV = "cuda"
H, W = D.H, D.W


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _d(t):
    return None if t is None else t.to(DEV)


_WORST = {}


@pytest.fixture(autouse=True)
def _margins(request):
    """The worst err / bound of the test's checks goes to the margin file (util.record_margin)."""
    _WORST.clear()
    yield
    if _WORST:
        util.record_margin("tile_conv_default", "%s: %s" % (request.node.name, _WORST["what"]), _WORST["err"], _WORST["tol"])


def _note(what, err, tol):
    if tol > 0 and (not _WORST or err / tol > _WORST["err"] / _WORST["tol"]):
        _WORST.update(what=what, err=err, tol=tol)


def _check(got, want, what):
    util.assert_finite(got, what)
    err = float((got.detach().double().cpu() - want.double()).abs().max()) if got.numel() else 0.0
    tol = T.bound(want)
    print("tile default %-84s err %.3e bound %.3e" % (what, err, tol), flush=True)
    _note(what, err, tol)
    assert tuple(got.shape) == tuple(want.shape) and err <= tol, (what, err, tol)


def _check_f16_staged(got, want, what):
    util.assert_finite(got, what)
    share = T.f16_outside(got, want)
    print("tile default %-84s err %.3e bound %.3e  (share outside)" % (what, share, T.F16_SHARE), flush=True)
    _note(what, share, T.F16_SHARE)
    assert tuple(got.shape) == tuple(want.shape) and share <= T.F16_SHARE, (what, share)


class _default:
    """hip.TILE3 = False inside the block; hip.tile_conv3_cl must not be called, and unless `launches` is None the library must have
    counted exactly `launches` launches."""

    def __init__(self, hip, launches=1):
        self.hip, self.launches, self.v3 = hip, launches, 0

    def __enter__(self):
        h = self.hip
        self.keep = (h.TILE3, h.tile_conv3_cl)

        def spy(*a, **k):
            self.v3 += 1
            return self.keep[1](*a, **k)

        h.TILE3, h.tile_conv3_cl = False, spy
        self.n0 = h.launch_count()
        return self

    def __exit__(self, et, ev, tb):
        h = self.hip
        counted = h.launch_count() - self.n0
        h.TILE3, h.tile_conv3_cl = self.keep
        if et is None:
            assert self.v3 == 0, "hip.tile_conv3_cl was called %d times" % self.v3
            assert self.launches is None or counted == self.launches, "library launches %d, expected %d" % (counted, self.launches)
        return False


# the forced block shapes of the measurement build: (mt, nb, waves).  NB = 2 and 8 waves exist at stride 1 only.
FORCED = [(mt, nb, waves) for waves in (4, 8) for mt, nb in ((16, 1), (16, 2), (32, 1), (32, 2))]
FORCED4 = [c for c in FORCED if c[2] == 4]  # (fp16 operands and fp16-stored caches: 4 waves only)
FORCED_NB1 = [(16, 1, 4), (32, 1, 4)]       # (split fp16 operands: NB = 1, 4 waves)
FORCED_S2 = [(16, 1, 4), (32, 1, 4)]
CFG_ID = lambda c: "product" if c is None else "mt%d_nb%d_w%d" % c  # noqa: E731


@contextlib.contextmanager
def _build(request, cfg):
    """The product build with the library's own block choice (cfg None), or the measurement build with (mt, nb, waves) forced."""
    if cfg is None:
        from sige_amd import hip as h

        yield h
        return
    h = request.getfixturevalue("tuning")
    h.conv_force_tile(cfg[0], cfg[1])
    h.conv_force_waves(cfg[2])
    try:
        yield h
    finally:
        h.conv_force_tile(0, 0)
        h.conv_force_waves(0)


def _pack(hip, geo, shape, B, compute="f32"):
    g = D.GEO[geo]
    w, _ = D.weights(geo, shape, B)
    keep = hip.TILE3
    hip.TILE3 = False  # (no v3 layout beside the pack)
    try:
        packed = hip.conv_pack_weights(w.to(DEV), g.block, g.block, (g.stride, g.stride), compute)
    finally:
        hip.TILE3 = keep
    assert packed is not None and packed.compute == D.compute_of(geo, compute) and getattr(packed, "geo", None) is None
    return packed


def _gather_args(geo, shape, B, name, form, packed, kind=None, alt=False):
    """Positional arguments of hip.gather_conv_cl for one case, (affine kind, upsample2x)."""
    g = D.GEO[geo]
    c, e = T.case(*shape, B), D.extra(*shape, B)
    aff, act, up = T.GATHER_FORMS[form]
    if kind is not None and aff != "none":
        aff = kind
    sc, sh = T.affine_of(c, aff)
    x, x2 = (c["lo"], c["lo2"]) if up else (e["x_alt"] if alt else c["x"], c["x2"])
    _, bias = D.weights(geo, shape, B)
    return (_cl(x), None if x2 is None else _cl(x2), (g.block, g.block), D.lists(geo)[name].to(DEV), _d(sc), _d(sh), act, packed,
            bias.to(DEV), shape[2], (g.kernel, g.kernel), (g.stride, g.stride)), aff, up


def _residual_fn(residual):
    return lambda t, b, hs, ws: t + residual[b, :, hs, ws].double()


def _run_gather(hip, geo, shape, B, name, form, packed, kind=None, compute="f32", to=("tiles", "full")):
    """One staging form of the gather source over one list: into tiles, and into a full tensor that holds earlier content (with a
    residual).  A refusal (tile_default_common.refused) returns None, launches nothing and leaves the destination as it was."""
    g = D.GEO[geo]
    cout = shape[2]
    idx = D.lists(geo)[name]
    N = idx.shape[0]
    args, aff, up = _gather_args(geo, shape, B, name, form, packed, kind)
    no = D.refused(geo, shape, B, N, aff == "batch", compute)
    ran = None if N == 0 else (0 if no else 1)
    f16 = D.compute_of(geo, compute) == "f16"
    exact = not f16 or aff == "none"
    check = _check if exact else _check_f16_staged
    want = None if no else D.want_gather(geo, shape, B, name, form, kind, half=f16)
    tag = "%s gather %s %s%s %s B%d %s" % (geo, shape, form, " per-batch" if aff == "batch" else "", compute, B, name)
    if "tiles" in to:
        with util.poisoned(), _default(hip, ran):
            got = hip.gather_conv_cl(*args, upsample2x=up)
        if no:
            assert got is None, tag + ": expected a refusal"
        else:
            assert got is not None, tag + ": refused"
            assert tuple(got.shape) == (B * N, cout, g.ro, g.ro)
            check(got, want, tag + " -> tiles")
    if "full" in to:
        prev, residual = D.dest(geo, shape, B)
        out = _cl(prev)
        with util.poisoned(), _default(hip, ran):
            got = hip.gather_conv_cl(*args, upsample2x=up, out=out, full=dict(offset=(g.offset, g.offset), out_res=g.res, residual=_cl(residual)))
        if no:
            torch.cuda.synchronize()
            assert got is None and torch.equal(out.cpu(), prev), tag + ": expected a refusal that writes nothing"
            return
        assert got is out, tag + ": refused"
        ref = D.place(geo, prev, want, idx, B, _residual_fn(residual))
        cover = D.covered(geo, idx)
        if exact:
            check(got, ref, tag + " -> full + residual")
        else:  # (the share is taken over the pixels the launch writes)
            check(got.cpu()[:, :, cover], ref[:, :, cover], tag + " -> full + residual")
        assert torch.equal(got.cpu()[:, :, ~cover], prev[:, :, ~cover]), tag + ": a pixel no tile covers changed"


# ---- 1. K31, source gather ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.IDS)
def test_k31_gather_forms_to_tiles_and_full(hip, shape, B):
    """The product build, the library's own block choice: five staging forms x six lists, to tiles and to full.  (20, 44, 64), and
    any cat at B = 2, is refused."""
    packed = _pack(hip, "K31", shape, B)
    for name in D.NAMES:
        for form in T.GATHER_FORMS:
            _run_gather(hip, "K31", shape, B, name, form, packed)


@pytest.mark.parametrize("cfg", FORCED, ids=CFG_ID)
@pytest.mark.parametrize("shape", D.SHAPES[:6], ids=D.IDS)
def test_k31_gather_forms_forced_blocks(request, shape, cfg):
    """The same on the measurement build with the output block and the wave count forced (a forced shape usable() rejects falls back
    to the library's choice; 8 waves to 4 where a cat does not split on a chunk PAIR)."""
    B = 1 if shape[1] else 2
    with _build(request, cfg) as hip:
        packed = _pack(hip, "K31", shape, B)
        for name in ("every", "holes", "corners"):
            for form in T.GATHER_FORMS:
                _run_gather(hip, "K31", shape, B, name, form, packed)


@pytest.mark.parametrize("cfg", [None] + FORCED, ids=CFG_ID)
@pytest.mark.parametrize("shape,B", [((68, 0, 24), 1), ((68, 0, 24), 2), ((64, 64, 72), 1), ((96, 0, 40), 2)], ids=lambda v: D.IDS(v) if isinstance(v, tuple) else "B%d" % v)
def test_k31_gather_full_epilogues(request, shape, B, cfg):
    """To full: residual + the consumer's out-affine + SiLU; two twins SiLU(ts * (conv + bias + residual) + tt), taken before the
    out-affine; a destination the LIBRARY allocates (the pixels no tile covers keep the allocation's poison, bit for bit)."""
    geo = "K31"
    c = T.case(*shape, B)
    cout = shape[2]
    prev, residual = D.dest(geo, shape, B)
    v = lambda t: t.double().view(-1, 1, 1)  # noqa: E731
    base = _residual_fn(residual)
    with _build(request, cfg) as hip:
        packed = _pack(hip, geo, shape, B)
        for name in ("every", "holes", "every34"):
            idx = T.LISTS[name]
            cover = T.covered(idx)
            args, _, _ = _gather_args(geo, shape, B, name, "affine+silu", packed)
            want = D.want_gather(geo, shape, B, name, "affine+silu")
            full = dict(offset=(1, 1), out_res=(H, W), residual=_cl(residual))
            tag = "K31 gather %s B%d %s %s" % (shape, B, name, CFG_ID(cfg))
            # out-affine + SiLU
            out = _cl(prev)
            with util.poisoned(), _default(hip):
                got = hip.gather_conv_cl(*args, out=out, full=full, out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "swish"))
            assert got is out
            _check(got, D.place(geo, prev, want, idx, B, lambda t, b, hs, ws: F.silu(v(c["os"]) * base(t, b, hs, ws) + v(c["oh"]))),
                   tag + " full + residual + out-affine + SiLU")
            assert torch.equal(got.cpu()[:, :, ~cover], prev[:, :, ~cover]), tag
            # two twins (and the out-affine: the twins see the sum before it)
            tw = [(_cl(prev), c["ts"][k].to(DEV), c["tt"][k].to(DEV)) for k in range(2)]
            out = _cl(prev)
            with util.poisoned(), _default(hip):
                got = hip.gather_conv_cl(*args, out=out, full=full, twins=tw, out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "identity"))
            assert got is out
            _check(got, D.place(geo, prev, want, idx, B, lambda t, b, hs, ws: v(c["os"]) * base(t, b, hs, ws) + v(c["oh"])), tag + " twins: out")
            assert torch.equal(got.cpu()[:, :, ~cover], prev[:, :, ~cover]), tag
            for k in range(2):
                _check(tw[k][0], D.place(geo, prev, want, idx, B, lambda t, b, hs, ws: F.silu(v(c["ts"][k]) * base(t, b, hs, ws) + v(c["tt"][k]))),
                       tag + " twins: twin %d" % k)
                assert torch.equal(tw[k][0].cpu()[:, :, ~cover], prev[:, :, ~cover]), tag
            # no `out=`: the library's own allocation, no residual
            with util.poisoned(), _default(hip):
                got = hip.gather_conv_cl(*args, full=dict(offset=(1, 1), out_res=(H, W), residual=None))
            assert got is not None and tuple(got.shape) == (B, cout, H, W)
            g_cpu = got.cpu()
            ref = D.place(geo, torch.zeros_like(prev), want, idx, B, lambda t, b, hs, ws: t)
            _check(g_cpu[:, :, cover], ref[:, :, cover], tag + " full, allocated by the library")
            assert bool(torch.isnan(g_cpu[:, :, ~cover]).all()), tag + ": a pixel no tile covers was written"


@pytest.mark.parametrize("cfg", [None] + FORCED, ids=CFG_ID)
@pytest.mark.parametrize("shape", D.SHAPES[:4], ids=D.IDS)
def test_k31_gather_per_batch_affine(request, shape, cfg):
    """A [2, C, 1, 1] affine needs every M block inside one image: on `every34` both block shapes do, on `every` (35) only MT = 16
    (one tile per block) -- usable() leaves it, so the result must be right whatever is forced."""
    B = 2
    with _build(request, cfg) as hip:
        packed = _pack(hip, "K31", shape, B)
        for name in ("every", "every34"):
            assert D.block_shapes("K31", shape[0], 0, B, T.LISTS[name].shape[0], True) == ([16] if name == "every" else [32, 16])
            for form in ("affine+silu", "affine", "up+affine+silu"):
                _run_gather(hip, "K31", shape, B, name, form, packed, kind="batch")


# ---- 2. K31, source scatter_gather -------------------------------------------------------------------------------------------------
def _run_sg(hip, shape, B, name, kind, packed, half_cache=False, compute="f32"):
    """Conv-1 tiles + the cached tensor through the oracle's scatter map: to tiles (hip.scatter_gather_conv_cl); into the full tensor
    with a plain residual and a twin (Scatter) and with the block residual over a 4x4 shortcut list (ScatterWithBlockResidual)."""
    cout = shape[2]
    cin = shape[0] + shape[1]
    c = T.case(*shape, B)
    idx = T.LISTS[name]
    N = idx.shape[0]
    act = "identity" if kind == "none" else "swish"
    f16 = compute == "f16"
    exact = not f16 or kind == "none"
    check = _check if exact else _check_f16_staged
    want = D.want_scatter_gather(shape, B, name, kind, half_cache, half=f16)
    t4 = c["t4"][:, :N].reshape(B * N, cin, 4, 4).contiguous()
    smap = T.scatter_map(idx)
    idx_d, smap_d, bd = idx.to(DEV), smap.to(DEV), c["bias"].to(DEV)
    sc, sh = (_d(t) for t in T.affine_of(c, kind))
    t4d = _cl(t4) if N else torch.zeros((0, cin, 4, 4), device=DEV).contiguous(memory_format=torch.channels_last)
    yd = _cl(c["y"]).half() if half_cache else _cl(c["y"])
    ran = 1 if N else None
    tag = "K31 scatter_gather %s %s%s %s B%d %s" % (shape, kind, " f16 cache" if half_cache else "", compute, B, name)
    cover = T.covered(idx)
    pick = (lambda t: t) if exact else (lambda t: t.cpu()[:, :, cover])  # noqa: E731
    args = (t4d, yd, (6, 6), idx_d, smap_d, sc, sh, act, packed, bd, cout, (3, 3))
    with util.poisoned(), _default(hip, ran):
        got = hip.scatter_gather_conv_cl(*args, (1, 1))
    assert got is not None and tuple(got.shape) == (B * N, cout, 4, 4), tag
    check(got, want, tag + " -> tiles")
    y1 = c["residual"]
    plain = _residual_fn(y1)
    out = _cl(c["prev"])
    tw = [(_cl(c["prev"]), c["ts"][0].to(DEV), c["tt"][0].to(DEV))]
    with util.poisoned(), _default(hip, ran):
        got = hip.scatter_gather_conv_scatter_cl(*args, (1, 1), out, residual=_cl(y1), twins=tw)
    assert got is out, tag
    check(pick(got), pick(T.place(c["prev"], want, idx, B, plain)), tag + " -> full + residual")
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag
    ts, tt = c["ts"][0].double().view(-1, 1, 1), c["tt"][0].double().view(-1, 1, 1)
    check(pick(tw[0][0]), pick(T.place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(ts * plain(t, b, hs, ws) + tt))), tag + " -> twin")
    assert torch.equal(tw[0][0].cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag
    idx1, table1 = T.shortcut(idx)
    N1 = idx1.shape[0]
    table1_d = hip.tile_table(idx1.to(DEV), (0, 0), (1, 1), (4, 4), (H, W)) if N1 else table1.to(DEV)
    assert torch.equal(table1_d.cpu(), table1)
    x1 = c["x1"][:, :N1].reshape(B * N1, cout, 4, 4).contiguous()
    x1d = _cl(x1) if N1 else torch.zeros((0, cout, 4, 4), device=DEV).contiguous(memory_format=torch.channels_last)
    r1 = y1.half().float() if half_cache else y1

    def block(t, b, hs, ws):
        n1 = int(table1[hs.start // 4, ws.start // 4])
        if n1 < 0:
            return t + r1[b, :, hs, ws].double()
        return t + x1[b * N1 + n1][:, :hs.stop - hs.start, :ws.stop - ws.start].double()

    out = _cl(c["prev"])
    with util.poisoned(), _default(hip, ran):
        got = hip.scatter_gather_conv_scatter_cl(*args, (1, 1), out, residual=_cl(y1).half() if half_cache else _cl(y1), x1=x1d, table1=table1_d)
    assert got is out, tag
    check(pick(got), pick(T.place(c["prev"], want, idx, B, block)), tag + " -> full + block residual")
    assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover]), tag


SG_SHAPES = D.SHAPES[:4] + [(64, 64, 72)]  # (one cached tensor of C1 + C2 channels: this source has no cat)


@pytest.mark.parametrize("cfg", [None] + FORCED, ids=CFG_ID)
@pytest.mark.parametrize("shape", SG_SHAPES, ids=D.IDS)
def test_k31_scatter_gather_to_tiles_and_full(request, shape, cfg):
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, "K31", shape, B)
            for name in (D.NAMES if cfg is None else ("every", "holes")):
                for kind in ("none", "shared"):
                    _run_sg(hip, shape, B, name, kind, packed)
            if B == 2:
                _run_sg(hip, shape, B, "every34", "batch", packed)


@pytest.mark.parametrize("cfg", [None] + FORCED4, ids=CFG_ID)
@pytest.mark.parametrize("shape", SG_SHAPES[:3], ids=D.IDS)
def test_k31_scatter_gather_f16_stored_cache(request, shape, cfg):
    """The cached tensor (and the cached shortcut tensor of the block residual) stored as fp16: the Y16 kernels (4 waves).  The
    reference is taken over y.half().float()."""
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, "K31", shape, B)
            for name in ("every", "holes", "corners", "interior"):
                for kind in ("none", "shared"):
                    _run_sg(hip, shape, B, name, kind, packed, half_cache=True)


# ---- 3. K11 --------------------------------------------------------------------------------------------------------------------------
def _run_plain_full(hip, geo, shape, B, name, form, packed, compute="f32"):
    """To full WITHOUT a residual, into a destination that holds earlier content."""
    g = D.GEO[geo]
    idx = D.lists(geo)[name]
    N = idx.shape[0]
    if D.refused(geo, shape, B, N, False, compute):
        return
    args, _, up = _gather_args(geo, shape, B, name, form, packed)
    prev, _ = D.dest(geo, shape, B)
    out = _cl(prev)
    with util.poisoned(), _default(hip, 1 if N else None):
        got = hip.gather_conv_cl(*args, upsample2x=up, out=out, full=dict(offset=(g.offset, g.offset), out_res=g.res, residual=None))
    assert got is out
    f16 = D.compute_of(geo, compute) == "f16"
    _check(got, D.place(geo, prev, D.want_gather(geo, shape, B, name, form, half=f16), idx, B, lambda t, b, hs, ws: t),
           "%s gather %s %s %s B%d %s -> full" % (geo, shape, form, compute, B, name))
    cover = D.covered(geo, idx)
    assert torch.equal(got.cpu()[:, :, ~cover], prev[:, :, ~cover])


@pytest.mark.parametrize("cfg", [None] + FORCED, ids=CFG_ID)
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.IDS)
def test_k11_gather_to_tiles_and_full(request, shape, cfg):
    """1x1 on 4x4 blocks, raw and behind an affine; to tiles, to full with and without residual.  The chunk is 128 / 256 channels:
    every cat of this file's shapes is refused (tile_default_common.EXPECTED)."""
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, "K11", shape, B)
            for name in (D.NAMES if cfg is None else ("every", "holes")):
                for form in ("raw", "affine"):
                    _run_gather(hip, "K11", shape, B, name, form, packed)
                    _run_plain_full(hip, "K11", shape, B, name, form, packed)


# ---- 4. K32 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [None] + FORCED_S2, ids=CFG_ID)
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.IDS)
def test_k32_gather_to_tiles_and_full(request, shape, cfg):
    """3x3 / stride 2 on 5x5 blocks: 8 (MT = 32) or 4 (MT = 16) tiles per M block -- 35 tiles leave a ragged last block, and at B = 2
    under a shared affine an M block holds tiles of both images.  To tiles and to the clipped 9 x 13 output."""
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, "K32", shape, B)
            for name in D.NAMES:
                for form in ("raw", "affine+silu"):
                    _run_gather(hip, "K32", shape, B, name, form, packed)
                _run_plain_full(hip, "K32", shape, B, name, "raw", packed)


@pytest.mark.parametrize("cfg", [None] + FORCED_S2, ids=CFG_ID)
@pytest.mark.parametrize("shape", D.SHAPES[:4], ids=D.IDS)
def test_k32_per_batch_affine(request, shape, cfg):
    """A per-batch affine at B = 2: accepted on 32 tiles (whole M blocks of 8 and of 4 per image), refused on `every` and `every34`
    with the destination untouched."""
    B = 2
    with _build(request, cfg) as hip:
        packed = _pack(hip, "K32", shape, B)
        assert D.refused("K32", shape, B, 35, True) and D.refused("K32", shape, B, 34, True) and not D.refused("K32", shape, B, 32, True)
        for name in ("every32", "every", "every34"):
            _run_gather(hip, "K32", shape, B, name, "affine+silu", packed, kind="batch")


# ---- 5. the pair launch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["tiles", "full"])
@pytest.mark.parametrize("shape", [(64, 0, 64), (64, 64, 72)], ids=D.IDS)
def test_pair_shortcut_and_conv1_in_one_launch(hip, shape, full):
    """Inside hip.conv_pair: the K11 shortcut (raw) is held and runs inside the K31 conv1's launch (affine + SiLU staging, out-affine);
    each result against its own fp64 reference; one pair fused, one launch counted.

    Each conv takes a cat the way the modules hand it over (sige_amd/nn/dense.py, nn/gather.py): fused as (x, x2) where
    hip.cat_fusable says so, concatenated by the caller where not.  At (64, 64, 72) the split is on a 3x3 chunk boundary (32 / 64
    channels) and on no 1x1 one (128 / 256; a chunk comes from ONE tensor -- conv_mfma.hpp: use2 per chunk): conv1 reads the two
    tensors, the shortcut the concatenated one.  The shortcut handed (x, x2) all the same is refused AT ITS OWN CALL, conv1 behind it
    runs alone and right (before this test such a shortcut was held, never launched, and handed back as a tensor nobody wrote --
    all NaN under poison -- while conv1 returned None; block_conv.hip hold_or_pair now holds only what plan_conv accepts)."""
    c1, c2, cout = shape
    for B in ((1,) if c2 else (1, 2)):
        c = T.case(*shape, B)
        p1, p3 = _pack(hip, "K11", shape, B), _pack(hip, "K31", shape, B)
        for name in ("every", "holes", "corners"):
            a1, _, _ = _gather_args("K11", shape, B, name, "raw", p1)
            a3, _, _ = _gather_args("K31", shape, B, name, "affine+silu", p3)
            prev, residual = D.dest("K31", shape, B)
            w3 = D.want_gather("K31", shape, B, name, "affine+silu")
            oa = (c["os"].to(DEV), c["oh"].to(DEV), "swish")
            if c2:
                assert hip.cat_fusable(B, c1, (3, 3)) and not hip.cat_fusable(B, c1, (1, 1)) and D.refused("K11", shape, B, a1[3].shape[0])
                # the unfusable cat handed over fused: refused at once, nothing held, conv1 alone in its one launch
                f0 = hip.conv_pairs_fused()
                with util.poisoned(), _default(hip, 1):
                    with hip.conv_pair(a1[0]):
                        assert hip.gather_conv_cl(*a1) is None, "a shortcut no block shape can stage was not refused at its call"
                        got3 = hip.gather_conv_cl(*a3, out_affine=oa)
                assert got3 is not None and hip.conv_pairs_fused() == f0
                _check(got3, F.silu(c["os"].double().view(-1, 1, 1) * w3 + c["oh"].double().view(-1, 1, 1)),
                       "pair %s B%d %s: conv1 behind a refused shortcut" % (shape, B, name))
                a1 = (_cl(T.full_input(c)), None) + a1[2:]  # (the caller's torch.cat, as nn/dense.py does it)
            o1, o3 = (_cl(prev), _cl(prev)) if full else (None, None)
            k1 = dict(out=o1, full=dict(offset=(0, 0), out_res=(H, W), residual=None)) if full else {}
            k3 = dict(out=o3, full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(residual))) if full else {}
            f0 = hip.conv_pairs_fused()
            with util.poisoned(), _default(hip, 1):
                with hip.conv_pair(a1[0]):
                    got1 = hip.gather_conv_cl(*a1, **k1)
                    got3 = hip.gather_conv_cl(*a3, out_affine=oa, **k3)
            tag = "pair %s B%d %s %s" % (shape, B, name, "full" if full else "tiles")
            assert got1 is not None and got3 is not None, tag + ": refused"
            assert hip.conv_pairs_fused() == f0 + 1, tag + ": no pair was fused"
            w1 = D.want_gather("K11", shape, B, name, "raw")
            v = lambda t: t.double().view(-1, 1, 1)  # noqa: E731
            if not full:
                _check(got1, w1, tag + ": shortcut")
                _check(got3, F.silu(v(c["os"]) * w3 + v(c["oh"])), tag + ": conv1")
                continue
            assert got1 is o1 and got3 is o3
            base = _residual_fn(residual)
            _check(got1, D.place("K11", prev, w1, D.LISTS0[name], B, lambda t, b, hs, ws: t), tag + ": shortcut")
            _check(got3, D.place("K31", prev, w3, T.LISTS[name], B, lambda t, b, hs, ws: F.silu(v(c["os"]) * base(t, b, hs, ws) + v(c["oh"]))),
                   tag + ": conv1")
            for got, geo in ((got1, "K11"), (got3, "K31")):
                cover = D.covered(geo, D.lists(geo)[name])
                assert torch.equal(got.cpu()[:, :, ~cover], prev[:, :, ~cover]), tag


# ---- 6. / 7. the K split ---------------------------------------------------------------------------------------------------------------
# None: the product build as it routes itself; else (split factor, second pass, forced (mt, nb) or None) on the measurement build
SPLITS = [None] + [(ks, second, blk) for ks in (2, 4) for second in (False, True) for blk in (None, (16, 1), (16, 2), (32, 1), (32, 2))]
COVER_SPLITS = [None, (2, False, None), (2, True, None), (4, True, None), (2, True, (16, 1)), (2, True, (32, 1)), (2, True, (32, 2)),
                (4, False, (32, 1))]


def SPLIT_ID(s):
    if s is None:
        return "product"
    return "ksplit%d_%s%s" % (s[0], "second_pass" if s[1] else "in_launch", "" if s[2] is None else "_mt%d_nb%d" % s[2])


@contextlib.contextmanager
def _split_build(request, split):
    """(hip, launches per call): the product build, or the measurement build with the K split factor, its finish and optionally
    the output block forced."""
    if split is None:
        from sige_amd import hip as h

        yield h, 1
        return
    h = request.getfixturevalue("tuning")
    h.conv_force_ksplit(split[0])
    h.conv_force_ksplit_pass(split[1])
    if split[2] is not None:
        h.conv_force_tile(*split[2])
    try:
        yield h, (2 if split[1] else 1)
    finally:
        h.conv_force_ksplit(0)
        h.conv_force_ksplit_pass(False)
        h.conv_force_tile(0, 0)


class _workspace:
    """Hands the K-split workspace request of hip.gather_conv_cl (torch.empty(8 * out.numel(), dtype=float32)) a buffer the TEST
    owns: the same memory in every run, whatever the allocator would do, and readable afterwards -- `copies()` counts the output
    copies the launch wrote partial sums into, i.e. the split factor it ran with (0: it did not split)."""

    def __init__(self, out_numel):
        self.buf = torch.full((8 * out_numel,), float("nan"), device=DEV)
        self.hits = 0

    def __enter__(self):
        self.real = torch.empty

        def empty(*a, **k):
            if len(a) == 1 and isinstance(a[0], int) and a[0] == self.buf.numel() and k.get("dtype") is torch.float32:
                self.hits += 1
                return self.buf
            return self.real(*a, **k)

        torch.empty = empty
        return self

    def __exit__(self, *exc):
        torch.empty = self.real
        return False

    def copies(self):
        wrote = [bool(torch.isfinite(c).any()) for c in self.buf.view(8, -1)]
        n = sum(wrote)
        assert wrote == [True] * n + [False] * (8 - n), wrote
        return n


def _splits(geo, split, B, N):
    """Does the launch split?  Forced: always (at least 2: (256, 0, 32) has 4 chunks at MT = 16, 8 at MT = 32).  The product build:
    below 112 blocks of 16 x 16 for 3x3 / s1 (B N x 2 blocks here), below 224 for stride 2 (plan_conv: kSplitBelow)."""
    return split is not None or geo == "K32" or B * N * 2 < 112


def _split_call(hip, geo, launches, B, name, alt, ws, full, out=None):
    """(256, 0, 32), raw staging, the first or the second image, with the workspace `ws`: to tiles, or to full with residual and
    out-affine + SiLU."""
    shape = D.SPLIT_SHAPE
    g = D.GEO[geo]
    c = T.case(*shape, B)
    packed = _pack(hip, geo, shape, B)
    args, _, _ = _gather_args(geo, shape, B, name, "raw", packed, alt=alt)
    kw = {}
    if full:
        _, residual = D.dest(geo, shape, B)
        kw = dict(out=out, full=dict(offset=(g.offset, g.offset), out_res=g.res, residual=_cl(residual)),
                  out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "swish"))
    h0 = ws.hits
    with util.poisoned(), ws, _default(hip, launches):
        got = hip.gather_conv_cl(*args, **kw)
    assert got is not None and ws.hits == h0 + 1, "the call asked for no workspace of 8 output copies"
    return got


def _split_full_ref(geo, B, name, alt, prev):
    shape = D.SPLIT_SHAPE
    c = T.case(*shape, B)
    _, residual = D.dest(geo, shape, B)
    v = lambda t: t.double().view(-1, 1, 1)  # noqa: E731
    base = _residual_fn(residual)
    return D.place(geo, prev, D.want_gather(geo, shape, B, name, "raw", alt=alt), D.lists(geo)[name], B,
                   lambda t, b, hs, ws: F.silu(v(c["os"]) * base(t, b, hs, ws) + v(c["oh"])))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("split", SPLITS, ids=SPLIT_ID)
def test_ksplit_to_tiles_and_full(request, split, B):
    """(256, 0, 32) on `every`, K = 2304: the launch splits K across workgroups -- ASSERTED from the workspace: at least two output
    copies hold partial sums (the product build at B = 2 has 140 blocks and stays unsplit: none).  In-launch finish: one launch;
    second pass: two.  Three runs, image 0 / 1 / 0, over ONE workspace the test owns: NaN before the first, then left holding the
    run before's partial sums -- a stale one would show."""
    shape = D.SPLIT_SHAPE
    cout = shape[2]
    prev, _ = D.dest("K31", shape, B)
    N = T.LISTS["every"].shape[0]
    with _split_build(request, split) as (hip, launches):
        split_here = _splits("K31", split, B, N)
        if not split_here:
            launches = 1
        ws_t, ws_f = _workspace(B * N * cout * 16), _workspace(B * cout * H * W)
        for run, alt in enumerate((False, True, False)):
            tag = "ksplit %s B%d run %d image %d" % (SPLIT_ID(split), B, run, alt)
            got = _split_call(hip, "K31", launches, B, "every", alt, ws_t, False)
            assert (ws_t.copies() >= 2) if split_here else (ws_t.copies() == 0), tag + ": %d copies written" % ws_t.copies()
            _check(got, D.want_gather("K31", shape, B, "every", "raw", alt=alt), tag + " -> tiles")
            got = _split_call(hip, "K31", launches, B, "every", alt, ws_f, True, _cl(prev))
            assert (ws_f.copies() >= 2) if split_here else (ws_f.copies() == 0), tag + ": %d copies written" % ws_f.copies()
            _check(got, _split_full_ref("K31", B, "every", alt, prev), tag + " -> full + residual + out-affine")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("geo", ["K31", "K32"])
@pytest.mark.parametrize("split", COVER_SPLITS, ids=SPLIT_ID)
def test_ksplit_full_leaves_uncovered_pixels(request, split, geo, B):
    """The coverage rule.  A K split into a full destination is allowed when tile pixels >= image pixels; the 34 tiles of `every34`
    pass it with the corner tile missing: 544 tile pixels for 468 image pixels at 3x3 / s1 (four live pixels missing: rows 16..17,
    columns 24..25), 136 for 117 at 3x3 / s2 (one: (8, 12) of 9 x 13 -- the second pass's division by the stride and its clipping).
    They must keep what the destination held, bit for bit, under both finishes: the second pass used to sum whole workspace copies
    and wrote uninitialised workspace there.  The split is asserted from the workspace."""
    shape = D.SPLIT_SHAPE
    g = D.GEO[geo]
    prev, _ = D.dest(geo, shape, B)
    idx = D.lists(geo)["every34"]
    N = idx.shape[0]
    assert N * g.ro * g.ro >= g.res[0] * g.res[1]
    miss = ~D.covered(geo, idx)
    assert int(miss.sum()) == (4 if geo == "K31" else 1)
    with _split_build(request, split) as (hip, launches):
        split_here = _splits(geo, split, B, N)
        if not split_here:
            launches = 1
        ws = _workspace(B * shape[2] * g.res[0] * g.res[1])
        for run, alt in enumerate((False, True)):
            tag = "coverage %s %s B%d run %d" % (geo, SPLIT_ID(split), B, run)
            got = _split_call(hip, geo, launches, B, "every34", alt, ws, True, _cl(prev))
            assert (ws.copies() >= 2) if split_here else (ws.copies() == 0), tag + ": %d copies written" % ws.copies()
            assert torch.equal(got.cpu()[:, :, miss], prev[:, :, miss]), tag + ": the missing tile's pixels were written"
            _check(got, _split_full_ref(geo, B, "every34", alt, prev), tag)


# ---- 8. fp16 and split fp16 operands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [None] + FORCED4, ids=CFG_ID)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.IDS)
def test_f16_k31_raw_staging(request, shape, B, cfg):
    """ConvGeoH, raw staging (also under upsample2x): the operand rounding is exactly .half() -- every element to the exact bound
    against fp64 of the rounded tiles and weights.  Chunks are 64 / 128 channels here: (32, 32, 64) is refused too.  The product
    build, and every forced output block (4 waves: the fp16 kernels have no 8-wave form)."""
    with _build(request, cfg) as hip:
        packed = _pack(hip, "K31", shape, B, "f16")
        for name in (D.NAMES if cfg is None else ("every", "holes", "corners")):
            for form in ("raw", "up"):
                _run_gather(hip, "K31", shape, B, name, form, packed, compute="f16")


@pytest.mark.parametrize("cfg", [None] + FORCED4, ids=CFG_ID)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", T.SHAPES, ids=D.IDS)
def test_f16_k31_affine_staging(request, shape, B, cfg):
    """ConvGeoH behind an affine / SiLU: the cases of tile3_common.f16_staged_cases(), the share criterion (that reference is held
    alone on the CPU by tests/test_tile_conv3_block6_inputs.py); product build and every forced output block."""
    mine = [(s, f) for s, sh, f in T.f16_staged_cases() if sh == shape]
    assert mine
    with _build(request, cfg) as hip:
        packed = _pack(hip, "K31", shape, B, "f16")
        for source, form in mine:
            for name in (T.NAMES if cfg is None else ("every", "holes", "corners")):
                if source == 1:
                    _run_gather(hip, "K31", shape, B, name, form, packed, compute="f16")
                else:
                    _run_sg(hip, shape, B, name, "shared", packed, compute="f16")


@pytest.mark.parametrize("geo,cfg", [("K11", c) for c in [None] + FORCED4] + [("K32", c) for c in [None] + FORCED_S2],
                         ids=lambda v: v if isinstance(v, str) else CFG_ID(v))
@pytest.mark.parametrize("shape", D.SHAPES[:4], ids=D.IDS)
def test_f16_k11_k32_raw_staging(request, geo, shape, cfg):
    """compute = "f16" on the two other geometries, raw staging.  (Stride 2 has no fp16 kernels: its pack is an fp32 one and the
    reference the unrounded one -- tile_default_common.compute_of.)"""
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, geo, shape, B, "f16")
            for name in (D.NAMES if cfg is None else ("every", "holes", "corners")):
                _run_gather(hip, geo, shape, B, name, "raw", packed, compute="f16")


@pytest.mark.parametrize("cfg", [None] + FORCED_NB1, ids=CFG_ID)
@pytest.mark.parametrize("geo", ["K31", "K11", "K32"])
@pytest.mark.parametrize("shape", [(64, 0, 64), (68, 0, 24)], ids=D.IDS)
def test_f16x3_gather_forms(request, geo, shape, cfg):
    """ConvGeoX (split fp16 operands) on the gather forms of items 1, 3 and 4: fp32-level results, held to the bound the project
    uses for this operand form (tests/test_gpu_round3.py: 2e-5 * (wmag + max |ref|), wmag = 1 here).  Product build, and MT = 16 and
    32 forced (this operand form has NB = 1 and 4 waves only; at stride 2 its pack is an fp32 one)."""
    forms = {"K31": list(T.GATHER_FORMS), "K11": ["raw", "affine"], "K32": ["raw", "affine+silu"]}[geo]
    with _build(request, cfg) as hip:
        for B in (1, 2):
            packed = _pack(hip, geo, shape, B, "f16x3")
            for name in D.NAMES:
                for form in forms:
                    _run_gather(hip, geo, shape, B, name, form, packed, compute="f16x3")
            if geo == "K31":
                for form in ("affine+silu", "up+affine+silu"):
                    _run_gather(hip, geo, shape, B, "every34", form, packed, kind="batch", compute="f16x3")
