"""The data-movement kernels of the sparse path against the CPU oracle on the ragged 18 x 26 image (tests/data_movement_common.py):
csrc/nhwc_ops.hip (gather, scatter_gather, both scatters fresh and in place, SPADE modulation), csrc/spade_ops.hip
(scatter_gather_split), csrc/gather.hip and csrc/scatter.hip (the NCHW forms, every launch form), the scatter map, the tile table and
the tile-list form of the first conv.  The last row and column of windows hang over the border in every geometry, the stride-2
scatters place 2x2 tiles at (off + origin) / 2 on a 9 x 13 output, the in-place scatters start from a buffer that is NOT the cached
tensor (a stray write of the right value shows), one block-residual case has shortcut tiles no main tile covers, and one case per
op is large enough for a second trip of the grid-stride loop.

Every case allocates under util.poisoned() (NaN), asserts its launch count and compares with the oracle: identity forms with
torch.equal, SiLU forms within util.SWISH_RTOL / SWISH_ATOL with the padding an exact 0.
tests/test_data_movement_inputs.py (CPU) shows that these references are right and that they discriminate."""
import pytest
import torch

from oracle import oracle
from tests import data_movement_common as D
from tests import tile3_common as T
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
DEV = torch.device("cuda")
CL = torch.channels_last
H, W = D.H, D.W
COMPARISONS = [0]


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    yield h
    print("\ndata movement on the ragged image: %d comparisons with the CPU references" % COMPARISONS[0])


def _cl(t, half=False):
    t = t.to(DEV).contiguous(memory_format=CL)
    return t.half() if half else t


def _dev(t):
    return None if t is None else t.to(DEV)


def _eq(got, want, tag):
    COMPARISONS[0] += 1
    assert tuple(got.shape) == tuple(want.shape), (tag, tuple(got.shape), tuple(want.shape))
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (
            tag, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


class _launches:
    """with _launches(hip, n): the library issued exactly n kernel launches inside (a fallback to torch, or a second pass, shows)."""

    def __init__(self, hip, n):
        self.hip, self.n = hip, n

    def __enter__(self):
        self.n0 = self.hip.launch_count()

    def __exit__(self, *exc):
        if exc[0] is None:
            got = self.hip.launch_count() - self.n0
            assert got == self.n, "expected %d launches, counted %d" % (self.n, got)
        return False


class _swish:
    """The SiLU criterion against the oracle and its worst margin of one test: |d| <= SWISH_RTOL |want| + SWISH_ATOL, i.e.
    |d| / (|want| + ATOL / RTOL) <= RTOL; padding an exact 0."""

    def __init__(self, test):
        self.test, self.worst = test, {}

    def check(self, op, got, want, live, tag):
        COMPARISONS[0] += 1
        got = got.cpu().contiguous()
        assert tuple(got.shape) == tuple(want.shape), tag
        if got.numel() == 0:
            return
        assert bool((got[~live.expand_as(got)] == 0).all()), tag + ": padding"
        m = float(((got - want).abs() / (want.abs() + util.SWISH_ATOL / util.SWISH_RTOL)).max())
        self.worst[op] = max(self.worst.get(op, 0.0), m)
        print("%s %s: %.3g (bound %.3g)" % (self.test, tag, m, util.SWISH_RTOL))
        assert m <= util.SWISH_RTOL, (tag, m)  # (NaN fails)

    def record(self):
        for op, m in self.worst.items():
            util.record_margin(self.test, op, m, util.SWISH_RTOL)


def _affine(c, kind):
    sc, sh = D.affine_of(c, kind)
    return _dev(sc), _dev(sh)


# ---- 1. scatter map and tile table ------------------------------------------------------------------------------------------------
def test_scatter_map_and_tile_table(hip):
    with util.poisoned():
        for name in D.NAMES + ["every34"]:
            idx = T.LISTS[name]
            idx_d = idx.to(DEV)
            with _launches(hip, 1):
                got = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx_d)
            _eq(got, oracle.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx), "map " + name)
        for geo, g in D.GEOS.items():
            for name in D.NAMES + ["every34"]:
                idx = g["lists"][name]
                with _launches(hip, 1):
                    got = hip.tile_table(idx.to(DEV), (g["offset"],) * 2, (g["stride"],) * 2, (g["tile"],) * 2, g["out_res"])
                _eq(got, D.hand_table(idx, geo), "table %s %s" % (geo, name))


# ---- 2. gather --------------------------------------------------------------------------------------------------------------------
def _run_gather(hip, geo, C, B, forms, test):
    c = D.case(C, B)
    b = D.GEOS[geo]["block"]
    sw = _swish("data_movement_ragged::%s[%s-%d-%d]" % (test, geo, C, B))
    with util.poisoned():
        x = {"cl": _cl(c["x"]), "cl f16": _cl(c["x"], half=True), "nchw": c["x"].to(DEV)}
        for name, kind, act in D.affine_cases(B):
            idx = D.GEOS[geo]["lists"][name]
            idx_d = idx.to(DEV)
            sc, sh = _affine(c, kind)
            n = 1 if idx.shape[0] else 0
            live = D.live(geo, idx, B)
            for form in forms:
                want = D.gather_ref(c, geo, idx, kind, act, half=form == "cl f16")
                with _launches(hip, n):
                    if form.startswith("cl"):
                        got = hip.gather_cl(x[form], b, b, idx_d, sc, sh, act)
                        assert hip.is_cl(got) or not n
                    else:
                        got = hip.gather(x["nchw"], b, b, idx_d, sc, sh, act, False)
                tag = "gather %s %s %s %s" % (form, name, kind, act)
                if act == "identity":
                    _eq(got, want, tag)
                else:
                    sw.check("gather " + form, got, want, live, tag)
    sw.record()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
@pytest.mark.parametrize("geo", list(D.GEOS))
def test_gather(hip, geo, C, B):
    """hip.gather_cl on an fp32 and an fp16-stored tensor and hip.gather in its automatic form: windows of 6, 4 and 5 pixels that
    leave the image at all four borders."""
    _run_gather(hip, geo, C, B, ("cl", "cl f16", "nchw"), "gather")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
@pytest.mark.parametrize("geo", list(D.GEOS))
def test_gather_one_tile_rows(hip, geo, C, B, tuning):
    """hip.gather with gather_force_rows(True) (a dispatch knob: the measurement build)."""
    hip.gather_force_rows(True)
    try:
        _run_gather(hip, geo, C, B, ("nchw rows",), "gather_one_tile_rows")
    finally:
        hip.gather_force_rows(False)


# ---- 3. scatter_gather ------------------------------------------------------------------------------------------------------------
def _run_scatter_gather(hip, C, B, forms, test):
    c = D.case(C, B)
    sw = _swish("data_movement_ragged::%s[%d-%d]" % (test, C, B))
    with util.poisoned():
        y = {"cl": _cl(c["y"]), "cl f16": _cl(c["y"], half=True), "nchw": c["y"].to(DEV)}
        for name, kind, act in D.affine_cases(B):
            idx = T.LISTS[name]
            idx_d = idx.to(DEV)
            smap = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx_d)
            sc, sh = _affine(c, kind)
            n = 1 if idx.shape[0] else 0
            live = D.live("G6", idx, B)
            for form in forms:
                t4, want = D.sg_ref(c, idx, kind, act, half=form == "cl f16")
                with _launches(hip, n):
                    if form.startswith("cl"):
                        got = hip.scatter_gather_cl(_cl(t4), y[form], 6, 6, idx_d, smap, sc, sh, act)
                        assert hip.is_cl(got) or not n
                    else:
                        got = hip.scatter_gather(t4.to(DEV), y["nchw"], 6, 6, idx_d, smap, sc, sh, act, False)
                tag = "scatter_gather %s %s %s %s" % (form, name, kind, act)
                if act == "identity":
                    _eq(got, want, tag)
                else:
                    sw.check("scatter_gather " + form, got, want, live, tag)
    sw.record()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
def test_scatter_gather(hip, C, B):
    """hip.scatter_gather_cl over an fp32 and an fp16-stored cache and hip.scatter_gather in its automatic form, through the device's
    own scatter map."""
    _run_scatter_gather(hip, C, B, ("cl", "cl f16", "nchw form 0"), "scatter_gather")


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
def test_scatter_gather_forced_forms(hip, C, B, form, tuning):
    """hip.scatter_gather with scatter_gather_force_elements(1 | 2): the element form and the one-tile row form (a dispatch knob: the
    measurement build)."""
    hip.scatter_gather_force_elements(form)
    try:
        _run_scatter_gather(hip, C, B, ("nchw form %d" % form,), "scatter_gather_forced_forms")
    finally:
        hip.scatter_gather_force_elements(0)


# ---- 4. scatter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
@pytest.mark.parametrize("geo", list(D.GEOS))
def test_scatter(hip, geo, C, B):
    """hip.scatter_cl fresh and in place over an fp32 and an fp16-stored cache, with and without a residual; hip.scatter and
    hip.scatter_fused.  In place the buffer starts as a random z: the oracle's value on the covered pixels, z's bits elsewhere; a
    second call with other tiles AND another list writes exactly its own covered pixels over that."""
    c = D.case(C, B)
    g = D.GEOS[geo]
    off, st = (g["offset"],) * 2, (g["stride"],) * 2
    with util.poisoned():
        for k, name in enumerate(D.NAMES):
            idx, idx2 = g["lists"][name], g["lists"][D.NAMES[(k + 1) % len(D.NAMES)]]
            idx_d, idx2_d = idx.to(DEV), idx2.to(DEV)
            N, N2 = idx.shape[0], idx2.shape[0]
            table = hip.tile_table(idx_d, off, st, (g["tile"],) * 2, g["out_res"])
            table2 = hip.tile_table(idx2_d, off, st, (g["tile"],) * 2, g["out_res"])
            cover, cover2 = D.covered(geo, idx), D.covered(geo, idx2)
            for half in (False, True):
                x, y, residual, z = D.scatter_inputs(c, geo, idx, "xa", half)
                x2 = D.scatter_inputs(c, geo, idx2, "xb", half)[0]
                x_cl, x2_cl, y_cl = _cl(x), _cl(x2), _cl(y, half=half)
                for r in (None, residual):
                    tag = "scatter %s %s%s%s" % (geo, name, " f16" if half else "", " + residual" if r is not None else "")
                    r_cl = None if r is None else _cl(r)
                    want, want2 = D.scatter_ref(x, y, geo, idx, r), D.scatter_ref(x2, y, geo, idx2, r)
                    with _launches(hip, 1):
                        got = hip.scatter_cl(x_cl, y_cl, off, st, idx_d, table, r_cl)
                    assert hip.is_cl(got)
                    _eq(got, want, tag + " fresh")
                    buf = _cl(z).clone(memory_format=torch.preserve_format)
                    with _launches(hip, 1 if N else 0):
                        out = hip.scatter_cl(x_cl, y_cl, off, st, idx_d, table, r_cl, out=buf)
                    assert out.data_ptr() == buf.data_ptr()
                    first = D.in_place(want, z, cover)
                    _eq(out, first, tag + " in place")
                    with _launches(hip, 1 if N2 else 0):
                        out = hip.scatter_cl(x2_cl, y_cl, off, st, idx2_d, table2, r_cl, out=buf)
                    _eq(out, D.in_place(want2, first, cover2), tag + " in place, second call")
                    if not half:
                        x_d, y_d, r_d = x.to(DEV), y.to(DEV), _dev(r)
                        with _launches(hip, 2):  # (the copy and the tile pass)
                            got = hip.scatter(x_d, y_d, off[0], off[1], st[0], st[1], idx_d, r_d)
                        _eq(got, want, tag + " nchw")
                        with _launches(hip, 1):
                            got = hip.scatter_fused(x_d, y_d, table, N, r_d)
                        _eq(got, want, tag + " nchw fused")


# ---- 5. block-residual scatter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
def test_scatter_with_block_residual(hip, C, B):
    """(a) every G6 list with shortcut cells inside its tiles; (b) holes with every other 4x4 cell as shortcut list: shortcut-only,
    main-only, doubly covered and uncovered pixels, so the in-place kernel's shortcut branch writes."""
    c = D.case(C, B)
    with util.poisoned():
        for tag0, idx0, idx1 in D.block_residual_lists():
            idx0_d, idx1_d = idx0.to(DEV), idx1.to(DEV)
            N0, N1 = idx0.shape[0], idx1.shape[0]
            t0 = hip.tile_table(idx0_d, (1, 1), (1, 1), (4, 4), (H, W))
            t1 = hip.tile_table(idx1_d, (0, 0), (1, 1), (4, 4), (H, W))
            _eq(t1, D.shortcut_table(idx1), "shortcut table " + tag0)
            cover = D.covered("G6", idx0) | D.covered_short(idx1)
            for half in (False, True):
                tag = "block residual %s%s" % (tag0, " f16" if half else "")
                x0, y0, x1, y1, z = D.block_residual_inputs(c, idx0, idx1, "xa", half)
                x0b = D.block_residual_inputs(c, idx0, idx1, "xb", half)[0]
                want, want_b = D.block_residual_ref(x0, y0, x1, y1, idx0, idx1), D.block_residual_ref(x0b, y0, x1, y1, idx0, idx1)
                a = (_cl(x0), _cl(y0, half=half), _cl(x1), _cl(y1, half=half))
                with _launches(hip, 1):
                    got = hip.scatter_with_block_residual_cl(*a, (1, 1), (1, 1), idx0_d, t0, idx1_d, t1)
                assert hip.is_cl(got)
                _eq(got, want, tag + " fresh")
                buf = _cl(z).clone(memory_format=torch.preserve_format)
                with _launches(hip, 1 if N0 + N1 else 0):
                    out = hip.scatter_with_block_residual_cl(*a, (1, 1), (1, 1), idx0_d, t0, idx1_d, t1, out=buf)
                assert out.data_ptr() == buf.data_ptr()
                _eq(out, D.in_place(want, z, cover), tag + " in place")
                with _launches(hip, 1 if N0 + N1 else 0):
                    out = hip.scatter_with_block_residual_cl(_cl(x0b), *a[1:], (1, 1), (1, 1), idx0_d, t0, idx1_d, t1, out=buf)
                _eq(out, D.in_place(want_b, z, cover), tag + " in place, second call")
                if not half:
                    n = tuple(t.to(DEV) for t in (x0, y0, x1, y1))
                    with _launches(hip, 3):  # (the copy, the main pass, the shortcut pass)
                        got = hip.scatter_with_block_residual(*n, 1, 1, 1, 1, idx0_d, idx1_d)
                    _eq(got, want, tag + " nchw")
                    with _launches(hip, 1):
                        got = hip.scatter_with_block_residual_fused(*n, t0, N0, t1, N1)
                    _eq(got, want, tag + " nchw fused")


# ---- 6. SPADE modulation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", D.CHANNELS)
def test_spade_modulate(hip, C, B):
    """Both normalized sources; gamma|beta through the map of ANOTHER list (holes), so some windows take them from tiles and some
    from the cache; with and without the leaky ReLU.  Reference: the oracle's tiles, then fp32 torch in the kernel's stated order."""
    c = D.case(C, B)
    idx_g = T.LISTS["holes"]
    with util.poisoned():
        map_g = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx_g.to(DEV))
        gb, gbt = _cl(c["gb"]), _cl(D.tiles_of(c["gbt"], idx_g.shape[0]))
        x, y = _cl(c["x"]), _cl(c["y"])
        for name in ("every", "corners", "empty"):
            idx = T.LISTS[name]
            idx_d = idx.to(DEV)
            smap = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx_d)
            t4 = _cl(D.tiles_of(c["t4"], idx.shape[0]))
            for kind in ("none", "shared") + (("batch",) if B == 2 else ()):
                sc, sh = _affine(c, kind)
                for slope in (None, D.SLOPE):
                    for source in (1, 2):
                        with _launches(hip, 1 if idx.shape[0] else 0):
                            if source == 1:
                                got = hip.spade_modulate_cl(x, None, None, sc, sh, gbt, gb, map_g, idx_d, (6, 6), slope)
                            else:
                                got = hip.spade_modulate_cl(y, t4, smap, sc, sh, gbt, gb, map_g, idx_d, (6, 6), slope)
                        _eq(got, D.spade_ref(c, idx, idx_g, source, kind, slope), "spade %s %s source %d slope %s" % (name, kind, source, slope))


# ---- 7. scatter_gather_split ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C,parts", D.SPLITS)
def test_scatter_gather_split(hip, C, parts, B):
    """Two and three parts of whole 4-channel units (24 channels divide both ways; 36 only by three, 64 only by two), ReLU and
    leaky: the oracle's scatter_gather, then the activation and the split on the CPU."""
    c = D.case(C, B)
    with util.poisoned():
        y = _cl(c["y"])
        for name in D.NAMES:
            idx = T.LISTS[name]
            idx_d = idx.to(DEV)
            smap = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx_d)
            for act in ("relu", "leaky"):
                t4, want = D.split_ref(c, idx, parts, act)
                with _launches(hip, 1 if idx.shape[0] else 0):
                    got = hip.scatter_gather_split_cl(_cl(t4), y, 6, 6, idx_d, smap, parts, act, D.SLOPE if act == "leaky" else 0.0)
                assert len(got) == parts
                for k in range(parts):
                    _eq(got[k], want[k], "split %s %s part %d of %d" % (name, act, k, parts))


def test_scatter_gather_split_refuses_half_units(hip):
    """36 channels in two parts would be four and a half units per part: refused, nothing launched."""
    c = D.case(36, 1)
    idx = T.LISTS["corners"]
    with util.poisoned():
        smap = hip.get_scatter_map(H, W, 6, 6, 3, 3, 1, 1, 1, 1, idx.to(DEV))
        with _launches(hip, 0), pytest.raises(RuntimeError):
            hip.scatter_gather_split_cl(_cl(D.tiles_of(c["t4"], 4)), _cl(c["y"]), 6, 6, idx.to(DEV), smap, 2, "relu")


# ---- 8. stacked edits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [36, 64])
def test_stacked_edits(hip, C):
    """hip.set_edit_batch(2): two different 16 x 26 images as one 32 x 26 tensor.  Every window equals that window of its own image
    ALONE through the oracle: rows 16.. of image 0's last windows are zero padding, not image 1's pixels.  B = 2 is refused."""
    c = D.stacked_case(C)
    idx = T.stacked_list()
    sw = _swish("data_movement_ragged::stacked[%d]" % C)
    live = torch.cat([D.live("G6", T.LIST_S, 1, (T.HS, W))] * 2, 0)
    hip.set_edit_batch(2)
    try:
        with util.poisoned():
            idx_d, smap = idx.to(DEV), T.stacked_map().to(DEV)
            x, y, gb = _cl(T.stack(c["xs"])), _cl(T.stack(c["ys"])), _cl(T.stack(c["gbs"]))
            t4, gbt = _cl(c["t4s"].reshape(2 * T.NS, C, 4, 4)), _cl(c["gbts"].reshape(2 * T.NS, 2 * C, 4, 4))
            sc, sh = c["scale1"].to(DEV), c["shift1"].to(DEV)
            for affine in (False, True):
                a = (sc, sh, "swish") if affine else (None, None, "identity")
                with _launches(hip, 1):
                    g1 = hip.gather_cl(x, 6, 6, idx_d, *a)
                with _launches(hip, 1):
                    g2 = hip.scatter_gather_cl(t4, y, 6, 6, idx_d, smap, *a)
                for source, got in ((1, g1), (2, g2)):
                    want = T.stacked_tiles(c, source, affine)
                    tag = "stacked source %d %s" % (source, "affine+silu" if affine else "raw")
                    if affine:
                        sw.check("stacked source %d" % source, got, want, live, tag)
                    else:
                        _eq(got, want, tag)
                    last = got[:T.NS].reshape(4, 7, C, 6, 6)[3]  # image 0's windows at origin row 11: row 5 is row 16
                    assert bool((last[..., 5, :] == 0).all()), tag + ": the row beyond image 0 is not zero"
            for slope in (None, D.SLOPE):
                with _launches(hip, 1):
                    got = hip.spade_modulate_cl(x, None, None, sc, sh, gbt, gb, smap, idx_d, (6, 6), slope)
                _eq(got, D.stacked_spade_ref(c, 1, slope), "stacked spade source 1 slope %s" % slope)
                with _launches(hip, 1):
                    got = hip.spade_modulate_cl(y, t4, smap, sc, sh, gbt, gb, smap, idx_d, (6, 6), slope)
                _eq(got, D.stacked_spade_ref(c, 2, slope), "stacked spade source 2 slope %s" % slope)
            # two stacked tensors in one batch: refused before anything is launched, so nothing is written
            x2, y2, gb2 = (torch.cat([t, t], 0) for t in (x, y, gb))
            t42, gbt2 = torch.cat([t4, t4], 0), torch.cat([gbt, gbt], 0)
            for call in (lambda: hip.gather_cl(x2, 6, 6, idx_d), lambda: hip.scatter_gather_cl(t42, y2, 6, 6, idx_d, smap),
                         lambda: hip.spade_modulate_cl(x2, None, None, sc, sh, gbt2, gb2, smap, idx_d, (6, 6), None)):
                with _launches(hip, 0), pytest.raises(RuntimeError):
                    call()
    finally:
        hip.set_edit_batch(1)
    sw.record()


# ---- 9. the tile-list form of the first conv --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["every", "corners", "holes"])
def test_conv3x3_small_cin_tiles(hip, name, layout):
    """Only the 6x6 windows of the list, clipped at all four borders, are evaluated, in place: inside them the fp64 conv of the whole
    image within 1e-5, outside them the buffer's bits."""
    c = D.conv_in_case()
    idx = T.LISTS[name]
    inside = D.window_mask(idx)
    with util.poisoned():
        x = _cl(c["x"]) if layout == "nhwc" else c["x"].to(DEV)
        buf = _cl(c["z"]).clone(memory_format=torch.preserve_format)
        with _launches(hip, 1):
            out = hip.conv3x3_small_cin_cl(x, c["w"].to(DEV), c["bias"].to(DEV), tiles=(idx.to(DEV), (6, 6)), out=buf)
        assert out is not None and out.data_ptr() == buf.data_ptr()
        got = out.cpu().contiguous()
    COMPARISONS[0] += 2
    d = (got.double() - c["want"])[:, :, inside].abs().max()
    print("conv3x3_small_cin tiles %s %s: %.3g (bound 1e-5)" % (name, layout, float(d)))
    assert float(d) <= 1e-5, float(d)  # (NaN fails)
    assert torch.equal(got[:, :, ~inside].view(torch.int32), c["z"][:, :, ~inside].view(torch.int32)), "a pixel outside the windows was written"


# ---- 10. the second trip of the grid-stride loop ------------------------------------------------------------------------------------
def _big(op):
    C, units = D.BIG_UNITS[op]
    assert units > 16384 * 256 == D.TRIP, (op, units)  # (csrc/nhwc_ops.hip grid_for; csrc/spade_ops.hip grid_of caps at half of it)
    return C, units


def test_second_trip_gather(hip):
    C, units = _big("gather")
    d = D.big_case("gather")
    assert D.NBIG * 36 * (C // 4) == units
    with util.poisoned():
        with _launches(hip, 1):
            got = hip.gather_cl(_cl(d["x"]), 6, 6, D.LIST_BIG.to(DEV))
        _eq(got, d["want"], "gather, %d units" % units)


def test_second_trip_scatter_gather(hip):
    C, units = _big("scatter_gather")
    d = D.big_case("scatter_gather")
    assert tuple(d["want"].shape) == (D.NBIG, C, 6, 6) and d["want"].numel() // 4 == units
    with util.poisoned():
        with _launches(hip, 1):
            got = hip.scatter_gather_cl(_cl(d["t4"]), _cl(d["y"]), 6, 6, D.LIST_BIG.to(DEV), d["smap"].to(DEV))
        _eq(got, d["want"], "scatter_gather, %d units" % units)


def test_second_trip_scatter_gather_split(hip):
    C, units = _big("split")
    d = D.big_case("scatter_gather")
    assert d["want"].numel() // 4 == units
    with util.poisoned():
        with _launches(hip, 1):
            got = hip.scatter_gather_split_cl(_cl(d["t4"]), _cl(d["y"]), 6, 6, D.LIST_BIG.to(DEV), d["smap"].to(DEV), 2, "relu")
        for k, want in enumerate(torch.split(torch.relu(d["want"]), C // 2, dim=1)):
            _eq(got[k], want, "split part %d, %d units" % (k, units))
    D._BIG.clear()


def test_second_trip_spade_modulate(hip):
    C, units = _big("spade")
    d = D.big_case("spade")
    assert d["want"].numel() // 4 == units
    with util.poisoned():
        idx_d, smap = D.LIST_BIG.to(DEV), d["smap"].to(DEV)
        with _launches(hip, 1):
            got = hip.spade_modulate_cl(_cl(d["x"]), None, None, d["scale1"].to(DEV), d["shift1"].to(DEV), _cl(d["gbt"]), _cl(d["gb"]), smap,
                                        idx_d, (6, 6), D.SLOPE)
        _eq(got, d["want"], "spade, %d units" % units)


def test_second_trip_scatter(hip):
    C, units = _big("scatter")
    units_in_place = _big("scatter_in_place")[1]
    d = D.big_case("scatter")
    assert d["y"].numel() // 4 == units and d["x"].numel() // 4 == units_in_place
    cover = T.covered(D.LIST_BIG, (D.BIG, D.BIG))
    with util.poisoned():
        idx_d = D.LIST_BIG.to(DEV)
        table = hip.tile_table(idx_d, (1, 1), (1, 1), (4, 4), (D.BIG, D.BIG))
        x, y = _cl(d["x"]), _cl(d["y"])
        with _launches(hip, 1):
            got = hip.scatter_cl(x, y, (1, 1), (1, 1), idx_d, table)
        _eq(got, d["want"], "scatter fresh, %d units" % units)
        buf = _cl(d["z"]).clone(memory_format=torch.preserve_format)
        with _launches(hip, 1):
            out = hip.scatter_cl(x, y, (1, 1), (1, 1), idx_d, table, out=buf)
        _eq(out, D.in_place(d["want"], d["z"], cover), "scatter in place, %d units" % units_in_place)


def test_second_trip_scatter_with_block_residual(hip):
    C, units = _big("block_residual")
    units_in_place = _big("block_residual_in_place")[1]
    d = D.big_case("block_residual")
    assert d["y"].numel() // 4 == units and (d["x"].numel() + d["x1"].numel()) // 4 == units_in_place
    cover = T.covered(D.LIST_BIG, (D.BIG, D.BIG))  # (the shortcut cells lie inside the main tiles)
    with util.poisoned():
        idx_d, idx1_d = D.LIST_BIG.to(DEV), d["idx1"].to(DEV)
        t0 = hip.tile_table(idx_d, (1, 1), (1, 1), (4, 4), (D.BIG, D.BIG))
        t1 = hip.tile_table(idx1_d, (0, 0), (1, 1), (4, 4), (D.BIG, D.BIG))
        a = (_cl(d["x"]), _cl(d["y"]), _cl(d["x1"]), _cl(d["y1"]))
        with _launches(hip, 1):
            got = hip.scatter_with_block_residual_cl(*a, (1, 1), (1, 1), idx_d, t0, idx1_d, t1)
        _eq(got, d["want"], "block residual fresh, %d units" % units)
        buf = _cl(d["z"]).clone(memory_format=torch.preserve_format)
        with _launches(hip, 1):
            out = hip.scatter_with_block_residual_cl(*a, (1, 1), (1, 1), idx_d, t0, idx1_d, t1, out=buf)
        _eq(out, D.in_place(d["want"], d["z"], cover), "block residual in place, %d units" % units_in_place)
