"""Shared by the tests of the data-movement kernels (csrc/nhwc_ops.hip, spade_ops.hip, gather.hip, scatter.hip, the scatter map and
the tile table) on the ragged 18 x 26 image of tests/tile3_common.py: geometries, lists, seeded CPU inputs and the CPU references
(the oracle, hand placement loops, fp32 torch in the kernels' stated order).  Nothing here touches a device
(tests/test_data_movement_inputs.py runs it without one).

Geometries, all over a 5 x 7 grid of windows whose last row and column hang over the border:
  G6   6x6 windows at 4i - 1, 4x4 outputs at origin + 1 (offset 1, stride 1)            -- the 3x3 convs
  G4   4x4 windows at 4i, offset 0: rows 16..19 of 18, columns 24..27 of 26               -- the 1x1 convs and shortcuts
  G5a  5x5 windows at 4i, stride 2, offset 0: 2x2 outputs at (off + origin) / 2 on 9 x 13  -- the DDPM Downsample
  G5b  5x5 windows at 4i - 1, stride 2, offset 1                                         -- the SD Downsample"""
import torch

from oracle import oracle
from tests import tile3_common as T
from tests.block10_common import tile_lists

H, W = T.H, T.W
CHANNELS = (4, 36, 64)   # one 4-channel unit per pixel; an odd unit count that is no power of two; the common case
NAMES = T.NAMES          # every, corners, interior, holes, empty (every34: the even list of a per-batch affine at B = 2)
NMAX = 35


def _lists(pad):
    d = dict(T.LISTS if pad == 1 else tile_lists(5, 7, 4, 0))
    d["every34"] = d["every"][:-1].contiguous()
    return d


# name -> window size, lists, scatter offset / stride, output tile and output resolution
GEOS = {
    "G6": dict(block=6, lists=_lists(1), offset=1, stride=1, tile=4, out_res=(H, W)),
    "G4": dict(block=4, lists=_lists(0), offset=0, stride=1, tile=4, out_res=(H, W)),
    "G5a": dict(block=5, lists=_lists(0), offset=0, stride=2, tile=2, out_res=(H // 2, W // 2)),
    "G5b": dict(block=5, lists=_lists(1), offset=1, stride=2, tile=2, out_res=(H // 2, W // 2)),
}
AFFINES = ("none", "shared", "batch")
ACTS = ("identity", "swish")

# 5(b): main list `holes` of G6, shortcut list every other 4x4 cell -- shortcut-only, main-only, doubly covered, uncovered pixels
SHORT_B = tile_lists(5, 7, 4, 0)["every"][::2].contiguous()
KINDS_B = {"shortcut_only": 76, "main_only": 152, "both": 160, "neither": 80}

BIG = 130                 # item 10: 33 x 33 G6 windows on 130 x 130 (the last row and column hang over), second grid-stride trip
LIST_BIG = tile_lists(33, 33, 4, 1)["every"]
TRIP = 16384 * 256        # csrc/nhwc_ops.hip grid_for: workgroups x lanes of the largest launch


def cdiv(a, b):
    """C's integer division (towards zero), as the kernels and the reference compute (off + origin) / stride."""
    return int(a / b)


def origin(geo, h0, w0):
    g = GEOS[geo] if isinstance(geo, str) else geo
    return cdiv(g["offset"] + h0, g["stride"]), cdiv(g["offset"] + w0, g["stride"])


_CASES = {}


def case(C, B):
    """Seeded CPU inputs of one channel count and batch, made once and never written to."""
    key = (C, B)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(100 * C + B + 11)
        r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        d = dict(x=r(B, C, H, W), y=r(B, C, H, W), scale=r(B, C, 1, 1), shift=r(B, C, 1, 1), scale1=r(1, C, 1, 1), shift1=r(1, C, 1, 1),
                 t4=r(B, NMAX, C, 4, 4), y1=r(B, C, H, W), x1=r(B, NMAX, C, 4, 4),
                 gb=r(B, 2 * C, H, W), gbt=r(B, NMAX, 2 * C, 4, 4))
        for t, res in ((4, (H, W)), (2, (H // 2, W // 2))):  # scatter: tiles of two calls, cached tensor, residual, the buffer z
            d[t] = dict(xa=r(B, NMAX, C, t, t), xb=r(B, NMAX, C, t, t), y=r(B, C, *res), residual=r(B, C, *res), z=r(B, C, *res))
        _CASES[key] = d
    return _CASES[key]


def tiles_of(t, N):
    """[B, NMAX, C, r, s] -> the first N tiles of every image as [B * N, C, r, s]."""
    return t[:, :N].reshape(t.shape[0] * N, *t.shape[2:]).contiguous()


def affine_of(c, kind):
    return {"none": (None, None), "shared": (c["scale1"], c["shift1"]), "batch": (c["scale"], c["shift"])}[kind]


def affine_cases(B):
    """(list name, affine kind, activation) of the gather / scatter_gather matrix: every list x {none, shared} x {identity, swish};
    at B = 2 the per-batch affine on the even list."""
    out = [(n, k, a) for n in NAMES for k in ("none", "shared") for a in ACTS]
    if B == 2:
        out += [("every34", "batch", a) for a in ACTS]
    return out


# ---- 1. scatter map and tile table ----------------------------------------------------------------------------------------------
def hand_table(idx, geo):
    """[gH, gW] int32: the tile of `idx` whose output starts in each out-tile-sized cell of the output (-1: none), built by hand."""
    g = GEOS[geo]
    t = g["tile"]
    table = torch.full((-(-g["out_res"][0] // t), -(-g["out_res"][1] // t)), -1, dtype=torch.int32)
    for n, (h0, w0) in enumerate(idx.tolist()):
        h, w = origin(g, h0, w0)
        if h >= 0 and w >= 0 and h // t < table.shape[0] and w // t < table.shape[1]:
            table[h // t, w // t] = n
    return table


def scatter_map(idx, res=(H, W)):
    return T.scatter_map(idx, res)


# ---- 2 / 3. gather and scatter_gather -------------------------------------------------------------------------------------------
def gather_ref(c, geo, idx, kind="none", act="identity", half=False):
    sc, sh = affine_of(c, kind)
    x = c["x"].half().float() if half else c["x"]
    b = GEOS[geo]["block"]
    return oracle.gather(x, b, b, idx, sc, sh, act)


def sg_ref(c, idx, kind="none", act="identity", half=False):
    """(conv-1 tiles [B*N,C,4,4], the oracle's 6x6 scatter_gather tiles) on G6."""
    sc, sh = affine_of(c, kind)
    y = c["y"].half().float() if half else c["y"]
    t4 = tiles_of(c["t4"], idx.shape[0])
    return t4, oracle.scatter_gather(t4, y, 6, 6, idx, scatter_map(idx), sc, sh, act)


def live(geo, idx, B, res=(H, W)):
    """[B*N,1,b,b] bool: the window pixels inside the image (the others are zero padding, also behind an affine)."""
    b = GEOS[geo]["block"]
    return oracle.gather(torch.ones(B, 1, *res), b, b, idx) > 0


# ---- 4. scatter -----------------------------------------------------------------------------------------------------------------
def scatter_inputs(c, geo, idx, which="xa", half=False):
    """(tiles [B*N,C,t,t], cached y, residual, the in-place buffer's start z) of one geometry."""
    d = c[GEOS[geo]["tile"]]
    y = d["y"].half().float() if half else d["y"]
    return tiles_of(d[which], idx.shape[0]), y, d["residual"], d["z"]


def scatter_ref(x, y, geo, idx, residual=None):
    g = GEOS[geo]
    return oracle.scatter(x, y, g["offset"], g["offset"], g["stride"], g["stride"], idx, residual)


def hand_scatter(x, y, geo, idx, residual=None, plain_offset=False):
    """The placement loop written out: y with tile n of image b on the pixels (off + origin) / stride + [0,t)^2, clipped at the bottom
    and right border, + the residual there.  plain_offset: the WRONG origin off + origin (the stride-2 division dropped)."""
    g = GEOS[geo]
    out = y.clone()
    B, N = y.shape[0], idx.shape[0]
    Ho, Wo = y.shape[2], y.shape[3]
    for b in range(B):
        for n, (h0, w0) in enumerate(idx.tolist()):
            h0, w0 = (g["offset"] + h0, g["offset"] + w0) if plain_offset else origin(g, h0, w0)
            h1, w1 = min(h0 + x.shape[2], Ho), min(w0 + x.shape[3], Wo)
            if h1 <= h0 or w1 <= w0:
                continue
            v = x[b * N + n][:, :h1 - h0, :w1 - w0]
            out[b, :, h0:h1, w0:w1] = v if residual is None else residual[b, :, h0:h1, w0:w1] + v
    return out


def covered(geo, idx):
    """[Ho, Wo] bool: the output pixels a tile of `idx` writes."""
    g = GEOS[geo]
    m = torch.zeros(g["out_res"], dtype=torch.bool)
    for h0, w0 in idx.tolist():
        h, w = origin(g, h0, w0)
        m[h:h + g["tile"], w:w + g["tile"]] = True
    return m


def in_place(want, z, cover):
    """What an in-place call leaves in a buffer that started as `z`: the reference on the covered pixels, z's bits elsewhere."""
    return torch.where(cover[None, None], want, z)


# ---- 5. block-residual scatter --------------------------------------------------------------------------------------------------
def shortcut_table(idx1):
    table = torch.full((-(-H // 4), -(-W // 4)), -1, dtype=torch.int32)
    for n, (h0, w0) in enumerate(idx1.tolist()):
        table[h0 // 4, w0 // 4] = n
    return table


def block_residual_lists():
    """(tag, main list, shortcut list): (a) every G6 list with the shortcut cells inside its tiles; (b) holes with every other cell."""
    out = [("a-" + name, T.LISTS[name], T.shortcut(T.LISTS[name])[0]) for name in NAMES]
    out.append(("b-holes", T.LISTS["holes"], SHORT_B))
    return out


def covered_short(idx1):
    m = torch.zeros((H, W), dtype=torch.bool)
    for h0, w0 in idx1.tolist():
        m[h0:h0 + 4, w0:w0 + 4] = True
    return m


def block_residual_inputs(c, idx0, idx1, which="xa", half=False):
    d = c[4]
    y0, y1 = (d["y"].half().float(), c["y1"].half().float()) if half else (d["y"], c["y1"])
    return tiles_of(d[which], idx0.shape[0]), y0, tiles_of(c["x1"], idx1.shape[0]), y1, d["z"]


def block_residual_ref(x0, y0, x1, y1, idx0, idx1):
    return oracle.scatter_with_block_residual(x0, y0, x1, y1, 1, 1, 1, 1, idx0, idx1)


def hand_block_residual(x0, y0, x1, y1, idx0, idx1):
    """scatter.cpp's two passes written out: main tiles x0 + y1 over a copy of y0, then + (x1 - y1) under the shortcut tiles."""
    out = hand_scatter(x0, y0, "G6", idx0, residual=y1)
    B, N1 = y0.shape[0], idx1.shape[0]
    for b in range(B):
        for n, (h0, w0) in enumerate(idx1.tolist()):
            h1, w1 = min(h0 + 4, H), min(w0 + 4, W)
            out[b, :, h0:h1, w0:w1] = out[b, :, h0:h1, w0:w1] + (x1[b * N1 + n][:, :h1 - h0, :w1 - w0] - y1[b, :, h0:h1, w0:w1])
    return out


# ---- 6. SPADE modulation ----------------------------------------------------------------------------------------------------------
SLOPE = 0.2


def sg_own_list(x, y, idx, smap, sc=None, sh=None):
    """scatter_gather of tiles that belong to ANOTHER list than `idx` (the gamma|beta tiles through their own map): one image per
    oracle call, since the oracle offsets image b's tiles by b * len(idx)."""
    B = y.shape[0]
    Nx = x.shape[0] // B
    one = lambda v, b: None if v is None else v[b % v.shape[0]][None].contiguous()  # noqa: E731
    return torch.cat([oracle.scatter_gather(x[b * Nx:(b + 1) * Nx].contiguous(), y[b:b + 1].contiguous(), 6, 6, idx, smap,
                                            one(sc, b), one(sh, b), "identity") for b in range(B)], 0)


def modulate(n, gb, slope):
    """fp32, the kernel's stated order: 1 + gamma, product, + beta, leaky (n = the oracle's scale, shift tiles; padding stays 0)."""
    C = n.shape[1]
    gamma, beta = gb[:, :C], gb[:, C:]
    z = n * (1.0 + gamma)
    z = z + beta
    return z if slope is None else torch.where(z > 0, z, z * torch.tensor(slope, dtype=torch.float32))


def spade_ref(c, idx, idx_g, source, kind, slope):
    """Normalized source 1: gather of x; 2: scatter_gather of (conv tiles, cache y) through idx's own map.  gamma|beta: (gb tiles of
    the list idx_g, gb cache) through idx_g's map, on the windows of idx."""
    sc, sh = affine_of(c, kind)
    if source == 1:
        n = oracle.gather(c["x"], 6, 6, idx, sc, sh, "identity")
    else:
        n = sg_own_list(tiles_of(c["t4"], idx.shape[0]), c["y"], idx, scatter_map(idx), sc, sh)
    g = sg_own_list(tiles_of(c["gbt"], idx_g.shape[0]), c["gb"], idx, scatter_map(idx_g))
    return modulate(n, g, slope)


# ---- 7. scatter_gather_split ----------------------------------------------------------------------------------------------------
SPLITS = ((24, 2), (24, 3), (36, 3), (64, 2))   # (C, parts): a part is a whole number of 4-channel units, C % (4 parts) == 0


def split_ref(c, idx, parts, act):
    t4, sg = sg_ref(c, idx)
    z = torch.relu(sg) if act == "relu" else torch.where(sg > 0, sg, sg * torch.tensor(SLOPE, dtype=torch.float32))
    return t4, torch.split(z, sg.shape[1] // parts, dim=1)


# ---- 8. stacked edits -------------------------------------------------------------------------------------------------------------
_STACKED = {}


def stacked_case(C):
    """Two different 16 x 26 images (tests/tile3_common.py: xs, ys, t4s) plus their gamma|beta cache and tiles."""
    if C not in _STACKED:
        c = dict(T.case(C, 0, 4, 1))
        gen = torch.Generator().manual_seed(C + 8)
        c["gbs"] = torch.randn(2, 2 * C, T.HS, W, generator=gen)
        c["gbts"] = torch.randn(2, T.NS, 2 * C, 4, 4, generator=gen)
        _STACKED[C] = c
    return _STACKED[C]


def stacked_spade_ref(c, source, slope):
    """Each image ALONE through the oracle (zero padding beyond its own 16 rows), image 0's tiles first."""
    out = []
    m = scatter_map(T.LIST_S, (T.HS, W))
    for e in range(2):
        if source == 1:
            n = oracle.gather(c["xs"][e:e + 1].contiguous(), 6, 6, T.LIST_S, c["scale1"], c["shift1"], "identity")
        else:
            n = oracle.scatter_gather(c["t4s"][e].contiguous(), c["ys"][e:e + 1].contiguous(), 6, 6, T.LIST_S, m, c["scale1"], c["shift1"],
                                      "identity")
        g = oracle.scatter_gather(c["gbts"][e].contiguous(), c["gbs"][e:e + 1].contiguous(), 6, 6, T.LIST_S, m)
        out.append(modulate(n, g, slope))
    return torch.cat(out, 0)


def seamless_gather(c, affine):
    """The WRONG stacked reference: the tall tensor as ONE image, so image 0's last windows read image 1's first rows."""
    sc, sh = (c["scale1"], c["shift1"]) if affine else (None, None)
    return oracle.gather(T.stack(c["xs"]), 6, 6, T.stacked_list(), sc, sh, "swish" if affine else "identity")


# ---- 9. the tile-list form of conv3x3_small_cin_cl ------------------------------------------------------------------------------
def window_mask(idx, block=6, res=(H, W)):
    """[H, W] bool: the pixels of the block x block windows at `idx`, clipped at all four borders."""
    m = torch.zeros(res, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[max(h0, 0):h0 + block, max(w0, 0):w0 + block] = True
    return m


_CONV_IN = {}


def conv_in_case(B=2, C=3, cout=128):
    key = (B, C, cout)
    if key not in _CONV_IN:
        gen = torch.Generator().manual_seed(B + C + cout)
        x = torch.randn(B, C, H, W, generator=gen)
        w = torch.randn(cout, C, 3, 3, generator=gen) / (3 * C ** 0.5)
        bias = torch.randn(cout, generator=gen)
        z = torch.randn(B, cout, H, W, generator=gen)
        want = torch.nn.functional.conv2d(x.double(), w.double(), bias.double(), 1, 1)
        _CONV_IN[key] = dict(x=x, w=w, bias=bias, z=z, want=want)
    return _CONV_IN[key]


# ---- 10. the second trip of the grid-stride loop ----------------------------------------------------------------------------------
NBIG = LIST_BIG.shape[0]
# op -> (channels, four-channel units of the launch) from the shapes alone
BIG_UNITS = {"gather": (512, NBIG * 36 * 128), "scatter_gather": (512, NBIG * 36 * 128), "split": (512, NBIG * 36 * 128),
             "spade": (512, NBIG * 36 * 128), "scatter": (1024, BIG * BIG * 256), "scatter_in_place": (1024, NBIG * 16 * 256),
             "block_residual": (1024, BIG * BIG * 256), "block_residual_in_place": (1024, (NBIG + (NBIG + 1) // 2) * 16 * 256)}
_BIG = {}


def big_case(op):
    """Inputs and the oracle's output of one large case: all 1089 G6 windows of a 130 x 130 image.  (scatter_gather's are kept: the
    split form shares them.)"""
    if op in _BIG:
        return _BIG[op]
    N = NBIG
    gen = torch.Generator().manual_seed(len(op) + 130)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    res = (BIG, BIG)
    smap = scatter_map(LIST_BIG, res)
    C = BIG_UNITS[op][0]
    if op == "gather":
        d = dict(x=r(1, C, BIG, BIG))
        d["want"] = oracle.gather(d["x"], 6, 6, LIST_BIG)
    elif op == "scatter_gather":
        d = dict(t4=r(N, C, 4, 4), y=r(1, C, BIG, BIG), smap=smap)
        d["want"] = oracle.scatter_gather(d["t4"], d["y"], 6, 6, LIST_BIG, smap)
        _BIG[op] = d
    elif op == "scatter":
        d = dict(x=r(N, C, 4, 4), y=r(1, C, BIG, BIG), z=r(1, C, BIG, BIG))
        d["want"] = oracle.scatter(d["x"], d["y"], 1, 1, 1, 1, LIST_BIG)
    elif op == "block_residual":
        d = dict(x=r(N, C, 4, 4), y=r(1, C, BIG, BIG), y1=r(1, C, BIG, BIG), z=r(1, C, BIG, BIG), idx1=(LIST_BIG[::2] + 1).contiguous())
        d["x1"] = r(d["idx1"].shape[0], C, 4, 4)
        d["want"] = oracle.scatter_with_block_residual(d["x"], d["y"], d["x1"], d["y1"], 1, 1, 1, 1, LIST_BIG, d["idx1"])
    elif op == "spade":
        d = dict(x=r(1, C, BIG, BIG), gb=r(1, 2 * C, BIG, BIG), gbt=r(N, 2 * C, 4, 4), scale1=r(1, C, 1, 1), shift1=r(1, C, 1, 1), smap=smap)
        n = oracle.gather(d["x"], 6, 6, LIST_BIG, d["scale1"], d["shift1"], "identity")
        g = oracle.scatter_gather(d["gbt"], d["gb"], 6, 6, LIST_BIG, smap)
        d["want"] = modulate(n, g, SLOPE)
    else:
        raise KeyError(op)
    d["C"] = C
    return d
