"""Shared by the tests of the DEFAULT channels-last tile conv (csrc/conv_mfma.hpp: ConvGeo / ConvGeoH / ConvGeoX, launched by
csrc/block_conv.hip: plan_conv, launch_conv) on a ragged image: what tests/tile3_common.py does not already hold -- the two other
tile geometries, the channel shapes chosen from the kernel's chunk sizes, cached fp64 references, and plan_conv's usable() restated.
Nothing here touches a device (tests/test_tile_conv_default_inputs.py runs it without one).

Geometries, all on tile3_common's 18 x 26 image (neither side a multiple of the 4-pixel step):
  K31  3x3 / stride 1 on 6x6 windows at origins (4i - 1, 4j - 1), 4x4 outputs at origin + 1 (tile3_common's own);
  K11  1x1 on 4x4 blocks at origins (4i, 4j), offset 0: the last row covers rows 16..19 of 18, the last column 24..27 of 26;
  K32  3x3 / stride 2 on 5x5 blocks at origins (4i, 4j), offset 0 (the Downsample with pad (0, 1, 0, 1)): output 9 x 13, 2x2
       outputs at (2i, 2j), row 9 and column 13 clipped; N = 35 leaves a ragged last M block at 8 and at 4 tiles per block."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import oracle
from tests import tile3_common as T
from tests.block10_common import tile_lists

H, W = T.H, T.W
Geo = namedtuple("Geo", "block kernel stride offset ro res")
GEO = {"K31": Geo(6, 3, 1, 1, 4, (H, W)), "K11": Geo(4, 1, 1, 0, 4, (H, W)), "K32": Geo(5, 3, 2, 0, 2, (9, 13))}

# lists of K11 / K32: the same 5 x 7 grid at pad 0
LISTS0 = dict(tile_lists(5, 7, 4, 0))
LISTS0["every34"] = LISTS0["every"][:-1].contiguous()
LISTS0["every32"] = LISTS0["every"][:32].contiguous()  # (K32: whole M blocks of 8 and of 4 tiles)
NAMES = T.NAMES + ["every34"]

# (C1, C2, Cout), from the kernel's constants: the chunk CC is 32 channels at MT = 32 and 64 at MT = 16 for 3x3 (fp32 operands;
# 64 / 128 for fp16 ones), 128 / 256 for 1x1; chunk counts are padded to even
SHAPES = [(64, 0, 64),     # the plain case
          (68, 0, 24),     # ragged last chunk, partial output block
          (96, 0, 40),     # odd chunk count at MT = 32
          (256, 0, 32),    # deep enough for the K split: 4 chunks at MT = 16
          (64, 64, 72),    # cat on a chunk boundary
          (32, 32, 64),    # cat usable at MT = 32 only
          (20, 44, 64)]    # cat on no chunk boundary: refused
SPLIT_SHAPE = (256, 0, 32)
IDS = lambda s: "%d+%d_%d" % tuple(s)  # noqa: E731


def lists(geo):
    return T.LISTS if geo == "K31" else LISTS0


_EXTRA = {}


def extra(c1, c2, cout, B):
    """What tile3_common.case does not hold: the 1x1 weights, a 9 x 13 destination and residual (K32), a second image for runs that
    alternate two inputs over one workspace.  Seeded, made once, never written to."""
    key = (c1, c2, cout, B)
    if key not in _EXTRA:
        gen = torch.Generator().manual_seed(1000 * c1 + 100 * c2 + 10 * cout + B + 11)
        C = c1 + c2
        r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        _EXTRA[key] = dict(w1=r(cout, C, 1, 1) / C ** 0.5, bias1=r(cout), prev2=r(B, cout, 9, 13), residual2=r(B, cout, 9, 13),
                           x_alt=r(B, c1, H, W))
    return _EXTRA[key]


def weights(geo, shape, B):
    """(weight, bias) of one geometry: the 3x3 of tile3_common.case, or the 1x1."""
    if geo == "K11":
        e = extra(*shape, B)
        return e["w1"], e["bias1"]
    c = T.case(*shape, B)
    return c["w"], c["bias"]


def dest(geo, shape, B):
    """(what the full destination held before, residual) of one geometry."""
    if geo == "K32":
        e = extra(*shape, B)
        return e["prev2"], e["residual2"]
    c = T.case(*shape, B)
    return c["prev"], c["residual"]


def conv64(geo, tiles, w, bias):
    g = GEO[geo]
    if tiles.shape[0] == 0:
        return torch.zeros((0, w.shape[0], g.ro, g.ro), dtype=torch.float64)
    return F.conv2d(tiles.double(), w.double(), None if bias is None else bias.double(), stride=g.stride)


def gather_tiles(geo, c, idx, kind, act, up=False, x=None):
    """The CPU oracle's tiles of one geometry and staging form (`x`: another first tensor than c["x"])."""
    if geo == "K31" and x is None:
        return T.gather_tiles(c, idx, kind, act, up)
    g = GEO[geo]
    sc, sh = T.affine_of(c, kind)
    src = T.full_input(c, up) if x is None else x.contiguous()
    return oracle.gather(src, g.block, g.block, idx, sc, sh, act)


@functools.lru_cache(maxsize=None)
def want_gather(geo, shape, B, name, form, kind=None, half=False, alt=False):
    """fp64 conv of the oracle's tiles of one case [B*N, Cout, ro, ro]; `kind`: the form's affine per batch ("batch") instead of
    shared; `half`: tiles and weights rounded to fp16 first (raw staging of the fp16-operand kernels); `alt`: the second image."""
    c = T.case(*shape, B)
    aff, act, up = T.GATHER_FORMS[form]
    if kind is not None and aff != "none":
        aff = kind
    tiles = gather_tiles(geo, c, lists(geo)[name], aff, act, up, x=extra(*shape, B)["x_alt"] if alt else None)
    w, bias = weights(geo, shape, B)
    return conv64(geo, tiles.half(), w.half(), bias) if half else conv64(geo, tiles, w, bias)


@functools.lru_cache(maxsize=None)
def want_scatter_gather(shape, B, name, kind, half_cache=False, half=False):
    """fp64 conv of the oracle's scatter_gather tiles (K31) over the cached tensor, or over its fp16-stored form."""
    c = T.case(*shape, B)
    y = c["y"].half().float() if half_cache else None
    tiles = T.sg_tiles(c, T.LISTS[name], B, kind, "identity" if kind == "none" else "swish", y=y)[1]
    return T.conv64(tiles.half(), c["w"].half(), c["bias"]) if half else T.conv64(tiles, c["w"], c["bias"])


def covered(geo, idx):
    """[Ho, Wo] bool: the output pixels some tile of `idx` writes."""
    if geo == "K31":
        return T.covered(idx)
    g = GEO[geo]
    m = torch.zeros(g.res, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        h0, w0 = (h0 + g.offset) // g.stride, (w0 + g.offset) // g.stride
        m[h0:h0 + g.ro, w0:w0 + g.ro] = True
    return m


def place(geo, prev, tiles, idx, B, fn):
    """The full destination: `prev` with fn(conv tile crop, b, rows, columns) on the ro x ro pixels at (origin + offset) / stride,
    clipped at the destination's edges."""
    if geo == "K31":
        return T.place(prev, tiles, idx, B, fn)
    g = GEO[geo]
    out = prev.double().clone()
    Ho, Wo = g.res
    N = idx.shape[0]
    for b in range(B):
        for n, (h0, w0) in enumerate(idx.tolist()):
            h0, w0 = (h0 + g.offset) // g.stride, (w0 + g.offset) // g.stride
            h1, w1 = min(h0 + g.ro, Ho), min(w0 + g.ro, Wo)
            out[b, :, h0:h1, w0:w1] = fn(tiles[b * N + n][:, :h1 - h0, :w1 - w0], b, slice(h0, h1), slice(w0, w1))
    return out


def shifted(idx):
    """`idx` moved by one tile along the row (a reference built from it must not pass)."""
    return (idx + torch.tensor([[0, 4]], dtype=torch.int32)).contiguous()


# ---- csrc/block_conv.hip plan_conv: usable(), restated ---------------------------------------------------------------------------
def compute_of(geo, compute):
    """The arithmetic a pack of `compute` runs in: the stride-2 geometry has fp32 kernels only (hip.conv_pack_weights)."""
    return "f32" if geo == "K32" else compute


def chunk(geo, mt, compute="f32"):
    """Channels per LDS chunk (conv_mfma.hpp: ConvGeo::CC, ConvGeoH::CC) of an MT-pixel output block."""
    nl = 64 // mt
    one = GEO[geo].kernel == 1
    cw = ((16 if one else 4) * nl) if compute_of(geo, compute) == "f32" else ((2 if one else 1) * nl * 8)
    return 4 * cw


def tiles_per_block(geo, mt):
    return mt // GEO[geo].ro ** 2


def usable(geo, mt, c1, c2, B, N, per_batch, compute="f32"):
    """A fused cat must split on a chunk boundary; a per-batch affine needs every M block inside one image."""
    if c2 and c1 % chunk(geo, mt, compute):
        return False
    if per_batch and B > 1 and N % tiles_per_block(geo, mt):
        return False
    return True


def block_shapes(geo, c1, c2, B, N, per_batch=False, compute="f32"):
    return [mt for mt in (32, 16) if usable(geo, mt, c1, c2, B, N, per_batch, compute)]


def refused(geo, shape, B, N, per_batch=False, compute="f32"):
    """The gather-source entry point returns None: no block shape is usable, or a fused cat comes with B > 1
    (block_conv.hip gather_conv_nhwc_impl: the second tensor is addressed without a batch stride)."""
    c1, c2, _ = shape
    if N == 0:
        return False  # (an empty list launches nothing and is no refusal)
    return bool(c2 and B != 1) or not block_shapes(geo, c1, c2, B, N, per_batch, compute)


# what the GPU file relies on, as literal facts (tests/test_tile_conv_default_inputs.py holds `refused` to them):
# (geometry, shape, B, N, per-batch affine, compute) -> refused
EXPECTED = [
    (("K31", (20, 44, 64), 1, 35, False, "f32"), True),    # cat on no chunk boundary
    (("K32", (20, 44, 64), 1, 35, False, "f32"), True),
    (("K11", (20, 44, 64), 1, 35, False, "f32"), True),
    (("K31", (64, 64, 72), 1, 35, False, "f32"), False),   # 64 = 2 x 32 = 1 x 64
    (("K31", (32, 32, 64), 1, 35, False, "f32"), False),   # MT = 32 only
    (("K31", (32, 32, 64), 1, 35, False, "f16"), True),    # fp16 operands: chunks of 64 / 128
    (("K31", (64, 64, 72), 1, 35, False, "f16"), False),
    (("K11", (64, 64, 72), 1, 35, False, "f32"), True),    # 1x1: chunks of 128 / 256
    (("K31", (64, 64, 72), 2, 35, False, "f32"), True),    # cat with B = 2
    (("K31", (64, 0, 64), 2, 35, True, "f32"), False),     # per-batch affine, odd list: one tile per M block at MT = 16
    (("K31", (64, 0, 64), 2, 34, True, "f32"), False),
    (("K11", (64, 0, 64), 2, 35, True, "f32"), False),
    (("K32", (64, 0, 64), 2, 35, True, "f32"), True),      # 8 or 4 tiles per M block: 35 is no multiple
    (("K32", (64, 0, 64), 2, 34, True, "f32"), True),
    (("K32", (64, 0, 64), 2, 32, True, "f32"), False),
    (("K32", (64, 0, 64), 1, 35, True, "f32"), False),     # (B = 1: one image, nothing to straddle)
    (("K32", (64, 0, 64), 2, 35, False, "f32"), False),    # a shared affine: an M block may hold tiles of both images
]
