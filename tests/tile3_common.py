"""Shared by the tests of the 6x6 tile conv v3 (csrc/conv_tile3.hpp: Tile3Geo<2>, fp32 and fp16 operands) on a ragged image:
geometry, tile lists, seeded CPU inputs, the CPU oracle's tiles, fp64 references and the CPU emulation of the fp16 staging path.
Nothing here touches a device (tests/test_tile_conv3_block6_inputs.py runs it without one).

Geometry.  Image 18 x 26, both even (upsample2x) and neither a multiple of the 4-pixel stride: 6x6 windows at origins
(4i - 1, 4j - 1) on a 5 x 7 grid, 4x4 outputs at origin + 1; the last row of windows writes rows 16..19 of 18, the last column
24..27 of 26.  Stacked edits: two 16 x 26 images as one 32 x 26 tensor, 4 x 7 windows each."""
import torch
import torch.nn.functional as F

from oracle import oracle
from tests.block10_common import tile_lists

H, W = 18, 26
LISTS = dict(tile_lists(5, 7, 4, 1))
LISTS["every34"] = LISTS["every"][:-1].contiguous()  # (even: a per-batch affine needs whole tile pairs per image)
NAMES = ["every", "corners", "interior", "holes", "empty"]
SHAPES = [(64, 0, 64), (128, 0, 64), (64, 0, 128), (64, 64, 64)]
NMAX = LISTS["every"].shape[0]
assert {k: v.shape[0] for k, v in LISTS.items()} == {"every": 35, "corners": 4, "interior": 1, "holes": 23, "empty": 0, "every34": 34}

HS = 16                                    # stacked edits: one image's height (a power of two)
LIST_S = tile_lists(4, 7, 4, 1)["every"]    # ... and its own tile list; rows 11..16 of the last window row hang over its image
NS = LIST_S.shape[0]

F16_ALLOW, F16_SHARE = 3e-4, 1e-3           # staged fp16 operands: |d| <= 3e-4 (1 + |want|) for all but 1e-3 of the elements


def bound(ref):
    """The suite's bound for exact-fp32 convs against fp64."""
    return 2e-5 * (1.0 + float(ref.abs().max())) if ref.numel() else 0.0


def f16_outside(got, want):
    """Share of the elements outside |got - want| <= 3e-4 (1 + |want|); NaN counts as outside."""
    if want.numel() == 0:
        return 0.0
    ok = (got.detach().double().cpu() - want.double()).abs() <= F16_ALLOW * (1.0 + want.double().abs())
    return float((~ok).double().mean())


_CASES = {}


def case(c1, c2, cout, B):
    """Seeded CPU inputs of one channel shape and batch, made once and never written to."""
    key = (c1, c2, cout, B)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * c1 + 100 * c2 + 10 * cout + B + 6)
        C = c1 + c2
        r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        _CASES[key] = dict(
            x=r(B, c1, H, W), x2=r(B, c2, H, W) if c2 else None, lo=r(B, c1, H // 2, W // 2), lo2=r(B, c2, H // 2, W // 2) if c2 else None,
            w=r(cout, C, 3, 3) / (3.0 * C ** 0.5), bias=r(cout), scale=r(B, C, 1, 1), shift=r(B, C, 1, 1),
            scale1=r(1, C, 1, 1), shift1=r(1, C, 1, 1), residual=r(B, cout, H, W), prev=r(B, cout, H, W), t4=r(B, NMAX, C, 4, 4),
            y=r(B, C, H, W), x1=r(B, NMAX, cout, 4, 4), os=r(cout), oh=r(cout), ts=[r(cout), r(cout)], tt=[r(cout), r(cout)],
            # stacked edits: two different images (and cached tensors, conv-1 tiles, buffers) of 16 rows each
            xs=r(2, c1, HS, W), xs2=r(2, c2, HS, W) if c2 else None, ys=r(2, C, HS, W), t4s=r(2, NS, C, 4, 4),
            prevs=r(2, cout, HS, W), residuals=r(2, cout, HS, W))
    return _CASES[key]


def conv64(tiles, w, bias):
    if tiles.shape[0] == 0:
        return torch.zeros((0, w.shape[0], tiles.shape[2] - 2, tiles.shape[3] - 2), dtype=torch.float64)
    return F.conv2d(tiles.double(), w.double(), None if bias is None else bias.double())


def covered(idx, res=(H, W)):
    m = torch.zeros(res, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[max(h0 + 1, 0):h0 + 5, max(w0 + 1, 0):w0 + 5] = True
    return m


def place(prev, tiles, idx, B, fn):
    """The full destination: `prev` with fn(conv tile crop, b, rows, columns) on the pixels origin + 1 + [0,4)^2, clipped."""
    out = prev.double().clone()
    Hh, Ww = prev.shape[2], prev.shape[3]
    N = idx.shape[0]
    for b in range(B):
        for n, (h0, w0) in enumerate(idx.tolist()):
            h0, w0 = h0 + 1, w0 + 1
            h1, w1 = min(h0 + 4, Hh), min(w0 + 4, Ww)
            out[b, :, h0:h1, w0:w1] = fn(tiles[b * N + n][:, :h1 - h0, :w1 - w0], b, slice(h0, h1), slice(w0, w1))
    return out


def full_input(c, up=False):
    """The tensor the windows index: x (cat x2), or the nearest x2 upsampling of the half-resolution pair."""
    a, b = (c["lo"], c["lo2"]) if up else (c["x"], c["x2"])
    t = a if b is None else torch.cat([a, b], 1)
    return F.interpolate(t, scale_factor=2.0, mode="nearest").contiguous() if up else t.contiguous()


# staging forms of the gather source: name -> (affine "none" | "shared" | "batch", activation, upsample2x)
GATHER_FORMS = {"raw": ("none", "identity", False), "affine+silu": ("shared", "swish", False), "affine": ("shared", "identity", False),
                "up": ("none", "identity", True), "up+affine+silu": ("shared", "swish", True)}


def affine_of(c, kind):
    return {"none": (None, None), "shared": (c["scale1"], c["shift1"]), "batch": (c["scale"], c["shift"])}[kind]


def gather_tiles(c, idx, kind, act, up):
    """The CPU oracle's 6x6 tiles [B*N,C,6,6] of one staging form."""
    sc, sh = affine_of(c, kind)
    return oracle.gather(full_input(c, up), 6, 6, idx, sc, sh, act)


def shortcut(idx, res=(H, W)):
    """A 4x4 shortcut list inside the main tiles: the output cell of every other main tile; its table over the 4x4 cells of `res`."""
    idx1 = (idx[::2] + 1).contiguous()
    table = torch.full((-(-res[0] // 4), -(-res[1] // 4)), -1, dtype=torch.int32)
    for n, (h0, w0) in enumerate(idx1.tolist()):
        table[h0 // 4, w0 // 4] = n
    return idx1, table


def scatter_map(idx, res=(H, W)):
    return oracle.get_scatter_map(res[0], res[1], 6, 6, 3, 3, 1, 1, 1, 1, idx)


def sg_tiles(c, idx, B, kind="none", act="identity", y=None):
    """(conv-1 tiles [B*N,C,4,4], the oracle's scatter_gather 6x6 tiles) over the cached tensor `y` (default c["y"])."""
    N = idx.shape[0]
    t4 = c["t4"][:, :N].reshape(B * N, c["t4"].shape[2], 4, 4).contiguous()
    sc, sh = affine_of(c, kind)
    return t4, oracle.scatter_gather(t4, c["y"] if y is None else y, 6, 6, idx, scatter_map(idx), sc, sh, act)


# ---- stacked edits: E = 2 images of 16 rows in one 32-row tensor with B = 1 ----------------------------------------------------
def stacked_list():
    """Image 0's list, then image 1's shifted by 16 rows."""
    return torch.cat([LIST_S, LIST_S + torch.tensor([[HS, 0]], dtype=torch.int32)], 0).contiguous()


def stack(t):
    """[2,C,16,W] -> [1,C,32,W]: the same pixels as one tall image."""
    return torch.cat([t[0:1], t[1:2]], 2).contiguous()


def stacked_map():
    """Each image's own scatter map, image 1's tile numbers behind image 0's."""
    m = scatter_map(LIST_S, (HS, W))
    m1 = m.clone()
    m1[..., 0] = torch.where(m[..., 0] >= 0, m[..., 0] + NS, m[..., 0])
    return torch.cat([m, m1], 0).contiguous()


def stacked_tiles(c, source, affine):
    """The oracle's tiles of each image ALONE (zero padding beyond its own 16 rows), image 0's first: [2 NS, C, 6, 6]."""
    sc, sh = (c["scale1"], c["shift1"]) if affine else (None, None)
    act = "swish" if affine else "identity"
    out = []
    for e in range(2):
        if source == 1:
            t = c["xs"][e:e + 1] if c["xs2"] is None else torch.cat([c["xs"][e:e + 1], c["xs2"][e:e + 1]], 1)
            out.append(oracle.gather(t.contiguous(), 6, 6, LIST_S, sc, sh, act))
        else:
            out.append(oracle.scatter_gather(c["t4s"][e].contiguous(), c["ys"][e:e + 1].contiguous(), 6, 6, LIST_S,
                                             scatter_map(LIST_S, (HS, W)), sc, sh, act))
    return torch.cat(out, 0)


# ---- the fp16 staging path on the CPU ------------------------------------------------------------------------------------------
def live_pixels(idx, B, res=(H, W)):
    """[B*N,1,6,6] bool: the window pixels inside the image (the others are zero padding, also behind an affine)."""
    return oracle.gather(torch.ones(B, 1, *res), 6, 6, idx) > 0


def stage_f16(raw, live, scale, shift, act, B, silu64):
    """Raw tiles [B*N,C,6,6] -> what the kernel stages: scale * z, + shift (each rounded to fp32), SiLU in fp32 or (silu64) in fp64,
    padding an exact 0, rounded to fp16 (round to nearest even)."""
    N = raw.shape[0] // B
    z = raw.reshape(B, N, *raw.shape[1:])
    z = scale.reshape(scale.shape[0], 1, -1, 1, 1) * z
    z = shift.reshape(shift.shape[0], 1, -1, 1, 1) + z
    if act == "swish":
        z = (z.double() * torch.sigmoid(z.double())) if silu64 else z * torch.sigmoid(z)
    z = z.reshape(raw.shape)
    return torch.where(live, z, torch.zeros_like(z)).half()


# the affine-staged fp16 cases of tests/test_gpu_tile_conv3_block6.py: (source, shape, form or affine kind, activation)
def f16_staged_cases():
    out = []
    for shape in SHAPES:
        for form, (kind, act, up) in GATHER_FORMS.items():
            if kind != "none":
                out.append((1, shape, form))
    for shape in SHAPES[:3]:
        out.append((2, shape, "affine+silu"))
    return out


def f16_staged_tiles(source, shape, form, name, B=1, half_cache=False):
    """(raw oracle tiles, the oracle's staged tiles, live pixels, scale, shift, activation) of one affine-staged case and list;
    half_cache (source 2): the cached tensor holds halves."""
    c1, c2, cout = shape
    c = case(c1, c2, cout, B)
    idx = LISTS[name]
    kind, act, up = GATHER_FORMS[form]
    sc, sh = affine_of(c, kind)
    if source == 1:
        return gather_tiles(c, idx, "none", "identity", up), gather_tiles(c, idx, kind, act, up), live_pixels(idx, B), sc, sh, act
    y = c["y"].half().float() if half_cache else None
    return sg_tiles(c, idx, B, y=y)[1], sg_tiles(c, idx, B, kind, act, y=y)[1], live_pixels(idx, B), sc, sh, act
