"""On the MI355X: block size 10.  The tile conv v3 over 10x10 windows (csrc/conv_tile3.hpp: Tile3GeoE10) against fp64
convs of the CPU oracle's tiles, what its entry point refuses, 1x1 on 8x8 and 3x3 / stride 2 on 9x9 through the modules, and the
smallest network with main_block = 10, shortcut_block = 8 against the CPU oracle backend.

Shapes.  Image 20x28, neither a multiple of 8: origins (8i - 1, 8j - 1) on a 3x4 grid, the last row of windows hangs over the image
(output rows 16..19 of 8) and so does the last column (24..27).  (Cin, Cout) = (64, 64): one chunk, one output block; (128, 64): two
chunks, so both stages and the ring's second parity run; (64, 128): two output blocks per window; 64 + 64: the fused cat, the
chunk that switches tensors.  Batches 1 and 2 (a per-sample affine).  One workgroup per window and output block: `every` is 12-48.
Bound: the suite's convention for exact-fp32 convs against fp64, 2e-5 * (1 + max |ref|)."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import util
from tests.block10_common import tile_lists
from tests.change_regions_common import small_cfg, small_inputs, small_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 20, 28
LISTS = tile_lists(3, 4, 8, 1)
NAMES = ["every", "corners", "interior", "holes", "empty"]
SHAPES = [(64, 0, 64), (128, 0, 64), (64, 0, 128), (64, 64, 64)]


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bound(ref):
    return 2e-5 * (1.0 + float(ref.abs().max())) if ref.numel() else 0.0


def _err(got, want):
    if got.numel() == 0:
        return 0.0
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max())


def _check(got, want, what):
    util.assert_finite(got, what)
    err, tol = _err(got, want), _bound(want)
    print("block10 %-60s err %.3e bound %.3e" % (what, err, tol), flush=True)
    assert tuple(got.shape) == tuple(want.shape) and err <= tol, (what, err, tol)


_CASES = {}


def _case(c1, c2, cout, B):
    """Seeded CPU inputs of one channel shape and batch, made once."""
    key = (c1, c2, cout, B)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(100 * c1 + 10 * c2 + cout + B)
        C = c1 + c2
        r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        _CASES[key] = dict(
            x=r(B, c1, H, W), x2=r(B, c2, H, W) if c2 else None, lo=r(B, c1, H // 2, W // 2),
            w=r(cout, C, 3, 3) / (3.0 * C ** 0.5), bias=r(cout), scale=r(B, C, 1, 1), shift=r(B, C, 1, 1),
            residual=r(B, cout, H, W), prev=r(B, cout, H, W), t8=r(B, 12, C, 8, 8), y=r(B, C, H, W),
            x1=r(B, 12, cout, 8, 8), os=r(cout), oh=r(cout), ts=[r(cout), r(cout)], tt=[r(cout), r(cout)])
    return _CASES[key]


def _conv64(tiles, c):
    if tiles.shape[0] == 0:
        return torch.zeros((0, c["w"].shape[0], 8, 8), dtype=torch.float64)
    return F.conv2d(tiles.double(), c["w"].double(), c["bias"].double())


def _covered(idx):
    m = torch.zeros(H, W, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[h0 + 1:h0 + 9, w0 + 1:w0 + 9] = True
    return m


def _place(prev, tiles, idx, B, fn):
    """The full destination: `prev` with fn(conv tile crop, b, rows, columns) on the pixels offset + origin + [0,8)^2, clipped."""
    out = prev.double().clone()
    N = idx.shape[0]
    for b in range(B):
        for n, (h0, w0) in enumerate(idx.tolist()):
            h0, w0 = h0 + 1, w0 + 1
            h1, w1 = min(h0 + 8, H), min(w0 + 8, W)
            out[b, :, h0:h1, w0:w1] = fn(tiles[b * N + n][:, :h1 - h0, :w1 - w0], b, slice(h0, h1), slice(w0, w1))
    return out


def _gather_sources(c, c1, c2, B, idx):
    """name -> (x, x2, scale, shift, act, upsample2x, oracle tiles [B*N,C,10,10])."""
    full = c["x"] if c2 == 0 else torch.cat([c["x"], c["x2"]], 1)
    out = {
        "raw": (c["x"], c["x2"], None, None, "identity", False, oracle.gather(full, 10, 10, idx)),
        "affine+silu": (c["x"], c["x2"], c["scale"], c["shift"], "swish", False, oracle.gather(full, 10, 10, idx, c["scale"], c["shift"], "swish")),
    }
    if c2 == 0:
        up = F.interpolate(c["lo"], scale_factor=2.0, mode="nearest")
        out["upsample2x"] = (c["lo"], None, None, None, "identity", True, oracle.gather(up, 10, 10, idx))
    return out


# ---- a. the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d+%d_%d" % s)
def test_gather_sources_to_tiles_and_full(hip, shape, B):
    """T3_GATHER: raw, cached affine + SiLU (per sample at B = 2), upsample2x addressing, one tensor and the fused cat; into tiles,
    and into the full tensor with a residual; every tile list."""
    c1, c2, cout = shape
    c = _case(c1, c2, cout, B)
    wd, bd = c["w"].to(DEV), c["bias"].to(DEV)
    packed = hip.conv_pack_weights(wd, 10, 10, (1, 1))
    assert packed is not None and packed.geo == "b10"
    for name in NAMES:
        idx = LISTS[name]
        idx_d = idx.to(DEV)
        for src, (x, x2, sc, sh, act, up, tiles) in _gather_sources(c, c1, c2, B, idx).items():
            want = _conv64(tiles, c)
            args = (_cl(x), None if x2 is None else _cl(x2), (10, 10), idx_d, None if sc is None else sc.to(DEV),
                    None if sh is None else sh.to(DEV), act, packed, bd, cout, (3, 3), (1, 1))
            with util.poisoned():
                got = hip.gather_conv_cl(*args, upsample2x=up)
            assert got is not None and tuple(got.shape) == (B * idx.shape[0], cout, 8, 8)
            _check(got, want, "gather %s %s B%d %s -> tiles" % (shape, src, B, name))
            # the full destination: conv + bias + residual on the covered pixels, the buffer's contents elsewhere
            out = _cl(c["prev"])
            got = hip.gather_conv_cl(*args, upsample2x=up, out=out,
                                     full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(c["residual"])))
            assert got is out
            ref = _place(c["prev"], want, idx, B, lambda t, b, hs, ws: t + c["residual"][b, :, hs, ws].double())
            _check(got, ref, "gather %s %s B%d %s -> full + residual" % (shape, src, B, name))
            assert torch.equal(got.cpu()[:, :, ~_covered(idx)], c["prev"][:, :, ~_covered(idx)])


@pytest.mark.parametrize("B", [1, 2])
def test_gather_full_with_twins_and_out_affine(hip, B):
    """The shared epilogue's twins (SiLU(ts * out + tt) into two more buffers) and the consumer's out-affine + SiLU."""
    c1, c2, cout = 64, 64, 128
    c = _case(c1, c2, cout, B)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    idx = LISTS["holes"]
    tiles = oracle.gather(torch.cat([c["x"], c["x2"]], 1), 10, 10, idx, c["scale"], c["shift"], "swish")
    want = _conv64(tiles, c)
    v = lambda t: t.double().view(-1, 1, 1)  # noqa: E731
    base = lambda t, b, hs, ws: t + c["residual"][b, :, hs, ws].double()  # noqa: E731
    tw = [(_cl(c["prev"]), c["ts"][k].to(DEV), c["tt"][k].to(DEV)) for k in range(2)]
    out = _cl(c["prev"])
    got = hip.gather_conv_cl(_cl(c["x"]), _cl(c["x2"]), (10, 10), idx.to(DEV), c["scale"].to(DEV), c["shift"].to(DEV), "swish", packed,
                             c["bias"].to(DEV), cout, (3, 3), (1, 1), out=out, twins=tw, out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "swish"),
                             full=dict(offset=(1, 1), out_res=(H, W), residual=_cl(c["residual"])))
    assert got is out
    _check(got, _place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(v(c["os"]) * base(t, b, hs, ws) + v(c["oh"]))),
           "gather B%d twins + out-affine: out" % B)
    for k in range(2):
        _check(tw[k][0], _place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(v(c["ts"][k]) * base(t, b, hs, ws) + v(c["tt"][k]))),
               "gather B%d twins + out-affine: twin %d" % (B, k))
    # tiles with the out-affine (what SIGEConv2d(out_affine=...) asks for)
    with util.poisoned():
        got = hip.gather_conv_cl(_cl(c["x"]), _cl(c["x2"]), (10, 10), idx.to(DEV), c["scale"].to(DEV), c["shift"].to(DEV), "swish", packed,
                                 c["bias"].to(DEV), cout, (3, 3), (1, 1), out_affine=(c["os"].to(DEV), c["oh"].to(DEV), "identity"))
    _check(got, v(c["os"]) * want + v(c["oh"]), "gather B%d tiles + out-affine" % B)


def _shortcut(idx):
    """A shortcut list inside the main tiles: the 8x8 cells of every other main tile; its table over the 3x4 cells."""
    idx1 = (idx[::2] + 1).contiguous()
    table = torch.full((3, 4), -1, dtype=torch.int32)
    for n, (h0, w0) in enumerate(idx1.tolist()):
        table[h0 // 8, w0 // 8] = n
    return idx1, table


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "%d+%d_%d" % s)
def test_scatter_gather_source_to_tiles_and_full(hip, shape, B):
    """T3_SCATTER_GATHER: conv-1 tiles [B*N,8,8,Cin] cover the inner 8x8 of each window, the ring comes from a neighbour's tile or
    from the cached tensor -- both branches of the map are read (`every`: neighbours; `corners`, `interior`, `holes`: the cache).
    Into tiles, into the full tensor with a residual (Scatter), with the block residual at R1 = 8 (ScatterWithBlockResidual), twins."""
    cin, _, cout = shape
    c = _case(cin, 0, cout, B)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    bd = c["bias"].to(DEV)
    for name in NAMES:
        idx = LISTS[name]
        N = idx.shape[0]
        idx_d = idx.to(DEV)
        smap = oracle.get_scatter_map(H, W, 10, 10, 3, 3, 1, 1, 1, 1, idx)
        if N:  # (`every` covers the image: its ring pixels come from neighbouring tiles; the other lists read the cache too)
            assert bool((smap[..., 0] >= 0).any()) and (name == "every" or bool((smap[..., 0] < 0).any()))
        t8 = c["t8"][:, :N].reshape(B * N, cin, 8, 8).contiguous()
        want = _conv64(oracle.scatter_gather(t8, c["y"], 10, 10, idx, smap), c)
        t8d = _cl(t8) if N else torch.zeros((0, cin, 8, 8), device=DEV).contiguous(memory_format=torch.channels_last)
        with util.poisoned():
            got = hip.scatter_gather_conv_cl(t8d, _cl(c["y"]), (10, 10), idx_d, smap.to(DEV), None, None, "identity", packed, bd, cout, (3, 3), (1, 1))
        assert got is not None and tuple(got.shape) == (B * N, cout, 8, 8)
        _check(got, want, "scatter_gather %s B%d %s -> tiles" % (shape, B, name))
        cover = _covered(idx)
        y1 = c["residual"]
        # Scatter: conv + bias + residual
        out = _cl(c["prev"])
        tw = [(_cl(c["prev"]), c["ts"][0].to(DEV), c["tt"][0].to(DEV))]
        got = hip.scatter_gather_conv_scatter_cl(t8d, _cl(c["y"]), (10, 10), idx_d, smap.to(DEV), None, None, "identity", packed, bd, cout, (3, 3),
                                                 (1, 1), out, residual=_cl(y1), twins=tw)
        assert got is out
        plain = lambda t, b, hs, ws: t + y1[b, :, hs, ws].double()  # noqa: E731
        _check(got, _place(c["prev"], want, idx, B, plain), "scatter_gather %s B%d %s -> full + residual" % (shape, B, name))
        assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover])
        ts, tt = c["ts"][0].double().view(-1, 1, 1), c["tt"][0].double().view(-1, 1, 1)
        _check(tw[0][0], _place(c["prev"], want, idx, B, lambda t, b, hs, ws: F.silu(ts * plain(t, b, hs, ws) + tt)),
               "scatter_gather %s B%d %s -> twin" % (shape, B, name))
        # ScatterWithBlockResidual: the shortcut tiles replace the cached shortcut tensor where they cover the pixel
        idx1, table1 = _shortcut(idx)
        N1 = idx1.shape[0]
        x1 = c["x1"][:, :N1].reshape(B * N1, cout, 8, 8).contiguous()
        x1d = _cl(x1) if N1 else torch.zeros((0, cout, 8, 8), device=DEV).contiguous(memory_format=torch.channels_last)

        def block(t, b, hs, ws):
            n1 = int(table1[hs.start // 8, ws.start // 8])
            if n1 < 0:
                return t + y1[b, :, hs, ws].double()
            return t + x1[b * N1 + n1][:, :hs.stop - hs.start, :ws.stop - ws.start].double()

        out = _cl(c["prev"])
        got = hip.scatter_gather_conv_scatter_cl(t8d, _cl(c["y"]), (10, 10), idx_d, smap.to(DEV), None, None, "identity", packed, bd, cout, (3, 3),
                                                 (1, 1), out, residual=_cl(y1), x1=x1d, table1=table1.to(DEV))
        assert got is out
        _check(got, _place(c["prev"], want, idx, B, block), "scatter_gather %s B%d %s -> full + block residual" % (shape, B, name))
        assert torch.equal(got.cpu()[:, :, ~cover], c["prev"][:, :, ~cover])


def test_block_residual_with_4x4_shortcut_cells(hip):
    """R1 = S1 = 4: a shortcut branch left at the default block size under main_block = 10."""
    cin, cout, B = 64, 64, 1
    c = _case(cin, 0, cout, B)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    idx = LISTS["holes"]
    N = idx.shape[0]
    smap = oracle.get_scatter_map(H, W, 10, 10, 3, 3, 1, 1, 1, 1, idx)
    t8 = c["t8"][:, :N].reshape(B * N, cin, 8, 8).contiguous()
    want = _conv64(oracle.scatter_gather(t8, c["y"], 10, 10, idx, smap), c)
    idx1 = torch.cat([idx + 1, idx + 5], 0)  # two of the four 4x4 cells of every main tile (its diagonal)
    idx1 = idx1[(idx1[:, 0] < H) & (idx1[:, 1] < W)].contiguous()
    N1 = idx1.shape[0]
    table1 = torch.full((5, 7), -1, dtype=torch.int32)
    for n, (h0, w0) in enumerate(idx1.tolist()):
        table1[h0 // 4, w0 // 4] = n
    gen = torch.Generator().manual_seed(5)
    x1 = torch.randn(N1, cout, 4, 4, generator=gen)
    y1 = c["residual"]
    ref = _place(c["prev"], want, idx, B, lambda t, b, hs, ws: t + y1[b, :, hs, ws].double())
    for n, (h0, w0) in enumerate(idx1.tolist()):
        h1, w1 = min(h0 + 4, H), min(w0 + 4, W)
        ref[0, :, h0:h1, w0:w1] += x1[n][:, :h1 - h0, :w1 - w0].double() - y1[0, :, h0:h1, w0:w1].double()
    out = _cl(c["prev"])
    got = hip.scatter_gather_conv_scatter_cl(_cl(t8), _cl(c["y"]), (10, 10), idx.to(DEV), smap.to(DEV), None, None, "identity", packed,
                                             c["bias"].to(DEV), cout, (3, 3), (1, 1), out, residual=_cl(y1), x1=_cl(x1), table1=table1.to(DEV))
    assert got is out
    _check(got, ref, "scatter_gather -> full + block residual, R1 = 4")


def test_slab_of_tiles_in(hip):
    """block_conv_cl over materialised 10x10 tiles: a batch of T 10x10 images with one window each."""
    c = _case(64, 0, 64, 2)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    tiles = oracle.gather(c["x"], 10, 10, LISTS["every"])
    with util.poisoned():
        got = hip.block_conv_cl(_cl(tiles), packed, c["bias"].to(DEV), 64, (3, 3), (1, 1))
    _check(got, _conv64(tiles, c), "slab [24,10,10,64] -> tiles")


# ---- b. refusals and packing ------------------------------------------------------------------------------------------------------
def _entry_args(hip, c, idx_d, packed, out, **over):
    """Positional arguments of sige_hip_tile_conv3_block_nhwc for a plain gather -> tiles call over `idx_d`."""
    x = over.pop("x")
    xptr = over.pop("xptr", x.data_ptr())
    a = dict(compute=0, source=1, x=xptr, x2=None, y_f16=0, B=x.shape[0], C1=x.shape[1], C2=0, H=H, W=W, bH=10, bW=10, up=0,
             idx=idx_d.data_ptr(), N=idx_d.shape[0], smap=None, Rx=0, Sx=0, scale=None, shift=None, affineB=0, act=0,
             packed=packed.data_ptr(), bias=None, Cout=out.shape[1], to_full=0, offH=0, offW=0, Ho=0, Wo=0, residual=None, residual_f16=0,
             x1=None, table1=None, gH1=0, gW1=0, N1=0, R1=0, S1=0, os=None, oh=None, oact=0, tw0=None, ts0=None, tt0=None, tw1=None,
             ts1=None, tt1=None, out=out.data_ptr(), stream=None)
    assert not set(over) - set(a), set(over) - set(a)
    a.update(over)
    return list(a.values())


def test_entry_point_refusals(hip):
    """Everything the 10x10 form does not cover answers UNSUPPORTED -- never a launch with wrong numbers: `out` stays poisoned."""
    L = hip.lib()
    c = _case(64, 0, 64, 1)
    xd, idx_d = _cl(c["x"]), LISTS["every"].to(DEV)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    out = _cl(torch.full((12, 64, 8, 8), float("nan")))
    call = lambda **kw: L.sige_hip_tile_conv3_block_nhwc(*_entry_args(hip, c, idx_d, packed, out, x=xd, **kw))  # noqa: E731
    assert L.sige_hip_tile_conv3_block_supported(64, 0, 64, 10, 10) == 1 and L.sige_hip_tile_conv3_block_supported(64, 64, 128, 6, 6) == 1
    for bad in ((32, 0, 64, 10, 10), (64, 32, 64, 10, 10), (64, 0, 96, 10, 10), (64, 0, 64, 8, 8), (64, 0, 64, 10, 6), (64, 0, 64, 12, 12)):
        assert L.sige_hip_tile_conv3_block_supported(*bad) == 0, bad
    U = hip.UNSUPPORTED
    assert call(compute=1) == U and call(compute=2) == U
    assert call(residual_f16=1) == U and call(y_f16=1) == U
    assert call(bH=8, bW=8) == U and call(bH=10, bW=6) == U
    assert call(C1=32) == U and call(Cout=96) == U                      # (refused on the counts, before anything is read)
    sd = c["scale"].to(DEV)
    assert call(source=2, x2=xd.data_ptr(), smap=idx_d.data_ptr(), Rx=8, Sx=8, scale=sd.data_ptr(), shift=sd.data_ptr(), affineB=1) == U
    assert call(source=2, x2=xd.data_ptr(), smap=idx_d.data_ptr(), Rx=4, Sx=4) == U
    hip.set_edit_batch(2)                                               # stacked edits
    try:
        xe = _cl(torch.zeros(1, 64, 32, W))  # (two stacked 16-row images)
        assert call(xptr=xe.data_ptr(), H=32) == U
    finally:
        hip.set_edit_batch(1)
    # a held 1x1 shortcut (conv_pair) and an armed side conv
    w1 = torch.randn(64, 64, 1, 1, device=DEV)
    p1 = hip.conv_pack_weights(w1, 4, 4, (1, 1))
    idx4 = hip.subtile_indices(LISTS["interior"].to(DEV) + 1, 2, 4)
    with hip.conv_pair(xd):
        held = hip.gather_conv_cl(xd, None, (4, 4), idx4, None, None, "identity", p1, None, 64, (1, 1), (1, 1))
        status = call()
    assert held is not None and status == U
    assert L.sige_hip_conv_side_begin(64) == 0
    try:
        assert call() == U
    finally:
        assert L.sige_hip_conv_side_flush() == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0                                                  # the same arguments with nothing held: it runs
    torch.cuda.synchronize()
    _check(out, _conv64(oracle.gather(c["x"], 10, 10, LISTS["every"]), dict(w=c["w"], bias=torch.zeros(64))), "entry point, plain call")
    # the routing entry points without v3 weights refuse the geometry as before
    p6 = hip.conv_pack_weights(c["w"].to(DEV), 6, 6, (1, 1))
    assert L.sige_hip_gather_conv_nhwc(0, xd.data_ptr(), None, 1, 64, 0, H, W, 10, 10, idx_d.data_ptr(), 12, None, 0, 0, None, 0, 0, 0,
                                       p6.data_ptr(), None, 64, 3, 3, 1, 1, 0, 0, 0, None, 0, 0, None, 0, None, None, 0, 0,
                                       None, None, None, None, None, None, None, 0, out.data_ptr(), None) == U


def test_refused_shapes_fall_back_within_tolerance(hip):
    """Channel counts without a 10x10 kernel (96 -> 32), fp16 compute and an fp16-stored cache: no packed weights / a refused call,
    and SIGEConv2d's fallback (materialised gather, the direct kernel) still meets the row's tolerance."""
    from sige_amd.nn import Gather, SIGEConv2d

    assert hip.conv_pack_weights(torch.randn(32, 96, 3, 3, device=DEV), 10, 10, (1, 1)) is None
    assert hip.conv_pack_weights(torch.randn(64, 64, 3, 3, device=DEV), 10, 10, (1, 1), "f16") is None
    assert hip.conv_pack_weights(torch.randn(64, 64, 3, 3, device=DEV), 10, 10, (1, 1), "f16x3") is None
    torch.manual_seed(3)
    for cin, cout, dtype in ((96, 32, "f32"), (64, 64, "f16")):
        conv = SIGEConv2d(cin, cout, 3, 1, 1).to(DEV).eval()
        conv.compute_dtype = dtype
        g = Gather(conv, 10)
        x = torch.randn(1, cin, H, W)
        with torch.no_grad():
            conv(g(_cl(x)))  # (full mode: the gather notes its input resolution)
        idx = _set_tiles(g, LISTS["holes"], (H, W), 4, "holes")
        for m in (g, conv):
            m.set_mode("sparse")
        seen = []
        real = hip.block_conv_direct
        hip.block_conv_direct = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
        try:
            with torch.no_grad():
                got = conv(g(_cl(x)))
        finally:
            hip.block_conv_direct = real
        want = F.conv2d(oracle.gather(x, 10, 10, idx).double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())
        assert seen and _err(got, want) <= util.CONV_ATOL, (cin, cout, dtype, seen, _err(got, want))
    # an fp16-stored cache behind the fused conv2 -> scatter: refused, the caller runs its unfused form
    c = _case(64, 0, 64, 1)
    packed = hip.conv_pack_weights(c["w"].to(DEV), 10, 10, (1, 1))
    idx = LISTS["holes"]
    smap = oracle.get_scatter_map(H, W, 10, 10, 3, 3, 1, 1, 1, 1, idx).to(DEV)
    t8 = _cl(c["t8"][:, :idx.shape[0]].reshape(-1, 64, 8, 8))
    assert hip.scatter_gather_conv_scatter_cl(t8, _cl(c["y"]).half(), (10, 10), idx.to(DEV), smap, None, None, "identity", packed, None, 64,
                                              (3, 3), (1, 1), _cl(c["prev"])) is None
    assert hip.scatter_gather_conv_cl(t8, _cl(c["y"]), (10, 10), idx.to(DEV), smap, c["scale"].to(DEV), c["shift"].to(DEV), "swish", packed,
                                      None, 64, (3, 3), (1, 1)) is None


def _set_tiles(g, idx, res, inner, stamp):
    """Give Gather `g` the tile list `idx` through its own mask pipeline: one masked pixel inside each wanted window (at origin +
    `inner`, which no neighbouring window contains).  Returns the list as the module holds it (CPU)."""
    m = torch.zeros(res, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[h0 + inner, w0 + inner] = True
    g.set_mask({tuple(res): m.to(DEV)}, {}, stamp)
    got = g.active_indices.cpu().to(torch.int32)
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, idx.tolist())), (got.tolist(), idx.tolist())
    return got


class _direct_spy:
    """Counts hip.block_conv_direct calls inside the block."""

    def __init__(self, hip):
        self.hip, self.n = hip, 0

    def __enter__(self):
        self.real = self.hip.block_conv_direct

        def spy(*a, **k):
            self.n += 1
            return self.real(*a, **k)

        self.hip.block_conv_direct = spy
        return self

    def __exit__(self, *exc):
        self.hip.block_conv_direct = self.real
        return False


def _conv_on_tiles(cin, cout, res, idx, seed, compute="f32"):
    """(conv, gather, x on the CPU, the module's tile list): a 3x3 SIGEConv2d behind Gather(conv, 10) after its full pass, in
    sparse mode on the windows `idx` of a [1, cin, *res] input."""
    from sige_amd.nn import Gather, SIGEConv2d

    torch.manual_seed(seed)
    conv = SIGEConv2d(cin, cout, 3, 1, 1).to(DEV).eval()
    conv.compute_dtype = compute
    g = Gather(conv, 10)
    x = torch.randn(1, cin, *res)
    with torch.no_grad():
        conv(g(_cl(x)))  # (full mode: the gather notes its input resolution)
    idx = _set_tiles(g, idx, res, 4, "tiles")
    for m in (g, conv):
        m.set_mode("sparse")
    return conv, g, x, idx


def _want_tiles(conv, x, idx):
    return F.conv2d(oracle.gather(x, 10, 10, idx).double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())


def test_refused_states_fall_back_through_the_modules(hip):
    """What the 10x10 form refuses by STATE -- split-fp16 compute, a held shortcut (conv_pair), an armed side conv, stacked edits,
    an fp16-stored cache -- through SIGEConv2d: the caller's fallback computes the same conv within the row's tolerance."""
    from sige_amd.nn import Gather, ScatterGather, SIGEConv2d

    # compute f16x3: tile convs without such a kernel run exact fp32 (the 10x10 form, or the direct kernel)
    conv, g, x, idx = _conv_on_tiles(64, 64, (H, W), LISTS["holes"], 21, compute="f16x3")
    with torch.no_grad():
        got = conv(g(_cl(x)))
    assert _err(got, _want_tiles(conv, x, idx)) <= util.CONV_ATOL, _err(got, _want_tiles(conv, x, idx))
    # a 1x1 shortcut on 4x4 blocks held by conv_pair() while conv1 runs: refused, the direct kernel; the shortcut is not lost
    conv, g, x, idx = _conv_on_tiles(64, 128, (H, W), LISTS["holes"], 22)
    xd = _cl(x)
    w1, b1 = torch.randn(128, 64, 1, 1) / 8.0, torch.randn(128)
    p1 = hip.conv_pack_weights(w1.to(DEV), 4, 4, (1, 1))
    idx4 = hip.subtile_indices(idx + 1, 2, 4)
    with torch.no_grad(), _direct_spy(hip) as spy:
        with hip.conv_pair(xd):
            short = hip.gather_conv_cl(xd, None, (4, 4), idx4.to(DEV), None, None, "identity", p1, b1.to(DEV), 128, (1, 1), (1, 1))
            got = conv(g(xd))
    assert short is not None and spy.n == 1
    assert _err(got, _want_tiles(conv, x, idx)) <= util.CONV_ATOL, _err(got, _want_tiles(conv, x, idx))
    want1 = F.conv2d(oracle.gather(x, 4, 4, idx4).double(), w1.double(), b1.double())
    assert _err(short, want1) <= util.CONV_ATOL, _err(short, want1)
    # an armed side conv (conv_side_begin waits for a conv of the default geometry)
    conv, g, x, idx = _conv_on_tiles(64, 64, (H, W), LISTS["corners"], 23)
    hip.conv_side_begin()
    try:
        with torch.no_grad(), _direct_spy(hip) as spy:
            got = conv(g(_cl(x)))
    finally:
        hip.conv_side_flush(_cl(x))
    assert spy.n == 1 and _err(got, _want_tiles(conv, x, idx)) <= util.CONV_ATOL, (spy.n, _err(got, _want_tiles(conv, x, idx)))
    # stacked edits: two 16-row images in one 32-row tensor, windows that lie inside one image each (rows -1..8 of image 0,
    # rows 23..32 of image 1): there the stacked gather is the plain one, and the oracle's tiles are the reference
    rows = tile_lists(5, 4, 8, 1)["every"]
    rows = rows[(rows[:, 0] == -1) | (rows[:, 0] == 23)].contiguous()
    conv, g, x, idx = _conv_on_tiles(64, 64, (32, W), rows, 24)
    hip.set_edit_batch(2)
    try:
        with torch.no_grad(), _direct_spy(hip) as spy:
            got = conv(g(_cl(x)))
    finally:
        hip.set_edit_batch(1)
    assert spy.n == 1 and _err(got, _want_tiles(conv, x, idx)) <= util.CONV_ATOL, (spy.n, _err(got, _want_tiles(conv, x, idx)))
    # an fp16-stored cache (set_cache_dtype("f16")) behind conv2: the scatter_gather is materialised from the halves, then convolved
    torch.manual_seed(25)
    conv1, conv2 = SIGEConv2d(64, 64, 3, 1, 1).to(DEV).eval(), SIGEConv2d(64, 64, 3, 1, 1).to(DEV).eval()
    g = Gather(conv1, 10)
    sg = ScatterGather(g)
    sg.cache_dtype = "f16"
    x, xe = torch.randn(1, 64, H, W), torch.randn(1, 64, H, W)
    mods = (g, conv1, sg, conv2)
    with torch.no_grad():
        for m in mods:
            m.set_mode("full")
        conv2(sg(conv1(g(_cl(x)))))
        idx = _set_tiles(g, LISTS["holes"], (H, W), 4, "holes")
        for m in mods:
            m.set_mode("sparse")
        cache = sg.original_outputs[sg.cache_id]
        assert cache.dtype == torch.float16
        t1 = conv1(g(_cl(xe)))
        got = conv2(sg(t1))
    smap = oracle.get_scatter_map(H, W, 10, 10, 3, 3, 1, 1, 1, 1, idx)
    tiles = oracle.scatter_gather(t1.float().cpu().contiguous(), cache.float().cpu().contiguous(), 10, 10, idx, smap)
    want = F.conv2d(tiles.double(), conv2.weight.detach().double().cpu(), conv2.bias.detach().double().cpu())
    assert tuple(got.shape) == tuple(want.shape) and _err(got, want) <= util.CONV_ATOL, _err(got, want)


class _entries:
    """Spy on the library: (entry point, bH, status) of the routed tile-conv calls and every direct-kernel call inside the block."""
    BH = {"sige_hip_gather_conv_nhwc": 8, "sige_hip_scatter_gather_conv_scatter_nhwc": 10, "sige_hip_tile_conv3_block_nhwc": 10}

    def __init__(self, hip):
        self.lib, self.seen, self.direct = hip.lib(), [], []

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in (*self.BH, "sige_hip_block_conv_direct_f32")}

        def wrap(name):
            real = self.real[name]

            def spy(*args):
                status = real(*args)
                if name in self.BH:
                    self.seen.append((name, int(args[self.BH[name]]), int(status)))
                else:  # (x, T, Cin, R, S, w, bias, Cout, kH, kW, strideH, ...)
                    self.direct.append((int(args[8]), int(args[10]), int(args[3])))
                return status
            return spy

        for n in self.real:
            setattr(self.lib, n, wrap(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.lib, n, f)
        return False


def test_packing_and_routing_through_the_modules(hip):
    """conv_pack_weights has a layout for block 10, and Gather -> SIGEConv2d -> Scatter runs it through the routed entry point."""
    from sige_amd.nn import Gather, Scatter, SIGEConv2d

    w = torch.randn(64, 64, 3, 3, device=DEV)
    packed = hip.conv_pack_weights(w, 10, 10, (1, 1))
    assert packed is not None and packed.geo == "b10" and packed.compute == "f32"
    torch.manual_seed(4)
    conv = SIGEConv2d(64, 128, 3, 1, 1).to(DEV).eval()
    g = Gather(conv, 10)
    s = Scatter(g)
    x = torch.randn(2, 64, H, W)
    xe = x + torch.randn(2, 64, H, W)
    mods = (g, conv, s)
    with torch.no_grad():
        for m in mods:
            m.set_mode("full")
        s(conv(g(_cl(x))))
        idx = _set_tiles(g, LISTS["holes"], (H, W), 4, "holes")
        for m in mods:
            m.set_mode("sparse")
        with _entries(hip) as spy:
            got = s(conv(g(_cl(xe))))
    assert ("sige_hip_gather_conv_nhwc", 10, 0) in spy.seen and not spy.direct, (spy.seen, spy.direct)
    full = F.conv2d(x.double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=1)
    tiles = F.conv2d(oracle.gather(xe, 10, 10, idx).double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())
    want = oracle.scatter(tiles.float(), full.float(), 1, 1, 1, 1, idx)
    assert _err(got, want) <= util.CONV_ATOL, _err(got, want)


# ---- c. 1x1 on 8x8 blocks, 3x3 / stride 2 on 9x9 blocks ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("kind", ["k1_8x8", "k3s2_9x9"])
def test_subtile_geometries_through_the_modules(hip, kind, C):
    """Gather -> SIGEConv2d -> Scatter against the oracle composition gather -> F.conv2d -> scatter: tiles-destination (the module
    forward) and the one-launch full destination (Scatter.forward_fused), every tile list.  The 1x1 never reaches the direct kernel;
    the 9x9 tiles destination does (by design) and its fused form does not."""
    from sige_amd.nn import Gather, Scatter, SIGEConv2d

    k, s_, pad, res = (1, 1, 0, (H, W)) if kind == "k1_8x8" else (3, 2, 1, (2 * H, 2 * W))
    block = 8 if k == 1 else 9
    torch.manual_seed(C + k)
    conv = SIGEConv2d(C, C, k, s_, pad).to(DEV).eval()
    g = Gather(conv, 8 if k == 1 else 10)
    sc = Scatter(g)
    sc.inplace = True
    gen = torch.Generator().manual_seed(C)
    x, xe = torch.randn(2, C, *res, generator=gen), torch.randn(2, C, *res, generator=gen)
    wc, bc = conv.weight.detach().cpu(), conv.bias.detach().cpu()
    mods = (g, conv, sc)
    with torch.no_grad():
        for m in mods:
            m.set_mode("full")
        sc(conv(g(_cl(x))))
        full = F.conv2d(x, wc, bc, stride=s_, padding=pad)
        for t, name in enumerate(NAMES):
            idx = _set_tiles(g, tile_lists(3, 4, 8 * s_, pad)[name], res, 3 if k == 1 else 4, name)
            for m in mods:
                m.set_mode("sparse")
            tiles = oracle.gather(xe, block, block, idx)
            o = F.conv2d(tiles, wc, bc, stride=s_) if idx.shape[0] else torch.zeros((0, C, 8 // s_, 8 // s_))
            want = oracle.scatter(o, full, pad, pad, s_, s_, idx)
            with _entries(hip) as spy:
                got = sc(conv(g(_cl(xe)))).clone()
            assert _err(got, want) <= util.CONV_ATOL, (kind, name, "modules", _err(got, want))
            assert (k == 3) or not spy.direct, spy.direct
            with _entries(hip) as spy:
                got = sc.forward_fused(conv, g(_cl(xe))).clone()
            assert _err(got, want) <= util.CONV_ATOL, (kind, name, "fused", _err(got, want))
            assert not spy.direct, (kind, name, spy.direct)
            if idx.shape[0]:
                assert ("sige_hip_gather_conv_nhwc", 4 if k == 1 else 5, 0) in spy.seen, spy.seen


# ---- d. the smallest network ------------------------------------------------------------------------------------------------------
def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


def _cfg10():
    return dataclasses.replace(small_cfg(), main_block=10, shortcut_block=8)


def _new_model(cfg, x0):
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(cfg).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        model(_cl(x0), torch.zeros(1, device=DEV))
    return model


def _with_oracle(cfg, names=("interior", "corner", "large")):
    """(GPU model of `cfg` after its full pass, x0, noise, t, {mask name: the same model's sparse output on the CPU oracle})."""
    from sige_amd import runtime
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    x0, noise = small_inputs()
    torch.manual_seed(0)
    cpu = DDPMSparseUNet(cfg).eval()
    wants = {}
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            cpu.set_mode("full")
            cpu(x0, torch.zeros(1))
            for name in names:
                m = small_masks()[name]
                cpu.set_masks(_build_masks(m))
                cpu.set_mode("sparse")
                wants[name] = cpu(x0 + noise * m, torch.zeros(1)).clone()
    finally:
        runtime.unregister_backend("cpu")
    return _new_model(cfg, x0), _cl(x0), _cl(noise), torch.zeros(1, device=DEV), wants


@pytest.fixture(scope="module")
def small10(hip):
    return _with_oracle(_cfg10())


def _sparse(model, x0, noise, t, mask, forwards=1):
    mask = mask.to(DEV)
    x1 = _cl(x0 + noise * mask)
    model.set_masks(_build_masks(mask))
    model.set_mode("sparse")
    out = None
    for _ in range(forwards):
        out = model(x1, t)
    return x1, out.clone()


@pytest.mark.parametrize("name", ["interior", "corner", "large"])
def test_small_network_blocks_10_8_vs_cpu_oracle(hip, small10, name):
    model, x0, noise, t, wants = small10
    with torch.no_grad(), _entries(hip) as spy:
        _, got = _sparse(model, x0, noise, t, small_masks()[name])
    err = util.record_margin("block10", "small %s blocks 10/8 vs oracle" % name, _err(got, wants[name]), util.CONV_ATOL)
    print("block10 small %-8s err %.3e  routed %d  direct %s" % (name, err, len(spy.seen), spy.direct), flush=True)
    assert err <= util.CONV_ATOL, err
    ran = [c for c in spy.seen if c[1] == 10 and c[2] == 0]
    assert ran, spy.seen                                                 # the new form ran ...
    assert not [d for d in spy.direct if d[:2] in ((3, 1), (1, 1))], spy.direct   # ... and no 3x3 / s1 or 1x1 conv fell to the direct kernel


@pytest.mark.parametrize("name", ["corner", "large"])
def test_small_network_main_block_10_default_shortcut_block(hip, name):
    """main_block = 10 alone (shortcut_block stays 4): the up path's blocks have a 1x1 shortcut on 4x4 cells next to a conv1 on 10x10
    windows.  The pair is not formed (nn.paired_convs: no pair kernel for this geometry), so nothing is held when conv1 runs: the
    3x3 convs stay on the 10x10 form, none reaches the direct kernel, and the block residual reads 4x4 shortcut cells."""
    model, x0, noise, t, wants = _with_oracle(dataclasses.replace(small_cfg(), main_block=10), names=(name,))
    assert any(getattr(b, "sparse_main", False) and b.cin != b.cout and getattr(b, "pair", True) for b in model.modules() if hasattr(b, "cin"))
    with torch.no_grad(), _entries(hip) as spy:
        _, got = _sparse(model, x0, noise, t, small_masks()[name])
    err = util.record_margin("block10", "small %s blocks 10/4 vs oracle" % name, _err(got, wants[name]), util.CONV_ATOL)
    print("block10 small 10/4 %-8s err %.3e  routed %d  direct %s" % (name, err, len(spy.seen), spy.direct), flush=True)
    assert err <= util.CONV_ATOL, err
    assert [c for c in spy.seen if c[1] == 10 and c[2] == 0], spy.seen
    assert not [c for c in spy.seen if c[1] == 10 and c[2] != 0], spy.seen          # no 10x10 call was refused ...
    assert not [d for d in spy.direct if d[:2] in ((3, 1), (1, 1))], spy.direct     # ... and no 3x3 / s1 or 1x1 conv ran on the direct kernel


def test_small_network_blocks_10_8_graph_replay(hip, small10):
    import bench

    model, x0, noise, t, _ = small10
    with torch.no_grad():
        x1, want = _sparse(model, x0, noise, t, small_masks()["interior"], forwards=3)
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), _err(out, want)
        del g, out


def test_launch_plan_refuses_block_10(hip, small10):
    from sige_amd.plan import LaunchPlan

    model, x0, noise, t, _ = small10
    m0 = small_masks()["interior"].to(DEV)
    xs = (x0 + noise * m0).clone(memory_format=torch.channels_last)
    with torch.no_grad():
        plan = LaunchPlan(model)
        with pytest.raises(RuntimeError, match="launch plans do not cover block size 10"):
            plan.record(m0, _build_masks, lambda: model(xs, t))
        del plan
    torch.cuda.synchronize()
    assert hip.plan_recorder() is None and hip.lib().sige_hip_plan_recording() == 0


def test_default_blocks_do_not_meet_the_new_form(hip):
    """The default configuration: no call carries a block of 8 / 9 / 10, none goes to the new entry point, and the output is the
    CPU oracle's within the row's tolerance.  (Its launch count is pinned by the existing small-network tests, unmodified.)"""
    model, x0, noise, t, wants = _with_oracle(small_cfg(), names=("large",))
    with torch.no_grad(), _entries(hip) as spy:
        _, got = _sparse(model, x0, noise, t, small_masks()["large"])
    err = util.record_margin("block10", "small large default blocks vs oracle", _err(got, wants["large"]), util.CONV_ATOL)
    assert err <= util.CONV_ATOL, err
    assert spy.seen and not [c for c in spy.seen if c[1] in (8, 9, 10)], spy.seen
    assert not [c for c in spy.seen if c[0] == "sige_hip_tile_conv3_block_nhwc"], spy.seen
