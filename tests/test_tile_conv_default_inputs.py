"""Without a GPU: what tests/test_gpu_tile_conv_default.py compares the default channels-last tile conv with -- the shapes and the
clipping of every reference builder in tests/tile_default_common.py, the oracle's tiles of the two geometries tile3_common does not
hold against a direct F.pad + unfold of the image, and the refusals the GPU file expects against plan_conv's usable() restated.
A wrong expectation must not pass as a refusal, a wrong reference not as a kernel error."""
import pytest
import torch
import torch.nn.functional as F

from tests import tile3_common as T
from tests import tile_default_common as D

H, W = D.H, D.W


def test_geometries_and_lists():
    assert (H, W) == (18, 26) and H % 4 and W % 4 and not (H % 2 or W % 2)
    assert D.GEO["K31"] == (6, 3, 1, 1, 4, (18, 26)) and D.GEO["K11"] == (4, 1, 1, 0, 4, (18, 26)) and D.GEO["K32"] == (5, 3, 2, 0, 2, (9, 13))
    for geo, g in D.GEO.items():
        assert g.ro == (g.block - g.kernel) // g.stride + 1
        L = D.lists(geo)
        assert {k: L[k].shape[0] for k in D.NAMES} == {"every": 35, "corners": 4, "interior": 1, "holes": 23, "empty": 0, "every34": 34}
        pad = 1 if geo == "K31" else 0
        assert L["every"].tolist() == [[4 * i - pad, 4 * j - pad] for i in range(5) for j in range(7)]
        assert torch.equal(L["every34"], L["every"][:-1]) and all(v.dtype == torch.int32 for v in L.values())
    assert D.LISTS0["every32"].shape[0] == 32 and 32 % 8 == 0 and 35 % 8 and 35 % 4 and 34 % 4
    # tile pixels against image pixels: the count passes with tiles missing (the rule of hip.gather_conv_cl / block_conv.hip)
    assert 35 * 16 == 560 and 34 * 16 >= H * W == 468 and 29 * 16 < H * W


@pytest.mark.parametrize("geo", ["K31", "K11", "K32"])
def test_cover_and_clipping(geo):
    g = D.GEO[geo]
    L = D.lists(geo)
    assert bool(D.covered(geo, L["every"]).all()) and not bool(D.covered(geo, L["empty"]).any())
    miss = ~D.covered(geo, L["every34"])
    # the missing corner tile: its LIVE pixels only -- rows 16..17, columns 24..25 of 18 x 26; the one pixel (8, 12) of 9 x 13
    want = torch.zeros(g.res, dtype=torch.bool)
    if geo == "K32":
        want[8, 12] = True
    else:
        want[16:18, 24:26] = True
    assert torch.equal(miss, want) and int(miss.sum()) == (1 if geo == "K32" else 4)
    assert int(D.covered(geo, L["corners"]).sum()) == {"K32": 4 + 2 + 2 + 1}.get(geo, 16 + 8 + 8 + 4)
    # place: every tile's crop lands where the cover says, clipped, and nothing else moves
    B, cout = 2, 3
    prev = torch.randn(B, cout, *g.res)
    for name in ("every", "holes", "corners", "empty"):
        idx = L[name]
        tiles = torch.ones(B * idx.shape[0], cout, g.ro, g.ro, dtype=torch.float64)
        seen = []
        out = D.place(geo, prev, tiles, idx, B, lambda t, b, hs, ws: (seen.append((hs.stop - hs.start, ws.stop - ws.start)), t * 0 + 7.0)[1])
        cover = D.covered(geo, idx)
        assert bool((out[:, :, cover] == 7.0).all()) and torch.equal(out[:, :, ~cover], prev.double()[:, :, ~cover])
        if name == "every":  # the last row of tiles is cut to 2 (1) rows, the last column to 2 (1) columns
            small = g.ro // 2
            assert (small, small) in seen and (g.ro, small) in seen and (small, g.ro) in seen and (g.ro, g.ro) in seen


@pytest.mark.parametrize("geo", ["K11", "K32"])
@pytest.mark.parametrize("B", [1, 2])
def test_oracle_tiles_equal_pad_and_unfold(geo, B):
    """oracle.gather at offset 0: block (i, j) is the image, zero-padded below and to the right, at rows 4i.., columns 4j..; behind
    an affine + SiLU the padding stays an exact 0."""
    g = D.GEO[geo]
    shape = (64, 64, 72)
    c = T.case(*shape, 1) if B == 1 else T.case(68, 0, 24, 2)
    x = T.full_input(c)
    C = x.shape[1]
    idx = D.lists(geo)["every"]
    hp, wp = 16 + g.block, 24 + g.block

    def unfold(t):
        t = F.pad(t.double(), (0, wp - W, 0, hp - H))
        u = t.unfold(2, g.block, 4).unfold(3, g.block, 4)  # [B, C, 5, 7, block, block]
        assert u.shape[2:4] == (5, 7)
        return u.permute(0, 2, 3, 1, 4, 5).reshape(B * 35, C, g.block, g.block)

    got = D.gather_tiles(geo, c, idx, "none", "identity")
    assert tuple(got.shape) == (B * 35, C, g.block, g.block) and torch.equal(got.double(), unfold(x))
    staged = D.gather_tiles(geo, c, idx, "shared", "swish")
    z = c["scale1"].double() * x.double() + c["shift1"].double()
    live = unfold(torch.ones_like(x)) > 0
    want = torch.where(live, unfold(z * torch.sigmoid(z)), torch.zeros((), dtype=torch.float64))
    assert float((staged.double() - want).abs().max()) <= 1e-5 and bool((staged[~live] == 0).all())
    assert not bool(live[-1, :, -1, -1].any()) and bool(live[0].all())


@pytest.mark.parametrize("geo", ["K31", "K11", "K32"])
def test_reference_builders_shapes(geo):
    g = D.GEO[geo]
    for shape, B in (((68, 0, 24), 2), ((64, 64, 72), 1)):
        cout = shape[2]
        for name in D.NAMES:
            N = D.lists(geo)[name].shape[0]
            want = D.want_gather(geo, shape, B, name, "affine+silu")
            assert want.dtype == torch.float64 and tuple(want.shape) == (B * N, cout, g.ro, g.ro)
            assert D.want_gather(geo, shape, B, name, "affine+silu") is want  # (cached: computed once per run)
        prev, residual = D.dest(geo, shape, B)
        assert tuple(prev.shape) == tuple(residual.shape) == (B, cout, *g.res)
        w, bias = D.weights(geo, shape, B)
        assert tuple(w.shape) == (cout, shape[0] + shape[1], g.kernel, g.kernel) and tuple(bias.shape) == (cout,)
    # a conv of the whole padded image gives the same numbers as the tiles (K32: F.pad (0, 1, 0, 1), stride 2 -> 9 x 13)
    shape, B = (68, 0, 24), 2
    c = T.case(*shape, B)
    w, bias = D.weights(geo, shape, B)
    pad = {"K31": (1, 1, 1, 1), "K11": (0, 0, 0, 0), "K32": (0, 1, 0, 1)}[geo]
    dense = F.conv2d(F.pad(c["x"].double(), pad), w.double(), bias.double(), stride=g.stride)
    assert tuple(dense.shape[2:]) == g.res
    zero = torch.zeros(B, shape[2], *g.res)
    full = D.place(geo, zero, D.want_gather(geo, shape, B, "every", "raw"), D.lists(geo)["every"], B, lambda t, b, hs, ws: t)
    assert float((full - dense).abs().max()) <= 1e-12
    # the mutations the GPU file is shown to fail under do change the reference
    moved = D.conv64(geo, D.gather_tiles(geo, c, D.shifted(D.lists(geo)["holes"]), "none", "identity"), w, bias)
    assert float((moved - D.want_gather(geo, shape, B, "holes", "raw")).abs().max()) > 0.1
    w0 = w.clone()
    w0[:, -1] = 0
    cut = D.conv64(geo, D.gather_tiles(geo, c, D.lists(geo)["holes"], "none", "identity"), w0, bias)
    assert float((cut - D.want_gather(geo, shape, B, "holes", "raw")).abs().max()) > 100 * T.bound(cut)


def test_half_rounded_and_scatter_gather_references():
    shape, B = (96, 0, 40), 2
    c = T.case(*shape, B)
    a, b = D.want_gather("K31", shape, B, "holes", "raw"), D.want_gather("K31", shape, B, "holes", "raw", half=True)
    assert a.shape == b.shape and 1e-5 < float((a - b).abs().max()) < 2e-2
    tiles = T.gather_tiles(c, T.LISTS["holes"], "none", "identity", False)
    assert torch.equal(b, T.conv64(tiles.half(), c["w"].half(), c["bias"]))
    s = D.want_scatter_gather(shape, B, "holes", "shared")
    assert tuple(s.shape) == (B * 23, 40, 4, 4)
    s16 = D.want_scatter_gather(shape, B, "holes", "shared", half_cache=True)
    assert 0 < float((s - s16).abs().max()) < 2e-2  # (`holes` reads the cached tensor: its fp16 storage shows)
    alt = D.want_gather("K31", shape, B, "every", "raw", alt=True)
    assert float((alt - D.want_gather("K31", shape, B, "every", "raw")).abs().max()) > 0.1


def test_chunk_sizes_and_tiles_per_block():
    """conv_mfma.hpp: ConvGeo::CC = 4 * (16 | 4) * (64 / MT), ConvGeoH::CC = 4 * (2 | 1) * 8 * (64 / MT); TPB = MT / (RO * RO)."""
    assert [D.chunk("K31", mt) for mt in (32, 16)] == [32, 64] and [D.chunk("K11", mt) for mt in (32, 16)] == [128, 256]
    assert [D.chunk("K32", mt) for mt in (32, 16)] == [32, 64]
    assert [D.chunk("K31", mt, "f16") for mt in (32, 16)] == [64, 128] and [D.chunk("K11", mt, "f16x3") for mt in (32, 16)] == [128, 256]
    assert [D.chunk("K32", mt, "f16") for mt in (32, 16)] == [32, 64]  # (no fp16 kernels at stride 2: the pack is an fp32 one)
    assert [D.tiles_per_block(g, mt) for g in ("K31", "K11", "K32") for mt in (32, 16)] == [2, 1, 2, 1, 8, 4]
    # the shapes are what their comments say: chunk counts at MT = 32 / 16 for 3x3
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    assert 68 % 32 and 68 % 64 and 24 % 16 and cdiv(96, 32) == 3 and cdiv(256, 64) == 4 and cdiv(256, 64) // 2 >= 2


def test_refusals_follow_usable():
    for args, want in D.EXPECTED:
        assert D.refused(*args) is want, args
    # usable() by hand for the three cat shapes: which block shapes are left
    assert D.block_shapes("K31", 64, 64, 1, 35) == [32, 16] and D.block_shapes("K31", 32, 32, 1, 35) == [32]
    assert D.block_shapes("K31", 20, 44, 1, 35) == [] and D.block_shapes("K11", 64, 64, 1, 35) == []
    # a per-batch affine: N % tiles-per-block, only with B > 1
    assert D.block_shapes("K31", 64, 0, 2, 35, True) == [16] and D.block_shapes("K31", 64, 0, 2, 34, True) == [32, 16]
    assert D.block_shapes("K32", 64, 0, 2, 35, True) == [] and D.block_shapes("K32", 64, 0, 2, 32, True) == [32, 16]
    assert D.block_shapes("K32", 64, 0, 2, 28, True) == [16]
    # no positive case of the GPU file is a refusal: shapes without a cat at either batch, on every list
    for geo in D.GEO:
        for shape in D.SHAPES[:4]:
            for B in (1, 2):
                for name in D.NAMES:
                    assert not D.refused(geo, shape, B, D.lists(geo)[name].shape[0])
    assert not D.refused("K31", (20, 44, 64), 1, 0)  # (an empty list is no refusal: nothing launches)
    # the callers' own rule (hip.cat_fusable: nn/dense.py and nn/gather.py concatenate where it says no) is the same arithmetic
    from sige_amd import hip

    for shape in D.SHAPES[4:]:
        for B in (1, 2):
            for geo, k in (("K31", 3), ("K11", 1), ("K32", 3)):
                assert hip.cat_fusable(B, shape[0], (k, k)) == (not D.refused(geo, shape, B, 35)), (geo, shape, B)
