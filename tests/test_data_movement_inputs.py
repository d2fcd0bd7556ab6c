"""CPU checks of tests/data_movement_common.py, the references of tests/test_gpu_data_movement_ragged.py: the oracle's scatters equal a
placement loop written out by hand on every geometry; the pixel kinds of the block-residual case are all present; the hand-built
tile table and the launch sizes are what the GPU file assumes; and every reference DISCRIMINATES -- a deliberately wrong variant
(the list shifted by one tile, the stride-2 division replaced by a plain offset, the seam rule dropped) differs from the right one on
every non-empty list, so a kernel with that defect cannot pass.  Nothing is broken on the GPU to show this."""
import pytest
import torch

from oracle import oracle
from tests import data_movement_common as D
from tests import tile3_common as T

NONEMPTY = [n for n in D.NAMES if n != "empty"]
# Every mutation test counts its comparisons of a right reference with a wrong one and asserts the count.  In all: 156 with the list (or
# the map's list) shifted by one tile, 16 with the stride-2 division replaced by a plain offset, 2 with the seam rule dropped.


def _shift(idx):
    return (idx + torch.tensor([[0, 4]], dtype=torch.int32)).contiguous()


def test_geometries_overhang_the_border():
    assert (D.H, D.W) == (18, 26) and D.H % 4 and D.W % 4
    for name, g in D.GEOS.items():
        every = g["lists"]["every"]
        assert every.shape[0] == D.NMAX and g["lists"]["every34"].shape[0] == 34
        h0, w0 = every[-1].tolist()
        assert h0 + g["block"] > D.H and w0 + g["block"] > D.W, name                          # the last window leaves the image
        h, w = D.origin(g, h0, w0)
        assert h < g["out_res"][0] < h + g["tile"] and w < g["out_res"][1] < w + g["tile"], name  # ... and so does its output tile
        for idx in g["lists"].values():  # outputs start on the out-tile grid (what a tile table requires) and never left of / above 0
            for a, b in idx.tolist():
                h, w = D.origin(g, a, b)
                assert h >= 0 and w >= 0 and h % g["tile"] == 0 and w % g["tile"] == 0
    assert D.GEOS["G5a"]["out_res"] == (9, 13) and D.origin("G5b", 15, 23) == (8, 12) and D.origin("G5a", 16, 24) == (8, 12)


@pytest.mark.parametrize("geo", list(D.GEOS))
@pytest.mark.parametrize("B,C", [(1, 4), (2, 36)])
def test_oracle_scatter_equals_the_placement_loop(geo, B, C):
    shifted = plain = 0
    c = D.case(C, B)
    for name in D.NAMES:
        idx = D.GEOS[geo]["lists"][name]
        x, y, residual, z = D.scatter_inputs(c, geo, idx)
        for r in (None, residual):
            want = D.scatter_ref(x, y, geo, idx, r)
            assert torch.equal(want, D.hand_scatter(x, y, geo, idx, r)), (geo, name)
            cover = D.covered(geo, idx)
            assert torch.equal(want[:, :, ~cover], y[:, :, ~cover])          # (the oracle writes the covered pixels only)
            assert (not bool(cover.any())) or bool(cover.all()) or not torch.equal(D.in_place(want, z, cover), want)  # (z is not y: a stray write shows)
        if name != "empty":
            shifted += 1
            assert not torch.equal(want, D.scatter_ref(x, y, geo, _shift(idx), residual)), (geo, name)
            if D.GEOS[geo]["stride"] == 2:
                plain += 1
                assert not torch.equal(want, D.hand_scatter(x, y, geo, idx, residual, plain_offset=True)), (geo, name)
    assert (shifted, plain) == (4, 4 if D.GEOS[geo]["stride"] == 2 else 0)


def test_hand_table_names_the_tile_under_every_covered_pixel():
    shifted = 0
    for geo, g in D.GEOS.items():
        for name in D.NAMES + ["every34"]:
            idx = g["lists"][name]
            table = D.hand_table(idx, geo)
            assert tuple(table.shape) == (5, 7) and int((table >= 0).sum()) == idx.shape[0]
            cover = D.covered(geo, idx)
            t = g["tile"]
            up = table.repeat_interleave(t, 0).repeat_interleave(t, 1)[:g["out_res"][0], :g["out_res"][1]]
            assert torch.equal(up >= 0, cover), (geo, name)
            for n, (a, b) in enumerate(idx.tolist()):
                h, w = D.origin(g, a, b)
                assert int(up[h, w]) == n
            if name in NONEMPTY:
                shifted += 1
                assert not torch.equal(table, D.hand_table(_shift(idx), geo)), (geo, name)
    assert shifted == 16
    # G6's table is the one the existing tests build for the shortcut cells
    for name in D.NAMES:
        idx1, table = T.shortcut(T.LISTS[name])
        assert torch.equal(table, D.shortcut_table(idx1))


def test_scatter_map_discriminates():
    shifted = 0
    for name in NONEMPTY:
        idx = T.LISTS[name]
        m = D.scatter_map(idx)
        assert torch.equal(m[..., 0] >= 0, D.covered("G6", idx)) and torch.equal(m[..., 0] >= 0, T.covered(idx))
        assert bool((m[m[..., 0] < 0] == -1).all())
        shifted += 1
        assert not torch.equal(m, D.scatter_map(_shift(idx)))
    assert shifted == 4


def test_block_residual_pixel_kinds_and_reference():
    shifted = 0
    main, short = D.covered("G6", T.LISTS["holes"]), D.covered_short(D.SHORT_B)
    kinds = {"shortcut_only": int((short & ~main).sum()), "main_only": int((main & ~short).sum()), "both": int((main & short).sum()),
             "neither": int((~main & ~short).sum())}
    assert kinds == D.KINDS_B and sum(kinds.values()) == D.H * D.W
    for B, C in ((1, 4), (2, 36)):
        c = D.case(C, B)
        for tag, idx0, idx1 in D.block_residual_lists():
            if not tag.startswith("b-"):  # (a): every shortcut cell lies inside a main tile
                assert not bool((D.covered_short(idx1) & ~D.covered("G6", idx0)).any()), tag
            x0, y0, x1, y1, z = D.block_residual_inputs(c, idx0, idx1)
            want = D.block_residual_ref(x0, y0, x1, y1, idx0, idx1)
            assert torch.equal(want, D.hand_block_residual(x0, y0, x1, y1, idx0, idx1)), tag
            cover = D.covered("G6", idx0) | D.covered_short(idx1)
            assert torch.equal(want[:, :, ~cover], y0[:, :, ~cover])
            if idx0.shape[0]:
                shifted += 2
                assert not torch.equal(want, D.block_residual_ref(x0, y0, x1, y1, _shift(idx0), idx1)), tag
                assert not torch.equal(want, D.block_residual_ref(x0, y0, x1, y1, idx0, _shift(idx1))), tag
    assert shifted == 20


@pytest.mark.parametrize("B,C", [(1, 4), (2, 36)])
def test_gather_family_references_discriminate(B, C):
    shifted = 0
    c = D.case(C, B)
    for geo, g in D.GEOS.items():
        for name in NONEMPTY:
            idx = g["lists"][name]
            want = D.gather_ref(c, geo, idx, "shared", "identity")
            lv = D.live(geo, idx, B)
            assert bool((want[~lv.expand_as(want)] == 0).all()) and (int((~lv).sum()) > 0 or name == "interior")  # padding: an exact 0
            shifted += 1
            assert not torch.equal(want, D.gather_ref(c, geo, _shift(idx), "shared", "identity")), (geo, name)
    for name in NONEMPTY:
        idx = T.LISTS[name]
        t4, want = D.sg_ref(c, idx, "shared", "identity")
        sc, sh = D.affine_of(c, "shared")
        shifted += 2
        assert not torch.equal(want, oracle.scatter_gather(t4, c["y"], 6, 6, _shift(idx), D.scatter_map(idx), sc, sh))            # the windows
        assert not torch.equal(want, oracle.scatter_gather(t4, c["y"], 6, 6, idx, D.scatter_map(_shift(idx)), sc, sh))            # the map
        # the same call through the per-image helper of the SPADE reference
        assert torch.equal(want, D.sg_own_list(t4, c["y"], idx, D.scatter_map(idx), sc, sh))
        for source in (1, 2):
            ref = D.spade_ref(c, idx, T.LISTS["holes"], source, "shared", D.SLOPE)
            shifted += 2
            assert not torch.equal(ref, D.spade_ref(c, _shift(idx), T.LISTS["holes"], source, "shared", D.SLOPE))
            assert not torch.equal(ref, D.spade_ref(c, idx, _shift(T.LISTS["holes"]), source, "shared", D.SLOPE))
            assert not torch.equal(ref, D.spade_ref(c, idx, T.LISTS["holes"], source, "shared", None))                           # the leaky
    if C == 36:
        for name in NONEMPTY:
            idx = T.LISTS[name]
            parts = D.split_ref(c, idx, 3, "relu")[1]
            assert len(parts) == 3 and all(p.shape[1] == C // 3 for p in parts)
            shifted += 1
            assert not all(torch.equal(a, b) for a, b in zip(parts, D.split_ref(c, _shift(idx), 3, "relu")[1]))
    assert shifted == (44 if C == 36 else 40)


def test_split_shapes_are_whole_units():
    # a part is a whole number of 4-channel units (csrc/spade_ops.hip: C % (4 parts) == 0); 24 divides by 2 and by 3 that way, 36
    # only by 3 (36 / 2 = 18 channels is four and a half units), 64 only by 2
    assert all(C % (4 * parts) == 0 for C, parts in D.SPLITS) and 36 % 8 and 64 % 12
    assert {p for _, p in D.SPLITS} == {2, 3}


def test_stacked_references_keep_the_seam():
    seam = 0
    c = D.stacked_case(36)
    idx = T.stacked_list()
    assert int(idx[T.NS - 1, 0]) == 11 and int(idx[T.NS, 0]) == 15  # image 0's last windows reach row 16, image 1's first start at 15
    for affine in (False, True):
        want = T.stacked_tiles(c, 1, affine)
        seam += 1
        wrong = D.seamless_gather(c, affine)
        assert not torch.equal(want, wrong)
        # the two differ exactly in the windows that cross the seam: image 0's last row of windows, image 1's first
        differ = (want != wrong).flatten(1).any(1).reshape(2, 4, 7)
        assert bool(differ[0, 3].all()) and bool(differ[1, 0].all()) and not bool(differ[0, :3].any()) and not bool(differ[1, 1:].any())
        # rows 16.. of image 0's overhanging windows are zero, not image 1's pixels
        last = want[:T.NS].reshape(4, 7, -1, 6, 6)[3]
        assert bool((last[..., 5, :] == 0).all()) and not bool((wrong[:T.NS].reshape(4, 7, -1, 6, 6)[3][..., 5, :] == 0).all())
    for source in (1, 2):
        ref = D.stacked_spade_ref(c, source, D.SLOPE)
        assert tuple(ref.shape) == (2 * T.NS, 36, 6, 6)
        assert bool((ref[:T.NS].reshape(4, 7, -1, 6, 6)[3][..., 5, :] == 0).all())
    assert seam == 2


def test_conv_in_window_mask():
    for name in ("every", "corners", "holes"):
        m = D.window_mask(T.LISTS[name])
        assert int(m.sum()) == {"every": 18 * 26, "corners": 25 + 15 + 15 + 9, "holes": int(m.sum())}[name]
        assert bool(m[0, 0]) and bool(m[17].any()) and bool(m[:, 25].any())  # windows clipped at each of the four borders in every list
    assert not bool(D.window_mask(T.LISTS["holes"]).all())


def test_large_cases_take_a_second_grid_stride_trip():
    assert D.NBIG == 1089 and D.LIST_BIG[-1].tolist() == [127, 127] and 127 + 6 > D.BIG
    for op, (C, units) in D.BIG_UNITS.items():
        assert D.TRIP < units < 2 * D.TRIP + D.TRIP and units < 2 ** 31, (op, units)
    assert D.BIG_UNITS["gather"][1] == 5018112 and D.BIG_UNITS["scatter"][1] == 4326400 and D.BIG_UNITS["scatter_in_place"][1] == 4460544
    # the matrix itself never gets there: its largest launch
    assert 2 * 18 * 26 * 16 < D.TRIP and 2 * 35 * 36 * 16 < D.TRIP
