"""The CPU reference of tests/commit_common.py against the oracle, and what its lists cover (no device): the kernel tests of
tests/test_gpu_commit_tiles.py are only as good as these."""
import pytest
import torch

from tests import commit_common as K
from tests import data_movement_common as D


@pytest.mark.parametrize("geo", K.GEOS)
def test_a_tile_source_commit_is_the_oracles_scatter(geo):
    for C in (4, 36):
        for name in K.NAMES:
            tiles, _, dst, idx = K.inputs(C, geo, name)
            want = D.scatter_ref(tiles, dst, geo, idx)  # oracle.scatter(tiles, y, offset, stride, idx, None)
            assert torch.equal(K.commit_ref(dst, tiles, geo, idx, True), want), (geo, C, name)
            assert torch.equal(want, D.hand_scatter(tiles, dst, geo, idx)), (geo, C, name)


@pytest.mark.parametrize("geo", K.GEOS)
def test_a_full_source_commit_is_a_select_under_the_covered_pixels(geo):
    for name in K.NAMES:
        _, src, dst, idx = K.inputs(36, geo, name)
        cover = D.covered(geo, idx)
        got = K.commit_ref(dst, src, geo, idx, False)
        assert torch.equal(got, torch.where(cover[None, None], src, dst)), (geo, name)
        # ... and a reference that wrote one pixel too many, or from the wrong place, would not pass
        if name != "empty":
            assert not torch.equal(got, dst) and not torch.equal(got, src) or bool(cover.all())


def test_the_lists_cover_border_tiles_and_leave_pixels_uncovered():
    for geo in K.GEOS:
        g = D.GEOS[geo]
        Ho, Wo = g["out_res"]
        clipped = 0
        for name in ("every", "corners", "holes"):
            for h0, w0 in g["lists"][name].tolist():
                h, w = D.origin(g, h0, w0)
                assert h >= 0 and w >= 0
                clipped += h + g["tile"] > Ho or w + g["tile"] > Wo
        assert clipped, geo
        assert bool(D.covered(geo, g["lists"]["every"]).all()), geo
        for name in ("corners", "interior", "holes"):
            cover = D.covered(geo, g["lists"][name])
            assert bool(cover.any()) and not bool(cover.all()), (geo, name)
        assert g["lists"]["empty"].shape[0] == 0
    # the block-residual pair: pixels under the main list only, the shortcut list only, both and neither
    main, short = D.covered("G6", D.GEOS["G6"]["lists"]["holes"]), D.covered_short(D.SHORT_B)
    assert {"shortcut_only": int((short & ~main).sum()), "main_only": int((main & ~short).sum()), "both": int((main & short).sum()),
            "neither": int((~main & ~short).sum())} == D.KINDS_B


def test_the_record_sets():
    specs = K.mixed_specs()
    assert {s[0] for s in specs} == set(K.GEOS) and {s[2] for s in specs} == {True, False}
    empties = [i for i, s in enumerate(specs) if s[1] == "empty"]
    assert empties and 0 < empties[0] < len(specs) - 1
    many = K.many_specs(2 * K.CAPACITY + 5)
    assert len(many) > 2 * K.CAPACITY and all(s[1] != "empty" for s in many)
    assert any(C > K.CHUNK and C % K.CHUNK for C in K.CHANNELS)


def test_the_affine_reference_is_the_oracles_gather_affine():
    """affine_swish is scale, then shift, then the reference's SiLU: the oracle's gather with an affine gives the same values up to
    the rounding of exp (fp32 here, one ulp = 1.2e-7 relative on the denominator) and of the final fp32 result (6e-8)."""
    from oracle import oracle

    c = D.case(36, 1)
    idx = D.GEOS["G4"]["lists"]["interior"]
    want = oracle.gather(c["x"], 4, 4, idx, c["scale1"], c["shift1"], "swish")
    raw = oracle.gather(c["x"], 4, 4, idx)
    got = K.affine_swish(raw, c["scale1"], c["shift1"])
    assert torch.allclose(got, want, rtol=3e-7, atol=1e-12)
