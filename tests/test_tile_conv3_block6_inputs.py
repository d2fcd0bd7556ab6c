"""The reference side of the 6x6 tile conv v3's tests on fp16 operands (tests/tile3_common.py, tests/test_gpu_tile_conv3_block6.py)
-- nothing here touches a device.

With affine or SiLU staging the kernel rounds a STAGED value to fp16, and its SiLU is not the reference's: a value next to an fp16
rounding boundary may round the other way.  The GPU test therefore allows 1e-3 of the outputs outside |d| <= 3e-4 (1 + |want|).
That share is a cap, not a measurement: here the staging is emulated twice on the CPU, with the SiLU in fp32 and in fp64 (the
widest disagreement two correct implementations can have), both rounded to half and convolved in fp64 with the fp16-rounded
weights -- and the share of outputs beyond the same bound must be at most 1e-4, a tenth of the cap, for every affine-staged case
and tile list of the GPU test.  The oracle's own staged tiles (the GPU test's reference) are held to the same figure.

Measured with these inputs: no output outside the bound in any case (share 0); the largest |d| / (3e-4 (1 + |want|)) is 0.64
(one staged value near 16 that rounds to the neighbouring half moves an output by up to 2^-6 x one weight)."""
import pytest
import torch

from tests import tile3_common as T

LISTS = ["every", "corners", "interior", "holes"]


def _id(v):
    return "src%d-%d+%d_%d-%s" % (v[0], *v[1], v[2])


def test_geometry_is_ragged_and_the_lists_are_what_the_gpu_test_needs():
    assert T.H % 2 == 0 and T.W % 2 == 0 and T.H % 4 and T.W % 4
    every = T.LISTS["every"]
    assert int(every[:, 0].max()) + 1 + 4 > T.H and int(every[:, 1].max()) + 1 + 4 > T.W     # the last row / column overhang
    assert int(every.min()) == -1
    assert every.shape[0] % 2 == 1 and T.LISTS["holes"].shape[0] % 2 == 1 and T.LISTS["every34"].shape[0] % 2 == 0
    assert bool(T.covered(every).all()) and not bool(T.covered(T.LISTS["holes"]).all())
    # `every`: ring pixels come from neighbouring tiles; the other lists read the cached tensor too
    assert bool((T.scatter_map(every)[..., 0] >= 0).all())
    for name in ("corners", "interior", "holes"):
        m = T.scatter_map(T.LISTS[name])[..., 0]
        assert bool((m >= 0).any()) and bool((m < 0).any())
    # stacked edits: image 0's last window row reads row 16 (image 1's first), image 1's first window row reads row 15
    s = T.stacked_list()
    assert s.shape[0] == 2 * T.NS and int(s[T.NS - 1, 0]) + 5 == T.HS and int(s[T.NS, 0]) == T.HS - 1
    m = T.stacked_map()
    assert tuple(m.shape) == (2 * T.HS, T.W, 3) and int(m[..., 0].max()) == 2 * T.NS - 1
    assert torch.equal(m, T.scatter_map(s, (2 * T.HS, T.W)))  # (4x4 conv-1 tiles never cross the seam: the tall map is the two maps)


    # the seam matters to the reference: the tall image gathered as ONE image is not the two images alone
    c = T.case(64, 0, 64, 1)
    assert not torch.equal(T.oracle.gather(T.stack(c["xs"]), 6, 6, s), T.stacked_tiles(c, 1, False))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("case", T.f16_staged_cases(), ids=_id)
def test_f16_staging_reference_stays_well_inside_the_cap(case, B):
    source, shape, form = case
    c = T.case(*shape, B)
    worst_share, worst_ratio = 0.0, 0.0
    for name in LISTS:
        for half_cache in ((False, True) if source == 2 else (False,)):
            raw, staged, live, sc, sh, act = T.f16_staged_tiles(source, shape, form, name, B, half_cache)
            w16 = c["w"].half()
            lo = T.conv64(T.stage_f16(raw, live, sc, sh, act, B, silu64=False), w16, c["bias"])
            hi = T.conv64(T.stage_f16(raw, live, sc, sh, act, B, silu64=True), w16, c["bias"])
            ref = T.conv64(staged.half(), w16, c["bias"])
            for a, b in ((lo, hi), (ref, hi), (ref, lo)):
                worst_share = max(worst_share, T.f16_outside(a, b))
                worst_ratio = max(worst_ratio, float(((a - b).abs() / (T.F16_ALLOW * (1.0 + b.abs()))).max()))
            assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.5
    print("tile3 f16 staging %s B%d: worst share outside %.2e, worst |d| / allowance %.3f" % (_id(case), B, worst_share, worst_ratio))
    assert worst_share <= 1e-4, worst_share


def test_raw_staging_rounds_exactly_like_half():
    """Raw staging: the staged value IS the tensor's value, so the operand is `.half()` of it -- also through the scatter map (a
    window pixel comes from the conv-1 tile or from the cache, the other addend is an exact 0) and from an fp16-stored cache."""
    c = T.case(64, 0, 64, 1)
    idx = T.LISTS["holes"]
    one = torch.ones(1, 64, 1, 1)
    raw = T.gather_tiles(c, idx, "none", "identity", False)
    assert torch.equal(T.stage_f16(raw, T.live_pixels(idx, 1), one, 0 * one, "identity", 1, False), raw.half())
    y16 = c["y"].half()
    _, tiles = T.sg_tiles(c, idx, 1, y=y16.float())
    _, tiles32 = T.sg_tiles(c, idx, 1)
    assert torch.equal(tiles.half(), tiles32.half())  # (rounding the cache to half first changes nothing after the operand rounding)
