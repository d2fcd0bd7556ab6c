"""sige_hip_commit_tiles (csrc/commit_tiles.hip) against the CPU reference of tests/commit_common.py on the ragged 18 x 26 image:
every geometry and list of tests/data_movement_common.py, full and tile sources, fp32 and fp16 destinations, the affine + SiLU form,
many records in one call, more records than one launch holds, and lists the library refuses.  Every destination starts from seeded
values that are neither the source nor the reference and is compared WHOLE after the call: a stray write shows.
tests/test_commit_tiles_inputs.py (CPU) shows that the reference is the oracle's scatter."""
import pytest
import torch

from tests import commit_common as K
from tests import data_movement_common as D
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
DEV = torch.device("cuda")
CL = torch.channels_last


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t, half=False):
    t = t.to(DEV).contiguous(memory_format=CL)
    return t.half() if half else t


def _eq(got, want, tag):
    want = want.to(got.device)
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (tag, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (
            tag, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


def _record(hip, C, geo, name, tile_source, which="xa", half=False, affine=None):
    """(record, its destination on the device, the CPU inputs (src, dst0, idx))."""
    tiles, full, dst0, idx = K.inputs(C, geo, name, which)
    src = tiles if tile_source else full
    if half:
        dst0 = dst0.half().float()
    dst = _cl(dst0, half)
    sc, sh = (None, None) if affine is None else (affine[0].to(DEV), affine[1].to(DEV))
    rec = hip.CommitRecord(_cl(src), dst, idx.to(DEV), tile_source=tile_source, scale=sc, shift=sh, **K.record_args(geo))
    return rec, dst, (src, dst0, idx)


def _commit(hip, recs, launches):
    n0 = hip.launch_count()
    got = hip.commit_tiles(recs)
    assert got == launches, (got, launches)
    assert hip.launch_count() - n0 == launches
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", K.CHANNELS)
def test_identity_records_are_bit_exact(hip, C):
    for geo in K.GEOS:
        for name in K.NAMES:
            for tile_source in (False, True):
                rec, dst, (src, dst0, idx) = _record(hip, C, geo, name, tile_source)
                _commit(hip, [rec], int(name != "empty"))
                _eq(dst, K.commit_ref(dst0, src, geo, idx, tile_source), "%s %s tiles=%s C=%d" % (geo, name, tile_source, C))


@pytest.mark.parametrize("C", (36, 132))
def test_fp16_destinations_are_the_rounded_reference(hip, C):
    for geo in K.GEOS:
        for name in ("corners", "holes", "empty"):
            for tile_source in (False, True):
                rec, dst, (src, dst0, idx) = _record(hip, C, geo, name, tile_source, half=True)
                assert dst.dtype == torch.float16
                _commit(hip, [rec], int(name != "empty"))
                _eq(dst, K.commit_ref(dst0, src, geo, idx, tile_source).half(), "f16 %s %s tiles=%s C=%d" % (geo, name, tile_source, C))


@pytest.mark.parametrize("C", (4, 36, 132))
def test_affine_records_match_the_cpu_formula_and_affine_act_cl(hip, C):
    c = D.case(C, 1)
    aff = (c["scale1"], c["shift1"])
    worst = 0.0
    for geo in K.GEOS:
        for name in ("every", "holes"):
            for tile_source in (False, True):
                tag = "affine %s %s tiles=%s C=%d" % (geo, name, tile_source, C)
                rec, dst, (src, dst0, idx) = _record(hip, C, geo, name, tile_source, affine=aff)
                _commit(hip, [rec], 1)
                # (a) the CPU formula, within the SiLU criterion on the covered pixels; the others keep their bits
                want = K.commit_ref(dst0, src, geo, idx, tile_source, value=lambda v: K.affine_swish(v, *aff))
                got = dst.cpu().contiguous()
                cover = D.covered(geo, idx)[None, None].expand_as(got)
                assert torch.equal(got[~cover], dst0[~cover]), tag
                m = float(((got - want).abs() / (want.abs() + util.SWISH_ATOL / util.SWISH_RTOL)).max())
                worst = max(worst, m)
                print("%s: %.3g (bound %.3g)" % (tag, m, util.SWISH_RTOL))
                assert m <= util.SWISH_RTOL, (tag, m)
                # (b) bit for bit what affine_act_cl makes of the same values
                act = hip.affine_act_cl(rec.src, aff[0].to(DEV), aff[1].to(DEV), "swish")
                assert act is not None
                _eq(dst, K.commit_ref(dst0, act.cpu().contiguous(), geo, idx, tile_source), tag + " vs affine_act_cl")
    util.record_margin("test_gpu_commit_tiles", "affine C=%d" % C, worst, util.SWISH_RTOL)


@pytest.mark.parametrize("t", (8, 12))
def test_tiles_above_4x4(hip, t):
    """8 x 8 (4 passes of 16 pixels) and 12 x 12 (16 passes) output tiles, full and tile sources, C above one chunk."""
    C, idx, geo = 68, K.LARGE_TILES[t], K.large_geo(t)
    gen = torch.Generator().manual_seed(t)
    full, dst0 = torch.randn(1, C, D.H, D.W, generator=gen), torch.randn(1, C, D.H, D.W, generator=gen)
    tiles = torch.randn(idx.shape[0], C, t, t, generator=gen)
    for tile_source, src in ((False, full), (True, tiles)):
        dst = _cl(dst0)
        rec = hip.CommitRecord(_cl(src), dst, idx.to(DEV), offset=(0, 0), stride=(1, 1), tile=(t, t), tile_source=tile_source)
        _commit(hip, [rec], 1)
        want = K.commit_ref(dst0, src, geo, idx, tile_source)
        assert not torch.equal(want, dst0)
        _eq(dst, want, "tile %d tiles=%s" % (t, tile_source))


def test_mixed_records_in_one_call(hip):
    """All four geometries, both source kinds, an empty record in the middle, fp32 and fp16 destinations, an affine record, and the
    ScatterWithBlockResidual pair -- one output over its main list (G6 `holes`) and over its shortcut list (SHORT_B, 4x4 cells) into
    ONE destination: one call, one launch."""
    C = 36
    c = D.case(C, 1)
    recs, checks = [], []
    for i, (geo, name, tile_source, which) in enumerate(K.mixed_specs()):
        half = i % 3 == 2
        affine = (c["scale1"], c["shift1"]) if i % 5 == 3 else None
        rec, dst, (src, dst0, idx) = _record(hip, C, geo, name, tile_source, which, half=half, affine=affine)
        recs.append(rec)
        if affine is not None:
            src = hip.affine_act_cl(rec.src, affine[0].to(DEV), affine[1].to(DEV), "swish").cpu().contiguous()
        want = K.commit_ref(dst0, src, geo, idx, tile_source)
        checks.append((dst, want.half() if half else want, "mixed %d %s %s" % (i, geo, name)))
    # main + shortcut into one destination
    _, out, dst0, idx0 = K.inputs(C, "G6", "holes")
    dst = _cl(dst0)
    out_d = _cl(out)
    recs.insert(7, hip.CommitRecord(out_d, dst, idx0.to(DEV), **K.record_args("G6")))
    recs.append(hip.CommitRecord(out_d, dst, D.SHORT_B.to(DEV), **K.record_args("G4")))
    both = D.covered("G6", idx0) | D.covered_short(D.SHORT_B)
    checks.append((dst, torch.where(both[None, None], out, dst0), "main + shortcut"))
    assert len(recs) <= K.CAPACITY
    _commit(hip, recs, 1)
    for got, want, tag in checks:
        _eq(got, want, tag)


def test_a_list_longer_than_one_launch(hip):
    n = 2 * K.CAPACITY + 5
    recs, checks = [], []
    for i, (geo, name, tile_source, which) in enumerate(K.many_specs(n)):
        rec, dst, (src, dst0, idx) = _record(hip, 4 if i % 2 else 36, geo, name, tile_source, which)
        recs.append(rec)
        checks.append((dst, K.commit_ref(dst0, src, geo, idx, tile_source), "many %d" % i))
        if i % 10 == 0:  # records without a tile take no room in a launch
            recs.append(_record(hip, 4, geo, "empty", tile_source)[0])
    assert len(recs) > n
    _commit(hip, recs, -(-n // K.CAPACITY))
    for got, want, tag in checks:
        _eq(got, want, tag)
    # exactly one launch's worth, and one more
    full = [r for r in recs if r.idx.shape[0]]
    _commit(hip, full[:K.CAPACITY], 1)
    _commit(hip, full[:K.CAPACITY + 1], 2)


def test_an_unsupported_list_is_refused_whole(hip):
    good, dst_good, (_, dst0_good, _) = _record(hip, 36, "G6", "every", True)
    # C % 4
    gen = torch.Generator().manual_seed(5)
    idx = D.GEOS["G4"]["lists"]["every"].to(DEV)
    dst0 = torch.randn(1, 6, D.H, D.W, generator=gen)
    bad = hip.CommitRecord(_cl(torch.randn(1, 6, D.H, D.W, generator=gen)), _cl(dst0), idx, **K.record_args("G4"))
    # a batch of two
    dst0_b = torch.randn(2, 8, D.H, D.W, generator=gen)
    batch = hip.CommitRecord(_cl(torch.randn(2, 8, D.H, D.W, generator=gen)), _cl(dst0_b), idx, **K.record_args("G4"))
    # NCHW
    dst0_n = torch.randn(1, 8, D.H, D.W, generator=gen)
    nchw = hip.CommitRecord(torch.randn(1, 8, D.H, D.W, generator=gen).to(DEV), dst0_n.to(DEV), idx, **K.record_args("G4"))
    assert not nchw.dst.is_contiguous(memory_format=CL)
    # a stride that is no power of two
    odd = hip.CommitRecord(good.src, good.dst, good.idx, offset=(1, 1), stride=(3, 3), tile_source=True)
    for rec, d, d0 in ((bad, bad.dst, dst0), (batch, batch.dst, dst0_b), (nchw, nchw.dst, dst0_n), (odd, dst_good, dst0_good)):
        n0 = hip.launch_count()
        assert hip.commit_tiles([good, rec]) is None  # (the good record in front is not executed either)
        assert hip.launch_count() == n0
        torch.cuda.synchronize()
        _eq(d, d0, "refused")
        _eq(dst_good, dst0_good, "refused: the record in front")
    assert hip.commit_tiles([]) == 0
