"""What sige_hip_resample_tiles_nhwc_f32 ANSWERS under stacked edits (sige_hip_set_edit_batch), pinned without a launch (the way of
tests/test_attention_wide_tiles_status.py).

Every case is answered by the host code before any device use, in the order include/sige_hip.h states: the existing checks, the
empty list and B == 0 (SIGE_HIP_OK), then the height -- E divides it and one image is a power of two of at least 4 rows --, then
the pooled image of a tiled DOWN launch, which needs 4 rows of its own.  The calls go through the raw ctypes function with made-up
16-byte aligned pointers that the host code never dereferences.  A case the code wrongly accepted would launch on them, so the
module skips itself where a device is present."""
import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
DOWN, UP = 0, 1

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: never where a wrongly accepted case could launch")

NAMES = ("x B C H W mode active_indices N bH bW scale shift tiles offsetH offsetW strideH strideW rH rW res stream").split()
TILED_DOWN = dict(x=0x1000, B=1, C=8, H=32, W=16, mode=DOWN, active_indices=0x2000, N=3, bH=6, bW=6, scale=0x3000, shift=0x4000,
                  tiles=0x5000, offsetH=1, offsetW=1, strideH=1, strideW=1, rH=4, rW=4, res=0x6000, stream=None)
TILED_UP = dict(TILED_DOWN, mode=UP, bH=0, bW=0, scale=None, shift=None, tiles=None)
WHOLE_DOWN = dict(TILED_DOWN, active_indices=None, N=0, bH=0, bW=0, scale=None, shift=None, tiles=None)
WHOLE_UP = dict(WHOLE_DOWN, mode=UP)

# (the edit batch around the call, the form, what the case changes, the status)
CASES = [
    (2, TILED_DOWN, dict(H=12), EUNSUPPORTED),       # 6 rows per image: not a power of two
    (2, TILED_UP, dict(H=12), EUNSUPPORTED),
    (3, TILED_DOWN, dict(H=16), EUNSUPPORTED),       # E does not divide H
    (3, TILED_UP, dict(H=16), EUNSUPPORTED),
    (3, WHOLE_DOWN, dict(H=16), EUNSUPPORTED),
    (3, WHOLE_UP, dict(H=16), EUNSUPPORTED),
    (2, WHOLE_DOWN, dict(H=4), EUNSUPPORTED),        # 2 rows per image: below 4
    (2, TILED_DOWN, dict(H=8), EUNSUPPORTED),        # 4 source rows per image: the pooled image has 2
    (2, TILED_DOWN, dict(H=8, tiles=None, bH=0, bW=0, scale=None, shift=None), EUNSUPPORTED),  # (the shortcut cells alone, too)
    (2, TILED_DOWN, dict(H=12, N=0), OK),            # the empty list is answered before the height is judged
    (2, TILED_UP, dict(H=12, N=0), OK),
    (3, TILED_DOWN, dict(H=16, N=0), OK),
    (2, TILED_DOWN, dict(H=12, B=0), OK),
    (2, TILED_DOWN, dict(H=12, x=None), EINVAL),     # (null pointers are asked before the height)
    (2, TILED_DOWN, dict(H=12, x=0x1004), EUNSUPPORTED),
    (2, TILED_DOWN, dict(H=12, C=6), EUNSUPPORTED),
    (1, TILED_DOWN, dict(H=12, tiles=None, res=None), OK),  # (E = 1: any even height passes; nothing to write)
]


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def answer(L, args, edits):
    fn = L.sige_hip_resample_tiles_nhwc_f32.fn  # (the raw ctypes function: no device guard)
    assert len(fn.argtypes) == len(NAMES)
    vals = [None if (t.__name__ == "c_void_p" and not args[n]) else args[n] for t, n in zip(fn.argtypes, NAMES)]
    L.sige_hip_set_edit_batch(edits)
    try:
        return fn(*vals)
    finally:
        L.sige_hip_set_edit_batch(1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_resample_tiles_status_under_stacked_edits(L, i):
    edits, base, change, want = CASES[i]
    assert set(change) <= set(base)
    got = answer(L, dict(base, **change), edits)
    assert got == want, (edits, change, got, want)
    assert L.sige_hip_get_edit_batch() == 1


def test_every_answer_comes_before_a_launch_and_the_version_stays(L):
    before = L.sige_hip_launch_count()
    for edits, base, change, _ in CASES:
        answer(L, dict(base, **change), edits)
    assert L.sige_hip_launch_count() == before
    assert L.sige_hip_version() == 310
