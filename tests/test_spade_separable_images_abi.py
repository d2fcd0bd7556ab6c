"""sige_hip_spade_separable_stats_nhwc_f32 and sige_hip_spade_separable_images_nhwc_f32 (csrc/spade_separable.hip) without a device:
both symbols are exported, and every refusal comes before a launch.  The raw ctypes functions are called with made-up addresses for
the WEIGHTS only (nothing dereferences them on the host) and null tensors: both entry points look at the tensors last, so a case
that was wrongly accepted would answer EINVAL there instead of launching -- also where a GPU is present."""
import ctypes
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000  # a 16-byte aligned address that is never read


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def _stats(L, H, W, Ch, dw_w=P):
    return L.sige_hip_spade_separable_stats_nhwc_f32.fn(None, H, W, Ch, dw_w, P, 1e-5, None, None, None)


def _images(L, H, W, Ch, oc, dw_w=P):
    return L.sige_hip_spade_separable_images_nhwc_f32.fn(None, H, W, Ch, dw_w, P, P, P, P, P, oc, None, None)


def test_both_symbols_are_exported(L):
    from sige_amd import hip

    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in ("sige_hip_spade_separable_stats_nhwc_f32", "sige_hip_spade_separable_images_nhwc_f32"):
        assert hasattr(handle, name), name
        assert name in hip.EXPORTS and name in hip._SIGNATURES


def test_null_operand_is_invalid(L):
    assert _stats(L, 8, 8, 16, dw_w=None) == EINVAL
    assert _images(L, 8, 8, 16, 8, dw_w=None) == EINVAL
    # (a supported shape with the tensors missing: the last check, in front of the launch)
    assert _stats(L, 8, 8, 16) == EINVAL
    assert _images(L, 8, 8, 16, 8) == EINVAL


def test_channel_counts_outside_the_range_are_unsupported(L):
    for Ch in (6, 132):
        assert _stats(L, 8, 8, Ch) == EUNSUPPORTED, Ch
        assert _images(L, 8, 8, Ch, 8) == EUNSUPPORTED, Ch
    assert _images(L, 8, 8, 16, 6) == EUNSUPPORTED


def test_image_heights_the_seam_shift_cannot_express_are_unsupported(L):
    """Under an edit batch of 2: h = 6 is no power of two, h = 2 is below the four rows stacked_shift asks for."""
    assert L.sige_hip_set_edit_batch(2) == 0
    try:
        for H in (12, 4):
            assert _stats(L, H, 8, 16) == EUNSUPPORTED, H
            assert _images(L, H, 8, 16, 8) == EUNSUPPORTED, H
    finally:
        assert L.sige_hip_set_edit_batch(1) == 0
    assert L.sige_hip_get_edit_batch() == 1
