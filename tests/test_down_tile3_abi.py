"""The four C-ABI entries of the stride-2 Downsample conv on the tile conv v3 (include/sige_hip.h, csrc/conv_tile3_s2.hip): exported,
bound with the header's signatures, their host-side shape rules -- and what stays as it was: the switch is off and this geometry's
tile pack is exact fp32 whatever compute is asked for.  Nothing here touches a device."""
import ctypes
import os
import re

import pytest
import torch

NAMES = ("sige_hip_down_tile3_supported", "sige_hip_down_tile3_packed_size", "sige_hip_down_tile3_pack", "sige_hip_down_tile3_nhwc")
EINVAL, EUNSUPPORTED = -1, -2
PAD_STEPS = 9  # kWidePadSteps (csrc/conv_wide.hpp): zero k-steps behind a v3 weight stream


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def _header_args(name):
    """The C types of `name`'s parameters as include/sige_hip.h declares them: 'p' pointer, 'i' int."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sige_hip.h")).read()
    decl = re.search(r"\b(int|size_t) %s\(([^;]*)\);" % name, text)
    assert decl, name
    return decl.group(1), ["p" if "*" in a else "i" for a in decl.group(2).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_bound_with_the_headers_signature(L, name):
    from sige_amd import hip

    assert hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    assert name in hip.EXPORTS
    ret, args = hip._SIGNATURES[name]
    want_ret, want = _header_args(name)
    assert ret is (ctypes.c_size_t if want_ret == "size_t" else ctypes.c_int)
    assert ["p" if a is ctypes.c_void_p else "i" for a in args] == want


@pytest.mark.parametrize("cout,cin,size", [(64, 64, None), (192, 128, None), (96, 64, 0), (64, 96, 0), (0, 64, 0), (64, -64, 0)])
def test_packed_size(L, cout, cin, size):
    """floats: [Cout / 64][4 waves][Cin / 64][9 taps] k-steps of 2 KB (2 x 64 lanes x 8 halves) + the padding; 0 off multiples of 64."""
    if size is None:
        size = ((cout // 64) * 4 * (cin // 64) * 9 + PAD_STEPS) * 2048 // 4
    assert L.sige_hip_down_tile3_packed_size(cout, cin) == size
    assert L.sige_hip_down_tile3_supported(cin, cout) == (1 if size else 0)


def test_validation_comes_before_any_pointer_is_read(L):
    run, pack = L.sige_hip_down_tile3_nhwc.fn, L.sige_hip_down_tile3_pack.fn  # (the raw ctypes functions: no device guard)
    p = 0x1000  # never dereferenced
    tail = [None, None, 0] + [None] * 6
    assert pack(None, 64, 64, p, None) == EINVAL and pack(p, 64, 64, None, None) == EINVAL
    assert pack(p, 64, 48, p, None) == EUNSUPPORTED
    assert run(3, p, 1, 64, 20, 28, p, 4, p, None, 64, 0, 0, None, 10, 14, *tail, 1, p, None) == EINVAL           # compute
    assert run(0, p, 1, 64, 20, 28, p, 4, p, None, 64, 0, 0, None, 10, 14, *tail, 1, p, None) == EUNSUPPORTED     # exact fp32
    assert run(1, p, 1, 96, 20, 28, p, 4, p, None, 64, 0, 0, None, 10, 14, *tail, 1, p, None) == EUNSUPPORTED     # C
    assert run(1, p, 1, 64, 20, 28, p, 4, p, None, 64, 0, 0, None, 10, 14, *tail, 2, p, None) == EUNSUPPORTED     # the grid is 1
    assert run(1, p, 1, 64, 20, 28, p, 0, p, None, 64, 0, 0, None, 10, 14, *tail, 1, p, None) == 0                # N == 0: OK, no launch


def test_today_is_unchanged_the_switch_is_off_and_the_tile_pack_stays_fp32():
    from sige_amd import hip
    from sige_amd.nn import Gather
    from sige_amd.nn.base import SIGEConv2d

    assert Gather.DOWNSAMPLE_TILE3 is False
    assert isinstance(hip.DOWN_TILE3_MIN_BLOCKS_F16, int) and hip.DOWN_TILE3_MIN_BLOCKS_F16 > 0
    conv = SIGEConv2d(64, 64, 3, stride=2)
    conv.compute_dtype = "f16"
    assert conv.down_tile3_packed() is None and conv._down3 is None  # CPU weights
    with pytest.raises(ValueError):
        hip.down_tile3_pack(torch.zeros(64, 64, 1, 1))


@pytest.mark.gpu
def test_conv_pack_weights_f16_for_the_stride_2_geometry_is_still_an_fp32_pack():
    from sige_amd import hip

    w = torch.randn(64, 64, 3, 3, device="cuda")
    assert hip.conv_pack_weights(w, 5, 5, (2, 2), "f16").compute == "f32"
    assert torch.equal(hip.conv_pack_weights(w, 5, 5, (2, 2), "f16"), hip.conv_pack_weights(w, 5, 5, (2, 2), "f32"))
