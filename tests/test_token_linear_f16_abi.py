"""The four C-ABI entries of the token linear on fp16 operands (include/sige_hip.h, csrc/token_linear_f16.hip): exported, bound, and
their host-side shape rules and argument validation -- nothing here touches a device."""
import ctypes

import pytest

NAMES = ("sige_hip_token_linear_packed_size_f16", "sige_hip_token_linear_supported_f16c", "sige_hip_token_linear_pack_f16",
         "sige_hip_token_linear_f16c")
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def test_the_four_symbols_are_exported_and_bound(L):
    from sige_amd import hip

    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in hip.EXPORTS and n in hip._SIGNATURES, n


@pytest.mark.parametrize("N,K,geglu,size", [(64, 64, 0, 8192), (64, 160, 0, 2 * 8192), (80, 320, 0, 2 * 3 * 8192), (320, 320, 1, 5 * 3 * 8192),
                                            (10, 64, 0, 0), (64, 48, 0, 0), (64, 16, 0, 0), (80, 64, 1, 0), (0, 64, 0, 0), (64, -32, 0, 0)])
def test_packed_size(L, N, K, geglu, size):
    """fp16 elements: 64-column blocks x 128-channel chunks x 8192; 0 for N % 16, K % 32, GEGLU with D % 32, non-positive sizes."""
    assert L.sige_hip_token_linear_packed_size_f16(N, K, geglu) == size
    if size:  # half the bytes of the fp32 pack or less (its chunks are 64 channels)
        assert size * 2 <= L.sige_hip_token_linear_packed_size(N, K, geglu) * 4


@pytest.mark.parametrize("args,want", [((2016, 960, 320, 1, 0, 3), 1), ((2016, 2560, 320, 1, 1, 1), 1), ((48, 1280, 5120, 0, 0, 1), 1),
                                       ((0, 64, 64, 0, 0, 1), 1), ((16, 64, 2080, 1, 0, 1), 0), ((16, 64, 2080, 0, 0, 1), 1),
                                       ((16, 240, 64, 0, 0, 3), 0), ((16, 192, 64, 0, 0, 3), 1), ((16, 128, 64, 0, 1, 2), 0),
                                       ((16, 64, 48, 0, 0, 1), 0), ((16, 64, 64, 0, 0, 4), 0), ((-1, 64, 64, 0, 0, 1), 0),
                                       ((2 ** 24, 64, 64, 0, 0, 1), 0)])
def test_supported(L, args, want):
    """LayerNorm needs K <= 2048; parts of whole 64-column blocks, no GEGLU with parts; K % 32; tensors below 2 GiB."""
    assert L.sige_hip_token_linear_supported_f16c(*args) == want


def test_null_pointers_are_invalid_and_no_rows_are_ok(L):
    run = L.sige_hip_token_linear_f16c.fn    # (the raw ctypes functions: no device guard)
    pack = L.sige_hip_token_linear_pack_f16.fn
    p = 0x1000  # never dereferenced: validation comes first
    assert run(None, 16, 64, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL       # x
    assert run(p, 16, 64, None, None, 0.0, None, None, 64, 0, None, 1, p, None, None, None) == EINVAL       # packed
    assert run(p, 16, 64, None, None, 0.0, p, None, 64, 0, None, 1, None, None, None, None) == EINVAL       # out0
    assert run(p, 16, 64, None, None, 0.0, p, None, 192, 0, None, 3, p, p, None, None) == EINVAL            # out2 of three parts
    assert run(p, 16, 64, p, None, 1e-5, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL            # gamma without beta
    assert run(p, -1, 64, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL
    assert run(None, 0, 64, None, None, 0.0, None, None, 64, 0, None, 1, None, None, None, None) == 0       # M == 0: OK, no launch
    assert run(p, 16, 48, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EUNSUPPORTED    # K % 32
    assert run(p, 16, 64, None, None, 0.0, p + 8, None, 64, 0, None, 1, p, None, None, None) == EUNSUPPORTED  # alignment
    assert pack(None, 64, 64, 0, p, None) == EINVAL and pack(p, 64, 64, 0, None, None) == EINVAL
    assert pack(p, 64, 48, 0, p, None) == EUNSUPPORTED and pack(p, 80, 64, 1, p, None) == EUNSUPPORTED
