"""The token linear's four C-ABI entries (include/sige_hip.h, csrc/token_linear.hip): exported, bound, and their host-side shape rules
and argument validation -- nothing here touches a device."""
import ctypes

import pytest

NAMES = ("sige_hip_token_linear_packed_size", "sige_hip_token_linear_supported", "sige_hip_token_linear_pack", "sige_hip_token_linear_f32")
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
    assert callable(hip.token_linear) and callable(hip.token_linear_pack)


@pytest.mark.parametrize("geglu", [0, 1])
@pytest.mark.parametrize("N,K", [(64, 64), (320, 320), (960, 320), (10240, 1280)])
def test_packed_size_of_supported_shapes(L, N, K, geglu):
    size = L.sige_hip_token_linear_packed_size(N, K, geglu)
    assert size > 0
    # zero padded to whole 64-column blocks and 64-channel chunks: never smaller than the weight itself
    assert size >= N * K and size % 4096 == 0


def test_packed_size_of_unsupported_shapes(L):
    assert L.sige_hip_token_linear_packed_size(10, 64, 0) == 0      # N % 16
    assert L.sige_hip_token_linear_packed_size(64, 24, 0) == 0      # K % 16
    assert L.sige_hip_token_linear_packed_size(80, 64, 1) == 0      # GEGLU with D = 40
    assert L.sige_hip_token_linear_packed_size(80, 64, 0) > 0       # (the same N without GEGLU is fine)
    assert L.sige_hip_token_linear_packed_size(0, 64, 0) == 0 and L.sige_hip_token_linear_packed_size(64, -16, 0) == 0


def test_supported(L):
    assert L.sige_hip_token_linear_supported(2016, 960, 320, 1, 0, 3) == 1
    assert L.sige_hip_token_linear_supported(2016, 2560, 320, 1, 1, 1) == 1
    assert L.sige_hip_token_linear_supported(48, 1280, 5120, 0, 0, 1) == 1
    assert L.sige_hip_token_linear_supported(0, 64, 64, 0, 0, 1) == 1
    assert L.sige_hip_token_linear_supported(16, 64, 2064, 1, 0, 1) == 0    # LayerNorm beyond K = 2048
    assert L.sige_hip_token_linear_supported(16, 64, 2064, 0, 0, 1) == 1    # (without it the depth is fine)
    assert L.sige_hip_token_linear_supported(16, 240, 64, 0, 0, 3) == 0     # 3 parts of 80 columns: not whole 64-column blocks
    assert L.sige_hip_token_linear_supported(16, 192, 64, 0, 0, 3) == 1
    assert L.sige_hip_token_linear_supported(16, 128, 64, 0, 1, 2) == 0     # GEGLU has one output
    assert L.sige_hip_token_linear_supported(16, 64, 64, 0, 0, 4) == 0 and L.sige_hip_token_linear_supported(16, 64, 64, 0, 0, 0) == 0
    assert L.sige_hip_token_linear_supported(-1, 64, 64, 0, 0, 1) == 0
    assert L.sige_hip_token_linear_supported(2 ** 24, 64, 64, 0, 0, 1) == 0  # x beyond 2 GiB: 32-bit offsets


def test_null_pointers_are_invalid_and_no_rows_are_ok(L):
    run = L.sige_hip_token_linear_f32.fn    # (the raw ctypes functions: no device guard)
    pack = L.sige_hip_token_linear_pack.fn
    p = 0x1000  # never dereferenced: validation comes first
    assert run(None, 16, 64, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL       # x
    assert run(p, 16, 64, None, None, 0.0, None, None, 64, 0, None, 1, p, None, None, None) == EINVAL       # packed
    assert run(p, 16, 64, None, None, 0.0, p, None, 64, 0, None, 1, None, None, None, None) == EINVAL       # out0
    assert run(p, 16, 64, None, None, 0.0, p, None, 192, 0, None, 3, p, p, None, None) == EINVAL            # out2 of three parts
    assert run(p, 16, 64, p, None, 1e-5, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL            # gamma without beta
    assert run(p, -1, 64, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL
    assert run(p, 16, 0, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EINVAL
    assert run(p, 16, 64, None, None, 0.0, p, None, 64, 0, None, 4, p, None, None, None) == EINVAL
    # M == 0: OK without a launch, whatever the pointers
    assert run(None, 0, 64, None, None, 0.0, None, None, 64, 0, None, 1, None, None, None, None) == 0
    # shapes the kernel does not take
    assert run(p, 16, 24, None, None, 0.0, p, None, 64, 0, None, 1, p, None, None, None) == EUNSUPPORTED
    assert run(p, 16, 64, None, None, 0.0, p, None, 10, 0, None, 1, p, None, None, None) == EUNSUPPORTED
    assert run(p, 16, 2064, p, p, 1e-5, p, None, 64, 0, None, 1, p, None, None, None) == EUNSUPPORTED
    assert run(p, 16, 64, None, None, 0.0, p, None, 80, 1, None, 1, p, None, None, None) == EUNSUPPORTED
    assert pack(None, 64, 64, 0, p, None) == EINVAL and pack(p, 64, 64, 0, None, None) == EINVAL
    assert pack(p, 64, 24, 0, p, None) == EUNSUPPORTED and pack(p, 80, 64, 1, p, None) == EUNSUPPORTED


def test_version_is_unchanged(L):
    """(by the token linear entry points, which were added without an ABI bump: the number is the library's current one)"""
    assert L.sige_hip_version() == 310
