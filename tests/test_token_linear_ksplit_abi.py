"""The three C-ABI entries of the token linear's in-launch K split (include/sige_hip.h, csrc/token_linear.hip, token_linear_f16.hip):
exported and bound with the header's signatures, and the split rule's host arithmetic -- nothing here touches a device."""
import ctypes

import pytest

NAMES = ("sige_hip_token_linear_ksplit", "sige_hip_token_linear_split_f32", "sige_hip_token_linear_split_f16c")


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def test_the_three_symbols_have_the_headers_signatures(L):
    """(tests/test_c_abi.py holds hip.EXPORTS to the header's declarations.)  The launching entries: their unsplit siblings' arguments
    with `int ksplit` in front of the stream."""
    from sige_amd import hip

    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in hip.EXPORTS, n
    assert hip._SIGNATURES[NAMES[0]] == (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 6)
    for split, base in ((NAMES[1], "sige_hip_token_linear_f32"), (NAMES[2], "sige_hip_token_linear_f16c")):
        ret, args = hip._SIGNATURES[base]
        assert hip._SIGNATURES[split] == (ret, args[:-1] + [ctypes.c_int, ctypes.c_void_p]), split


@pytest.mark.parametrize("f16", [0, 1])
def test_rule_is_zero_where_unsupported_and_one_on_the_64_token_form(L, f16):
    q = L.sige_hip_token_linear_ksplit
    assert q(16, 10, 64, 0, 0, 1, f16) == 0          # N % 16
    assert q(16, 64, 2080, 1, 0, 1, f16) == 0        # LayerNorm beyond K = 2048
    assert q(16, 240, 64, 0, 0, 3, f16) == 0         # 3 parts of 80 columns
    assert q(-1, 64, 64, 0, 0, 1, f16) == 0
    assert q(16, 64, 48, 0, 0, 1, 1) == 0            # K % 32 on fp16 operands
    assert q(0, 64, 5120, 0, 0, 1, f16) == 1         # no rows, no launch
    assert q(2016, 1024, 5120, 0, 0, 1, f16) == 1    # 32 x 16 = 512 blocks of 64 rows: the 64-token form
    assert q(2016, 320, 5120, 0, 0, 1, f16) == 1     # 126 x 5 16-token workgroups: the chip is full
    assert q(128, 1280, 1280, 0, 0, 1, f16) == 1     # K too shallow for the finish to pay back
    assert q(128, 1280, 5120, 0, 0, 1, f16) == 4     # the few-row second feed-forward layer: 160 workgroups, 80 | 40 chunks


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("K", [64, 320, 336, 1312, 2048, 5120, 5152])
@pytest.mark.parametrize("N", [80, 1280])
@pytest.mark.parametrize("M", [16, 128, 288])
def test_rule_never_leaves_a_split_empty(L, M, N, K, f16):
    """Split s walks chunks [s cps, (s + 1) cps) with cps = ceil(nchunks / ksplit): the last one starts inside K.  And the rule's own
    terms: 1 | 2 | 4 | 8, only below 384 workgroups of the 16-token form, at most 1280 after the split, every split
    1280 channels or more."""
    ks = L.sige_hip_token_linear_ksplit(M, N, K, 0, 0, 1, f16)
    if f16 and K % 32:
        assert ks == 0
        return
    nchunks = -(-K // (128 if f16 else 64))
    grid = -(-M // 16) * -(-N // 64)
    assert ks in (1, 2, 4, 8)
    assert (ks - 1) * -(-nchunks // ks) < nchunks
    assert ks == 1 or (grid < 384 and grid * ks <= 1280 and nchunks - (ks - 1) * -(-nchunks // ks) >= (10 if f16 else 20))
