"""The C-ABI entries of the fp16-stored K / V path (include/sige_hip.h; csrc/attention_tokens_f16kv.hip, csrc/kv_rows_f16.hip): exported,
bound with the header's signatures, their status rules without a launch, the wrappers' ValueErrors -- and the switch is off.
Nothing here touches a device."""
import ctypes
import os
import re

import pytest
import torch

NAMES = ("sige_hip_attention_tokens_f16kv_supported", "sige_hip_attention_tokens_f16kv", "sige_hip_attention_tokens_tiles_f16kv",
         "sige_hip_kv_rows_store_f16")
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_bound_with_the_headers_signature(L, name):
    from sige_amd import hip

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sige_hip.h")).read()
    want = ["p" if "*" in a else "f" if "float" in a else "i" for a in re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1).split(",")]
    ret, args = hip._SIGNATURES[name]
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), name) and name in hip.EXPORTS and ret is ctypes.c_int
    assert ["p" if a is ctypes.c_void_p else "f" if a is ctypes.c_float else "i" for a in args] == want


@pytest.mark.parametrize("Nq,Nk,C,heads,ok", [(16, 17, 40, 1, 1), (32, 77, 320, 8, 1), (16, 64, 160, 1, 1), (16, 16, 44, 1, 0),
                                              (16, 16, 168, 1, 0), (8, 16, 64, 1, 0)])
def test_supported_is_the_token_predicate_and_a_head_of_whole_16_byte_loads(L, Nq, Nk, C, heads, ok):
    assert L.sige_hip_attention_tokens_f16kv_supported(Nq, Nk, C, heads) == ok <= L.sige_hip_attention_tokens_supported(Nq, Nk, C, heads)


def test_status_rules_are_the_f16c_entries_and_come_before_any_pointer_is_read(L):
    run, f16c = L.sige_hip_attention_tokens_f16kv.fn, L.sige_hip_attention_tokens_f16c.fn  # (the raw ctypes functions: no device guard)
    tiles, store = L.sige_hip_attention_tokens_tiles_f16kv.fn, L.sige_hip_kv_rows_store_f16.fn
    p = 0x1000  # never dereferenced
    for a in ((None, None, None, 0, 16, 16, 64, 1, 1.0, None, None), (None, p, p, 1, 16, 16, 64, 1, 1.0, p, None),
              (p, p, p, 1, 16, 0, 64, 1, 1.0, p, None), (p, p, p, 1, 16, 16, 164, 1, 1.0, p, None), (p, p + 8, p, 1, 16, 16, 64, 1, 1.0, p, None),
              (p, p, p, 1, 8, 16, 64, 1, 1.0, p, None)):
        assert run(*a) == f16c(*a)
    assert run(p, p, p, 1, 16, 16, 44, 1, 1.0, p, None) == EUNSUPPORTED       # d % 8
    assert run(p, p, p, 1, 16, 2 ** 24, 64, 1, 1.0, p, None) == EUNSUPPORTED  # one batch's K: 2 GiB of halves
    assert tiles(p, p, p, p, -1, 8, 8, 64, 1, 1.0, p, None) == EINVAL
    assert tiles(None, None, None, None, 0, 8, 8, 64, 1, 1.0, None, None) == OK
    assert tiles(p, p, p, None, 2, 8, 8, 64, 1, 1.0, p, None) == EINVAL
    assert tiles(p, p, p, p, 2, 8, 8, 44, 1, 1.0, p, None) == EUNSUPPORTED
    assert store(p, p, p, p, p, -1, 1, 8, 8, 64, None) == EINVAL
    assert store(None, None, None, None, None, 0, 1, 8, 8, 64, None) == OK    # T = 0: nothing launched
    assert store(p, None, p, p, p, 2, 1, 8, 8, 64, None) == EINVAL
    assert store(p, p, p, p, p, 2, 1, 8, 8, 68, None) == EUNSUPPORTED         # C % 8
    assert store(p, p, p + 8, p, p, 2, 1, 8, 8, 64, None) == EUNSUPPORTED


def test_wrappers_refuse_wrong_dtypes():
    from sige_amd import hip

    q, k16, idx = torch.zeros(1, 16, 40), torch.zeros(1, 16, 40, dtype=torch.float16), torch.zeros(1, 2, dtype=torch.int32)
    assert hip.attention_tokens_kv16(q, k16, k16, 1, 1.0) is None  # (CPU tensors: where attention_tokens returns None)
    for bad in ((q, q, k16), (q, k16, q), (k16, k16, k16)):
        with pytest.raises(ValueError):
            hip.attention_tokens_kv16(*bad, 1, 1.0)
    for bad in ((k16, q, k16, k16, idx), (q, q, q, k16, idx), (q, q, k16, k16, idx.long()), (q[:, :8], q, k16, k16, idx)):
        with pytest.raises(ValueError):
            hip.kv_rows_store_f16(*bad, 4, 4)
