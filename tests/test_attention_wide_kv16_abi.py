"""The C-ABI entries of the wide-head attention on fp16-stored K / V (include/sige_hip.h; csrc/attention_wide_f16kv.hip, the second
entry of csrc/kv_rows_f16.hip): exported and bound, the _f16kv signatures those of the _f16c entries, their status rules without a
launch.  Nothing here touches a device."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def test_names_signatures_and_status_rules():
    from sige_amd import build, hip

    build.build(verbose=False)
    L, S = hip.lib(), hip._SIGNATURES
    for name in ("sige_hip_attention_wide_f16kv_supported", "sige_hip_attention_wide_f16kv", "sige_hip_attention_wide_tiles_f16kv",
                 "sige_hip_kv_tiles_store_f16"):
        assert name in hip.EXPORTS and hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    for tail in ("wide_f16", "wide_tiles_f16"):
        assert S["sige_hip_attention_%skv" % tail] == S["sige_hip_attention_%sc" % tail]
    run, tiles, store = L.sige_hip_attention_wide_f16kv.fn, L.sige_hip_attention_wide_tiles_f16kv.fn, L.sige_hip_kv_tiles_store_f16.fn
    p, C = 0x1000, 192  # (never dereferenced)
    args = lambda q=p, k=p, ldk=C, v=p, ldv=C: (q, C, k, ldk, v, ldv, 1, 16, 16, C, 1, 1.0, p, C, None)  # noqa: E731
    assert run(*args(q=None)) == EINVAL and run(*args(ldk=C - 8)) == EINVAL
    assert run(*args(k=p + 8)) == EUNSUPPORTED and run(*args(ldv=C + 4)) == EUNSUPPORTED  # pointer % 16, stride % 8 halves
    assert run(p, 128, p, 128, p, 128, 1, 16, 16, 128, 1, 1.0, p, 128, None) == EUNSUPPORTED  # d <= 160
    assert L.sige_hip_attention_wide_f16kv_supported(16, 16, C, 1) == 1 and L.sige_hip_attention_wide_f16kv_supported(16, 16, 128, 1) == 0
    assert tiles(p, C, p, C, p, C, None, 0, 8, 8, C, 1, 1.0, p, C, None) == OK  # T = 0: nothing launched
    assert tiles(p, C, p, C, p, C, None, 2, 8, 8, C, 1, 1.0, p, C, None) == EINVAL
    assert tiles(p, C, p, C + 4, p, C, p, 2, 8, 8, C, 1, 1.0, p, C, None) == EUNSUPPORTED
    assert store(p, p, p, -1, 8, 8, 64, None) == EINVAL and store(p, None, p, 2, 8, 8, 64, None) == EINVAL
    assert store(None, None, None, 0, 8, 8, 64, None) == OK
    assert store(p, p, p, 2, 8, 8, 68, None) == EUNSUPPORTED and store(p, p + 8, p, 2, 8, 8, 64, None) == EUNSUPPORTED


def test_wrappers_refuse_wrong_dtypes():
    from sige_amd import hip

    q, k16 = torch.zeros(1, 16, 192), torch.zeros(1, 16, 192, dtype=torch.float16)
    assert hip.attention_wide(q, k16, k16, 1, 1.0, compute="f16kv") is None  # (CPU tensors: where the other forms return None)
    assert hip.attention_wide(q, k16, k16, 1, 1.0, compute="f16") is None    # (as before: nothing is converted, nothing raised)
    img = torch.zeros(1, 8, 4, 4).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        hip.attention_wide(q, q, k16, 1, 1.0, compute="f16kv")
    with pytest.raises(ValueError):
        hip.kv_tiles_store_f16(img, img, torch.zeros(1, 2, dtype=torch.int32))
