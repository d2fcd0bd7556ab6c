"""The fp16-stored K / V forms (csrc/attention_tokens_f16kv.hip, csrc/attention_wide_f16kv.hip) through the move of the token
trio's merge, launcher and entry checks into csrc/attention_tokens_image.hpp and of the fp16-operand kernels' shared pieces into
csrc/attention_rows.hpp: every case below equals, with torch.equal, what the library of the commit BEFORE the move gave on an MI355X
for the same CPU-drawn inputs, K / V handed over as .half().  tests/test_gpu_attention_one_home.py does this for the f32 / f16
forms; its fixture has no f16kv outputs, this one (tests/golden/attention_kv16_one_home_parent.npz) holds only those.  To keep the
file small an output is stored as the int32 difference of its bit patterns from the "f16" output of the same case in that module's
fixture (the same arithmetic on the same inputs but for the one rounding of k, v: small numbers, which compress; lossless); the one
case that module does not have is stored as it is.

The recorder is this module's __main__: `SIGE_HIP_LIB=<the parent commit's libsige_hip.so> python tests/test_gpu_attention_kv16_one_home.py [DIR]`
on the GPU writes the fixture anew (into DIR, by default tests/golden)."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import test_gpu_attention_one_home as H  # noqa: E402
from tests import util  # noqa: E402

NAME = "attention_kv16_one_home_parent"

# (B, Nq, Nk, heads, d): that module's four -- the XCD dealing, a dead 8-channel lane, groups 2 + 1 and a tail step; fewer steps than
# waves (merge weight 0); one group of four; groups 4 + 4 + 2 -- and U = 5, an instance only this unit has
TOKENS = H.TOKENS + [(1, 16, 33, 1, 72)]


def _halves(c):
    """q, k16, v16 of a batched case; strided: k16 | v16 are the halves of ONE [B,Nk,2C] fp16 tensor (row stride 2C, a multiple of 8)"""
    q, k, v = H._batched(*c)
    if len(c) > 5 and c[5]:
        kv = torch.cat([k, v], dim=2).half()
        return q, kv[:, :, :k.shape[2]], kv[:, :, k.shape[2]:]
    return q, k.half(), v.half()


def _run_stacked(hip, fn, case, **kw):
    E, h, W, heads, d, tiles = case
    q, k, v, idx = H._stacked(*case)
    prev = hip.get_edit_batch()
    hip.set_edit_batch(E)
    try:
        return fn(q, k.half(), v.half(), heads, d ** -0.5, tiles=(idx, E * h, W), **kw)
    finally:
        hip.set_edit_batch(prev)


def _cases(hip):
    """{key: thunk -> output tensor}; a key is that module's "f16" key with f16kv in its place"""
    out = {}
    for c in H.WIDE:
        out["wide/f16kv/%s" % "-".join(map(str, c[:5]))] = lambda c=c: hip.attention_wide(*_halves(c), c[3], c[4] ** -0.5, compute="f16kv")
    for c in TOKENS:
        out["tokens/f16kv/%s" % "-".join(map(str, c))] = lambda c=c: hip.attention_tokens_kv16(*_halves(c), c[3], c[4] ** -0.5)
    out["wide_tiles/f16kv"] = lambda: _run_stacked(hip, hip.attention_wide, H.WIDE_TILES, compute="f16kv")
    out["tokens_tiles/f16kv"] = lambda: _run_stacked(hip, hip.attention_tokens_kv16, H.TOKENS_TILES)
    return out


def _base(key):
    """the bit patterns an output is stored against: the "f16" output of the same case, zeros where that module has none"""
    f16 = key.replace("/f16kv", "/f16")
    return H._recorded(util.golden(H.NAME), f16).view(np.int32) if f16 in util.golden(H.NAME).files else np.int32(0)


def _keys():
    class _Names:  # (the keys need no library)
        attention_wide = attention_tokens_kv16 = None

    return list(_cases(_Names))


@pytest.mark.gpu
@pytest.mark.parametrize("key", _keys())
def test_outputs_keep_the_bits_of_the_commit_before(key):
    from sige_amd import hip

    got = _cases(hip)[key]()
    assert got is not None, "unsupported"
    torch.cuda.synchronize()
    util.assert_finite(got, key)
    want = torch.from_numpy((_base(key) + util.golden(NAME)[key]).view(np.float32))
    diff = (got.cpu() - want).abs().max().item()
    assert torch.equal(got.cpu(), want), (key, "max |now - recorded| = %.3e" % diff)


if __name__ == "__main__":
    from sige_amd import hip as _hip

    rec = {}
    for _key, _thunk in _cases(_hip).items():
        _t = _thunk()
        assert _t is not None, _key
        torch.cuda.synchronize()
        _bits = _t.contiguous().cpu().numpy().view(np.int32)
        rec[_key] = _bits - _base(_key)
        assert np.array_equal(_base(_key) + rec[_key], _bits)
        print(_key, rec[_key].shape, "largest stored |difference| %d" % np.abs(rec[_key].astype(np.int64)).max())
    _dst = sys.argv[1] if len(sys.argv) > 1 else util.GOLDEN  # (a directory)
    np.savez_compressed(os.path.join(_dst, NAME + ".npz"), **rec)
    print("library %s -> %s" % (os.environ.get("SIGE_HIP_LIB", "(the tree's)"), os.path.join(_dst, NAME + ".npz")))
