"""The four token-attention units (attention_tokens / _f16, attention_wide / _f16) share their wave merge, split publish, workgroup
mapping, argument checks and launch plan (csrc/attention_rows.hpp, csrc/attention_wide_image.hpp).  Moving that code changed no
output bit: every case below equals, with torch.equal, what the library of the commit BEFORE the move gave on an MI355X for the same
CPU-drawn inputs (tests/golden/attention_one_home_parent.npz holds the outputs only; a mismatch says by how much).  The kernels are
deterministic run to run -- test_graph_replay_equals_eager_bit_for_bit relies on it.  To keep the fixture small an "f16" output is
stored as the int32 difference of its bit patterns from the "f32" output of the same case (small numbers, which compress; lossless).

The recorder is this module's __main__: `SIGE_HIP_LIB=<the parent commit's libsige_hip.so> python tests/test_gpu_attention_one_home.py [DIR]`
on the GPU writes the fixture anew (into DIR, by default tests/golden)."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402

DEV = "cuda"
NAME = "attention_one_home_parent"

# (B, Nq, Nk, heads, d, strided): the smallest shapes that reach each shared piece of the wide pair
WIDE = [
    (1, 16, 5, 1, 512, False),    # fewer key blocks than waves (merge weight 0), tail keys, one split
    (1, 16, 16, 1, 176, False),   # G = 3, a 16-channel unit past d, the c < d store guards
    (2, 32, 256, 1, 512, False),  # a split with <= 4 slices
    (1, 16, 784, 1, 192, False),  # 10 fp32 / 5 f16 splits: the clamped tail of the four-in-flight loop; tail keys
    (1, 64, 64, 2, 256, False),   # heads as strides
    (1, 32, 96, 1, 512, True),    # k | v the halves of one [B,Nk,2C] tensor, q a column slice of a wider matrix
]
# (B, Nq, Nk, heads, d): d = 40 a padded unit and VC = 1, 64 VC = 4, 160 VC = 2; B * heads = 8 the XCD dealing, 2 the plain mapping
TOKENS = [(1, 32, 77, 8, 40), (2, 32, 5, 1, 40), (1, 32, 77, 2, 64), (2, 32, 5, 1, 160)]
# two edits: (E, h, W, heads, d, tile origins in the tall image) -- a tile in each image
WIDE_TILES = (2, 4, 4, 1, 192, [(0, 0), (4, 0)])
TOKENS_TILES = (2, 8, 8, 4, 40, [(4, 4), (8, 0), (12, 4)])
COMPUTES = ("f32", "f16")


def _batched(B, Nq, Nk, heads, d, strided=False):
    g = torch.Generator().manual_seed(7 * Nq + 3 * Nk + d + heads)
    C = heads * d
    if strided:
        kv = torch.randn(B, Nk, 2 * C, generator=g).to(DEV)
        wide = torch.randn(B, Nq, C + 64, generator=g).to(DEV)
        wide[:, :, :C] *= 2.0
        return wide[:, :, :C], kv[:, :, :C], kv[:, :, C:]
    q, k, v = (torch.randn(B, n, C, generator=g).to(DEV) for n in (Nq, Nk, Nk))
    return q * 2.0, k, v


def _stacked(E, h, W, heads, d, tiles):
    g = torch.Generator().manual_seed(100 * E + 10 * h + d)
    C, N = heads * d, h * W
    q = (torch.randn(1, 16 * len(tiles), C, generator=g) * 2.0).to(DEV)
    k = torch.randn(1, E * N, C, generator=g).to(DEV)
    v = (torch.randn(E, N, C, generator=g) + 10.0 * torch.arange(E, dtype=torch.float32).reshape(E, 1, 1)).reshape(1, E * N, C).to(DEV)
    return q, k, v, torch.tensor(tiles, dtype=torch.int32, device=DEV)


def _run_stacked(hip, fn, case, compute):
    E, h, W, heads, d, tiles = case
    q, k, v, idx = _stacked(*case)
    prev = hip.get_edit_batch()
    hip.set_edit_batch(E)
    try:
        return fn(q, k, v, heads, d ** -0.5, compute=compute, tiles=(idx, E * h, W))
    finally:
        hip.set_edit_batch(prev)


def _cases(hip):
    """{key: thunk -> output tensor}"""
    out = {}
    for compute in COMPUTES:
        for c in WIDE:
            out["wide/%s/%s" % (compute, "-".join(map(str, c[:5])))] = (
                lambda c=c, compute=compute: hip.attention_wide(*_batched(*c), c[3], c[4] ** -0.5, compute=compute))
        for c in TOKENS:
            out["tokens/%s/%s" % (compute, "-".join(map(str, c)))] = (
                lambda c=c, compute=compute: hip.attention_tokens(*_batched(*c), c[3], c[4] ** -0.5, compute=compute))
        out["wide_tiles/%s" % compute] = lambda compute=compute: _run_stacked(hip, hip.attention_wide, WIDE_TILES, compute)
        out["tokens_tiles/%s" % compute] = lambda compute=compute: _run_stacked(hip, hip.attention_tokens, TOKENS_TILES, compute)
    return out


def _recorded(rec, key):
    if "/f16" not in key:
        return rec[key]
    return (rec[key.replace("/f16", "/f32")].view(np.int32) + rec[key]).view(np.float32)


def _keys():
    class _Names:  # (the keys need no library)
        attention_wide = attention_tokens = None

    return list(_cases(_Names))


@pytest.mark.gpu
@pytest.mark.parametrize("key", _keys())
def test_outputs_keep_the_bits_of_the_commit_before(key):
    from sige_amd import hip

    got = _cases(hip)[key]()
    assert got is not None, "unsupported"
    torch.cuda.synchronize()
    util.assert_finite(got, key)
    want = torch.from_numpy(_recorded(util.golden(NAME), key))
    diff = (got.cpu() - want).abs().max().item()
    assert torch.equal(got.cpu(), want), (key, "max |now - recorded| = %.3e" % diff)


if __name__ == "__main__":
    from sige_amd import hip as _hip

    rec = {}
    for _key, _thunk in _cases(_hip).items():
        _t = _thunk()
        assert _t is not None, _key
        torch.cuda.synchronize()
        rec[_key] = _t.contiguous().cpu().numpy()
        print(_key, rec[_key].shape)
    for _key in [_k for _k in rec if "/f16" in _k]:
        _f16 = rec[_key].copy()
        rec[_key] = _f16.view(np.int32) - rec[_key.replace("/f16", "/f32")].view(np.int32)
        assert np.array_equal(_recorded(rec, _key).view(np.int32), _f16.view(np.int32))
    _dst = sys.argv[1] if len(sys.argv) > 1 else util.GOLDEN  # (a directory)
    np.savez_compressed(os.path.join(_dst, NAME + ".npz"), **rec)
    print("library %s -> %s" % (os.environ.get("SIGE_HIP_LIB", "(the tree's)"), os.path.join(_dst, NAME + ".npz")))
