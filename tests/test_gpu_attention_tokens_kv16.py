"""hip.attention_tokens_kv16 = sige_hip_attention_tokens_f16kv / _tiles_f16kv (csrc/attention_tokens_f16kv.hip) on the GPU.  K / V are
handed over as k.half(), v.half(); the truth is tests.attention_stress.chain(..., float64) on the inputs AS GIVEN, the allowance
tests.attention_f16.bound16 with `emulate`'s error -- the rule of tests/test_gpu_attention_f16.py.  Every output is NaN before the
launch."""
import pytest
import torch

from tests import attention_f16 as F
from tests import attention_stress as A
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, Nq, Nk, heads, d); d = 48: a 32-channel unit half live beside d = 40's quarter-live one
SHAPES = [(1, 16, 17, 1, 40), (1, 16, 33, 2, 80), (2, 32, 77, 8, 40), (1, 16, 64, 1, 160), (1, 32, 96, 2, 48)]


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _run(hip, q, k, v, heads, scale, tiles=None):
    with util.poisoned() as p:
        got = hip.attention_tokens_kv16(q.to(DEV), k.to(DEV).half(), v.to(DEV).half(), heads, scale, tiles=tiles)
    assert p.n > 0 and got is not None and tuple(got.shape) == tuple(q.shape)
    return got.double().cpu()


def _judge(what, got, want, e16, tol):
    util.assert_finite(got, "attention_tokens_kv16 %s" % what)
    err = float((got - want).abs().max())
    print("attention_tokens_kv16 %s: err %.3e, emulation %.3e, bound %.3e, err / bound %.3f" % (what, err, e16, tol, err / tol))
    util.record_margin("test_gpu_attention_tokens_kv16", what, err, tol)
    assert err <= tol, "%s: max |diff| %.3e > bound %.3e (emulation %.3e)" % (what, err, tol, e16)


@pytest.mark.parametrize("shape", SHAPES + ["dust"], ids=lambda s: s if s == "dust" else "B%d_Nq%d_Nk%d_h%d_d%d" % s)
def test_against_fp64(hip, shape):
    """Unrounded randn inputs (their rounding is part of what is judged); `dust`: fp16-subnormal probabilities carry 3.4 % of the mass."""
    heads, d = (1, 40) if shape == "dust" else shape[3:]
    q, k, v, want, e16, tol = F.dust_case() if shape == "dust" else F.randn_case(*shape)
    _judge(str(shape), _run(hip, q, k, v, heads, d ** -0.5), want, e16, tol)


@pytest.mark.parametrize("head", [0, 1])
def test_infinities_in_the_neighbouring_head_do_not_reach_a_head(hip, head):
    """d = 40: the lanes of the second 32-channel unit past channel 39 would read the NEXT head's channels (head 0) or the next key
    row's first head (head 1, the last): that head's K holds +-Inf, and 0 x Inf is NaN -- unless those lanes load exact zeros."""
    shape = (1, 16, 33, 1, 40)
    q, k, v, want, e16, tol = F.randn_case(*shape)
    other = torch.full_like(k, float("inf"))
    other[:, ::2] = -float("inf")
    cat = (lambda mine, fill: torch.cat([mine, fill], dim=2)) if head == 0 else (lambda mine, fill: torch.cat([fill, mine], dim=2))
    got = _run(hip, cat(q, torch.zeros_like(q)), cat(k, other), cat(v, torch.zeros_like(v)), 2, 40 ** -0.5)
    _judge("Inf beside head %d" % head, got[:, :, 40 * head:40 * head + 40], want, e16, tol)


def test_tiles_attend_to_their_own_image(hip):
    """Stacked edits, E = 2 images of 8 x 8 tokens, three tiles over both: every tile against the fp64 attention over ITS image's 64
    keys, with the OTHER image's K / V all NaN (one launch per image judged; the other image's tiles are then NaN and not looked at)."""
    E, h, W, heads, d = 2, 8, 8, 2, 40
    N, C, rows = h * W, heads * d, [4, 8, 12]  # origin rows in the tall image: image 0, image 1, image 1
    g = torch.Generator().manual_seed(816)
    q, k, v = torch.randn(1, 48, C, generator=g) * 2.0, torch.randn(1, E * N, C, generator=g), torch.randn(1, E * N, C, generator=g)
    idx = torch.tensor([(r, 4 * (i % 2)) for i, r in enumerate(rows)], dtype=torch.int32, device=DEV)
    prev = hip.get_edit_batch()
    hip.set_edit_batch(E)
    try:
        for e in range(E):
            sel = torch.cat([torch.arange(16 * t, 16 * t + 16) for t, r in enumerate(rows) if r // h == e])
            ks, vs = k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N]
            want = A.chain(q[:, sel], ks, vs, heads, d ** -0.5, torch.float64)
            e16 = float((F.emulate(q[:, sel], ks, vs, heads, d ** -0.5).double() - want).abs().max())
            kn, vn = torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))
            kn[:, e * N:(e + 1) * N], vn[:, e * N:(e + 1) * N] = ks, vs
            got = _run(hip, q, kn, vn, heads, d ** -0.5, tiles=(idx, E * h, W))
            _judge("tiles, image %d" % e, got[:, sel], want, e16, F.bound16(want, e16))
    finally:
        hip.set_edit_batch(prev)
