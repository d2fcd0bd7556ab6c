"""hip.attention_wide(..., compute="f16kv") (csrc/attention_wide_f16kv.hip) on the GPU, K / V handed over as .half(): truth, allowance
and poisoned outputs as in tests/test_gpu_attention_tokens_kv16.py (fp64 chain on the inputs as given; tests.attention_f16.bound16)."""
import pytest
import torch

from tests import attention_f16 as F
from tests import attention_stress as A
from tests import attention_wide_f16 as WF
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _run(hip, q, k, v, heads, scale, tiles=None, fused=False):
    """`fused`: K and V as the two column halves of ONE fp16 [B,Nk,2C] tensor, read in place."""
    k16, v16 = k.to(DEV).half(), v.to(DEV).half()
    if fused:
        C = k.shape[2]
        kv = torch.cat([k16, v16], dim=2)
        k16, v16 = kv[:, :, :C], kv[:, :, C:]
    with util.poisoned() as p:
        got = hip.attention_wide(q.to(DEV), k16, v16, heads, scale, tiles=tiles, compute="f16kv")
    assert p.n > 0 and got is not None and tuple(got.shape) == tuple(q.shape)
    return got.double().cpu()


def _judge(what, got, want, e16, tol):
    util.assert_finite(got, "attention_wide f16kv %s" % what)
    err = float((got - want).abs().max())
    print("attention_wide f16kv %s: err %.3e, emulation %.3e, bound %.3e, err / bound %.3f" % (what, err, e16, tol, err / tol))
    util.record_margin("test_gpu_attention_wide_kv16", what, err, tol)
    assert err <= tol, "%s: max |diff| %.3e > bound %.3e (emulation %.3e)" % (what, err, tol, e16)


FUSED = [(1, 16, 40, 1, 176), (1, 16, 33, 1, 512)]  # at d = 176 the 16 channels past a K row's head are V's first channels


@pytest.mark.parametrize("shape,fused", [(s, False) for s in WF.WIDE_F16_SHAPES + ["dust"]] + [(s, True) for s in FUSED],
                         ids=lambda s: s if isinstance(s, str) else ("fused" if s else "apart") if isinstance(s, bool) else WF.shape_id(s))
def test_against_fp64(hip, shape, fused):
    """Unrounded randn inputs (their rounding is part of what is judged); `dust`: fp16-subnormal probabilities carry 3.4 % of the mass;
    WF.SPLIT_SHAPE: the shared launch plan gives two workgroups per query tile."""
    heads, d = (1, WF.DUST_D) if shape == "dust" else shape[3:]
    if shape == WF.SPLIT_SHAPE:
        splits = getattr(hip.lib().sige_hip_attention_wide_f16c_splits, "fn", hip.lib().sige_hip_attention_wide_f16c_splits)
        assert splits(*shape[:3], heads * d, heads) == 2
    q, k, v, want, e16, tol = WF.dust_case() if shape == "dust" else F.randn_case(*shape)
    _judge("%s%s" % (shape, " fused K | V" if fused else ""), _run(hip, q, k, v, heads, d ** -0.5, fused=fused), want, e16, tol)


@pytest.mark.parametrize("head", [0, 1])
def test_infinities_in_the_neighbouring_head_do_not_reach_a_head(hip, head):
    """d = 176: the last unit's upper half lies in the next head (or key row), whose K is +-Inf: NaN unless those lanes load zeros."""
    d = 176
    q, k, v, want, e16, tol = F.randn_case(1, 16, 33, 1, d)
    other = torch.full_like(k, float("inf"))
    other[:, ::2] = -float("inf")
    cat = (lambda mine, fill: torch.cat([mine, fill], dim=2)) if head == 0 else (lambda mine, fill: torch.cat([fill, mine], dim=2))
    got = _run(hip, cat(q, torch.zeros_like(q)), cat(k, other), cat(v, torch.zeros_like(v)), 2, d ** -0.5)
    _judge("Inf beside head %d" % head, got[:, :, d * head:d * head + d], want, e16, tol)


def test_tiles_attend_to_their_own_image(hip):
    """E = 2 images of 8 x 8 tokens, three tiles over both: every tile against fp64 over ITS image's keys, the OTHER image all NaN."""
    E, h, W, d = 2, 8, 8, 192
    N, rows = h * W, [4, 8, 12]  # origin rows in the tall image: image 0, image 1, image 1
    g = torch.Generator().manual_seed(834)
    q, k, v = torch.randn(1, 48, d, generator=g) * 2.0, torch.randn(1, E * N, d, generator=g), torch.randn(1, E * N, d, generator=g)
    idx = torch.tensor([(r, 4 * (i % 2)) for i, r in enumerate(rows)], dtype=torch.int32, device=DEV)
    prev = hip.get_edit_batch()
    hip.set_edit_batch(E)
    try:
        for e in range(E):
            sel = torch.cat([torch.arange(16 * t, 16 * t + 16) for t, r in enumerate(rows) if r // h == e])
            ks, vs = k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N]
            want = A.chain(q[:, sel], ks, vs, 1, d ** -0.5, torch.float64)
            e16 = float((F.emulate(q[:, sel], ks, vs, 1, d ** -0.5).double() - want).abs().max())
            kn, vn = torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))
            kn[:, e * N:(e + 1) * N], vn[:, e * N:(e + 1) * N] = ks, vs
            got = _run(hip, q, kn, vn, 1, d ** -0.5, tiles=(idx, E * h, W))
            _judge("tiles, image %d" % e, got[:, sel], want, e16, F.bound16(want, e16))
    finally:
        hip.set_edit_batch(prev)
