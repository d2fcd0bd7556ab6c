"""The reference side of the fp16-operand token attention's tests (tests/attention_f16.py), the binding's argument checks and the
entry point's status rules -- nothing here touches a device.

Measured with these inputs: the clean emulation's error against the fp64 truth is at most 4.5e-4 over F16_SHAPES x every regime (each case's
bound is 4 x its own e16, floor 2e-5 (1 + max|want|)); its worst f16_check ratio on unrounded randn inputs is 0.047; every mutant ends
non-finite or at >= 3.7e4 x the bound at (2, 48, 100, 2, 40); `dust`: max|want| 4.5, clean error 1.3e-3, bound 5.4e-3, error with the
subnormal probabilities flushed 0.83 (the quarter of the keys that shares a wave with the heavy key)."""
import ctypes

import pytest
import torch

from sige_amd.tolerance import f16_check
from tests import attention_f16 as F
from tests import attention_stress as A

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _cases():
    return [pytest.param(s, r, j, id="B%d_Nq%d_Nk%d_h%d_d%d-%s" % (s + (A.regime_id(r, j),))) for s in F.F16_SHAPES for r, j in A.regimes_for(s[2])]


@pytest.mark.parametrize("shape,regime,spike", _cases())
def test_clean_emulation_is_finite_and_inside_both_criteria(shape, regime, spike):
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.case(B, Nq, Nk, heads, d, regime, spike)
    assert torch.equal(F.r16(q), q) and torch.equal(F.r16(k), k) and torch.equal(F.r16(v), v)  # (the inputs ARE fp16 values)
    got = F.emulate(q, k, v, heads, d ** -0.5)
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - want).abs().max())
    print("%s %s: e16 %.3e, bound %.3e, max|want| %.3g" % (shape, A.regime_id(regime, spike), e16, tol, float(want.abs().max())))
    assert err == e16 and err <= tol
    chk = f16_check(got, want)
    assert chk["ok"], chk


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_mutant_shows_in_some_regime(mutant):
    shape = (2, 48, 100, 2, 40)
    B, Nq, Nk, heads, d = shape
    worst = 0.0
    for regime, spike in A.regimes_for(Nk):
        q, k, v, want, e16, tol = F.case(B, Nq, Nk, heads, d, regime, spike)
        got = F.emulate(q, k, v, heads, d ** -0.5, mutant=mutant)
        ratio = float("inf") if not bool(torch.isfinite(got).all()) else float((got.double() - want).abs().max()) / tol
        worst = max(worst, ratio)
    print("%s: worst error / bound %.3g" % (mutant, worst))
    assert worst > 1.0, "%s passes every regime (worst error / bound %.3g)" % (mutant, worst)


@pytest.mark.parametrize("shape", F.F16_SHAPES, ids=lambda s: "B%d_Nq%d_Nk%d_h%d_d%d" % s)
def test_unrounded_randn_inputs_meet_the_f16_criterion(shape):
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.randn_case(*shape)
    assert not torch.equal(F.r16(q), q)
    chk = f16_check(F.emulate(q, k, v, heads, d ** -0.5), want)
    print("%s: e16 %.3e, bound %.3e, f16_check %s" % (shape, e16, tol, chk))
    assert chk["ok"], chk


def test_dust_needs_the_subnormal_probabilities():
    q, k, v, want, e16, tol = F.dust_case()
    p = torch.softmax((q[0].double() @ k[0].double().T) * 40 ** -0.5, dim=1)
    small = p[0][p[0] < 0.5]
    assert small.numel() == 2047 and float(small.max()) < 2.0 ** -14 and 0.03 < float(small.sum()) < 0.04
    flushed = float((F.emulate(q, k, v, 1, 40 ** -0.5, flush=True).double() - want).abs().max())
    print("dust: max|want| %.3g, clean error %.3e, bound %.3e, flushed error %.3e" % (float(want.abs().max()), e16, tol, flushed))
    assert e16 <= tol
    assert flushed > tol


def test_binding_validates_compute_first_and_the_switch_is_off():
    from sige_amd import hip
    from sige_amd.workloads import sd_transformer

    q = torch.zeros(1, 16, 8)
    with pytest.raises(ValueError):
        hip.attention_tokens(q, q, q, 1, 1.0, compute="bf16")
    assert hip.attention_tokens(q, q, q, 1, 1.0, compute="f16") is None  # (CPU tensors: where the fp32 form returns None)
    assert hip.attention_tokens(q, q, q, 1, 1.0) is None
    assert sd_transformer.ATTENTION_COMPUTE == "f32"
    assert "sige_hip_attention_tokens_f16c" in hip._SIGNATURES
    assert hip._SIGNATURES["sige_hip_attention_tokens_f16c"] == hip._SIGNATURES["sige_hip_attention_tokens_f32"]


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def test_entry_status_rules_without_a_launch(L):
    from sige_amd import hip

    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "sige_hip_attention_tokens_f16c")
    run = L.sige_hip_attention_tokens_f16c.fn  # (the raw ctypes function: no device guard)
    p = 0x1000  # never dereferenced: every call below returns before a launch
    # B * Nq == 0: OK, whatever the pointers
    assert run(None, None, None, 0, 16, 16, 64, 1, 1.0, None, None) == OK
    assert run(None, None, None, 2, 0, 16, 64, 1, 1.0, None, None) == OK
    # null pointers with work to do
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert run(args[0], args[1], args[2], 1, 16, 16, 64, 1, 1.0, args[3], None) == EINVAL
    assert run(p, p, p, 1, 16, 0, 64, 1, 1.0, p, None) == EINVAL           # no keys
    # shapes the predicate refuses, and what the kernel's addressing cannot take
    assert run(p, p, p, 1, 16, 16, 164, 1, 1.0, p, None) == EUNSUPPORTED   # d = 164
    assert run(p, p, p, 1, 8, 16, 64, 1, 1.0, p, None) == EUNSUPPORTED     # Nq = 8
    assert run(p, p, p, 1, 16, 16, 6, 1, 1.0, p, None) == EUNSUPPORTED     # d % 4
    for args in ((p + 4, p, p, p), (p, p + 8, p, p), (p, p, p + 4, p), (p, p, p, p + 12)):
        assert run(args[0], args[1], args[2], 1, 16, 16, 64, 1, 1.0, args[3], None) == EUNSUPPORTED  # a misaligned pointer
    assert run(p, p, p, 1, 16, 2 ** 23, 64, 1, 1.0, p, None) == EUNSUPPORTED  # one batch's K: 2 GiB
    # the same answers as the fp32 entry
    f32 = L.sige_hip_attention_tokens_f32.fn
    for a in ((None, None, None, 0, 16, 16, 64, 1, 1.0, None, None), (None, p, p, 1, 16, 16, 64, 1, 1.0, p, None),
              (p, p, p, 1, 16, 16, 164, 1, 1.0, p, None), (p + 4, p, p, 1, 16, 16, 64, 1, 1.0, p, None)):
        assert run(*a) == f32(*a)
