"""The reference side of the fp16-operand wide-head attention's tests (tests/attention_wide_f16.py), the binding's argument checks and
the two entry points' status rules -- nothing here touches a device.

Measured with these inputs: see the printed lines (e16, bound, worst mutant ratio per mutant); a mutant that no wide case can tell
apart fails its test -- the bound is not loosened for it."""
import ctypes

import pytest
import torch

from sige_amd.tolerance import f16_check
from tests import attention_f16 as F
from tests import attention_stress as A
from tests import attention_wide_f16 as WF

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.mark.parametrize("shape,regime,spike", [pytest.param(s, r, j, id="%s-%s" % (WF.shape_id(s), A.regime_id(r, j))) for s, r, j in WF.cases()])
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
def test_every_mutant_shows_in_some_wide_case(mutant):
    worst, where = 0.0, None
    for shape, regime, spike in WF.cases():
        B, Nq, Nk, heads, d = shape
        q, k, v, want, e16, tol = F.case(B, Nq, Nk, heads, d, regime, spike)
        got = F.emulate(q, k, v, heads, d ** -0.5, mutant=mutant)
        ratio = float("inf") if not bool(torch.isfinite(got).all()) else float((got.double() - want).abs().max()) / tol
        if ratio > worst:
            worst, where = ratio, (shape, A.regime_id(regime, spike))
        if worst > 1.0:
            break
    print("%s: error / bound %.3g at %s" % (mutant, worst, where))
    assert worst > 1.0, "%s passes every wide case (worst error / bound %.3g)" % (mutant, worst)


@pytest.mark.parametrize("shape", WF.WIDE_F16_SHAPES, ids=WF.shape_id)
def test_unrounded_randn_inputs_meet_the_f16_criterion(shape):
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.randn_case(*shape)
    assert not torch.equal(F.r16(q), q)
    chk = f16_check(F.emulate(q, k, v, heads, d ** -0.5), want)
    print("%s: e16 %.3e, bound %.3e, f16_check %s" % (shape, e16, tol, chk))
    assert chk["ok"], chk


def test_dust_at_a_wide_head_needs_the_subnormal_probabilities():
    q, k, v, want, e16, tol = WF.dust_case()
    d = WF.DUST_D
    p = torch.softmax((q[0].double() @ k[0].double().T) * d ** -0.5, dim=1)
    small = p[0][p[0] < 0.5]
    assert small.numel() == 2047 and float(small.max()) < 2.0 ** -14 and 0.03 < float(small.sum()) < 0.04
    flushed = float((F.emulate(q, k, v, 1, d ** -0.5, flush=True).double() - want).abs().max())
    print("dust d=%d: max|want| %.3g, clean error %.3e, bound %.3e, flushed error %.3e" % (d, float(want.abs().max()), e16, tol, flushed))
    assert e16 <= tol
    assert flushed > tol


def test_binding_validates_compute_first_and_the_default_is_the_policy():
    from sige_amd import hip
    from sige_amd.workloads import sd_vae

    q = torch.zeros(1, 16, 192)
    with pytest.raises(ValueError):
        hip.attention_wide(q, q, q, 1, 1.0, compute="bf16")
    assert hip.attention_wide(q, q, q, 1, 1.0, compute="f16") is None  # (CPU tensors: where the fp32 form returns None)
    assert hip.attention_wide(q, q, q, 1, 1.0) is None
    assert sd_vae.ATTENTION_COMPUTE is None
    for name in ("sige_hip_attention_wide", "sige_hip_attention_wide_tiles"):
        assert hip._SIGNATURES[name + "_f16c"] == hip._SIGNATURES[name + "_f32"]


def test_the_switch_follows_q_and_the_derived_conv_follows_k_and_v():
    """sd_vae.ATTENTION_COMPUTE = None resolves from `q`; folded_kv() takes the higher precision of `k` and `v`, re-labels the SAME
    conv when only the dtype changed, and has the dtype in its cache key."""
    from sige_amd.workloads import sd_vae
    from tests.golden import vae_inputs
    from tests.golden.model_init import init_by_name
    from tests.test_sd_vae import vae_config

    model = sd_vae.SparseVAEDecoder(vae_config(vae_inputs.SMALL)).eval()
    init_by_name(model)
    attn = model.mid.attn_1
    conv = attn.folded_kv()
    assert conv.compute_dtype == "f32" and attn.attention_compute() == "f32"
    model.set_compute_dtype("f16")
    assert attn.attention_compute() == "f16"
    assert attn.folded_kv() is conv and conv.compute_dtype == "f16" and attn.__dict__["_kv_conv"][0][-1] == "f16"
    model.set_compute_dtype("f16", keep=("mid.attn_1.v",))
    assert attn.folded_kv().compute_dtype == "f16x3" and attn.attention_compute() == "f16"
    model.set_compute_dtype("f16", keep=("mid.attn_1.q", "mid.attn_1.k"))
    assert attn.folded_kv().compute_dtype == "f16x3" and attn.attention_compute() == "f32"
    model.set_compute_dtype("f16x3")
    assert attn.folded_kv().compute_dtype == "f16x3" and attn.attention_compute() == "f32"
    model.set_compute_dtype("f32")
    assert attn.folded_kv() is conv and conv.compute_dtype == "f32" and attn.attention_compute() == "f32"
    keep = sd_vae.ATTENTION_COMPUTE
    try:
        sd_vae.ATTENTION_COMPUTE = "f16"
        assert attn.attention_compute() == "f16"
        sd_vae.ATTENTION_COMPUTE = "bf16"
        with pytest.raises(ValueError):
            attn.attention_compute()
    finally:
        sd_vae.ATTENTION_COMPUTE = keep
    for cls in (sd_vae.SparseVAEDecoder, sd_vae.SparseVAEEncoder):
        assert cls.F16_KEEP == () and cls.F16_KEEP_ABOVE == 0.0


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def test_batched_entry_status_rules_without_a_launch(L):
    from sige_amd import hip

    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "sige_hip_attention_wide_f16c")
    run, f32 = L.sige_hip_attention_wide_f16c.fn, L.sige_hip_attention_wide_f32.fn  # (the raw ctypes functions: no device guard)
    p = 0x1000  # never dereferenced: every call below returns before a launch

    def args(q=p, k=p, v=p, out=p, B=1, Nq=32, Nk=100, C=512, heads=1, ld=None):
        ldq, ldk, ldv, ldo = ld or (C, C, C, C)
        return (q, ldq, k, ldk, v, ldv, B, Nq, Nk, C, heads, 0.1, out, ldo, None)

    n0 = hip.launch_count()
    for kw, want in ((dict(B=0), OK), (dict(Nq=0), OK), (dict(B=0, q=None, k=None, v=None, out=None), OK),
                     (dict(B=-1), EINVAL), (dict(Nk=0), EINVAL), (dict(C=0), EINVAL), (dict(heads=0), EINVAL),
                     (dict(ld=(256, 512, 512, 512)), EINVAL), (dict(q=None), EINVAL), (dict(k=None), EINVAL), (dict(v=None), EINVAL),
                     (dict(out=None), EINVAL), (dict(B=0, ld=(256, 512, 512, 512)), EINVAL),  # (the stride check comes first)
                     (dict(C=160), EUNSUPPORTED), (dict(C=528), EUNSUPPORTED), (dict(C=200), EUNSUPPORTED), (dict(Nq=24), EUNSUPPORTED),
                     (dict(C=512, heads=4), EUNSUPPORTED), (dict(q=p + 4), EUNSUPPORTED), (dict(out=p + 8), EUNSUPPORTED),
                     (dict(ld=(514, 512, 512, 512)), EUNSUPPORTED), (dict(ld=(512, 512, 512, 513)), EUNSUPPORTED),
                     (dict(Nk=2 ** 21), EUNSUPPORTED)):  # (one batch's K: 4 GiB)
        a = args(**kw)
        assert run(*a) == want, kw
        assert f32(*a) == want, kw  # the same answers as the fp32 entry
    assert hip.launch_count() == n0


def test_tiles_entry_status_rules_without_a_launch(L):
    """Every case of tests/test_attention_wide_tiles_status.py (imported, not copied) gets the fp32 entry's answer, before a launch."""
    from tests.test_attention_wide_tiles_status import BASE, CASES, NAMES, answer

    before = L.sige_hip_launch_count()
    for edits, change, want in CASES:
        got = answer(L, "sige_hip_attention_wide_tiles_f16c", NAMES, dict(BASE, **change), edits)
        assert got == want, (edits, change, got, want)
    assert L.sige_hip_launch_count() == before


def test_the_host_split_formula(L):
    """Splits are counted in 32-key steps, at least four (one per wave) per split, about one workgroup per CU in all."""
    fn = L.sige_hip_attention_wide_f16c_splits
    fn = getattr(fn, "fn", fn)  # (no status to check: the binding may hand the ctypes function out as it is)
    assert fn(*WF.SPLIT_SHAPE[:3], WF.SPLIT_SHAPE[3] * WF.SPLIT_SHAPE[4], WF.SPLIT_SHAPE[3]) == 2
    assert fn(1, 16, 4096, 512, 1) == 16 and fn(1, 16 * 20, 4096, 512, 1) == 12  # (11 steps each: 12 splits, none empty)
    assert fn(1, 16, 100, 192, 1) == 1 and fn(2, 32 * 65, 256, 512, 1) == 1
    assert fn(1, 16, 100, 160, 1) == 0
