"""The five attention kernels where the scaled scores are large or far apart (tests/attention_stress.py: the regimes, the fp64 truth
and the bound; tests/test_attention_stress_inputs.py: what each regime sees that randn inputs cannot).

Every case is one launch on tiny tensors: the output is pre-filled with NaN where the wrapper takes `out=`, else the call runs inside
util.poisoned() (the score workspace of the two-launch forms, every torch-allocated scratch); then util.assert_finite, the error
against the fp64 chain, and the bound max(4 * e32, 2e-5 * (1 + max|want|)) with e32 the fp32 torch chain's error on the GPU.  Every
margin is recorded (util.record_margin; kept as profiles/attention_softmax_stress_test_margins.jsonl).

Measured on an MI355X (275 cases, one margin line each): every kernel passes unchanged; worst error / bound per entry 0.13 (NCHW),
0.21 (channels-last pair and one-launch form), 0.46 (attention_tokens, each form), 0.61 (attention_wide) -- profiles/README.md."""
import pytest
import torch

from tests import attention_stress as A
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
_HW = {16: (4, 4), 272: (16, 17)}


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


_gpu = {}


def _case(B, Nq, Nk, heads, d, regime, spike, layout="tokens"):
    """(q, k, v) on the GPU as tokens, the fp64 truth on the CPU, the fp32 chain's error (computed on the GPU) and the bound: once
    per process, shared by every entry and form that runs the case."""
    key = (B, Nq, Nk, heads, d, regime, spike, layout)
    if key not in _gpu:
        q, k, v, want = A.case(*key)
        qg, kg, vg = (t.contiguous().to(DEV) for t in (q, k, v))
        e32 = float((A.chain(qg, kg, vg, heads, d ** -0.5, torch.float32).double().cpu() - want).abs().max())
        _gpu[key] = (qg, kg, vg, want, e32, A.bound(want, e32))
    return _gpu[key]


def _judge(entry, what, got, want, e32, tol):
    """`got` [B,Nq,C] (any device / strides): finite first, then the error against fp64, then the bound."""
    util.assert_finite(got, "%s %s" % (entry, what))
    err = float((got.double().cpu() - want).abs().max())
    print("%s %s: err %.3e, fp32 chain %.3e, bound %.3e" % (entry, what, err, e32, tol))
    util.record_margin("test_gpu_attention_stress %s" % entry, what, err, tol)
    assert err <= tol, "%s %s: max |diff| %.3e > bound %.3e (fp32 chain %.3e)" % (entry, what, err, tol, e32)


def _token_cases(shapes):
    return [pytest.param(s, r, j, id="B%d_Nq%d_Nk%d_h%d_d%d-%s" % (s + (A.regime_id(r, j),))) for s in shapes for r, j in A.regimes_for(s[2])]


def _what(shape, regime, spike):
    return "B=%d Nq=%d Nk=%d heads=%d d=%d %s" % (tuple(shape) + (A.regime_id(regime, spike),))


# ---- hip.attention_tokens: forms 0 (transposed scores, the default), 1 and 2 -------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("shape,regime,spike", _token_cases(A.TOKEN_SHAPES))
def test_attention_tokens(shape, regime, spike, form, tuning):
    hip = tuning
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e32, tol = _case(B, Nq, Nk, heads, d, regime, spike)
    hip.tuning_set("attention_form", form)
    try:
        with util.poisoned() as p:
            got = hip.attention_tokens(q, k, v, heads, d ** -0.5)
    finally:
        hip.tuning_set("attention_form", 0)
    assert p.n > 0 and got is not None and tuple(got.shape) == (B, Nq, heads * d)
    _judge("attention_tokens form %d" % form, _what(shape, regime, spike), got, want, e32, tol)


# ---- hip.attention_wide ------------------------------------------------------------------------------------------------------------
def _run_wide(hip, q, k, v, heads, d):
    out = torch.full(tuple(q.shape), float("nan"), device=DEV)
    with util.poisoned():
        got = hip.attention_wide(q, k, v, heads, d ** -0.5, out=out)
    assert got is out
    return out


@pytest.mark.parametrize("shape,regime,spike", _token_cases(A.WIDE_SHAPES))
def test_attention_wide(hip, shape, regime, spike):
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e32, tol = _case(B, Nq, Nk, heads, d, regime, spike)
    _judge("attention_wide", _what(shape, regime, spike), _run_wide(hip, q, k, v, heads, d), want, e32, tol)


def test_attention_wide_strided_ramp(hip):
    """k | v the halves of ONE [B,Nk,2C] tensor, read in place."""
    shape = (1, 48, 100, 1, 192)
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e32, tol = _case(B, Nq, Nk, heads, d, "ramp", None)
    C = heads * d
    kv = torch.cat([k, v], dim=2)
    ks, vs = kv[:, :, :C], kv[:, :, C:]
    assert ks.stride(1) == 2 * C and not vs.is_contiguous()
    _judge("attention_wide", _what(shape, "ramp", None) + " strided", _run_wide(hip, q, ks, vs, heads, d), want, e32, tol)


# ---- the qkv layouts: [B,3C,H,W], one head, d = C, Nq = Nk = HW --------------------------------------------------------------------
def _image(t, H, W):
    """Tokens [B,HW,C] -> [B,C,H,W] (contiguous)."""
    B, HW, C = t.shape
    return t.transpose(1, 2).reshape(B, C, H, W).contiguous()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _qkv_cases(shapes):
    return [pytest.param(s, r, j, id="B%d_C%d_H%d_W%d-%s" % (s + (A.regime_id(r, j),))) for s in shapes for r, j in A.regimes_for(s[2] * s[3], qkv=True)]


def _qkv_case(shape, regime, spike):
    B, C, H, W = shape
    q, k, v, want, e32, tol = _case(B, H * W, H * W, 1, C, regime, spike, "qkv")
    return torch.cat([_image(t, H, W) for t in (q, k, v)], dim=1), want, e32, tol


@pytest.mark.parametrize("shape,regime,spike", _qkv_cases([(1, 32, 4, 4), (2, 64, 16, 17)]))
def test_attention_nchw(hip, shape, regime, spike):
    B, C, H, W = shape
    assert hip.attention_supported(C, H * W)
    qkv, want, e32, tol = _qkv_case(shape, regime, spike)
    with util.poisoned() as p:
        got = hip.attention(qkv, C ** -0.5)
    assert p.n > 0  # (the score workspace and the output)
    _judge("attention", "B=%d C=%d H=%d W=%d %s" % (shape + (A.regime_id(regime, spike),)), A.tokens_of(got), want, e32, tol)


_CL_SHAPES = [(b, c) + _HW[hw] for b, c, hw in [(2, 64, 16), (1, 64, 272), (1, 128, 16)]]  # (the SUPPORTED shapes of the key-fold test)


@pytest.mark.parametrize("fused", [False, True], ids=["two_launches", "fused"])
@pytest.mark.parametrize("shape,regime,spike", _qkv_cases(_CL_SHAPES))
def test_attention_cl(hip, monkeypatch, shape, regime, spike, fused):
    """The channels-last score / apply pair and the one-launch form (HW = 272: the HW > 256 softmax path; five fused key slices, the
    last one partial)."""
    B, C, H, W = shape
    qkv, want, e32, tol = _qkv_case(shape, regime, spike)
    qkv = _cl(qkv)
    monkeypatch.setattr(hip, "FUSED_ATTENTION", fused)
    if fused:
        assert hip.lib().sige_hip_attention_fused_workspace(B, C, H * W) > 0
    n0 = hip.launch_count()
    with util.poisoned() as p:
        got = hip.attention_cl(qkv, C ** -0.5)
    assert got is not None and hip.is_cl(got) and p.n > 0
    assert hip.launch_count() == n0 + (1 if fused else 2)
    _judge("attention_cl %s" % ("fused" if fused else "two launches"),
           "B=%d C=%d H=%d W=%d %s" % (shape + (A.regime_id(regime, spike),)), A.tokens_of(got), want, e32, tol)


@pytest.mark.parametrize("regime", ["ramp", "rows"])
@pytest.mark.parametrize("shape", _CL_SHAPES, ids=lambda s: "B%d_C%d_H%d_W%d" % s)
@pytest.mark.parametrize("entry", ["residual", "residual_qv"])
def test_residual_entries_keep_attention_cls_bits(hip, entry, shape, regime):
    """Without bias / residual / twins the two epilogue entries ARE attention_cl: bit-identical where the row maxima are hundreds
    apart, as test_old_entries_keep_their_bits_and_strides_do_not_matter holds at randn."""
    B, C, H, W = shape
    qkv, want, e32, tol = _qkv_case(shape, regime, None)
    qkv = _cl(qkv)
    plain = hip.attention_cl(qkv, C ** -0.5)
    with util.poisoned() as p:
        if entry == "residual":
            got, made = hip.attention_residual_cl(qkv, C ** -0.5)
        else:
            q, k, v = qkv.split(C, dim=1)
            got, made = hip.attention_residual_qv_cl(_cl(torch.cat([q, v], 1)), _cl(k), C ** -0.5)
    assert p.n > 0 and made == {}
    util.assert_finite(got, "attention_%s_cl %s" % (entry, regime))
    assert torch.equal(got, plain)
    _judge("attention_%s_cl" % entry, "B=%d C=%d H=%d W=%d %s" % (shape + (regime,)), A.tokens_of(got), want, e32, tol)


def test_residual_qv_qscale_ramp(hip):
    """`qscale`: the queries arrive divided by s = 1 + 0.3 randn per channel (the steering channel too) and the score kernel
    multiplies s back in; truth = the fp64 chain of the fp64 product s * (q / s)."""
    B, C, H, W = 1, 64, 16, 17
    q, k, v, _, _, _ = _case(B, H * W, H * W, 1, C, "ramp", None, "qkv")
    g = torch.Generator().manual_seed(C + H * W)
    s = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    assert float(s.abs().min()) > 1e-3
    qd = q / s  # [B,HW,C] / [C]
    want = A.chain(qd.double().cpu() * s.double().cpu(), k.cpu(), v.cpu(), 1, C ** -0.5, torch.float64)
    e32 = float((A.chain(qd * s, k, v, 1, C ** -0.5, torch.float32).double().cpu() - want).abs().max())
    tol = A.bound(want, e32)
    qv = _cl(torch.cat([_image(qd, H, W), _image(v, H, W)], dim=1))
    with util.poisoned() as p:
        got, made = hip.attention_residual_qv_cl(qv, _cl(_image(k, H, W)), C ** -0.5, qscale=s.reshape(1, C, 1, 1))
    assert p.n > 0 and made == {}
    _judge("attention_residual_qv_cl qscale", "B=%d C=%d H=%d W=%d ramp" % (B, C, H, W), A.tokens_of(got), want, e32, tol)
