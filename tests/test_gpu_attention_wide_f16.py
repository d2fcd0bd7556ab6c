"""hip.attention_wide(..., compute="f16") = sige_hip_attention_wide_f16c (csrc/attention_wide_f16.hip) on the GPU: fp16 operands, fp32
accumulation, fp32 tensors in memory (tests/attention_wide_f16.py: the shapes; tests/attention_f16.py: the contract's emulation and the
bound; tests/test_attention_wide_f16_inputs.py: the reference side on the CPU).

Every kernel case is one launch on tiny tensors inside util.poisoned(); then util.assert_finite, the error against the fp64 truth of the
inputs as given, and bound16 = max(4 * e16, 2e-5 * (1 + max|want|)) with e16 the CPU emulation's error on the same inputs.  Every margin
is recorded (util.record_margin; kept as profiles/attention_wide_f16_test_margins.jsonl)."""
import pytest
import torch

from sige_amd.tolerance import f16_check
from tests import attention_f16 as F
from tests import attention_stress as A
from tests import attention_wide_f16 as WF
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _run(hip, q, k, v, heads, d):
    with util.poisoned() as p:
        got = hip.attention_wide(q.to(DEV), k.to(DEV), v.to(DEV), heads, d ** -0.5, compute="f16")
    assert p.n > 0 and got is not None and tuple(got.shape) == tuple(q.shape)
    return got


def _judge(what, got, want, e16, tol):
    util.assert_finite(got, "attention_wide f16 %s" % what)
    err = float((got.double().cpu() - want).abs().max())
    print("attention_wide f16 %s: err %.3e, emulation %.3e, bound %.3e" % (what, err, e16, tol))
    util.record_margin("test_gpu_attention_wide_f16", what, err, tol)
    assert err <= tol, "%s: max |diff| %.3e > bound %.3e (emulation %.3e)" % (what, err, tol, e16)


def _what(shape, tag):
    return "B=%d Nq=%d Nk=%d heads=%d d=%d %s" % (tuple(shape) + (tag,))


@pytest.mark.parametrize("shape,regime,spike", [pytest.param(s, r, j, id="%s-%s" % (WF.shape_id(s), A.regime_id(r, j))) for s, r, j in WF.cases()])
def test_regimes(hip, shape, regime, spike):
    """The softmax regimes of tests/attention_stress.py, inputs rounded to fp16 first."""
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.case(B, Nq, Nk, heads, d, regime, spike)
    _judge(_what(shape, A.regime_id(regime, spike)), _run(hip, q, k, v, heads, d), want, e16, tol)


@pytest.mark.parametrize("shape", WF.WIDE_F16_SHAPES, ids=WF.shape_id)
def test_unrounded_randn_inputs(hip, shape):
    """The kernel rounds its inputs itself: against the fp64 truth of the UNROUNDED inputs."""
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.randn_case(*shape)
    got = _run(hip, q, k, v, heads, d)
    _judge(_what(shape, "randn"), got, want, e16, tol)
    chk = f16_check(got, want)
    assert chk["ok"], chk


def test_dust(hip):
    """2047 probabilities below 2^-14 -- fp16 subnormals -- carry 3.4 % of the mass: they must arrive in the product with V."""
    q, k, v, want, e16, tol = WF.dust_case()
    _judge("dust Nq=16 Nk=2048 d=%d" % WF.DUST_D, _run(hip, q, k, v, 1, WF.DUST_D), want, e16, tol)


def test_the_key_split_runs_and_agrees_with_a_launch_that_cannot_split(hip):
    """(2, 32, 256, 1, 512): the host's own formula gives two workgroups per query tile.  The same queries repeated 65 times are 260
    query tiles -- more than a workgroup per CU without any split -- so that launch has no split available: both inside the bound."""
    B, Nq, Nk, heads, d = WF.SPLIT_SHAPE
    splits = getattr(hip.lib().sige_hip_attention_wide_f16c_splits, "fn", hip.lib().sige_hip_attention_wide_f16c_splits)
    assert splits(B, Nq, Nk, heads * d, heads) == 2 and splits(B, 65 * Nq, Nk, heads * d, heads) == 1
    q, k, v, want, e16, tol = F.randn_case(*WF.SPLIT_SHAPE)
    got = _run(hip, q, k, v, heads, d)
    _judge(_what(WF.SPLIT_SHAPE, "randn split"), got, want, e16, tol)
    many = _run(hip, q.repeat(1, 65, 1), k, v, heads, d)
    for rep in (0, 64):
        _judge(_what(WF.SPLIT_SHAPE, "randn unsplit copy %d" % rep), many[:, rep * Nq:(rep + 1) * Nq], want, e16, tol)
    assert torch.equal(many[:, :Nq], many[:, 64 * Nq:])
    err = float((got - many[:, :Nq]).abs().max())
    print("split against unsplit: max |diff| %.3e" % err)
    assert err <= 2.0 * tol


def _strided(B, Nq, Nk, C, seed):
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(B, Nk, 2 * C, generator=g).to(DEV)
    wide = (torch.randn(B, Nq, C + 64, generator=g) * 2.0).to(DEV)
    return wide[:, :, :C], kv[:, :, :C], kv[:, :, C:]


@pytest.mark.parametrize("B,Nq,Nk,d", [(1, 32, 96, 512), (2, 32, 256, 512), (1, 16, 40, 176)])  # (unsplit, split, a padded last unit)
def test_strided_views_equal_contiguous_copies_bit_for_bit(hip, B, Nq, Nk, d):
    """k | v the two halves of ONE [B,Nk,2C] tensor, q a column slice of a wider matrix, `out` a column slice of a NaN matrix: the
    result equals the result on contiguous copies bit for bit, and nothing outside out's rows and columns is written.  At d = 176 the
    16 channels past d of a K row are V's first channels and, poisoned below, NaN: they must not reach a score."""
    q, k, v = _strided(B, Nq, Nk, d, Nq + Nk + d)
    assert not k.is_contiguous() and k.stride(1) == 2 * d and not q.is_contiguous()
    want = hip.attention_wide(q.contiguous(), k.contiguous(), v.contiguous(), 1, d ** -0.5, compute="f16")
    util.assert_finite(want, "contiguous copies")
    # (rows past Nq only at B = 1: with a batch stride that is not Nq rows the binding asks for another `out`)
    big = torch.full((B, Nq + (16 if B == 1 else 0), d + 32), float("nan"), device=DEV)
    out = big[:, :Nq, :d]
    with util.poisoned():
        got = hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, compute="f16")
    assert got is out
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    bits = big.view(torch.int32)
    assert bool((bits[:, Nq:] == NAN_BITS).all()), "a row past Nq was written"
    assert bool((bits[:, :, d:] == NAN_BITS).all()), "a column past C was written"
    # K rows followed by NaN: the half-unit past d is zeroed on the K side, not multiplied by Q's zeros
    kn = torch.full((B, Nk, 2 * d), float("nan"), device=DEV)
    kn[:, :, :d] = k
    assert torch.equal(hip.attention_wide(q, kn[:, :, :d], v, 1, d ** -0.5, compute="f16"), want)


@pytest.mark.parametrize("Nq,Nk,d", [(32, 256, 512), (16, 40, 192)])  # (with and without the key split)
def test_graph_replay_equals_eager_bit_for_bit(hip, Nq, Nk, d):
    q, k, v = (t.to(DEV) for t in F.randn_case(1, Nq, Nk, 1, d)[:3])
    out = torch.empty(1, Nq, d, device=DEV)
    eager = hip.attention_wide(q, k, v, 1, d ** -0.5, compute="f16").clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, compute="f16")
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            hip.attention_wide(q, k, v, 1, d ** -0.5, out=out, compute="f16")
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del g


@pytest.mark.parametrize("Nq,d", [(16, 160), (16, 528), (16, 200), (24, 512)])
def test_refused_shapes_return_none_and_launch_nothing(hip, Nq, d):
    q, k = torch.zeros(1, Nq, d, device=DEV), torch.zeros(1, 16, d, device=DEV)
    torch.cuda.synchronize()
    n0 = hip.launch_count()
    assert hip.attention_wide(q, k, k, 1, 1.0, compute="f16") is None
    assert hip.attention_wide(q, k, k, 1, 1.0) is None
    assert hip.launch_count() == n0
    with pytest.raises(ValueError):
        hip.attention_wide(q, k, k, 1, 1.0, compute="bf16")


def test_fp32_form_is_unchanged_by_the_keyword(hip):
    shape = (1, 48, 100, 1, 192)
    B, Nq, Nk, heads, d = shape
    q, k, v = (t.to(DEV) for t in F.randn_case(*shape)[:3])
    plain = hip.attention_wide(q, k, v, heads, d ** -0.5)
    n0 = hip.launch_count()
    keyed = hip.attention_wide(q, k, v, heads, d ** -0.5, compute="f32")
    assert hip.launch_count() == n0 + 1
    assert torch.equal(plain, keyed)
    n0 = hip.launch_count()
    half = hip.attention_wide(q, k, v, heads, d ** -0.5, compute="f16")
    assert hip.launch_count() == n0 + 1
    assert not torch.equal(plain, half)
