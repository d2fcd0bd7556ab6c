"""hip.attention_tokens(..., compute="f16") = sige_hip_attention_tokens_f16c (csrc/attention_tokens_f16.hip) on the GPU: fp16 operands,
fp32 accumulation, fp32 tensors in memory (tests/attention_f16.py: the contract's emulation, the inputs and the bound;
tests/test_attention_f16_inputs.py: the reference side on the CPU).

Every kernel case is one launch on tiny tensors inside util.poisoned(); then util.assert_finite, the error against the fp64 truth of the
inputs as given, and bound16 = max(4 * e16, 2e-5 * (1 + max|want|)) with e16 the CPU emulation's error on the same inputs.  Every margin
is recorded (util.record_margin; kept as profiles/attention_tokens_f16_test_margins.jsonl).

Measured on an MI355X (85 margin lines): worst error / bound 0.36 (B=1 Nq=16 Nk=33 heads=2 d=80 offset+: 2.0e-4 against 5.5e-4); `dust` 1.3e-4
against 5.4e-3; the transformer and the small U-Net with the switch on: worst element at 0.007 / 0.006 of the f16 criterion's allowance."""
import pytest
import torch

from sige_amd.tolerance import f16_check
from tests import attention_f16 as F
from tests import attention_stress as A
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _run(hip, q, k, v, heads, d):
    with util.poisoned() as p:
        got = hip.attention_tokens(q.to(DEV), k.to(DEV), v.to(DEV), heads, d ** -0.5, compute="f16")
    assert p.n > 0 and got is not None and tuple(got.shape) == tuple(q.shape)
    return got


def _judge(what, got, want, e16, tol):
    util.assert_finite(got, "attention_tokens f16 %s" % what)
    err = float((got.double().cpu() - want).abs().max())
    print("attention_tokens f16 %s: err %.3e, emulation %.3e, bound %.3e" % (what, err, e16, tol))
    util.record_margin("test_gpu_attention_f16", what, err, tol)
    assert err <= tol, "%s: max |diff| %.3e > bound %.3e (emulation %.3e)" % (what, err, tol, e16)


def _what(shape, tag):
    return "B=%d Nq=%d Nk=%d heads=%d d=%d %s" % (tuple(shape) + (tag,))


_SHAPE_ID = lambda s: "B%d_Nq%d_Nk%d_h%d_d%d" % s  # noqa: E731


@pytest.mark.parametrize("shape,regime,spike", [pytest.param(s, r, j, id="%s-%s" % (_SHAPE_ID(s), A.regime_id(r, j)))
                                                 for s in F.F16_SHAPES for r, j in A.regimes_for(s[2])])
def test_regimes(hip, shape, regime, spike):
    """The softmax regimes of tests/attention_stress.py, inputs rounded to fp16 first."""
    B, Nq, Nk, heads, d = shape
    q, k, v, want, e16, tol = F.case(B, Nq, Nk, heads, d, regime, spike)
    _judge(_what(shape, A.regime_id(regime, spike)), _run(hip, q, k, v, heads, d), want, e16, tol)


@pytest.mark.parametrize("shape", F.F16_SHAPES, ids=_SHAPE_ID)
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
    q, k, v, want, e16, tol = F.dust_case()
    _judge("dust Nq=16 Nk=2048 d=40", _run(hip, q, k, v, 1, 40), want, e16, tol)


def test_views_are_read_like_contiguous_copies(hip):
    """q from channels-last tiles [T,C,4,4], k and v from channels-last [B,C,H,W] tensors -- as views of those bytes, and as channel
    slices of a wider tensor (strided rows): the result equals the result on contiguous copies bit for bit."""
    B, heads, d, H, W, T = 2, 2, 40, 6, 7, 6
    C = heads * d
    g = torch.Generator().manual_seed(5)
    tiles = torch.randn(T, C, 4, 4, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    kv = torch.randn(B, 2 * C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    q = tiles.permute(0, 2, 3, 1).reshape(B, T * 16 // B, C)
    assert q.data_ptr() == tiles.data_ptr()
    k_img, v_img = kv[:, :C].contiguous(memory_format=torch.channels_last), kv[:, C:].contiguous(memory_format=torch.channels_last)
    as_tokens = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, C)  # noqa: E731
    k, v = as_tokens(k_img), as_tokens(v_img)
    assert k.data_ptr() == k_img.data_ptr() and v.data_ptr() == v_img.data_ptr()
    ks, vs = kv.permute(0, 2, 3, 1).reshape(B, H * W, 2 * C)[:, :, :C], kv.permute(0, 2, 3, 1).reshape(B, H * W, 2 * C)[:, :, C:]
    assert not ks.is_contiguous() and ks.stride(1) == 2 * C
    want = hip.attention_tokens(q.clone().contiguous(), k.clone().contiguous(), v.clone().contiguous(), heads, d ** -0.5, compute="f16")
    util.assert_finite(want, "contiguous copies")
    for name, args in (("views", (q, k, v)), ("channel slices", (q, ks, vs))):
        with util.poisoned():
            got = hip.attention_tokens(*args, heads, d ** -0.5, compute="f16")
        assert got is not None and torch.equal(got, want), name


@pytest.mark.parametrize("Nq,Nk,C,heads", [(8, 16, 64, 1), (16, 16, 164, 1), (16, 16, 6, 1), (24, 16, 64, 1)])
def test_refused_shapes_return_none_and_launch_nothing(hip, Nq, Nk, C, heads):
    assert not hip.lib().sige_hip_attention_tokens_supported(Nq, Nk, C, heads)
    q, k = torch.zeros(1, Nq, C, device=DEV), torch.zeros(1, Nk, C, device=DEV)
    torch.cuda.synchronize()
    n0 = hip.launch_count()
    assert hip.attention_tokens(q, k, k, heads, 1.0, compute="f16") is None
    assert hip.attention_tokens(q, k, k, heads, 1.0) is None
    assert hip.launch_count() == n0
    with pytest.raises(ValueError):
        hip.attention_tokens(q, k, k, heads, 1.0, compute="bf16")


def test_fp32_form_is_unchanged_by_the_keyword(hip):
    shape = (2, 48, 100, 2, 40)
    B, Nq, Nk, heads, d = shape
    q, k, v = (t.to(DEV) for t in F.randn_case(*shape)[:3])
    plain = hip.attention_tokens(q, k, v, heads, d ** -0.5)
    n0 = hip.launch_count()
    keyed = hip.attention_tokens(q, k, v, heads, d ** -0.5, compute="f32")
    assert hip.launch_count() == n0 + 1
    assert torch.equal(plain, keyed)
    assert not torch.equal(plain, hip.attention_tokens(q, k, v, heads, d ** -0.5, compute="f16"))


def test_graph_replay_returns_the_eager_bits(hip):
    shape = (2, 48, 100, 2, 40)
    B, Nq, Nk, heads, d = shape
    q1, k, v = (t.to(DEV) for t in F.randn_case(*shape)[:3])
    q0 = F.case(B, Nq, Nk, heads, d, "ramp")[0].to(DEV)
    eager1 = hip.attention_tokens(q1, k, v, heads, d ** -0.5, compute="f16").clone()
    eager0 = hip.attention_tokens(q0, k, v, heads, d ** -0.5, compute="f16").clone()
    assert not torch.equal(eager0, eager1)
    qin = q1.clone()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.attention_tokens(qin, k, v, heads, d ** -0.5, compute="f16")
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            captured = hip.attention_tokens(qin, k, v, heads, d ** -0.5, compute="f16")
    torch.cuda.current_stream().wait_stream(s)
    for x, want in ((q0, eager0), (q1, eager1)):
        qin.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, want)
    del g


class _switch:
    """sd_transformer.ATTENTION_COMPUTE for the duration of a `with`."""

    def __init__(self, compute):
        from sige_amd.workloads import sd_transformer

        self.sdt, self.compute = sd_transformer, compute

    def __enter__(self):
        self.keep = self.sdt.ATTENTION_COMPUTE
        self.sdt.ATTENTION_COMPUTE = self.compute
        return self

    def __exit__(self, *exc):
        self.sdt.ATTENTION_COMPUTE = self.keep
        return False


def _f16_against_f32(what, f16, f32):
    chk = f16_check(f16, f32)
    print("%s, switch f16 vs f32: %s" % (what, chk))
    util.record_margin("test_gpu_attention_f16 %s" % what, "f16_check worst / allowed", chk["worst_over_allowed"], 1.0)
    assert chk["ok"], (what, chk)
    assert not torch.equal(f16, f32), "%s: the switch changed nothing" % what


@pytest.mark.oracle_parity
def test_spatial_transformer_with_the_switch(hip):
    """SD's level-1 transformer (320 channels, 8 heads of 40, 64 x 64 tokens, 15 % edit): the switch changes the full and the sparse
    output within the f16 criterion and no launch count; the fp32 pair is still the fixture's."""
    from sige_amd.workloads import sd_transformer
    from tests.test_models_golden import _check, _sd_transformer

    assert sd_transformer.ATTENTION_COMPUTE == "f32"
    with _switch("f32"):
        n0 = hip.launch_count()
        full32, sparse32 = _sd_transformer(DEV, True, True)
        n32 = hip.launch_count() - n0
    with _switch("f16"):
        n0 = hip.launch_count()
        full16, sparse16 = _sd_transformer(DEV, True, True)
        n16 = hip.launch_count() - n0
    assert sd_transformer.ATTENTION_COMPUTE == "f32"
    assert n16 == n32 and n32 > 0
    util.assert_finite(full16, "full, f16 attention")
    util.assert_finite(sparse16, "sparse, f16 attention")
    _f16_against_f32("SpatialTransformer full", full16, full32)
    _f16_against_f32("SpatialTransformer sparse", sparse16, sparse32)
    _check("sdt/full", full32)
    _check("sdt/sparse", sparse32, 1e-3)


def test_small_sd_unet_with_the_switch(hip, monkeypatch):
    """The SD U-Net at model_channels 128 in the f16 compute mode on BOTH sides (set_compute_dtype("f16"): tests.test_models_golden._sd_unet
    builds the model itself, so the mode is set where it sets the scatter form, before the first forward), so the comparison isolates
    the attention."""
    from sige_amd.workloads.sd_unet import SDUNet
    from tests.test_models_golden import _sd_unet

    base = SDUNet.set_scatter_inplace

    def set_scatter_inplace_and_f16(self, *a, **kw):
        out = base(self, *a, **kw)
        self.set_compute_dtype("f16")
        return out

    monkeypatch.setattr(SDUNet, "set_scatter_inplace", set_scatter_inplace_and_f16)
    with _switch("f32"):
        n0 = hip.launch_count()
        _, sparse32 = _sd_unet(DEV, True, True)
        n32 = hip.launch_count() - n0
    with _switch("f16"):
        n0 = hip.launch_count()
        _, sparse16 = _sd_unet(DEV, True, True)
        n16 = hip.launch_count() - n0
    assert n16 == n32 and n32 > 0
    util.assert_finite(sparse16, "SD U-Net sparse, f16 attention")
    _f16_against_f32("SD U-Net (f16 compute) sparse", sparse16, sparse32)
