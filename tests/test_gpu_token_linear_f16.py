"""The token linear on fp16 operands (csrc/token_linear_f16.hip, hip.token_linear(compute="f16")) against fp64, against an fp64
emulation of its rounding, under poisoned allocations, and as the SD transformer block's opt-in compute
(sd_transformer.TOKEN_LINEAR_COMPUTE)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


# name -> (M, N, K, options), built as tests/test_gpu_token_linear.py builds its table.  The library takes the 64-token form where the
# ceil(M / 64) * ceil(N / 64) workgroups fill at least 0.7 of their rounds of 256 with real rows (csrc/token_linear_f16.hip:
# kTokFillF16, kTokRoundF16), else the 16-token form: the "w64" cases fill 0.99 of two rounds (32 x 16 = 512, 34 x 15 = 510, 32 x 16 = 512
# workgroups) and have M % 64, N % 64 and K % 128 tails of their own; every other case has at most 30 such workgroups, a fill below 0.06,
# and takes the 16-token form.
def _cases():
    c = {}
    for m, n, k in ((5, 64, 64), (16, 64, 64), (48, 80, 320)):
        for epi in ("plain", "bias", "bias_res"):
            c["%s_%dx%dx%d" % (epi, m, n, k)] = (m, n, k, dict(bias=epi != "plain", res=epi == "bias_res"))
    c["deep_16x64x5120"] = (16, 64, 5120, dict())            # 40 chunks
    c["slice_70x192x160"] = (70, 192, 160, dict(bias=True))  # K % 128 = 32: one live wave slice in the last chunk
    for k in (64, 320, 1280):
        for off in (0.0, 12.0):  # row means of 0 and of 4 sigma
            c["ln_k%d_off%d" % (k, off)] = (70, 80, k, dict(ln=True, bias=True, off=off))
    for d in (32, 160):
        c["geglu_d%d" % d] = (48, 2 * d, 320, dict(geglu=True, bias=True))
    for n1 in (64, 320):
        c["parts3_n%d" % n1] = (70, 3 * n1, 320, dict(parts=3))
    c["ln_parts3"] = (70, 3 * 320, 320, dict(ln=True, parts=3, off=12.0))
    c["ln_geglu"] = (70, 2 * 160, 320, dict(ln=True, geglu=True, bias=True, off=12.0))
    c["w64_plain"] = (2021, 976, 352, dict())
    c["w64_bias_res"] = (2021, 976, 352, dict(bias=True, res=True))
    c["w64_ln_parts3"] = (2165, 3 * 320, 320, dict(ln=True, parts=3, off=12.0))
    c["w64_ln_geglu"] = (2021, 2 * 512, 352, dict(ln=True, geglu=True, bias=True, off=12.0))
    return c


CASES = _cases()
_made = {}


def _formula(d, a, w):
    """Everything behind the operands, in fp64: a [M,K] = prologue(x), w [N,K] -> list of `parts` outputs."""
    r = a @ w.t()
    if d["bias"] is not None:
        r = r + d["bias"].double()
    if d["geglu"]:
        v, gate = r.chunk(2, dim=1)
        r = v * F.gelu(gate)
    if d["res"] is not None:
        r = d["res"].double() + r
    return list(r.chunk(d["parts"], dim=1))


def _case(name):
    """Seeded CPU inputs of a case, its fp64 truth and the fp64 emulation of the contract (prologue(x) and W through .half()),
    computed once per process."""
    if name in _made:
        return _made[name]
    m, n, k, o = CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    geglu, parts = bool(o.get("geglu")), int(o.get("parts", 1))
    no = n // 2 if geglu else n // parts
    d = {"x": 3 * rn(m, k) + o.get("off", 0.0), "w": 0.08 * rn(n, k), "bias": rn(n) if o.get("bias") else None,
         "res": 3 * rn(m, no) if o.get("res") else None, "gamma": rn(k) if o.get("ln") else None, "beta": rn(k) if o.get("ln") else None,
         "geglu": geglu, "parts": parts, "N": n, "ln": bool(o.get("ln"))}
    a = d["x"].double()
    if d["ln"]:
        var, mean = torch.var_mean(a, dim=1, unbiased=False, keepdim=True)
        a = (a - mean) / torch.sqrt(var + EPS) * d["gamma"].double() + d["beta"].double()
    d["ref"] = _formula(d, a, d["w"].double())
    d["emu"] = _formula(d, a.half().double(), d["w"].half().double())
    top = float(torch.cat(d["ref"], dim=1).abs().max())
    d["e16"] = max(float((e - r).abs().max()) for e, r in zip(d["emu"], d["ref"]))
    d["tight"] = 2e-5 * (1.0 + top)              # fp32 accumulation against fp64, the exact-fp32 kernel's bound
    d["tol"] = max(4.0 * d["e16"], d["tight"])   # the project's rule for fp16-operand kernels
    _made[name] = d
    return d


def _run(hip, d, compute="f16"):
    """pack + one launch on the GPU -> list of `parts` outputs."""
    up = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    w = up(d["w"])
    packed = hip.token_linear_pack(list(w.chunk(d["parts"], dim=0)) if d["parts"] > 1 else w, geglu=d["geglu"], compute=compute)
    assert packed is not None and packed.dtype == (torch.float16 if compute == "f16" else torch.float32)
    norm = None
    if d["ln"]:
        norm = torch.nn.LayerNorm(d["x"].shape[1], eps=EPS).to(DEV)
        with torch.no_grad():
            norm.weight.copy_(d["gamma"])
            norm.bias.copy_(d["beta"])
    out = hip.token_linear(up(d["x"]), packed, d["N"], bias=up(d["bias"]), norm=norm, residual=up(d["res"]), geglu=d["geglu"],
                           parts=d["parts"], compute=compute)
    assert out is not None
    return list(out) if isinstance(out, tuple) else [out]


def _worst(outs, refs):
    return max(float((o.double().cpu() - r).abs().max()) for o, r in zip(outs, refs))


def _check(d, outs, what):
    """The bound(s) of a case: against truth; without LayerNorm also against the emulation at the exact-fp32 figure (the operands'
    rounding is then determined; e16 is 13 - 17 x that figure, so a call that ran the fp32 kernel fails it)."""
    err = _worst(outs, d["ref"])
    assert err <= d["tol"], (what, err, d["tol"], d["e16"])
    demu = None
    if not d["ln"]:
        demu = _worst(outs, d["emu"])
        assert demu <= d["tight"], (what, demu, d["tight"], d["e16"])
    return err, demu


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_linear_f16_vs_fp64(hip, name):
    d = _case(name)
    outs = _run(hip, d)
    for o, r in zip(outs, d["ref"]):
        assert tuple(o.shape) == tuple(r.shape)
        util.assert_finite(o, name)
    print("%s: e16 %.3g, bound %.3g, tight %.3g" % (name, d["e16"], d["tol"], d["tight"]))
    err, demu = _check(d, outs, name)
    util.record_margin("test_token_linear_f16_vs_fp64", name, err, d["tol"])
    if demu is not None:
        util.record_margin("test_token_linear_f16_vs_fp64", name + " vs emulation", demu, d["tight"])
    print("%s: max |out - truth| %.3g, max |out - emu| %s" % (name, err, demu))
    again = _run(hip, d)
    assert all(torch.equal(p, q) for p, q in zip(outs, again)), name


@pytest.mark.parametrize("value", [float("nan"), 1e30])
def test_token_linear_f16_under_poisoned_allocations(hip, value):
    """Every allocation (uploads, the fp16 pack, outputs) pre-filled with NaN / 1e30 (65504 in the pack): row tails, column tails, the
    pack's zero padding and the absent wave slices of K % 128 != 0 must not let any of it into a result."""
    for name in sorted(CASES):
        d = _case(name)
        with util.poisoned(value) as p:
            outs = _run(hip, d)
        assert p.n > 0
        for o in outs:
            util.assert_finite(o, "%s under %r" % (name, value))
        _check(d, outs, (name, value))


def test_refusals_and_the_pack_contract(hip):
    w = lambda n, k: torch.randn(n, k, device=DEV)  # noqa: E731
    assert hip.token_linear_pack(w(64, 48), compute="f16") is None                  # K % 32 (fp32 takes it)
    assert hip.token_linear_pack(w(64, 48)) is not None
    p16, p32 = hip.token_linear_pack(w(64, 2080), compute="f16"), hip.token_linear_pack(w(64, 2080))
    assert p16.dtype == torch.float16 and p32.dtype == torch.float32 and p16.numel() * 2 < p32.numel() * 4
    x = torch.randn(16, 2080, device=DEV)
    assert hip.token_linear(x, p16, 64, norm=torch.nn.LayerNorm(2080).to(DEV), compute="f16") is None   # LayerNorm beyond K = 2048
    assert hip.token_linear(x, p16, 64, compute="f16") is not None
    p80 = hip.token_linear_pack(w(240, 64), compute="f16")
    assert hip.token_linear(torch.randn(16, 64, device=DEV), p80, 240, parts=3, compute="f16") is None    # 3 parts of 80 columns
    with pytest.raises(RuntimeError, match="pack"):
        hip.token_linear(x, p32, 64, compute="f16")
    with pytest.raises(RuntimeError, match="pack"):
        hip.token_linear(x, p16, 64)
    n0 = hip.launch_count()
    out = hip.token_linear(torch.empty(0, 2080, device=DEV), p16, 64, compute="f16")
    assert tuple(out.shape) == (0, 64) and hip.launch_count() == n0                   # no rows: the empty result, no launch


# ---- the SD transformer block with TOKEN_LINEAR on and the compute switched ----------------------------------------------------------
def _model():
    """tests/test_gpu_token_linear.py's model: 320 channels, 8 heads of 40, the 64 x 64 latent, 15 % edit, channels-last, in-place
    scatters."""
    from sige_amd.nn import SIGEModel
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads.sd_transformer import SpatialTransformer
    from tests.golden.model_init import init_by_name, sd_transformer_inputs

    class Wrap(SIGEModel):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x, **kw):
            return self.m(x, **kw)

    model = Wrap(SpatialTransformer(320, 8, 40, depth=1, context_dim=768, block_size=4, sparse_kv=True)).eval()
    init_by_name(model)
    x0, noise, ctx, mask512 = (t.to(DEV) for t in sd_transformer_inputs())
    model = model.to(DEV).to(memory_format=torch.channels_last)
    x0, noise = x0.contiguous(memory_format=torch.channels_last), noise.contiguous(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    masks = downsample_mask(mask512, min_res=8, dilation=1)
    x1 = (x0 + noise * masks[(64, 64)]).contiguous(memory_format=torch.channels_last)
    return model, x0, x1, ctx, masks


def test_sd_transformer_with_token_linear_f16(hip):
    """TOKEN_LINEAR on, TOKEN_LINEAR_COMPUTE "f16" against "f32": the full pass is untouched, the sparse pass differs within the f16
    criterion at the same launch count, and flipping the switch back re-packs (the fp32 bits return)."""
    from sige_amd import tolerance
    from sige_amd.workloads import sd_transformer as sdt

    model, x0, x1, ctx, masks = _model()
    keep = sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_COMPUTE

    def passes(compute):
        sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_COMPUTE = True, compute
        with torch.no_grad():
            model.set_mode("full")
            full = model(x0, context=ctx).clone()
            model.set_masks(masks)
            model.set_mode("sparse")
            model(x1, context=ctx)
            n0 = hip.launch_count()
            sparse = model(x1, context=ctx).clone()
        return full, sparse, hip.launch_count() - n0

    try:
        full32, sparse32, n32 = passes("f32")
        full16, sparse16, n16 = passes("f16")
        assert model.m.transformer_blocks[0].attn1._sige_tl_packed.dtype == torch.float16
        full_back, sparse_back, _ = passes("f32")
    finally:
        sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_COMPUTE = keep
    assert torch.equal(full32, full16) and torch.equal(full32, full_back)
    chk = tolerance.f16_check(sparse16, sparse32)
    util.record_margin("test_sd_transformer_with_token_linear_f16", "sparse f16 vs f32, worst over allowed", chk["worst_over_allowed"], 1.0)
    print(chk)
    assert chk["ok"], chk
    assert not torch.equal(sparse16, sparse32)
    assert n16 == n32 and n32 > 0
    assert torch.equal(sparse_back, sparse32)
