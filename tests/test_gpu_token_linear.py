"""The token linear (csrc/token_linear.hip: LayerNorm -> x . W^T -> bias / GEGLU / residual / q | k | v parts in one launch) against
fp64, under poisoned allocations, and as the SD transformer block's opt-in path (sd_transformer.TOKEN_LINEAR)."""
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


def _bound(ref):
    """Exact-fp32 MFMA products against fp64: the project's bound (test_attention_tokens_vs_fp64, test_gpu_attention_keyfold.py)."""
    return 2e-5 * (1.0 + float(ref.abs().max()))


# name -> (M, N, K, options).  N is the width of the product (2 D for GEGLU, 3 x one output for parts = 3).  The library picks the
# 64-token form where its ceil(M / 64) * ceil(N / 64) workgroups fill at least 0.8 of their rounds of 512 with real rows
# (csrc/token_linear.hip: kTokSlots), else the 16-token form: the "w64" cases take the 64-token form, with row, column and channel
# tails of their own; every other case takes the 16-token form.
def _cases():
    c = {}
    for m, n, k in ((5, 64, 64), (16, 64, 64), (48, 80, 320), (208, 320, 1280), (16, 64, 5120), (2016, 320, 320)):
        for epi in ("plain", "bias", "bias_res"):
            c["%s_%dx%dx%d" % (epi, m, n, k)] = (m, n, k, dict(bias=epi != "plain", res=epi == "bias_res"))
    for k in (64, 320, 1280):
        for off in (0.0, 12.0):  # row means of 0 and of 4 sigma
            c["ln_k%d_off%d" % (k, off)] = (208, 80, k, dict(ln=True, bias=True, off=off))
    for d in (32, 160, 1280):
        c["geglu_d%d" % d] = (208 if d == 1280 else 48, 2 * d, 320, dict(geglu=True, bias=True))
    c["geglu_d32_res_nobias"] = (5, 64, 64, dict(geglu=True, res=True))
    for n1 in (64, 320):
        c["parts3_n%d" % n1] = (208, 3 * n1, 320, dict(parts=3))
    c["parts2_n128"] = (48, 256, 64, dict(parts=2, bias=True))
    c["ln_parts3"] = (208, 3 * 320, 320, dict(ln=True, parts=3, off=12.0))
    c["ln_geglu"] = (208, 2 * 1280, 320, dict(ln=True, geglu=True, bias=True, off=12.0))
    # the 64-token form: 32 x 16 = 512, 29 x 15 = 435, 29 x 16 = 464, 8 x 64 = 512 workgroups; M % 64, N % 64 and K % 64 tails
    c["w64_plain"] = (2021, 976, 336, dict())
    c["w64_bias_res"] = (2021, 976, 336, dict(bias=True, res=True))
    c["w64_ln_parts3"] = (1829, 3 * 320, 320, dict(ln=True, parts=3, off=12.0))
    c["w64_ln_geglu"] = (1829, 2 * 512, 336, dict(ln=True, geglu=True, bias=True, off=12.0))
    c["w64_ln_k64"] = (500, 4096, 64, dict(ln=True, bias=True, res=True))
    c["w64_ln_k1280"] = (2000, 1024, 1280, dict(ln=True, off=12.0))  # (the statistics' looped form at 4 lanes per row)
    return c


CASES = _cases()
_made = {}


def _case(name):
    """Seeded CPU inputs of a case and its fp64 reference (a list of `parts` tensors), computed once per process."""
    if name in _made:
        return _made[name]
    m, n, k, o = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    geglu, parts = bool(o.get("geglu")), int(o.get("parts", 1))
    no = n // 2 if geglu else n // parts
    d = {"x": 3 * rn(m, k) + o.get("off", 0.0), "w": 0.08 * rn(n, k), "bias": rn(n) if o.get("bias") else None,
         "res": 3 * rn(m, no) if o.get("res") else None, "gamma": rn(k) if o.get("ln") else None, "beta": rn(k) if o.get("ln") else None,
         "geglu": geglu, "parts": parts, "N": n}
    a = d["x"].double()
    if o.get("ln"):
        var, mean = torch.var_mean(a, dim=1, unbiased=False, keepdim=True)
        a = (a - mean) / torch.sqrt(var + EPS) * d["gamma"].double() + d["beta"].double()
    r = a @ d["w"].double().t()
    if d["bias"] is not None:
        r = r + d["bias"].double()
    if geglu:
        v, gate = r.chunk(2, dim=1)
        r = v * F.gelu(gate)
    if d["res"] is not None:
        r = d["res"].double() + r
    d["ref"] = list(r.chunk(parts, dim=1))
    _made[name] = d
    return d


def _run(hip, d):
    """pack + one launch on the GPU -> list of `parts` outputs."""
    up = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    w = up(d["w"])
    packed = hip.token_linear_pack(list(w.chunk(d["parts"], dim=0)) if d["parts"] > 1 else w, geglu=d["geglu"])
    assert packed is not None
    norm = None
    if d["gamma"] is not None:
        norm = torch.nn.LayerNorm(d["x"].shape[1], eps=EPS).to(DEV)
        with torch.no_grad():
            norm.weight.copy_(d["gamma"])
            norm.bias.copy_(d["beta"])
    out = hip.token_linear(up(d["x"]), packed, d["N"], bias=up(d["bias"]), norm=norm, residual=up(d["res"]), geglu=d["geglu"],
                           parts=d["parts"])
    assert out is not None
    return list(out) if isinstance(out, tuple) else [out]


def _worst(outs, refs):
    return max(float((o.double().cpu() - r).abs().max()) for o, r in zip(outs, refs))


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


@pytest.mark.parametrize("name", sorted(CASES))
def test_token_linear_vs_fp64(hip, name):
    """One launch against the fp64 evaluation of the same formula, |d| <= 2e-5 (1 + max |ref|); two calls give the same bits."""
    d = _case(name)
    outs = _run(hip, d)
    for o, r in zip(outs, d["ref"]):
        assert tuple(o.shape) == tuple(r.shape)
        util.assert_finite(o, name)
    tol = _bound(torch.cat(d["ref"], dim=1))
    err = util.record_margin("test_token_linear_vs_fp64", name, _worst(outs, d["ref"]), tol)
    print("%s: max |d| %.3g, bound %.3g" % (name, err, tol))
    assert err <= tol, (name, err, tol)
    again = _run(hip, d)
    assert all(torch.equal(p, q) for p, q in zip(outs, again)), name


@pytest.mark.parametrize("value", [float("nan"), 1e30])
def test_token_linear_under_poisoned_allocations(hip, value):
    """Every allocation (uploads, packed weights, outputs) pre-filled with NaN / 1e30: the row tails at M = 5 / 208 / 2021, the column
    tails at N = 80 / 976, the zero padding of the packed weights and the dead channel slices of K % 64 != 0 must not let any of it
    into a result."""
    for name in sorted(CASES):
        d = _case(name)
        with util.poisoned(value) as p:
            outs = _run(hip, d)
        assert p.n > 0
        for o in outs:
            util.assert_finite(o, "%s under %r" % (name, value))
        tol = _bound(torch.cat(d["ref"], dim=1))
        err = _worst(outs, d["ref"])
        assert err <= tol, (name, value, err, tol)


def test_unsupported_shapes_return_none(hip):
    w = lambda n, k: torch.randn(n, k, device=DEV)  # noqa: E731
    assert hip.token_linear_pack(w(64, 24)) is None                 # K % 16
    assert hip.token_linear_pack(w(10, 64)) is None                 # N % 16
    assert hip.token_linear_pack(w(80, 64), geglu=True) is None     # GEGLU with D = 40
    assert hip.token_linear_pack(w(80, 64)) is not None
    packed = hip.token_linear_pack(w(64, 2064))
    assert packed is not None
    x = torch.randn(16, 2064, device=DEV)
    assert hip.token_linear(x, packed, 64, norm=torch.nn.LayerNorm(2064).to(DEV)) is None    # LayerNorm beyond K = 2048
    assert hip.token_linear(x, packed, 64) is not None
    p80 = hip.token_linear_pack(w(240, 64))
    assert hip.token_linear(torch.randn(16, 64, device=DEV), p80, 240, parts=3) is None       # 3 parts of 80 columns
    # no rows: the empty result, no launch
    n0 = hip.launch_count()
    out = hip.token_linear(torch.empty(0, 2064, device=DEV), packed, 64)
    assert tuple(out.shape) == (0, 64) and hip.launch_count() == n0


# ---- the SD transformer block with the switch on ----------------------------------------------------------------------------------
class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.workloads import sd_transformer as sdt

        self.sdt, self.keep = sdt, sdt.TOKEN_LINEAR
        sdt.TOKEN_LINEAR = self.on

    def __exit__(self, *exc):
        self.sdt.TOKEN_LINEAR = self.keep
        return False


def _model():
    """tests.test_models_golden._sd_transformer("cuda", True, True)'s model after its full pass, with its inputs: 320 channels, 8 heads
    of 40, the 64 x 64 latent, 15 % edit, channels-last, in-place scatters."""
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
    with torch.no_grad():
        model.set_mode("full")
        model(x0, context=ctx)
        model.set_masks(masks)
        model.set_mode("sparse")
    return model, x0, x1, ctx


@pytest.mark.oracle_parity
def test_sd_transformer_with_token_linear(hip):
    """Switch on against switch off (the full pass is untouched: identical; the sparse pass: the same products in another summation
    order, the bound test_sd_transformer_native_attention_and_linears holds the tile-kernel linears to) and against the reference's
    fixture."""
    from tests.test_models_golden import _check, _sd_transformer

    with _switch(False):
        full0, sparse0 = _sd_transformer(DEV, True, True)
    with _switch(True):
        n0 = hip.launch_count()
        full1, sparse1 = _sd_transformer(DEV, True, True)
        assert hip.launch_count() > n0
    assert torch.equal(full0, full1)
    err = util.record_margin("test_sd_transformer_with_token_linear", "sparse on vs off", float((sparse1 - sparse0).abs().max()), 2e-4)
    print("sparse, switch on vs off: max |d| %.3g" % err)
    assert err <= 2e-4
    _check("sdt/full", full1)
    _check("sdt/sparse", sparse1, 1e-3)


def test_no_aten_gemm_left_in_the_block(hip):
    """A sparse forward under a TorchDispatchMode (tools/torch_ops_probe.py): with the switch on no matrix product, LayerNorm or
    GELU is an aten op any more; the block runs 6 library launches in place of the 5 helpers between its GEMMs."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Log(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    model, _, x1, ctx = _model()
    found, launches = {}, {}
    for on in (False, True):
        with _switch(on), torch.no_grad():
            for _ in range(2):
                model(x1, context=ctx)
            log = Log()
            n0 = hip.launch_count()
            with log:
                model(x1, context=ctx)
            launches[on] = hip.launch_count() - n0
            found[on] = sorted({n for n in log.names if any(k in n for k in ("mm", "matmul", "linear", "layer_norm", "gelu"))})
    assert found[True] == [], found[True]
    assert found[False], "the switch-off forward was expected to run its GEMMs through aten"
    blocks = len(model.m.transformer_blocks)
    assert launches[True] == launches[False] + blocks, launches


def test_packed_weights_follow_the_parameters(hip):
    """The packed copies are plain attributes (the state dict keeps the reference's keys) and an in-place update of a weight re-packs."""
    model, _, x1, ctx = _model()
    keys = list(model.state_dict().keys())
    with torch.no_grad():
        with _switch(True):
            before = model(x1, context=ctx).clone()
            assert torch.equal(model(x1, context=ctx), before)
        assert list(model.state_dict().keys()) == keys
        blk = model.m.transformer_blocks[0]
        assert blk.attn1._sige_tl_packed is not None and blk.ff.net[2]._sige_tl_packed is not None
        blk.attn2.to_q.weight.mul_(2)
        with _switch(True):
            after = model(x1, context=ctx).clone()
        with _switch(False):
            want = model(x1, context=ctx).clone()
    assert float((after - before).abs().max()) > 1e-3
    err = float((after - want).abs().max())
    print("after to_q.weight.mul_(2), switch on vs off: max |d| %.3g" % err)
    assert err <= 2e-4
    assert list(model.state_dict().keys()) == keys


def test_token_linear_forward_replays_from_a_graph(hip):
    """The switch-on sparse forward captured after warm-up: a replay returns the eager bits, for the captured input and for another."""
    model, x0, x1, ctx = _model()
    with _switch(True), torch.no_grad():
        eager1 = model(x1, context=ctx).clone()
        eager0 = model(x0, context=ctx).clone()
        assert not torch.equal(eager0, eager1)
        xin = x1.clone(memory_format=torch.channels_last)
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(xin, context=ctx)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                captured = model(xin, context=ctx)
        torch.cuda.current_stream().wait_stream(s)
        for x, want in ((x0, eager0), (x1, eager1)):
            xin.copy_(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, want)
        del g


@pytest.mark.oracle_parity
def test_sd_unet_with_token_linear(hip):
    """The whole SD U-Net (16 transformer blocks at four widths, 8 x 8 to 64 x 64 tokens) with the switch on, against the fixture."""
    from tests.test_models_golden import _check, _sd_unet

    with _switch(True):
        n0 = hip.launch_count()
        full, sparse = _sd_unet(DEV, True, True)
        assert hip.launch_count() > n0
    _check("sdunet/full", full)
    _check("sdunet/sparse", sparse, 1e-3)
