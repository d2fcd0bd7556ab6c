"""The token linear's in-launch K split (hip.token_linear(ksplit=...): csrc/token_linear.hip, token_linear_f16.hip, the finish in
token_linear.hpp) against fp64 at the smallest shapes at which the split can go wrong, forced, in both computes; its refusals; and the
SD transformer block's switch (sd_transformer.TOKEN_LINEAR_KSPLIT)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.test_gpu_token_linear_f16 import _formula, _model, _worst, hip  # noqa: E402,F401  (the fp64 formula, the block, the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5

# name -> (M, N, K on fp32 operands, K on fp16 operands, forced ksplit, options).  A chunk is 64 channels (fp32) | 128 (f16); split s
# walks chunks [s cps, (s + 1) cps), cps = ceil(chunks / ksplit).  The f16 K where it differs keeps the chunk structure: 256 = one
# chunk per split; 640 = 5 chunks under ksplit 4 (cps 2: three splits, the last one chunk; at K = 320 the f16 unit has 3 chunks and
# refuses 4); K % 32 == 0 is the f16 unit's contract, so for K = 400 the two nearest: 416 (a last chunk with one live wave slice behind
# a whole one) and 288 (that chunk as the last split's whole share).
CASES = {
    "one_chunk_per_split_row_tail": (5, 64, 128, 256, 2, dict()),
    "uneven_k2": (48, 80, 320, 320, 2, dict()),
    "uneven_k4": (48, 80, 320, 640, 4, dict()),
    "k_tail_last_split": (21, 64, 336, 416, 2, dict()),
    "k_tail_alone": (21, 64, 144, 288, 2, dict()),
    "bias_residual": (48, 320, 1280, 1280, 4, dict(bias=True, res=True)),
    "ln_off12": (21, 80, 320, 320, 2, dict(ln=True, off=12.0)),
    "geglu_ln_bias": (48, 64, 320, 320, 2, dict(geglu=True, ln=True, bias=True)),
    "parts3": (21, 192, 320, 320, 2, dict(parts=3)),
    "deep_k8": (16, 64, 5120, 5120, 8, dict()),
}
_made = {}


def _case(name, compute):
    """Seeded CPU inputs of a case, the fp64 evaluation of the formula (tests/test_gpu_token_linear.py's) and, for fp16 operands, of
    the contract (prologue(x) and W through .half()), computed once per process."""
    if (name, compute) in _made:
        return _made[(name, compute)]
    m, n, k32, k16, ks, o = CASES[name]
    k = k32 if compute == "f32" else k16
    g = torch.Generator().manual_seed(3000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    geglu, parts = bool(o.get("geglu")), int(o.get("parts", 1))
    no = n // 2 if geglu else n // parts
    d = {"x": 3 * rn(m, k) + o.get("off", 0.0), "w": 0.08 * rn(n, k), "bias": rn(n) if o.get("bias") else None,
         "res": 3 * rn(m, no) if o.get("res") else None, "gamma": rn(k) if o.get("ln") else None, "beta": rn(k) if o.get("ln") else None,
         "geglu": geglu, "parts": parts, "N": n, "ksplit": ks}
    a = d["x"].double()
    if o.get("ln"):
        var, mean = torch.var_mean(a, dim=1, unbiased=False, keepdim=True)
        a = (a - mean) / torch.sqrt(var + EPS) * d["gamma"].double() + d["beta"].double()

    d["ref"] = _formula(d, a, d["w"].double())
    d["tight"] = 2e-5 * (1.0 + float(torch.cat(d["ref"], dim=1).abs().max()))  # fp32 accumulation against fp64 (test_token_linear_vs_fp64)
    d["tol"] = d["tight"]
    if compute == "f16":  # tests/test_gpu_token_linear_f16.py's rule for an unsplit launch
        emu = _formula(d, a.half().double(), d["w"].half().double())
        d["tol"] = max(4.0 * max(float((e - r).abs().max()) for e, r in zip(emu, d["ref"])), d["tight"])
    _made[(name, compute)] = d
    return d


def _run(hip, d, compute, ksplit, packed=None):
    """(pack +) one launch on the GPU -> (list of `parts` outputs or None, the pack)."""
    up = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    if packed is None:
        w = up(d["w"])
        packed = hip.token_linear_pack(list(w.chunk(d["parts"], dim=0)) if d["parts"] > 1 else w, geglu=d["geglu"], compute=compute)
        assert packed is not None
    norm = None
    if d["gamma"] is not None:
        norm = torch.nn.LayerNorm(d["x"].shape[1], eps=EPS).to(DEV)
        with torch.no_grad():
            norm.weight.copy_(d["gamma"])
            norm.bias.copy_(d["beta"])
    out = hip.token_linear(up(d["x"]), packed, d["N"], bias=up(d["bias"]), norm=norm, residual=up(d["res"]), geglu=d["geglu"],
                           parts=d["parts"], compute=compute, ksplit=ksplit)
    return (None if out is None else list(out) if isinstance(out, tuple) else [out]), packed


@pytest.mark.parametrize("compute", ["f32", "f16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_token_linear_ksplit_vs_fp64(hip, name, compute):
    """A forced split (a refusal fails) under NaN-poisoned allocations against fp64; against the unsplit launch of the same pack (the
    split changes the order of fp32 additions only); the same call twice gives the same bits (the ticket went back to 0, the slices
    are added in a fixed order); ksplit=1 through the new entry is the old entry's 16-token launch."""
    d = _case(name, compute)
    with util.poisoned(float("nan")) as p:
        outs, packed = _run(hip, d, compute, d["ksplit"])
    assert p.n > 0 and outs is not None, "the forced split was refused"
    for o, r in zip(outs, d["ref"]):
        assert tuple(o.shape) == tuple(r.shape) and bool(torch.isfinite(o).all()), name
    err = util.record_margin("test_token_linear_ksplit_vs_fp64", "%s %s" % (name, compute), _worst(outs, d["ref"]), d["tol"])
    plain, _ = _run(hip, d, compute, None, packed)
    gap = util.record_margin("test_token_linear_ksplit_vs_fp64", "%s %s vs unsplit" % (name, compute),
                             _worst(outs, [t.double().cpu() for t in plain]), d["tight"])
    print("%s %s: max |d| %.3g (bound %.3g), vs unsplit %.3g (bound %.3g)" % (name, compute, err, d["tol"], gap, d["tight"]))
    assert err <= d["tol"], (name, compute, err, d["tol"])
    assert gap <= d["tight"], (name, compute, gap, d["tight"])
    again, _ = _run(hip, d, compute, d["ksplit"], packed)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), name
    one, _ = _run(hip, d, compute, 1, packed)
    assert all(torch.equal(a, b) for a, b in zip(one, plain)), name


@pytest.mark.parametrize("compute", ["f32", "f16"])
def test_a_forced_split_that_cannot_run_is_refused_without_a_launch(hip, compute):
    d, deep = _case("uneven_k2", compute), _case("deep_k8", compute)  # 5 | 3 chunks; 80 | 40 chunks
    packed, deep_packed = _run(hip, d, compute, None)[1], _run(hip, deep, compute, None)[1]
    n0 = hip.launch_count()
    assert _run(hip, d, compute, 6, packed)[0] is None             # above the chunk count
    assert _run(hip, deep, compute, 17, deep_packed)[0] is None    # above the 16 slices a finish adds up
    assert hip.launch_count() == n0


def test_sd_transformer_with_token_linear_ksplit(hip):
    """One SpatialTransformer (tests/test_gpu_token_linear_f16.py's fixture, under a 64 x 64 pixel edit: its own mask gives 2016
    token rows) with TOKEN_LINEAR on: TOKEN_LINEAR_KSPLIT on -- the six launches through the split entry, under the library's rule --
    against off within the fp32 bound at the same launch count, and the off bits return when the switch is flipped back.  (At this
    block's 320 channels K is 1280 at most, where the measured rule does not split: DESIGN.md 5.32.)"""
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads import sd_transformer as sdt
    from tests.golden.model_init import sd_transformer_inputs

    model, x0, x1, ctx, _ = _model()
    mask512 = torch.zeros_like(sd_transformer_inputs()[3]).to(DEV)
    mask512[200:264, 200:264] = True
    masks = downsample_mask(mask512, min_res=8, dilation=1)
    x1 = (x0 + (x1 - x0) * masks[(64, 64)]).contiguous(memory_format=torch.channels_last)
    keep = sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_KSPLIT

    def sparse(on):
        sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_KSPLIT = True, on
        with torch.no_grad():
            model(x1, context=ctx)
            n0 = hip.launch_count()
            out = model(x1, context=ctx).clone()
        return out, hip.launch_count() - n0

    try:
        with torch.no_grad():
            model.set_mode("full")
            model(x0, context=ctx)
            model.set_masks(masks)
            model.set_mode("sparse")
        off, n_off = sparse(False)
        on, n_on = sparse(True)
        back, _ = sparse(False)
    finally:
        sdt.TOKEN_LINEAR, sdt.TOKEN_LINEAR_KSPLIT = keep
    tol = 2e-5 * (1.0 + float(off.abs().max()))
    err = util.record_margin("test_sd_transformer_with_token_linear_ksplit", "sparse on vs off", float((on - off).abs().max()), tol)
    print("switch on vs off: max |d| %.3g, bound %.3g" % (err, tol))
    assert err <= tol
    assert n_on == n_off and n_off > 0
    assert torch.equal(back, off)
