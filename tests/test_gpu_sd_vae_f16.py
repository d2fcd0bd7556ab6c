"""The SD VAE decoder and encoder in the f16 compute mode (SIGEModel.set_compute_dtype("f16"); sige_amd/workloads/sd_vae.py, DESIGN.md
5.28) on the GPU: channels-last tensors, in-place scatters, the fixture masks.

Two yardsticks per output.  (a) sige_amd.tolerance.f16_check against the fp32 GPU output -- the mode's stated tolerance, a hundred
times too loose to notice a broken attention or conv here.  (b) the emulation rule: within max(4 * e16, 2e-5 * (1 + max|ref|)) of the
fp32 CPU-oracle output `ref`, e16 the error of tests.vae_f16's emulation (fp16-rounded conv operands and attention, fp32 sums, on the
CPU oracle) against that same output, computed here.  Margins are recorded (util.record_margin; kept as
profiles/sd_vae_f16_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from sige_amd.tolerance import f16_check  # noqa: E402
from tests import test_sd_vae as dec  # noqa: E402
from tests import test_sd_vae_encoder as enc  # noqa: E402
from tests import util, vae_f16  # noqa: E402
from tests.golden import vae_encoder_inputs as enc_inputs  # noqa: E402
from tests.golden import vae_inputs  # noqa: E402
from tests.test_gpu_sd_vae import _attention_block_chain_ops  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
KINDS = ("decoder", "encoder")
SMALL = {"decoder": (vae_inputs.SMALL, 16), "encoder": (enc_inputs.SMALL, 64)}
REAL = {"decoder": (vae_inputs.SD, dec.SD_LATENT), "encoder": (enc_inputs.SD, enc_inputs.SD_IMAGE)}


class _attention:
    """sd_vae.ATTENTION_COMPUTE for the duration of a `with`."""

    def __init__(self, compute):
        from sige_amd.workloads import sd_vae

        self.mod, self.compute = sd_vae, compute

    def __enter__(self):
        self.keep = self.mod.ATTENTION_COMPUTE
        self.mod.ATTENTION_COMPUTE = self.compute
        return self

    def __exit__(self, *exc):
        self.mod.ATTENTION_COMPUTE = self.keep
        return False


def _setup(kind, cfg, size, dtype="f32"):
    """(model, forwards {name: fn(x)}, x0, x1, masks) on the GPU, channels-last, in-place scatters, `dtype` set before any forward."""
    if kind == "decoder":
        model = dec.build_model(cfg, "cuda", True, True)
        _, masks = dec.make_masks(cfg, size, "cuda")
        x0, x1 = dec.inputs(cfg, size, 0, masks, "cuda", True)
        fns = {"": model}
    else:
        model, quant = enc.build_model(cfg, "cuda", True, True)
        mask, masks = enc.make_masks(cfg, size, "cuda")
        x0, x1 = enc.inputs(cfg, size, 0, mask, "cuda", True)
        fns = {"": model, "_moments": lambda x: model.moments(x, quant)}
    if dtype != "f32":
        model.set_compute_dtype(dtype)
    return model, fns, x0, x1, masks


def _forwards(model, fns, x0, x1, masks, which=("full", "sparse")):
    """{"full", "sparse"[, "full_moments", "sparse_moments"]}: the fixture's sequence (tests.test_sd_vae.run_vae / run_encoder)."""
    out = {}
    with torch.no_grad():
        model.set_mode("full")
        for tag, fn in fns.items():
            full = fn(x0).clone()
            if "full" in which:
                out["full" + tag] = full
        model.set_masks(masks)
        model.set_mode("sparse")
        if "sparse" in which:
            for tag, fn in fns.items():
                with util.poisoned():
                    out["sparse" + tag] = fn(x1).clone()
    return out


def _gpu_outputs(kind, cfg, size, dtype="f32"):
    model, fns, x0, x1, masks = _setup(kind, cfg, size, dtype)
    return model, _forwards(model, fns, x0, x1, masks)


_ref = {}


def _oracle(kind, real=False):
    """(fp32 CPU-oracle outputs, their f16 emulation) of a model at a size: once per process, left unchanged."""
    key = (kind, real)
    if key not in _ref:
        cfg, size = (REAL if real else SMALL)[kind]
        _ref[key] = vae_f16.decoder_outputs(cfg, size) if kind == "decoder" else vae_f16.encoder_outputs(cfg, size)
    return _ref[key]


def _inside_bound(test, kind, name, got, real=False):
    ref, emu = _oracle(kind, real)
    e16 = vae_f16.err(emu[name], ref[name])
    tol = vae_f16.bound(ref[name], e16)
    err = vae_f16.err(got.cpu(), ref[name])
    print("%s %s %s: err %.3e vs the fp32 oracle, emulation %.3e, bound %.3e" % (test, kind, name, err, e16, tol))
    util.record_margin("test_gpu_sd_vae_f16 %s" % test, "%s %s vs oracle" % (kind, name), err, tol)
    assert err <= tol, "%s %s: max |diff| %.3e > bound %.3e (emulation %.3e)" % (kind, name, err, tol, e16)


def _check_small_f32(kind, outs):
    record = lambda what, value, tol: util.record_margin("test_gpu_sd_vae_f16 f32 %s" % kind, what, value, tol)  # noqa: E731
    if kind == "decoder":
        dec.check_small([(outs["full"], outs["sparse"])], util.CONV_ATOL, record)
    else:
        enc.check_small([outs], util.CONV_ATOL, record)


@pytest.mark.parametrize("kind", KINDS)
def test_f16_mode_against_the_fp32_outputs_and_the_emulation(kind):
    """Point 1: sparse and full (the encoder's moments() too) in f16 mode pass f16_check against the fp32 GPU outputs -- which pass the
    fixture --, lie within the emulation bound of the fp32 CPU oracle, and are not the fp32 bits."""
    cfg, size = SMALL[kind]
    _, out32 = _gpu_outputs(kind, cfg, size)
    _check_small_f32(kind, out32)
    model, out16 = _gpu_outputs(kind, cfg, size, "f16")
    assert model.compute_policy == {"dtype": "f16", "keep": ()}
    assert set(out16) == set(out32) and len(out16) == (2 if kind == "decoder" else 4)
    for name in sorted(out16):
        util.assert_finite(out16[name], "%s %s in f16 mode" % (kind, name))
        chk = f16_check(out16[name], out32[name])
        print("%s %s f16 vs f32: %s" % (kind, name, chk))
        util.record_margin("test_gpu_sd_vae_f16 f16_check", "%s %s worst / allowed" % (kind, name), chk["worst_over_allowed"], 1.0)
        assert chk["ok"], (kind, name, chk)
        assert not torch.equal(out16[name], out32[name]), "%s %s: the mode changed nothing" % (kind, name)
        _inside_bound("f16", kind, name, out16[name])


@pytest.mark.parametrize("kind", KINDS)
def test_attention_switch_inside_f16_mode(kind):
    """Point 2: ATTENTION_COMPUTE "f16" against "f32" with every conv in f16 -- the same library launch count, outputs that differ, both
    inside the emulation bound, and no torch bmm / softmax / copy kernel in the block either way."""
    from sige_amd import hip
    from sige_amd.workloads import sd_vae

    cfg, size = SMALL[kind]
    model, fns, x0, x1, masks = _setup(kind, cfg, size, "f16")
    _forwards(model, fns, x0, x1, masks)  # (full pass, masks, the first sparse forward: packs and buffers)
    outs, launches = {}, {}
    for compute in ("f32", "f16"):
        with _attention(compute), torch.no_grad():
            assert model.mid.attn_1.attention_compute() == compute
            model(x1)
            n0 = hip.launch_count()
            with util.poisoned():
                outs[compute] = model(x1).clone()
            launches[compute] = hip.launch_count() - n0
            assert _attention_block_chain_ops(model, x1) == []
    assert sd_vae.ATTENTION_COMPUTE is None
    print("%s f16 mode: %d library launches with either attention" % (kind, launches["f16"]))
    assert launches["f16"] == launches["f32"] and launches["f32"] > 0
    assert not torch.equal(outs["f16"], outs["f32"]), "the switch changed nothing"
    for compute in ("f32", "f16"):
        util.assert_finite(outs[compute], "%s sparse, attention %s" % (kind, compute))
        _inside_bound("attention %s" % compute, kind, "sparse", outs[compute])


def _sparse(model, fns, x1):
    """{"sparse"[, "sparse_moments"]} of the model as it stands: masks set, sparse mode, the caches of the last full pass."""
    with torch.no_grad():
        return {"sparse" + tag: fn(x1).clone() for tag, fn in fns.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_the_derived_kv_conv_follows_the_mode_and_leaves_no_stale_pack(kind):
    """Point 3: folded_kv()'s conv reports "f16" after set_compute_dtype("f16") and "f32" after set_compute_dtype("f32"); the fp32
    forward afterwards equals the fp32 forward before, bit for bit.

    The forwards compared are SPARSE forwards over the caches of ONE fp32 full pass: before the round trip, in f16 mode, and back in
    fp32.  A new full pass per mode cannot be compared this way -- the fp32 full pass runs the GEMM / conv libraries' kernels and does
    not repeat bit for bit from one call to the next without any mode change (measured on an MI355X: max |diff| 1.8e-7 between two
    fp32 full passes in a row, 2.1e-7 in the sparse outputs over their caches) --, while the sparse forward over fixed caches is the
    library's own launches and does repeat (asserted first, so that a failure of the premise reads as one)."""
    cfg, size = SMALL[kind]
    model, fns, x0, x1, masks = _setup(kind, cfg, size)
    attn = model.mid.attn_1
    _forwards(model, fns, x0, x1, masks)  # (the one full pass, masks, a first sparse forward: packs and buffers)
    before = _sparse(model, fns, x1)
    again = _sparse(model, fns, x1)
    for name in sorted(before):
        assert torch.equal(again[name], before[name]), "%s %s: the fp32 sparse forward does not repeat" % (kind, name)
    assert attn.folded_kv().compute_dtype == "f32"
    tiles = torch.randn(8, attn.ch, 4, 4, generator=torch.Generator().manual_seed(3)).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        kv_before = attn.folded_kv()(tiles).clone()
    model.set_compute_dtype("f16")
    assert attn.folded_kv().compute_dtype == "f16" and attn.attention_compute() == "f16"
    half = _sparse(model, fns, x1)
    assert attn.folded_kv().compute_dtype == "f16"
    with torch.no_grad():
        assert not torch.equal(attn.folded_kv()(tiles), kv_before)
    for name in sorted(before):
        util.assert_finite(half[name], "%s %s in f16 mode over fp32 caches" % (kind, name))
        assert not torch.equal(half[name], before[name]), "%s %s: the mode changed nothing" % (kind, name)
    model.set_compute_dtype("f32")
    assert attn.folded_kv().compute_dtype == "f32" and attn.attention_compute() == "f32"
    after = _sparse(model, fns, x1)
    with torch.no_grad():
        assert torch.equal(attn.folded_kv()(tiles), kv_before), "the derived K | V conv reads a stale pack"
    for name in sorted(before):
        assert torch.equal(after[name], before[name]), "%s %s: fp32 after f16 is not fp32 before" % (kind, name)


@pytest.mark.parametrize("kind", KINDS)
def test_stacked_edits_in_f16_mode(kind):
    """Point 4: E = 2 stacked edits in f16 mode -- each image's output against its own single-edit f16 forward (util.SELF_ATOL) and
    against the fp32 oracle of that edit within the emulation bound of this model (the fixture mask's e16: the edits are the
    stacked tests' two ~5 % rectangles, the first of them the fixture's)."""
    from sige_amd import hip, stacked
    from tests import test_gpu_sd_vae_stacked as S

    E = 2
    want = S.oracle_outputs(kind)
    model, run = S.build(kind, "cuda", True, True)
    model.set_compute_dtype("f16")
    pyrs = S.pyramids(kind, "cuda")[:E]
    x0, edits, noise = S.edit_inputs(kind, pyrs, "cuda")
    x0, edits = S._fmt(x0, True), [S._fmt(x, True) for x in edits[:E]]
    nz = (lambda e: None) if noise is None else (lambda e: noise[e])
    with torch.no_grad():
        model.set_mode("full")
        run(x0, nz(0))
        model.set_mode("sparse")
        singles = []
        for e in range(E):
            model.set_masks(pyrs[e])
            run(edits[e], nz(e))
            singles.append(run(edits[e], nz(e)).clone())
        xs = S._fmt(torch.cat(edits, 0), True)
        ns = None if noise is None else torch.cat(noise[:E], 0)
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                run(xs, ns)
                calls, orig = [], hip.attention_wide

                def counted(*a, **kw):
                    calls.append((kw.get("tiles") is not None, kw.get("compute")))
                    return orig(*a, **kw)

                hip.attention_wide = counted
                try:
                    with util.poisoned():
                        got = run(xs, ns).clone()
                finally:
                    hip.attention_wide = orig
        finally:
            stacked.unstack_caches(model)
    assert calls == [(True, "f16")], calls  # ONE attention launch: the per-image form, fp16 operands
    util.assert_finite(got, "stacked f16 output")
    ref, emu = _oracle(kind)
    name = "sparse" if kind == "decoder" else "sparse_moments"
    e16 = vae_f16.err(emu[name], ref[name])
    for e in range(E):
        own = float((got[e] - singles[e][0]).abs().max())
        err = float((got[e].cpu() - want[e]).abs().max())
        tol = vae_f16.bound(want[e], e16)
        print("sd_vae f16 %s E=%d edit %d: vs single %.3e, vs oracle %.3e (bound %.3e)" % (kind, E, e, own, err, tol))
        util.record_margin("test_gpu_sd_vae_f16 stacked vs single", "%s edit %d" % (kind, e), own, util.SELF_ATOL)
        util.record_margin("test_gpu_sd_vae_f16 stacked vs oracle", "%s edit %d" % (kind, e), err, tol)
        assert own <= util.SELF_ATOL, (e, own)
        assert err <= tol, (e, err, tol)


@pytest.mark.parametrize("kind", KINDS)
def test_f16x3_mode_stays_inside_the_fp32_tolerance(kind):
    """Point 5: set_compute_dtype("f16x3") runs and passes the fixture at 1e-3; its attention is the fp32 form."""
    cfg, size = SMALL[kind]
    model, outs = _gpu_outputs(kind, cfg, size, "f16x3")
    assert model.mid.attn_1.attention_compute() == "f32" and model.mid.attn_1.folded_kv().compute_dtype == "f16x3"
    for name in sorted(outs):
        util.assert_finite(outs[name], "%s %s in f16x3 mode" % (kind, name))
    record = lambda what, value, tol: util.record_margin("test_gpu_sd_vae_f16 f16x3 %s" % kind, what, value, tol)  # noqa: E731
    if kind == "decoder":
        dec.check_small([(outs["full"], outs["sparse"])], 1e-3, record)
    else:
        enc.check_small([outs], 1e-3, record)


@pytest.mark.parametrize("kind", KINDS)
def test_real_configuration_in_f16_mode(kind):
    """Point 6: the real configuration (as test_real_configuration_on_the_gpu_matches_the_reference_fixture sizes it), once, in f16:
    the emulation bound against the CPU oracle at that size, the emulation run there; f16_check against the oracle as well."""
    cfg, size = REAL[kind]
    model, outs = _gpu_outputs(kind, cfg, size, "f16")
    assert model.mid.attn_1.ch == 512 and model.mid.attn_1.attention_compute() == "f16"
    ref, _ = _oracle(kind, True)
    for name in sorted(outs):
        util.assert_finite(outs[name], "%s %s, real configuration, f16 mode" % (kind, name))
        chk = f16_check(outs[name].cpu(), ref[name])
        util.record_margin("test_gpu_sd_vae_f16 real f16_check", "%s %s worst / allowed" % (kind, name), chk["worst_over_allowed"], 1.0)
        assert chk["ok"], (kind, name, chk)
        _inside_bound("real", kind, name, outs[name], real=True)
