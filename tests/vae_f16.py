"""The f16 compute mode of the SD VAE models (sige_amd/workloads/sd_vae.py) WITHOUT a GPU: the emulation, the
model-level bound of tests/test_gpu_sd_vae_f16.py, and the error trace.  No test lives here.

    python -m tests.vae_f16 [--per-layer R] [--out profiles/sd_vae_f16_error_trace.json]

The method is tests/f16_error_trace.py's.  Both models run on the CPU oracle backend with `init_by_name` weights; "f16 compute" is
emulated where the GPU kernels apply it:
  * the input (after the cached GroupNorm affine + SiLU) and the weights of every ELIGIBLE conv are rounded to fp16, nearest even,
    products and sums stay fp32 -- tests.f16_error_trace.Emulator, imported.  Eligible (`eligible`): every 3x3 / stride-1 and 1x1
    conv but `conv_in` / `conv_out` -- the residual blocks, their shortcuts, q / k / v / proj_out, the Upsample conv.  Not eligible,
    as on the GPU: conv_in, conv_out (the decoder's conv3x3_small_cout_cl head, the encoder's latent head), the stride-2
    Downsample conv; quant_conv is not part of the model.
  * the attention of a SPARSE forward (`chain16`): q, k, v and the probabilities rounded to fp16, scores, softmax state and the
    sums fp32, l from the unrounded probabilities -- the contract of sige_hip_attention_tokens_f16c.  The full-mode attention stays
    on the fp32 chain, as on the GPU.

Model-level bound (`bound`): max(4 * e16, 2e-5 * (1 + max|ref|)), ref the fp32 CPU-oracle output and e16 the emulation's error against
it -- the project's rule (tests/attention_f16.py) one level up: another blocking or summation order of the same roundings.

The trace: both models, the real size at 1.2 / 5 / 15 % (`square_mask`; the encoder's 5 % row is the fixture mask), the small size on
the fixture mask; per row the max |diff| from the fp32 sparse output and the worst element's share of the tolerance.f16_check
allowance; with --per-layer R one conv (or the attention) at a time at the real size and ratio R."""
import argparse
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.f16_error_trace import Emulator, f16_eligible  # noqa: E402

SD_LATENT, SD_IMAGE, SMALL_LATENT, SMALL_IMAGE = 64, 512, 16, 64
ATTENTION = "<attention>"  # the name of the attention launch in a set of active layers


def r16(t):
    return t.half().float()


def eligible(name: str, conv) -> bool:
    """The convs the f16 mode runs on the fp16 tile / dense kernels (section 4 of the module docstring above)."""
    return f16_eligible(name, conv)


def chain16(self, q, k, v):
    """VAEAttnBlock._chain under the f16c contract: q [b,nq,c] tokens, k / v [b,c,h,w] -> [b,c,nq]."""
    b, c, h, w = k.shape
    s = torch.bmm(r16(q), r16(k.reshape(b, c, h * w))) * (int(c) ** (-0.5))
    p = torch.exp(s - s.max(dim=2, keepdim=True).values)
    l = p.sum(dim=2, keepdim=True)                                    # (the unrounded probabilities)
    o = torch.bmm(r16(v.reshape(b, c, h * w)), r16(p).permute(0, 2, 1))
    return o / l.permute(0, 2, 1)


class VAEEmulator:
    """f16 compute of `model` (SparseVAEDecoder / SparseVAEEncoder on the CPU oracle backend), switched with set_active()."""

    def __init__(self, model):
        from sige_amd.workloads.sd_vae import VAEAttnBlock

        self.model = model
        self.emu = Emulator(model)
        assert all(eligible(n, m) for n, m in self.emu.convs.items())
        self.attention = False
        self.layers = list(self.emu.convs) + [ATTENTION]
        for m in model.modules():
            if isinstance(m, VAEAttnBlock):
                m._chain = types.MethodType(self._chain_of(type(m)._chain), m)

    def _chain_of(self, plain):
        emulator = self

        def chain(block, q, k, v):
            if emulator.attention and block.mode == "sparse":
                return chain16(block, q, k, v)
            return plain(block, q, k, v)
        return chain

    def set_active(self, names):
        """`names`: conv names and / or ATTENTION; True = every layer, () = the fp32 model."""
        names = self.layers if names is True else list(names)
        self.attention = ATTENTION in names
        self.emu.set_active([n for n in names if n != ATTENTION])


def bound(ref, e16):
    return max(4.0 * float(e16), 2e-5 * (1.0 + float(ref.abs().max())))


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def _on_oracle(fn):
    from oracle import oracle
    from sige_amd import runtime

    n = min(32, os.cpu_count() or 1)
    torch.set_num_threads(n)
    oracle.set_num_threads(n)
    runtime.register_backend("cpu", oracle)
    try:
        with torch.no_grad():
            return fn()
    finally:
        runtime.unregister_backend("cpu")


# ---- the two models on the CPU oracle: {name: tensor} of the fp32 model and of the emulation -------------------------------------------
def _decoder_masks(cfg, latent, ratio):
    from sige_amd.utils import dilate_mask, downsample_mask
    from tests.golden import vae_inputs

    size = vae_inputs.image_size(cfg, latent)
    mask = vae_inputs.edit_mask(size) if ratio is None else vae_inputs.square_mask(size, ratio)
    return vae_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)


def decoder_outputs(cfg, latent, ratio=None, active=True, model=None):
    """({"full", "sparse"} fp32, the same emulated with `active` layers in f16) of SparseVAEDecoder on the fixture's inputs of step 0;
    `ratio` None: the fixture mask, else a centred square.  As a forward in f16 mode, the emulated full pass fills the caches."""
    from tests import test_sd_vae as T

    def run():
        m = model or T.build_model(cfg, "cpu", False)
        emu = m.__dict__.get("_vae_f16_emulator") or VAEEmulator(m)
        m.__dict__["_vae_f16_emulator"] = emu
        masks = _decoder_masks(cfg, latent, ratio)
        z0, z1 = T.inputs(cfg, latent, 0, masks, "cpu", False)
        outs = []
        for names in ((), active):
            emu.set_active(names)
            try:
                m.set_mode("full")
                full = m(z0).clone()
                m.set_masks(masks)
                m.set_mode("sparse")
                outs.append({"full": full, "sparse": m(z1).clone()})
            finally:
                emu.set_active(())
        return tuple(outs)
    return _on_oracle(run)


def encoder_outputs(cfg, image, ratio=None, active=True, model=None, moments=True):
    """As decoder_outputs for SparseVAEEncoder: {"full", "sparse"[, "full_moments", "sparse_moments"]}."""
    from sige_amd.utils import dilate_mask, downsample_mask
    from tests import test_sd_vae_encoder as T
    from tests.golden import vae_encoder_inputs as enc_inputs
    from tests.golden import vae_inputs

    def run():
        m, quant = model or T.build_model(cfg, "cpu", False)
        emu = m.__dict__.get("_vae_f16_emulator") or VAEEmulator(m)
        m.__dict__["_vae_f16_emulator"] = emu
        mask = enc_inputs.edit_mask(image) if ratio is None else vae_inputs.square_mask(image, ratio)
        masks = enc_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)
        x0, x1 = T.inputs(cfg, image, 0, mask, "cpu", False)
        outs = []
        for names in ((), active):
            emu.set_active(names)
            try:
                m.set_mode("full")
                got = {"full": m(x0).clone()}
                if moments:
                    got["full_moments"] = m.moments(x0, quant).clone()
                m.set_masks(masks)
                m.set_mode("sparse")
                got["sparse"] = m(x1).clone()
                if moments:
                    got["sparse_moments"] = m.moments(x1, quant).clone()
                outs.append(got)
            finally:
                emu.set_active(())
        return tuple(outs)
    return _on_oracle(run)


def _row(ref, emu):
    from sige_amd import tolerance

    c = tolerance.f16_check(emu["sparse"], ref["sparse"])
    return {"max_abs_diff": err(emu["sparse"], ref["sparse"]), "worst_over_allowed": c["worst_over_allowed"], "ok": bool(c["ok"]),
            "full_max_abs_diff": err(emu["full"], ref["full"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-layer", type=float, default=0.0, help="edit ratio of the one-layer-at-a-time trace at the real size (0 = skip)")
    ap.add_argument("--out", default="profiles/sd_vae_f16_error_trace.json")
    args = ap.parse_args()

    from sige_amd import tolerance
    from tests import test_sd_vae as TD
    from tests import test_sd_vae_encoder as TE
    from tests.golden import vae_encoder_inputs as enc_inputs
    from tests.golden import vae_inputs

    report = {"weights": "tests.golden.model_init.init_by_name (no checkpoint)", "criterion": tolerance.F16_CRITERION, "decoder": {}, "encoder": {}}
    rows = [("small, fixture mask", vae_inputs.SMALL, SMALL_LATENT, None)] + [("sd, %g" % r, vae_inputs.SD, SD_LATENT, r) for r in (0.012, 0.05, 0.15)]
    models = {}
    for what, cfg, latent, ratio in rows:
        key = id(cfg)
        models[key] = models.get(key) or TD.build_model(cfg, "cpu", False)
        report["decoder"][what] = _row(*decoder_outputs(cfg, latent, ratio, model=models[key]))
        print("decoder", what, report["decoder"][what], flush=True)
    sd_decoder = models[id(vae_inputs.SD)]
    rows = [("small, fixture mask", enc_inputs.SMALL, SMALL_IMAGE, None)] + [("sd, %s" % ("fixture mask" if r is None else "%g" % r), enc_inputs.SD, SD_IMAGE, r)
                                                                            for r in (0.012, None, 0.15)]
    models = {}
    for what, cfg, image, ratio in rows:
        key = id(cfg)
        models[key] = models.get(key) or TE.build_model(cfg, "cpu", False)
        report["encoder"][what] = _row(*encoder_outputs(cfg, image, ratio, model=models[key], moments=False))
        print("encoder", what, report["encoder"][what], flush=True)
    if args.per_layer > 0:
        r = args.per_layer
        report["per_layer_at"] = r
        for name, fn, model, size, cfg in (("decoder", decoder_outputs, sd_decoder, SD_LATENT, vae_inputs.SD),
                                           ("encoder", encoder_outputs, models[id(enc_inputs.SD)], SD_IMAGE, enc_inputs.SD)):
            emu = model[0].__dict__["_vae_f16_emulator"] if isinstance(model, tuple) else model.__dict__["_vae_f16_emulator"]
            contrib = {}
            for layer in emu.layers:
                kw = {} if name == "decoder" else {"moments": False}
                ref, one = fn(cfg, size, r, active=[layer], model=model, **kw)
                contrib[layer] = tolerance.f16_check(one["sparse"], ref["sparse"])["worst_over_allowed"]
                print("%s %-40s worst/allowed %.5f" % (name, layer, contrib[layer]), flush=True)
            report[name]["per_layer_worst_over_allowed"] = contrib
    if args.out:
        with open(os.path.join(REPO, args.out), "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
