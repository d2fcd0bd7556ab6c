#!/usr/bin/env python3
"""Generate tests/golden/sd_vae_encoder.npz from the REAL reference's SD VAE encoder (build container only: the reference tree
must be mounted).

    python tests/golden/make_vae_encoder_golden.py

stable-diffusion/ldm/modules/diffusionmodules/sige_model.py::SIGEEncoder, unmodified, on the reference's own sige.nn + its
compiled sige/cpu backend (oracle/_ref), weights by tests/golden/model_init.py::init_by_name, inputs by
tests/golden/vae_encoder_inputs.py.  quant_conv is a plain nn.Conv2d(2z, 2z, 1) initialised the same way (SIGEAutoencoderKL
itself pulls in the training stack and is not imported).  Two groups:
  small/  the small configuration (middle block 192 channels wide), two cached steps (cache_id 0 / 1): per step the full forward
          on the original image and the sparse forward on the edited one -- encoder outputs and moments = quant_conv(output), whole;
  sd/     configs/sige.yaml's ddconfig: one step at image 128 x 128 (latent 16 x 16) as model_init.summarize() keeps it.
Both keep the sorted state-dict keys of the reference model, the edit ratio and the active-tile counts per resolution.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIGE_REFERENCE", "/root/reference")
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.append(REPO)
from oracle import build_ref  # noqa: E402
from tests.golden import vae_encoder_inputs as enc_inputs  # noqa: E402
from tests.golden.model_init import init_by_name, summarize  # noqa: E402

build_ref.build(REF, verbose=False)
ref_cpu = build_ref.load()
import sige  # noqa: E402

assert os.path.abspath(sige.__file__).startswith(REF), sige.__file__
sys.modules["sige.cpu"] = ref_cpu
sige.cpu = ref_cpu
from sige.utils import dilate_mask, downsample_mask, reduce_mask  # noqa: E402

# (ldm/modules/diffusionmodules/model.py imports numpy, torch and sige.nn only: no stub modules needed)
sys.path.insert(1, os.path.join(REF, "stable-diffusion"))
from ldm.modules.diffusionmodules.sige_model import SIGEEncoder  # noqa: E402

torch.set_num_threads(8)
out = {}


def run(group: str, cfg: dict, image: int, steps: int, whole: bool):
    model = SIGEEncoder(**cfg).eval()
    init_by_name(model)
    quant = enc_inputs.quant_conv(cfg)
    out[group + "/keys"] = np.array(sorted(model.state_dict().keys()))
    mask = enc_inputs.edit_mask(image)
    masks = enc_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)
    with torch.no_grad():
        for step in range(steps):
            x0, noise = enc_inputs.images(cfg, image, step)
            x1 = enc_inputs.edited(x0, noise, mask)
            model.set_cache_id(step)
            model.set_mode("full")
            full = model(x0)
            model.set_masks(masks)
            model.set_mode("sparse")
            sparse = model(x1)
            for name, t in (("full", full), ("sparse", sparse), ("full_moments", quant(full)), ("sparse_moments", quant(sparse))):
                if whole:
                    out["%s/%s%d" % (group, name, step)] = t.numpy().astype(np.float32)
                else:
                    s = summarize(t, step=1)  # (a 16 x 16 latent: every pixel)
                    out["%s/%s/sub" % (group, name)] = s["sub"]
                    out["%s/%s/sums" % (group, name)] = np.array([s["sum"], s["abs_sum"]], dtype=np.float64)
                    out["%s/%s/shape" % (group, name)] = np.array(s["shape"], dtype=np.int64)
            model.set_mode("full")
            dense_edit = model(x1)  # (overwrites this step's cache: nothing reads it again)
            print("%s step %d (%.1fM params): |sparse - full| max %.3f, |sparse - dense(edited)| max %.1e, |out| max %.2f"
                  % (group, step, sum(p.numel() for p in model.parameters()) / 1e6, float((sparse - full).abs().max()),
                     float((sparse - dense_edit).abs().max()), float(sparse.abs().max())))
    out[group + "/edit_ratio"] = np.array([float(mask.float().mean())])
    out[group + "/tiles"] = enc_inputs.tile_counts(masks, reduce_mask)


if __name__ == "__main__":
    import warnings

    warnings.simplefilter("ignore")
    run("small", enc_inputs.SMALL, 64, 2, True)
    run("sd", enc_inputs.SD, enc_inputs.SD_IMAGE, 1, False)
    path = os.path.join(HERE, "sd_vae_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
