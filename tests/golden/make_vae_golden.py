#!/usr/bin/env python3
"""Generate tests/golden/sd_vae_decoder.npz from the REAL reference's SD VAE decoder (build container only: the reference tree
must be mounted).

    python tests/golden/make_vae_golden.py [--sd-outputs]

stable-diffusion/ldm/modules/diffusionmodules/sige_model.py::SIGEDecoder, unmodified, on the reference's own sige.nn + its
compiled sige/cpu backend (oracle/_ref), weights by tests/golden/model_init.py::init_by_name, inputs by tests/golden/vae_inputs.py.
Two groups:
  small/  the small configuration (middle block 192 channels wide), two cached latents (cache_id 0 / 1): per step the full
          forward on the original latent and the sparse forward on the edited one, whole outputs;
  sd/     configs/sige.yaml's ddconfig: the sorted state-dict keys always; with --sd-outputs also one step at latent 64 x 64 as
          model_init.summarize() keeps it (every 4th pixel of both outputs + sums over all values).
Both keep the sorted state-dict keys of the reference model; groups with outputs also the edit ratio and the active-tile counts
per resolution.
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
from tests.golden import vae_inputs  # noqa: E402
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
from ldm.modules.diffusionmodules.sige_model import SIGEDecoder  # noqa: E402

torch.set_num_threads(8)
out = {}


def run(group: str, cfg: dict, latent: int, steps: int, whole: bool):
    model = SIGEDecoder(**cfg).eval()
    init_by_name(model)
    out[group + "/keys"] = np.array(sorted(model.state_dict().keys()))
    if steps == 0:
        return
    size = vae_inputs.image_size(cfg, latent)
    mask = vae_inputs.edit_mask(size)
    masks = vae_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)
    with torch.no_grad():
        for step in range(steps):
            z0, noise = vae_inputs.latents(cfg, latent, step)
            z1 = vae_inputs.edited(z0, noise, masks)
            model.set_cache_id(step)
            model.set_mode("full")
            full = model(z0)
            model.set_masks(masks)
            model.set_mode("sparse")
            sparse = model(z1)
            for name, t in (("full", full), ("sparse", sparse)):
                if whole:
                    out["%s/%s%d" % (group, name, step)] = t.numpy().astype(np.float32)
                else:
                    s = summarize(t)
                    out["%s/%s/sub" % (group, name)] = s["sub"]
                    out["%s/%s/sums" % (group, name)] = np.array([s["sum"], s["abs_sum"]], dtype=np.float64)
                    out["%s/%s/shape" % (group, name)] = np.array(s["shape"], dtype=np.int64)
            model.set_mode("full")
            dense_edit = model(z1)  # (overwrites this step's cache: nothing reads it again)
            print("%s step %d (%.1fM params): |sparse - full| max %.3f, |sparse - dense(edited)| max %.1e, |out| max %.2f"
                  % (group, step, sum(p.numel() for p in model.parameters()) / 1e6, float((sparse - full).abs().max()),
                     float((sparse - dense_edit).abs().max()), float(sparse.abs().max())))
    out[group + "/edit_ratio"] = np.array([float(mask.float().mean())])
    out[group + "/tiles"] = vae_inputs.tile_counts(masks, reduce_mask)


if __name__ == "__main__":
    import warnings

    warnings.simplefilter("ignore")
    run("small", vae_inputs.SMALL, 16, 2, True)
    run("sd", vae_inputs.SD, 64, 1 if "--sd-outputs" in sys.argv else 0, False)
    path = os.path.join(HERE, "sd_vae_decoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
