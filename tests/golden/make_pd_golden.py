#!/usr/bin/env python3
"""Generate tests/golden/pd_unet.npz from the REAL reference's Progressive Distillation U-Net (build container only: the
reference tree must be mounted).

    python tests/golden/make_pd_golden.py

diffusion/models/pd_arch/sige_unet.py::SIGEUNet on the reference's own sige.nn + its compiled sige/cpu backend (oracle/_ref),
weights by tests/golden/model_init.py::init_by_name, inputs by tests/golden/pd_inputs.py.  Two groups:
  small/  the small configuration, two cached steps (cache_id 0 / 1, two logsnr values): per step the full forward on the
          original and the sparse forward on the edited image, whole outputs;
  pd128/  church_pd128-sige.yml, one step: every 4th pixel of both outputs + sums over all values.
Both keep the edit ratio, the active-tile counts per resolution and the sorted state-dict keys of the reference model.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIGE_REFERENCE", "/root/reference")
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.append(REPO)
from oracle import build_ref  # noqa: E402
from tests.golden import pd_inputs  # noqa: E402
from tests.golden.model_init import init_by_name, summarize  # noqa: E402

build_ref.build(REF, verbose=False)
ref_cpu = build_ref.load()
import sige  # noqa: E402

assert os.path.abspath(sige.__file__).startswith(REF), sige.__file__
sys.modules["sige.cpu"] = ref_cpu
sige.cpu = ref_cpu
from sige.utils import dilate_mask, downsample_mask, reduce_mask  # noqa: E402

sys.path.insert(1, os.path.join(REF, "diffusion"))
from models.pd_arch.sige_unet import SIGEUNet  # noqa: E402

torch.set_num_threads(8)
out = {}


def config(cfg: dict):
    """The fields SIGEUNet.__init__ reads, as the namespace the YAML loader would build."""
    model = types.SimpleNamespace(**{k: v for k, v in cfg.items() if k != "image_size"})
    model.sige_block_size = types.SimpleNamespace(**pd_inputs.BLOCKS)
    return types.SimpleNamespace(data=types.SimpleNamespace(image_size=cfg["image_size"]), model=model)


def run(group: str, cfg: dict, steps: int, whole: bool):
    model = SIGEUNet(None, config(cfg)).eval()
    init_by_name(model)
    size = cfg["image_size"]
    x0, noise = pd_inputs.images(size)
    mask = pd_inputs.edit_mask(size)
    x1 = x0 + noise * mask
    masks = pd_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)
    with torch.no_grad():
        for step in range(steps):
            logsnr = torch.full((1,), pd_inputs.LOGSNR[step])
            model.set_cache_id(step)
            model.set_mode("full")
            full = model(x0, logsnr)
            model.set_masks(masks)
            model.set_mode("sparse")
            sparse = model(x1, logsnr)
            model.set_mode("full")
            dense_edit = model(x1, logsnr)  # (overwrites this step's cache: nothing reads it again)
            for name, t in (("full", full), ("sparse", sparse)):
                if whole:
                    out["%s/%s%d" % (group, name, step)] = t.numpy().astype(np.float32)
                else:
                    s = summarize(t)
                    out["%s/%s/sub" % (group, name)] = s["sub"]
                    out["%s/%s/sums" % (group, name)] = np.array([s["sum"], s["abs_sum"]], dtype=np.float64)
                    out["%s/%s/shape" % (group, name)] = np.array(s["shape"], dtype=np.int64)
            print("%s step %d (%.1fM params): |sparse - full| max %.3f, |sparse - dense(edited)| max %.1e, |out| max %.2f"
                  % (group, step, sum(p.numel() for p in model.parameters()) / 1e6, float((sparse - full).abs().max()),
                     float((sparse - dense_edit).abs().max()), float(sparse.abs().max())))
    out[group + "/edit_ratio"] = np.array([float(mask.float().mean())])
    out[group + "/tiles"] = pd_inputs.tile_counts(masks, reduce_mask)
    out[group + "/keys"] = np.array(sorted(model.state_dict().keys()))


if __name__ == "__main__":
    import warnings

    warnings.simplefilter("ignore")
    run("small", pd_inputs.SMALL, 2, True)
    run("pd128", pd_inputs.PD128, 1, False)
    path = os.path.join(HERE, "pd_unet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
