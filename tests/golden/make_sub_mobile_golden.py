#!/usr/bin/env python3
"""Generate tests/golden/gaugan_sub_mobile.npz from the REAL reference's GAN-Compression GauGAN generator (build container only:
the reference tree must be mounted).

    python tests/golden/make_sub_mobile_golden.py

gaugan/models/sub_mobile_spade_generators/sige_fused_sub_mobile_spade_generator.py::SIGEFusedSubMobileSPADEGenerator, unmodified,
on the reference's own sige.nn + its compiled sige/cpu backend (oracle/_ref); weights by tests/golden/sub_mobile_inputs.py::
init_weights (init_by_name, damped so that the tanh does not saturate), label maps by model_init.gaugan_labels, masks by the
gaugan/test.py recipe.  Groups (sub_mobile_inputs.GROUPS): small5/ and small7/ keep every 2nd pixel of the full and sparse outputs,
readme/ what model_init.summarize(step=4) keeps; all keep sums over every value, the sorted state-dict keys of the reference model,
the edit ratio and the active-tile counts per resolution.  The full pass does not depend on num_sparse_layers: small7/full is
bit-identical to small5/full and stored as an alias of it ("small7/full/alias"), which keeps the file under 512 KB.
"""
import argparse
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
from tests.golden import sub_mobile_inputs as inputs  # noqa: E402
from tests.golden.model_init import summarize  # noqa: E402

build_ref.build(REF, verbose=False)
ref_cpu = build_ref.load()
import sige  # noqa: E402

assert os.path.abspath(sige.__file__).startswith(REF), sige.__file__
sys.modules["sige.cpu"] = ref_cpu
sige.cpu = ref_cpu
from sige.utils import compute_difference_mask, dilate_mask, downsample_mask, reduce_mask  # noqa: E402

sys.path.insert(1, os.path.join(REF, "gaugan"))
from models.sub_mobile_spade_generators.sige_fused_sub_mobile_spade_generator import SIGEFusedSubMobileSPADEGenerator  # noqa: E402

torch.set_num_threads(8)
out = {}


def run(group: str):
    config_str, ngf, crop, _, k, step = inputs.GROUPS[group]
    opt = argparse.Namespace(ngf=ngf, semantic_nc=36, norm_G="spadesyncbatch3x3", num_upsampling_layers="more", main_block_size=6,
                             shortcut_block_size=4, num_sparse_layers=k, crop_size=crop, aspect_ratio=2,
                             separable_conv_norm="instance")
    config = {"channels": list(inputs.channels(config_str))}  # (what gaugan/utils.py decode_config returns)
    model = SIGEFusedSubMobileSPADEGenerator(opt, config).eval()
    inputs.init_weights(model)
    out[group + "/keys"] = np.array(sorted(model.state_dict().keys()))
    x0, x1 = inputs.labels(group)
    with torch.no_grad():
        model.set_mode("full")
        full = model(x0)
        diff = compute_difference_mask(x0, x1)
        masks = downsample_mask(dilate_mask(diff, 1), (model.sh, model.sw), dilation=2)  # gaugan/test.py recipe
        model.set_masks(masks)
        model.set_mode("sparse")
        sparse = model(x1)
        model.set_mode("full")
        dense_edit = model(x1)
    for name, t in (("full", full), ("sparse", sparse)):
        s = summarize(t, step=step or 4)
        out["%s/%s/sub" % (group, name)] = s["sub"]
        out["%s/%s/sums" % (group, name)] = np.array([s["sum"], s["abs_sum"]], dtype=np.float64)
        out["%s/%s/shape" % (group, name)] = np.array(s["shape"], dtype=np.int64)
        out["%s/%s/step" % (group, name)] = np.array([step or 4], dtype=np.int64)
    out[group + "/edit_ratio"] = np.array([float(diff.float().mean())])
    out[group + "/tiles"] = inputs.tile_counts(masks, reduce_mask)
    print("%s (%d keys, %.2fM params): edit ratio %.3f, out std %.3f, beyond 0.99 %.4f, |sparse - full| max %.3f, "
          "|sparse - dense(edited)| max %.1e, tiles %s"
          % (group, len(model.state_dict()), sum(p.numel() for p in model.parameters()) / 1e6, float(diff.float().mean()),
             float(sparse.std()), float((sparse.abs() > 0.99).float().mean()), float((sparse - full).abs().max()),
             float((sparse - dense_edit).abs().max()), out[group + "/tiles"].tolist()))


if __name__ == "__main__":
    import warnings

    warnings.simplefilter("ignore")
    for g in inputs.GROUPS:
        run(g)
    assert np.array_equal(out["small7/full/sub"], out["small5/full/sub"]) and np.array_equal(out["small7/full/sums"], out["small5/full/sums"])
    for k in ("sub", "sums", "shape", "step"):
        del out["small7/full/" + k]
    out["small7/full/alias"] = np.array("small5/full")
    path = os.path.join(HERE, "gaugan_sub_mobile.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
