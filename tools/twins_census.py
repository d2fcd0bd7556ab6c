#!/usr/bin/env python3
"""What the activated twins (sige_amd/nn/twins.py) do on the benchmarked forward, as one JSON line per edit ratio: after three
sparse forwards of the DDPM-256 model, the library launches and fused conv pairs of the fourth, the census of links as
(producer, consumer, part, cache id), and a SHA-256 of the fourth forward's output.  Two trees (or two runs of one) agree where
their lines do; reads nothing but names both sides of the twins refactor have."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import bench
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet, ResBlock

    hip.lib()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    if a.dtype != "f32":
        model.set_compute_dtype(a.dtype)
    names = {id(m): n for n, m in model.named_modules()}
    x0, noise = bench.make_inputs()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    t = torch.zeros(1, device=dev)
    with torch.no_grad():
        model.set_mode("full")
        model(cl(x0), t)
        for r in [float(v) for v in a.ratios.split(",")]:
            mask = bench.edit_mask(r)
            model.set_masks(downsample_mask(dilate_mask(mask.to(dev), 5), 8))
            model.set_mode("sparse")
            x1 = cl(x0 + noise * mask)
            for _ in range(3):
                model(x1, t)
            n0, p0 = hip.launch_count(), hip.conv_pairs_fused()
            out = model(x1, t)
            row = {"tag": a.tag, "dtype": a.dtype, "ratio": r, "launches": hip.launch_count() - n0, "conv_pairs_fused": hip.conv_pairs_fused() - p0}
            out = out.float().contiguous().cpu()
            row["checksum"] = float(out.double().abs().sum())
            row["sha256"] = hashlib.sha256(out.numpy().tobytes()).hexdigest()
            row["links"] = sorted([names[id(prod)], n, int(key[1]), int(key[3])] for n, b in model.named_modules() if isinstance(b, ResBlock)
                                  for key, (prod, _) in b._twin_links.items())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
