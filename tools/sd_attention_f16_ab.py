"""The SD U-Net's sparse forward in the f16 compute mode (bench.py --workload sd --dtype f16: same model, latent, context, mask;
SIGEModel.set_compute_dtype("f16")) with the attention on exact fp32 products or on fp16 operands
(sd_transformer.ATTENTION_COMPUTE "f32" / "f16"), hipGraph replay each, alternating, in one process.  Every setting runs its own full
pass first (the switch applies there too); every output is held against the all-fp32 model's by the f16 criterion.

    python tools/sd_attention_f16_ab.py --out profiles/sd_attention_f16_ab.json
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from benchlib.common import _replay_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="f32,f16,f32,f16")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sige_amd import hip
    from sige_amd.tolerance import f16_check
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads import sd_transformer
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet

    dev = torch.device("cuda:0")
    hip.lib()
    torch.manual_seed(0)
    model = SDUNet(SDConfig()).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    gen = torch.Generator().manual_seed(1)
    cl = lambda t_: t_.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    x0, noise = cl(torch.randn(2, 4, 64, 64, generator=gen)), cl(torch.randn(2, 4, 64, 64, generator=gen))
    ctx = torch.randn(2, 77, 768, generator=gen).to(dev)
    ts = torch.full((2,), 500.0, device=dev)
    mask512 = torch.zeros(512, 512, dtype=torch.bool, device=dev)
    mask512[150:348, 120:318] = True
    masks = downsample_mask(mask512, min_res=8, dilation=1)
    x1 = cl(x0 + noise * masks[(64, 64)])
    run = lambda x: model(x, ts, context=ctx)  # noqa: E731

    def prepare():
        model.set_mode("full")
        run(x0)
        model.set_masks(masks)
        model.set_mode("sparse")

    rows = []
    keep = sd_transformer.ATTENTION_COMPUTE
    try:
        with torch.no_grad():
            sd_transformer.ATTENTION_COMPUTE = "f32"
            model.set_compute_dtype("f32")
            prepare()
            ref = run(x1).float().clone()
            model.set_compute_dtype("f16")
            for st in args.settings.split(","):
                sd_transformer.ATTENTION_COMPUTE = st
                prepare()
                run(x1)
                n0 = hip.launch_count()
                run(x1)
                launches = hip.launch_count() - n0
                ms, out, g = _replay_ms(lambda: run(x1), k=args.replays, warm=3)
                o = out.float().clone()
                del g
                rows.append({"attention_compute": st, "forward_ms": round(ms, 3), "library_launches": launches,
                             "f16_check_vs_fp32_model": f16_check(o, ref)})
                print(json.dumps(rows[-1]), flush=True)
    finally:
        sd_transformer.ATTENTION_COMPUTE = keep
    res = {"workload": "bench.py --workload sd --dtype f16 (SD v1 U-Net, latent [2,4,64,64], 15 % edit), hipGraph replay", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
