"""The SD U-Net's sparse forward (bench.py --workload sd: same model, latent, context) with the token linears of its transformer
blocks on the library's token GEMM (sd_transformer.TOKEN_LINEAR: six launches per block, LayerNorm / bias / GEGLU / residual folded in)
or on the GEMM libraries plus the five helper launches, hipGraph replay each, alternating, in one process -- under the benchmarked mask
and under one whose token counts the shipped TunableOp table does not hold.  One session per TunableOp setting: the table is off
unless --tuned is given (a process-wide PyTorch setting).

    python tools/sd_token_linear_ab.py --out out/sd_token_linear.json
    python tools/sd_token_linear_ab.py --tuned --out out/sd_token_linear_tuned.json
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from benchlib.common import _replay_ms  # noqa: E402

MASKS = {"bench": (150, 348, 120, 318), "other": (100, 260, 200, 440)}  # rows, columns of the 512 x 512 edit mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="0,1,0,1")
    ap.add_argument("--masks", default="bench,other")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--tuned", action="store_true", help="TunableOp on with the shipped table (sige_amd/workloads/gemm_tuning.py)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sige_amd import hip
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads import gemm_tuning, sd_transformer
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet

    dev = torch.device("cuda:0")
    hip.lib()
    tuned = bool(args.tuned and gemm_tuning.enable_tuned_gemms())
    if args.tuned and not tuned:
        raise SystemExit("the TunableOp table was rejected by this stack")
    torch.manual_seed(0)
    model = SDUNet(SDConfig()).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    gen = torch.Generator().manual_seed(1)
    cl = lambda t_: t_.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    x0, noise = cl(torch.randn(2, 4, 64, 64, generator=gen)), cl(torch.randn(2, 4, 64, 64, generator=gen))
    ctx = torch.randn(2, 77, 768, generator=gen).to(dev)
    ts = torch.full((2,), 500.0, device=dev)
    run = lambda x: model(x, ts, context=ctx)  # noqa: E731
    res = {"workload": "bench.py --workload sd (SD v1 U-Net, latent [2,4,64,64]), hipGraph replay", "tunableop_table": tuned, "masks": {}}
    keep = sd_transformer.TOKEN_LINEAR
    try:
        with torch.no_grad():
            for name in args.masks.split(","):
                model.set_mode("full")  # (the caches of the original image, fresh for every mask)
                run(x0)
                r0, r1, c0, c1 = MASKS[name]
                mask512 = torch.zeros(512, 512, dtype=torch.bool, device=dev)
                mask512[r0:r1, c0:c1] = True
                masks = downsample_mask(mask512, min_res=8, dilation=1)
                x1 = cl(x0 + noise * masks[(64, 64)])
                model.set_masks(masks)
                model.set_mode("sparse")
                rows, ref = [], None
                for st in args.settings.split(","):
                    sd_transformer.TOKEN_LINEAR = bool(int(st))
                    run(x1)
                    n0 = hip.launch_count()
                    run(x1)
                    launches = hip.launch_count() - n0
                    ms, out, g = _replay_ms(lambda: run(x1), k=args.replays, warm=3)
                    o = out.float().clone()
                    del g
                    if ref is None:
                        ref = o
                    rows.append({"mask": name, "token_linear": bool(int(st)), "forward_ms": round(ms, 3), "library_launches": launches,
                                 "max_abs_vs_first_setting": round(float((o - ref).abs().max()), 8)})
                    print(json.dumps(rows[-1]), flush=True)
                res["masks"][name] = {"box": MASKS[name], "edit_ratio": round(float(mask512.float().mean()), 4), "rows": rows}
    finally:
        sd_transformer.TOKEN_LINEAR = keep
        if tuned:
            gemm_tuning.disable_tuned_gemms()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
