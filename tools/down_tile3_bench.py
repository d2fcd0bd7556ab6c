#!/usr/bin/env python3
"""The stride-2 Downsample conv on the tile conv v3, fp16 operands against what the same call takes today -- the
exact-fp32 ConvGeo<3, 2, 5, *> launch of conv_mfma.hpp, which is what f16 mode runs for this geometry -- on the MI355X.
Writes profiles/down_tile3_bench.json.  (The forward A/B: tools/vae_encoder_bench.py --dtype f16 --down-tile3.)

launch / launch_stacked: the launch alone.  The three Downsample convs of the SD VAE encoder (128 ch from 512^2, 256 ch from 256^2,
512 ch from 128^2; offset 0) and of the SD U-Net (320 / 640 / 1280 ch from 64^2 / 32^2 / 16^2; padding 1) under square edits of
1.2 / 5 / 15 % of the image, and (launch_stacked) E = 8 stacked edits of 5 %, as hip.gather_conv_cl(..., down3=pack) with
hip.DOWN_TILE3_MIN_BLOCKS_F16 = 1 beside the same call with down3=None.  Each a hipGraph of 20 back-to-back launches between HIP
events, the two alternating `--batches` times; median and [min, max].

launch_crossover: the three VAE-encoder shapes with the 15 % list cut to the tile counts that make 40 / 48 / 56 / 64 workgroups: where
between the largest measured loss and the smallest measured win the two launches cross.

The parent never touches the GPU: one child per job under `timeout -k 10`, and it stops at the first child that fails.

    python tools/down_tile3_bench.py [--jobs launch,launch_stacked,launch_crossover]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "down_tile3_bench.json")
TAG = "DOWN_TILE3_ROW "
JOBS = ["launch", "launch_stacked", "launch_crossover"]
# (workload, channels, input edge, image edge, mask dilation, offset of the window origins)
SHAPES = [("sd_vae_encoder", 128, 512, 512, 2, 0), ("sd_vae_encoder", 256, 256, 512, 2, 0), ("sd_vae_encoder", 512, 128, 512, 2, 0),
          ("sd_unet", 320, 64, 512, 2, 1), ("sd_unet", 640, 32, 512, 2, 1), ("sd_unet", 1280, 16, 512, 2, 1)]


def _stat(v):
    return round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]


def child_launch(a, E, grids=(None,)):
    import torch

    from benchlib.common import time_graph_of
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, reduce_mask
    from tests.golden import vae_inputs

    hip.lib()
    dev = torch.device("cuda")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    rows = []
    hip.DOWN_TILE3_MIN_BLOCKS_F16 = 1
    hip.set_edit_batch(E)
    try:
        for workload, C, r, image, dil, off in (SHAPES if grids == (None,) else SHAPES[:3]):
            for ratio, grid in ([(0.15, k) for k in grids] if grids != (None,) else [(q, None) for q in ((0.05,) if E > 1 else (0.012, 0.05, 0.15))]):
                g = torch.Generator().manual_seed(C + r)
                m = dilate_mask(vae_inputs.square_mask(image, ratio).to(dev), dil)
                if r != image:  # the level's mask: any edited pixel under a cell
                    m = torch.nn.functional.max_pool2d(m[None, None].float(), image // r)[0, 0] > 0
                idx = reduce_mask(m.repeat(E, 1), 5, 4, off)  # (stacked edits: the same edit in every image, stacked along H)
                if grid is not None:  # (the first tiles of the list: grid = ceil(N / 8) x (C / 64) workgroups)
                    idx = idx[:8 * grid // (C // 64)].contiguous()
                N = int(idx.shape[0])
                x, out = cl(torch.randn(1, C, E * r, r, generator=g)), cl(torch.randn(1, C, E * r // 2, r // 2, generator=g))
                w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
                bias = torch.randn(C, generator=g).to(dev)
                packed = hip.conv_pack_weights(w, 5, 5, (2, 2), "f16")  # (exact fp32 for this geometry: .compute says so)
                d3 = hip.down_tile3_pack(w)
                full = dict(offset=(off, off), out_res=(E * r // 2, r // 2), residual=None)

                def call(pk):
                    return hip.gather_conv_cl(x, None, (5, 5), idx, None, None, "identity", packed, bias, C, (3, 3), (2, 2), full=full,
                                              out=out, down3=pk)

                real, seen = hip.lib().sige_hip_down_tile3_nhwc, []

                def spy(*args):
                    seen.append(int(real(*args)))
                    return seen[-1]

                hip.lib().sige_hip_down_tile3_nhwc = spy
                try:
                    call(d3)
                finally:
                    hip.lib().sige_hip_down_tile3_nhwc = real
                new, old = [], []
                for i in range(a.batches):
                    for name in (("n", "o") if i % 2 == 0 else ("o", "n")):
                        (new if name == "n" else old).append(time_graph_of((lambda: call(d3)) if name == "n" else (lambda: call(None)), 20))
                un, mmn = _stat(new)
                uo, mmo = _stat(old)
                flop = 2.0 * N * 4 * C * C * 9
                rows.append({"workload": workload, "C": C, "in_res": r, "E": E, "ratio": ratio, "tiles": N, "today_pack_compute": packed.compute,
                             "workgroups_new": -(-N // 8) * (C // 64), "new_entry_point_status": seen,
                             "new_us": un, "new_us_min_max": mmn, "today_us": uo, "today_us_min_max": mmo, "new_over_today": round(un / uo, 3),
                             "ranges_apart": bool(mmn[1] < mmo[0]), "new_TFLOPs": round(flop / un / 1e6, 1), "today_TFLOPs": round(flop / uo / 1e6, 1)})
                print("launch E%d %s C%d from %d^2 %.3f: %d tiles %d workgroups  new %.2f us %s  today %.2f us %s" % (
                    E, workload, C, r, ratio, N, rows[-1]["workgroups_new"], un, mmn, uo, mmo), file=sys.stderr, flush=True)
    finally:
        hip.set_edit_batch(1)
    print(TAG + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default=",".join(JOBS))
    ap.add_argument("--child", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("down_tile3_bench: needs the GPU (no timing is taken anywhere else)")
        if a.child == "launch_crossover":
            return child_launch(a, 1, (40, 48, 56, 64)) or 0
        return child_launch(a, 8 if a.child == "launch_stacked" else 1) or 0
    from sige_amd import build

    code = 0
    for job in a.jobs.split(","):
        path = a.out
        res = {}
        if os.path.isfile(path):
            with open(path) as f:
                res = json.load(f)
        res.update({"method": "hipGraph replay between HIP events; new and today alternate batch by batch, medians and [min, max] over "
                              "%d batches; graphs of 20 back-to-back launches, weights L2-warm" % a.batches,
                    "source_hash": build.source_hash()})
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", job, "--steps", str(a.steps),
               "--batches", str(a.batches)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-6000:])
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": job, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            code = 1
        else:
            res.pop("failed", None)
            res[job] = json.loads(line[len(TAG):])
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        if code:
            break
    return code


if __name__ == "__main__":
    sys.exit(main())
