#!/usr/bin/env python3
"""Progressive Distillation U-Net (church_pd128-sige.yml) on the MI355X: fp32, channels-last, hipGraph replay.

    python tools/pd_bench.py            -> profiles/pd128_bench.json

Per edit ratio (1.2 / 5 / 15 %), in ONE child process so that the comparison stays inside one session:
  (a) the sparse forward;
  (b) the same forward with the resampling blocks forced onto the torch-op chain (pd_unet.FUSED_RESAMPLE = False) -- (b) - (a) is
      what sige_hip_resample_tiles_nhwc_f32 is worth;
  (c) the dense forward on MIOpen (set_plain_dense): the figure to set beside the reference's dense / sparse ratio.
Timing: HIP events around `--steps` replays, after warm-up replays; (a) and (b) alternate batch by batch, the edited image in the
graph's input buffer changes from batch to batch, the medians over `--batches` batches are reported.  Also: library launches of
(a), and the kernel alone per resampling block (a graph of `--reps` identical launches: its sources are cache-resident, so the
bytes/s is NOT an HBM figure), with the bytes the algorithm needs from the shapes, against 8 TB/s.

The parent process never touches the GPU: it starts one child per ratio under `timeout -k 10` and stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_HBM_BYTES = 8.0e12


def square_mask(size, ratio):
    import torch

    e = max(1, int(round(size * ratio ** 0.5)))
    m = torch.zeros(size, size, dtype=torch.bool)
    top, left = size // 3, size // 4
    m[top:top + e, left:left + e] = True
    return m


def events_ms(graph, steps, warm):
    import torch

    for _ in range(warm):
        graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def kernel_rows(model, reps, steps):
    """The kernel alone, per tiled resampling block, on that block's shapes and index list."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.workloads.pd_unet import PDResBlock

    rows = []
    for name, blk in model.named_modules():
        if not (isinstance(blk, PDResBlock) and blk.resample and blk.sparse_main and blk._res_buf is not None):
            continue
        g, res = blk.main_gather, blk._res_buf
        B, C, Ho, Wo = res.shape
        H, W = (2 * Ho, 2 * Wo) if blk.resample == "down" else (Ho // 2, Wo // 2)
        x = torch.randn(B, C, H, W, device=res.device).contiguous(memory_format=torch.channels_last)
        idx = g.indices_on(res.device)
        N = idx.shape[0]
        s1, t1 = blk.affine[blk.cache_id][:2]
        scratch = torch.empty_like(res)
        geo = dict(res=scratch, offset=tuple(g.offset), stride=tuple(g.model_stride), cells=tuple(g.out_tile))
        if blk.resample == "down":
            fn = lambda: [hip.resample_tiles(x, "down", idx, tuple(g.block_size), s1, t1, **geo) for _ in range(reps)]  # noqa: E731
            need = N * C * 4 * (12 * 12 + 36 + 16)  # the 12x12 source window of a tile, its 36 tile and 16 shortcut pixels
        else:
            fn = lambda: [hip.resample_tiles(x, "up", idx, None, **geo) for _ in range(reps)]  # noqa: E731
            need = N * C * 4 * (4 + 16)             # 2x2 source pixels, 16 shortcut pixels
        graph, _ = capture_fn(fn)
        us = statistics.median(events_ms(graph, steps, 3) for _ in range(5)) * 1e3 / reps
        rows.append({"block": name, "mode": blk.resample, "C": C, "source": [H, W], "tiles": N, "us": round(us, 3), "bytes_needed": need,
                     "bytes_per_s": round(need / (us * 1e-6), 1), "of_8TBs": round(need / (us * 1e-6) / PEAK_HBM_BYTES, 4)})
    return rows


def child(a):
    import torch

    from benchlib.common import capture
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import pd_unet

    hip.lib()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = pd_unet.PDConfig()
    model = pd_unet.PDSparseUNet(cfg).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g)
    noises = [torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g) for _ in range(4)]
    logsnr = torch.zeros(1, device=dev)
    mask = square_mask(cfg.image_size, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    with torch.no_grad():
        model.set_mode("full")
        model(cl(x0), logsnr)
        masks = downsample_mask(dilate_mask(mask.to(dev), 2), cfg.image_size // 2 ** (len(cfg.ch_mult) - 1))
        model.set_masks(masks)
        model.set_mode("sparse")
        edits = [cl(x0 + n * mask) for n in noises]
        x1 = edits[0].clone()
        graphs, outs = {}, {}
        for name, fused in (("a_sparse", True), ("b_sparse_torch_resample", False)):
            pd_unet.FUSED_RESAMPLE = fused
            model(x1, logsnr)
            n0 = hip.launch_count()
            model(x1, logsnr)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture(model, x1, logsnr)
        pd_unet.FUSED_RESAMPLE = True
        ms = {k: [] for k in graphs}
        for batch in range(a.batches):
            x1.copy_(edits[batch % len(edits)])  # (another edited image in the graphs' input buffer)
            for name in (list(graphs) if batch % 2 == 0 else list(graphs)[::-1]):
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        # (a capture runs nothing: the outputs hold values only after a replay -- both graphs last ran on the same image)
        row["a_minus_b_max_abs"] = float((outs["a_sparse"] - outs["b_sparse_torch_resample"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["resample_kernel"] = kernel_rows(model, a.reps, a.steps)
        del graphs
        # (c) the stock dense network on MIOpen, on the edited image
        model.set_mode("full")
        model.set_plain_dense(True)
        gd, _ = capture(model, x1, logsnr)
        kd = max(10, a.steps // 4)
        row["c_dense_miopen_ms"] = round(statistics.median(events_ms(gd, kd, 3) for _ in range(5)), 4)
        row["dense_over_sparse"] = round(row["c_dense_miopen_ms"] / row["a_sparse_ms"], 3)
    print("PD_BENCH_ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--ratio", type=float, default=None, help="(child) one ratio, on the GPU")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pd128_bench.json"))
    a = ap.parse_args()
    if a.ratio is not None:
        return child(a)
    from sige_amd import build

    res = {"workload": "church_pd128-sige.yml, fp32, channels-last, hipGraph replay, default-initialised weights (seed 0)",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    for r in a.ratios.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ratio", r, "--steps", str(a.steps),
               "--batches", str(a.batches), "--reps", str(a.reps)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith("PD_BENCH_ROW ")), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"ratio": r, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        res["rows"].append(json.loads(line[len("PD_BENCH_ROW "):]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
