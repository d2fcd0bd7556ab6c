#!/usr/bin/env python3
"""Progressive Distillation U-Net (church_pd128-sige.yml) on the MI355X: fp32, channels-last, hipGraph replay.

    python tools/pd_bench.py            -> profiles/pd128_bench.json
    python tools/pd_bench.py --stacked  -> profiles/pd_stacked_bench.json: stacked edits (sige_amd/stacked.py), see below

Per edit ratio (1.2 / 5 / 15 %), in ONE child process so that the comparison stays inside one session:
  (a) the sparse forward;
  (b) the same forward with the resampling blocks forced onto the torch-op chain (pd_unet.FUSED_RESAMPLE = False) -- (b) - (a) is
      what sige_hip_resample_tiles_nhwc_f32 is worth;
  (c) the dense forward on MIOpen (set_plain_dense): the figure to set beside the reference's dense / sparse ratio.
Timing: HIP events around `--steps` replays, after warm-up replays; (a) and (b) alternate batch by batch, the edited image in the
graph's input buffer changes from batch to batch, the medians over `--batches` batches are reported.  Also: library launches of
(a), and the kernel alone per resampling block (a graph of `--reps` identical launches: its sources are cache-resident, so the
bytes/s is NOT an HBM figure), with the bytes the algorithm needs from the shapes, against 8 TB/s.

--stacked, in the protocol of `tools/vae_bench.py --stacked`: per ratio, in ONE child process, two models with the same weights (those
of the test fixtures, tests/golden/model_init.py: well conditioned, so that max |stacked - single| means something); one stays on
single edits, the other is stacked for E = 2, 4, 8 in turn (E edited versions of the same original under the same square, another
noise per edit).  Both forwards are hipGraphs; the stacked and the single-edit graph alternate batch by batch, the
edited inputs in the graphs' buffers change from batch to batch; medians over `--batches` batches.  `speedup` = E x the single-edit
time OF THE SAME RUN over the stacked time.  Also: library launches, max |stacked - single| per edit after both graphs replayed on
the same inputs, and once per run, in a child of its own, the tiled DOWN launch of hip.resample_tiles ALONE at E = 8 (the first
downsample block's shapes: 64 channels, 128 x 128 -> 64 x 64 per image, the tiles of each ratio's edit in every image) beside eight
single launches on the eight images, each as one graph of `--reps` repetitions, alternating, medians of 7.  No threshold hangs on any figure.

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
TAG = "PD_STACKED_ROW "


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


def _stat(v):
    return round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]


def resample_alone(a):
    """E = 8: one stacked DOWN launch for the tiles of all edits beside eight single launches, on the same images and lists."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask, reduce_mask

    hip.lib()
    E, C, S = 8, 64, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(E, C, S, S, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    sc, sh = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    tall = x.permute(0, 2, 3, 1).reshape(1, E * S, S, C).permute(0, 3, 1, 2)  # (stacked.tall: the same bytes)
    Ho = S // 2
    geo = dict(offset=(1, 1), stride=(1, 1), cells=(4, 4))
    rows = []
    for r in a.ratios.split(","):
        m = downsample_mask(dilate_mask(square_mask(S, float(r)).cuda(), 2), Ho)[(Ho, Ho)]
        one = reduce_mask(m, 6, 4, 1).to(torch.int32)
        one = one[one[:, 0] != Ho - 1].contiguous()  # (the candidates of the last row: in a tall list the next image's origin -1)
        N = int(one.shape[0])
        idx = torch.cat([one + torch.tensor([e * Ho, 0], dtype=torch.int32, device=one.device) for e in range(E)]).contiguous()
        res_tall = torch.zeros(1, C, E * Ho, Ho, device="cuda").contiguous(memory_format=torch.channels_last)
        res_each = torch.zeros(E, C, Ho, Ho, device="cuda").contiguous(memory_format=torch.channels_last)

        def stacked_launch():
            hip.set_edit_batch(E)
            try:
                return [hip.resample_tiles(tall, "down", idx, (6, 6), sc, sh, res=res_tall, **geo) for _ in range(a.reps)][-1]
            finally:
                hip.set_edit_batch(1)

        def each():
            for _ in range(a.reps):
                out = [hip.resample_tiles(x[e:e + 1], "down", one, (6, 6), sc, sh, res=res_each[e:e + 1], **geo) for e in range(E)]
            return out

        # (graphs of `--reps` repetitions: a replay's own cost, ~5 us, is shared by them; the sources are cache-resident)
        gt, out_t = capture_fn(stacked_launch)
        ge, out_e = capture_fn(each)
        tt, te = [], []
        for i in range(7):
            for name in (("t", "e") if i % 2 == 0 else ("e", "t")):
                (tt if name == "t" else te).append(events_ms(gt if name == "t" else ge, a.steps, 3) * 1e3 / a.reps)
        ut, mmt = _stat(tt)
        ue, mme = _stat(te)
        each_tall = res_each.permute(0, 2, 3, 1).reshape(1, E * Ho, Ho, C).permute(0, 3, 1, 2)
        same = torch.equal(out_t, torch.cat(out_e)) and torch.equal(res_tall, each_tall)
        rows.append({"ratio": float(r), "E": E, "reps": a.reps, "C": C, "source_per_image": [S, S], "tiles_per_edit": N,
                     "one_launch_us": ut, "one_launch_us_min_max": mmt, "E_single_launches_us": ue, "E_single_launches_us_min_max": mme,
                     "E_single_over_one": round(ue / ut, 3), "one_launch_ns_per_tile": round(ut * 1e3 / (E * N), 2),
                     "single_launch_ns_per_tile": round(ue * 1e3 / (E * N), 2), "bit_identical": bool(same)})
        del gt, ge
    print(TAG + json.dumps(rows), flush=True)


def child_stacked(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip, stacked
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import pd_unet
    from tests.golden.model_init import init_by_name

    hip.lib()
    dev = torch.device("cuda")
    cfg = pd_unet.PDConfig()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731

    def make_model():
        # the test fixtures' weights (tests/golden/model_init.py): under torch's default initialisation this network turns the last
        # bit of a sum into O(1) output differences (two roundings of one forward differ by 1.6 at a 15 % edit), which says nothing
        # about stacking; the timings do not depend on the values
        m = pd_unet.PDSparseUNet(cfg).eval()
        init_by_name(m)
        m = m.to(dev).to(memory_format=torch.channels_last)
        m.set_scatter_inplace(True)
        return m

    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g)
    noises = [torch.randn(1, 3, cfg.image_size, cfg.image_size, generator=g) for _ in range(8)]
    logsnr = torch.zeros(1, device=dev)
    mask = square_mask(cfg.image_size, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    with torch.no_grad():
        single, tall_model = make_model(), make_model()
        masks = downsample_mask(dilate_mask(mask.to(dev), 2), cfg.image_size // 2 ** (len(cfg.ch_mult) - 1))
        for m in (single, tall_model):
            m.set_mode("full")
            m(cl(x0), logsnr)
            m.set_masks(masks)
            m.set_mode("sparse")
        edits = [cl(x0 + n * mask) for n in noises]
        x1 = edits[0].clone()
        single(x1, logsnr)
        n0 = hip.launch_count()
        single(x1, logsnr)
        row["single_edit_library_launches"] = hip.launch_count() - n0
        g1, out1 = capture_fn(lambda: single(x1, logsnr))
        row["E"] = {}
        for E in (2, 4, 8):
            xs = cl(torch.cat(edits[:E], 0))
            stacked.stack_caches(tall_model, E)
            try:
                stacked.set_masks(tall_model, [masks] * E)
                with stacked.edit_batch(tall_model, E):
                    tall_model(xs, logsnr)
                    n0 = hip.launch_count()
                    tall_model(xs, logsnr)
                    launches = hip.launch_count() - n0
                    gE, outE = capture_fn(lambda: tall_model(xs, logsnr))
                tE, t1 = [], []
                for batch in range(a.batches):
                    for e in range(E):
                        xs[e].copy_(edits[(batch + e) % len(edits)][0])
                    x1.copy_(edits[batch % len(edits)])
                    for name in (("E", "1") if batch % 2 == 0 else ("1", "E")):
                        (tE if name == "E" else t1).append(events_ms(gE if name == "E" else g1, a.steps, 5))
                worst = 0.0
                for e in range(E):
                    xs[e].copy_(edits[e][0])
                gE.replay()
                for e in range(E):
                    x1.copy_(edits[e])
                    g1.replay()
                    worst = max(worst, float((outE[e] - out1[0]).abs().max()))
                del gE
            finally:
                stacked.unstack_caches(tall_model)
            mE, mmE = _stat(tE)
            m1, mm1 = _stat(t1)
            row["E"][str(E)] = {"forward_ms": mE, "forward_ms_min_max": mmE, "ms_per_edit": round(mE / E, 4), "single_edit_ms": m1,
                                "single_edit_ms_min_max": mm1, "speedup": round(m1 * E / mE, 3), "library_launches": launches,
                                "max_abs_stacked_minus_single": worst,
                                "peak_allocated_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    print(TAG + json.dumps(row), flush=True)


def main_stacked(a):
    """The parent of --stacked: one child per job."""
    from sige_amd import build

    res = {"workload": "church_pd128-sige.yml, exact fp32, channels-last, hipGraph replay, the test fixtures' weights (tests/golden/model_init.py); stacked "
                       "edits: E edited versions of one original under one square mask each, another noise per edit",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    common = ["--stacked", "--steps", str(a.steps), "--batches", str(a.batches), "--reps", str(a.reps)]
    jobs = [("resample", ["--resample", "--ratios", a.ratios])] + [(r, ["--ratio", r]) for r in a.ratios.split(",")]
    for tag, extra in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), *extra, *common]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": tag, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        if tag == "resample":
            res["resample_down_alone_E8"] = json.loads(line[len(TAG):])
        else:
            res["rows"].append(json.loads(line[len(TAG):]))
        print("pd_bench.py --stacked: %s done" % tag, file=sys.stderr, flush=True)
    with open(a.stacked_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


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
    ap.add_argument("--stacked", action="store_true", help="stacked edits E = 2, 4, 8 against single edits -> profiles/pd_stacked_bench.json")
    ap.add_argument("--resample", action="store_true", help="(child of --stacked) the tiled DOWN launch alone at E = 8, on the GPU")
    ap.add_argument("--stacked-out", default=os.path.join(REPO, "profiles", "pd_stacked_bench.json"))
    a = ap.parse_args()
    if a.stacked:
        if a.resample:
            return resample_alone(a)
        return child_stacked(a) if a.ratio is not None else main_stacked(a)
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
