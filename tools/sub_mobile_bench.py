#!/usr/bin/env python3
"""The GAN-Compression GauGAN generator (sub-mobile SPADE, --config_str 32_32_32_48_32_24_24_32, 256 x 512, num_sparse_layers 4) on
the MI355X: exact fp32, channels-last, hipGraph replay.

    python tools/sub_mobile_bench.py            -> profiles/gaugan_sub_mobile_bench.json

Per relabelled rectangle of 1.2 / 5 / 15 % of the label map, in ONE child process so that the comparison stays inside one session:
  (a) the sparse forward with ONE hip.spade_separable_cl launch per SPADE layer (gaugan_sub_mobile.SEPARABLE_NATIVE = True);
  (b) the same forward with the separable convs as the reference's module chain (SEPARABLE_NATIVE = False): per branch a grouped
      tile conv, a torch affine, a 1x1 tile conv, then torch.cat -- (b) - (a) is what the one-launch form is worth;
  (c) the dense forward of the same generator on torch / MIOpen (full mode, cudnn.benchmark) on the edited label map.
(b) and (c) consist of code that exists without the new kernel.  Timing: HIP events around `--steps` replays, after warm-up replays;
(a) and (b) alternate batch by batch, the edited label map in the graphs' input buffer changes from batch to batch; median, min and
max over `--batches` batches.  Also: the library launches of (a) and (b), max |a - b| after both graphs replayed on the same input,
and -- once, in a child of its own -- one hip.spade_separable_cl launch ALONE at the up_1 shapes (Ch 48, oc 256 and 96, the tiles of a
5 % edit) against the chain's launches for the same layer, each as a graph of `--reps` repetitions, alternating, medians of 9.

`default_on`: at 5 % the native forward's median is not above the chain's by more than the chain's own min-max spread over the
batches -- the rule SEPARABLE_NATIVE's default follows.

    python tools/sub_mobile_bench.py --stacked  -> profiles/gaugan_sub_mobile_stacked_bench.json

--stacked: stacked edits (sige_amd/stacked.py) and the statistics switch, per ratio in ONE child process with the same protocol.  Two
models with the same weights: one stays on single edits, the other is stacked for E = 2, 4, 8 in turn, so that every graph's caches and
index lists stay alive while it is replayed.
  * E = 1, the switch A/B: the native forward with gaugan_sub_mobile.SEPARABLE_STATS_NATIVE off (the torch prologue) and on (one
    hip.spade_separable_stats_cl launch per dense SPADE layer), alternating batch by batch.  `stats_native_default_on`: at ALL ratios
    the switch-on median is below the switch-off median by more than the larger of the two min-max spreads of that run.
  * E = 2, 4, 8: ONE stacked forward of E relabellings of the same rectangle (each edit its own label map, mask and InstanceNorm
    statistics), alternating with the single-edit forward (the switch at the module's default: `single_edit_form`); ms per edit =
    forward / E, `speedup` = single-edit median over ms per edit (`speedup_vs_stats_torch`: over the switch-off median of the A/B),
    and max |stacked - single| per edit after both graphs replayed on the same label maps.

The parent process never touches the GPU: it starts one child per measurement under `timeout -k 10` and stops at the first that
fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
H, W, NC = 256, 512, 36
TAG = "SUB_MOBILE_BENCH_ROW "


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


def relabelled(lab0, ratio, shift):
    """The label map with a centred rectangle of `ratio` of its area (aspect 1:2, as the map) moved `shift` classes on."""
    import numpy as np

    hh, ww = max(1, int(round(H * ratio ** 0.5))), max(1, int(round(W * ratio ** 0.5)))
    h0, w0 = (H - hh) // 2, (W - ww) // 2
    lab1 = lab0.copy()
    lab1[h0:h0 + hh, w0:w0 + ww] = (lab0[h0:h0 + hh, w0:w0 + ww] + shift) % NC
    return np.ascontiguousarray(lab1)


def layer_alone(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.nn import SIGEConv2d

    hip.lib()
    Ch, T = 48, a.tiles
    g = torch.Generator().manual_seed(2)
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
    slabs = [cl(torch.randn(T, Ch, 6, 6, generator=g)) for _ in range(4)]
    rows = []
    for oc in (256, 96):
        torch.manual_seed(oc)
        dw = [SIGEConv2d(Ch, Ch, 3, padding=1, groups=Ch).cuda().to(memory_format=torch.channels_last) for _ in range(2)]
        pw = [SIGEConv2d(Ch, oc, 1).cuda().to(memory_format=torch.channels_last) for _ in range(2)]
        for m in dw + pw:
            m.set_mode("sparse")
        sc = (1.0 + 0.3 * torch.randn(2, Ch, generator=g)).cuda()
        sh = (0.3 * torch.randn(2, Ch, generator=g)).cuda()
        with torch.no_grad():
            ops = (torch.stack([m.weight.reshape(Ch, 3, 3) for m in dw]).contiguous(), torch.stack([m.bias for m in dw]).contiguous(),
                   sc, sh, torch.stack([m.weight.reshape(oc, Ch) for m in pw]).contiguous(), torch.stack([m.bias for m in pw]).contiguous())
        out = torch.empty(T, 2 * oc, 4, 4, device="cuda").contiguous(memory_format=torch.channels_last)

        def native():
            for i in range(a.reps):
                hip.spade_separable_cl(slabs[i % 4], *ops, out=out, tiled=True)
            return out

        def chain():
            with torch.no_grad():
                for i in range(a.reps):
                    o = torch.cat([pw[b](dw[b](slabs[i % 4]) * sc[b].view(1, -1, 1, 1) + sh[b].view(1, -1, 1, 1)) for b in range(2)], dim=1)
            return o

        assert native() is not None
        n0 = hip.launch_count()
        chain()
        chain_launches = (hip.launch_count() - n0) // a.reps
        gn, on = capture_fn(native)
        gc, oc_out = capture_fn(chain)
        tn, tc = [], []
        for i in range(9):
            for name in (("n", "c") if i % 2 == 0 else ("c", "n")):
                (tn if name == "n" else tc).append(events_ms(gn if name == "n" else gc, a.steps, 3) * 1e3 / a.reps)
        un, uc = statistics.median(tn), statistics.median(tc)
        rows.append({"Ch": Ch, "oc": oc, "tiles": T, "reps_per_graph": a.reps, "kernel_us": round(un, 2),
                     "kernel_us_min_max": [round(min(tn), 2), round(max(tn), 2)], "chain_us": round(uc, 2),
                     "chain_us_min_max": [round(min(tc), 2), round(max(tc), 2)], "chain_library_launches": chain_launches,
                     "chain": "2 x (grouped tile conv, torch affine, 1x1 tile conv) + torch.cat",
                     "kernel_over_chain": round(un / uc, 3), "max_abs_kernel_minus_chain": float((on - oc_out).abs().max())})
    print(TAG + json.dumps(rows), flush=True)


def child(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import compute_difference_mask, dilate_mask, downsample_mask
    from sige_amd.workloads import gaugan_sub_mobile as gsm
    from tests.golden.model_init import gaugan_labels

    hip.lib()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = gsm.SubMobileSpadeGenerator(gsm.SubMobileSPADEConfig()).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0 = gaugan_labels(H, W)[0]
    lab0 = x0[0].argmax(0).numpy()
    onehot = lambda l: torch.nn.functional.one_hot(torch.from_numpy(l), NC).permute(2, 0, 1)[None].float()  # noqa: E731
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    edits = [cl(onehot(relabelled(lab0, a.ratio, s))) for s in (5, 11, 17, 23)]
    x0 = cl(x0)
    row = {"ratio": a.ratio}
    with torch.no_grad():
        model.set_mode("full")
        model(x0)
        diff = compute_difference_mask(x0, edits[0])
        row["edit_ratio"] = float(diff.float().mean())
        model.set_masks(downsample_mask(dilate_mask(diff, 1), (model.sh, model.sw), dilation=2))
        model.set_mode("sparse")
        x1 = edits[0].clone()
        row["up_3_tiles"] = int(model.up_3.main_gather.active_indices.shape[0])
        row["up_1_tiles"] = int(model.up_1.main_gather.active_indices.shape[0])
        graphs, outs = {}, {}
        for name, native in (("a_native", True), ("b_chain", False)):
            gsm.SEPARABLE_NATIVE = native
            model(x1)
            n0 = hip.launch_count()
            model(x1)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture_fn(lambda: model(x1))
        ms = {k: [] for k in graphs}
        for batch in range(a.batches):
            x1.copy_(edits[batch % len(edits)])  # (another relabelling of the same rectangle in the graphs' input buffer)
            for name in (list(graphs) if batch % 2 == 0 else list(graphs)[::-1]):
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        row["a_minus_b_max_abs"] = float((outs["a_native"] - outs["b_chain"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        spread = row["b_chain_ms_min_max"][1] - row["b_chain_ms_min_max"][0]
        row["chain_spread_ms"] = round(spread, 4)
        row["a_not_above_b_beyond_spread"] = bool(row["a_native_ms"] <= row["b_chain_ms"] + spread)
        row["chain_over_native"] = round(row["b_chain_ms"] / row["a_native_ms"], 3)
        del graphs
        # (c) the dense forward of the same generator on torch / MIOpen, on the edited label map
        model.set_mode("full")
        gd, _ = capture_fn(lambda: model(x1))
        kd = max(5, a.steps // 4)
        row["c_dense_torch_ms"] = round(statistics.median(events_ms(gd, kd, 2) for _ in range(5)), 4)
        row["dense_over_native"] = round(row["c_dense_torch_ms"] / row["a_native_ms"], 3)
        row["dense_over_chain"] = round(row["c_dense_torch_ms"] / row["b_chain_ms"], 3)
    print(TAG + json.dumps(row), flush=True)


def child_stacked(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip, stacked
    from sige_amd.utils import compute_difference_mask, dilate_mask, downsample_mask
    from sige_amd.workloads import gaugan_sub_mobile as gsm
    from tests.golden.model_init import gaugan_labels

    hip.lib()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")

    def make_model():
        torch.manual_seed(0)
        m = gsm.SubMobileSpadeGenerator(gsm.SubMobileSPADEConfig()).eval().to(dev).to(memory_format=torch.channels_last)
        m.set_scatter_inplace(True)
        return m

    x0 = gaugan_labels(H, W)[0]
    lab0 = x0[0].argmax(0).numpy()
    onehot = lambda l: torch.nn.functional.one_hot(torch.from_numpy(l), NC).permute(2, 0, 1)[None].float()  # noqa: E731
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    edits = [cl(onehot(relabelled(lab0, a.ratio, s))) for s in (5, 11, 17, 23, 29, 31, 7, 13)]
    x0 = cl(x0)
    row = {"ratio": a.ratio}
    stat = lambda v: (round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)])  # noqa: E731
    with torch.no_grad():
        single, tall_model = make_model(), make_model()
        pyramid = None
        for m in (single, tall_model):
            m.set_mode("full")
            m(x0)
            diff = compute_difference_mask(x0, edits[0])
            pyramid = downsample_mask(dilate_mask(diff, 1), (m.sh, m.sw), dilation=2)
            m.set_masks(pyramid)
            m.set_mode("sparse")
        row["edit_ratio"] = float(diff.float().mean())
        row["up_3_tiles"] = int(single.up_3.main_gather.active_indices.shape[0])
        # ---- E = 1: the statistics switch off / on, alternating ----
        x1 = edits[0].clone()
        graphs, outs = {}, {}
        keep = gsm.SEPARABLE_STATS_NATIVE
        try:
            for name, on in (("stats_torch", False), ("stats_native", True)):
                gsm.SEPARABLE_STATS_NATIVE = on
                single(x1)
                n0 = hip.launch_count()
                single(x1)
                row[name + "_library_launches"] = hip.launch_count() - n0
                graphs[name], outs[name] = capture_fn(lambda: single(x1))
        finally:
            gsm.SEPARABLE_STATS_NATIVE = keep
        ms = {k: [] for k in graphs}
        for batch in range(a.batches):
            x1.copy_(edits[batch % len(edits)])
            for name in (list(graphs) if batch % 2 == 0 else list(graphs)[::-1]):
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        for name, v in ms.items():
            row[name + "_ms"], row[name + "_ms_min_max"] = stat(v)
        row["stats_native_minus_torch_max_abs"] = float((outs["stats_native"] - outs["stats_torch"]).abs().max())
        spread = max(row[n + "_ms_min_max"][1] - row[n + "_ms_min_max"][0] for n in ms)
        row["switch_spread_ms"] = round(spread, 4)
        row["stats_native_faster_beyond_spread"] = bool(row["stats_native_ms"] < row["stats_torch_ms"] - spread)
        base = "stats_native" if gsm.SEPARABLE_STATS_NATIVE else "stats_torch"  # (the single-edit forward as the module ships it)
        row["single_edit_form"] = base
        g1, out1 = graphs[base], outs[base]
        del graphs
        # ---- E = 2, 4, 8: one stacked forward against the single-edit forward, alternating ----
        row["E"] = {}
        for E in (2, 4, 8):
            xs = torch.cat(edits[:E], 0).contiguous(memory_format=torch.channels_last)
            stacked.stack_caches(tall_model, E)
            try:
                stacked.set_masks(tall_model, [pyramid] * E)
                with stacked.edit_batch(tall_model, E):
                    tall_model(xs)
                    n0 = hip.launch_count()
                    tall_model(xs)
                    launches = hip.launch_count() - n0
                    gE, outE = capture_fn(lambda: tall_model(xs))
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
            mE, mmE = stat(tE)
            m1, mm1 = stat(t1)
            row["E"][str(E)] = {"forward_ms": mE, "forward_ms_min_max": mmE, "ms_per_edit": round(mE / E, 4), "single_edit_ms": m1,
                                "single_edit_ms_min_max": mm1, "speedup": round(m1 * E / mE, 3),
                                "speedup_vs_stats_torch": round(row["stats_torch_ms"] * E / mE, 3), "library_launches": launches,
                                "max_abs_stacked_minus_single": worst}
    print(TAG + json.dumps(row), flush=True)


def main_stacked(a, build):
    res = {"workload": "GAN-Compression GauGAN generator (sub-mobile SPADE, 32_32_32_48_32_24_24_32, num_sparse_layers 4), label map "
                       "[1,36,256,512], exact fp32, channels-last, hipGraph replay, default-initialised weights (seed 0); stacked edits: E "
                       "relabellings of one rectangle, one label map, mask and InstanceNorm affine per edit",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    for r in a.ratios.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--stacked", "--ratio", r,
               "--steps", str(a.steps), "--batches", str(a.batches)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": r, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        res["rows"].append(json.loads(line[len(TAG):]))
        print("sub_mobile_bench --stacked: %s done" % r, file=sys.stderr, flush=True)
    if "failed" not in res and res["rows"]:
        res["stats_native_default_on"] = all(r["stats_native_faster_beyond_spread"] for r in res["rows"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--ratio", type=float, default=None, help="(child) one ratio, on the GPU")
    ap.add_argument("--layer", action="store_true", help="(child) the separable launch alone, on the GPU")
    ap.add_argument("--tiles", type=int, default=60, help="tiles of the up_1 layer at a 5 %% edit")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    ap.add_argument("--stacked", action="store_true", help="stacked edits E = 1, 2, 4, 8 and the statistics switch A/B")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "gaugan_sub_mobile_stacked_bench.json" if a.stacked else "gaugan_sub_mobile_bench.json")
    if a.layer:
        return layer_alone(a)
    if a.ratio is not None:
        return child_stacked(a) if a.stacked else child(a)
    from sige_amd import build

    if a.stacked:
        return main_stacked(a, build)
    res = {"workload": "GAN-Compression GauGAN generator (sub-mobile SPADE, 32_32_32_48_32_24_24_32, num_sparse_layers 4), label map "
                       "[1,36,256,512], exact fp32, channels-last, hipGraph replay, default-initialised weights (seed 0)",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    common = ["--steps", str(a.steps), "--batches", str(a.batches), "--reps", str(a.reps), "--tiles", str(a.tiles)]
    jobs = [("layer", ["--layer"])] + [(r, ["--ratio", r]) for r in a.ratios.split(",")]
    for tag, extra in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), *extra, *common]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": tag, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        row = json.loads(line[len(TAG):])
        print("sub_mobile_bench: %s done" % tag, file=sys.stderr, flush=True)
        if tag == "layer":
            res["layer_alone_up_1"] = row
        else:
            res["rows"].append(row)
    at5 = next((r for r in res["rows"] if abs(r["ratio"] - 0.05) < 1e-9), None)
    if at5 is not None:
        res["default_on"] = at5["a_not_above_b_beyond_spread"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
