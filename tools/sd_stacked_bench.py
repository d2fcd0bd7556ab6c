#!/usr/bin/env python3
"""Stacked edits (sige_amd/stacked.py) through the Stable Diffusion v1 U-Net on the MI355X, in the protocol of tools/vae_stacked.py
and `tools/pd_bench.py --stacked`.  Writes profiles/sd_unet_stacked_bench.json.

Workload: SDUNet(SDConfig()) -- SD v1, 860 M parameters --, latent [1,4,64,64], one prompt [1,77,768], one timestep, exact fp32,
channels-last, in-place Scatters, default-initialised weights (seed 0).  B = 1: one sample, not the classifier-free-guidance pair of
`bench.py --workload sd` (stacked edits are E edits of ONE original).

Per square edit of 1.2 / 5 / 15 % of the 512 x 512 image, in ONE child process: two models with the same weights, one stays on single
edits, the other is stacked for E = 2, 4, 8 in turn (E edited versions of the same original under the same square, another noise per
edit).  Both forwards are hipGraphs; HIP events around `--steps` replays after warm-up replays; the stacked and the single-edit graph
alternate batch by batch and the edited inputs in the graphs' buffers change from batch to batch; medians over `--batches` batches.
`speedup` = E x the single-edit time OF THE SAME RUN over the stacked time.  Also: library launches per forward, stacked and single,
and max |stacked - single| per edit after both graphs replayed on the same inputs.

Once per run, in a child of its own: the self-attention launch ALONE at the 64 x 64 level with E = 8 --
hip.attention_tokens(tiles=...) on the tall K / V ([1, 8 x 4096, 320], 8 heads of 40), the tiles of a 5 % edit in every image -- beside
8 single launches of hip.attention_tokens on the same rows, each as one graph, alternating, medians of 7; both computes.

No threshold hangs on any figure.  The parent process never touches the GPU: it starts one child per measurement under
`timeout -k 10` and stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
IMAGE, LATENT = 512, 64
TAG = "SD_STACKED_ROW "
OUT = os.path.join(REPO, "profiles", "sd_unet_stacked_bench.json")


def square_mask(size, ratio):
    import torch

    a = int(round(size * ratio ** 0.5))
    o = (size - a) // 2
    m = torch.zeros(size, size, dtype=torch.bool)
    m[o:o + a, o:o + a] = True
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


def _stat(v):
    return round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]


def attention_alone(a):
    """E = 8: one per-image launch for the tiles of all edits beside eight single launches, on the same q and K / V rows."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import downsample_mask, reduce_mask

    hip.lib()
    E, heads, d, N = 8, 8, 40, LATENT * LATENT
    C = heads * d
    m64 = downsample_mask(square_mask(IMAGE, 0.05).cuda(), min_res=8, dilation=1)[(LATENT, LATENT)]
    one = reduce_mask(m64, 4, 4, 0).to(torch.int32)  # the transformer's 4x4 tiles of ONE edit
    T = int(one.shape[0])
    idx = torch.cat([one + torch.tensor([e * LATENT, 0], dtype=torch.int32, device=one.device) for e in range(E)]).contiguous()
    g = torch.Generator().manual_seed(T)
    q = (torch.randn(1, 16 * T * E, C, generator=g) * 2.0).cuda()
    k, v = (torch.randn(1, E * N, C, generator=g).cuda() for _ in range(2))
    scale = d ** -0.5
    row = {"E": E, "tiles_per_edit": T, "Nq": 16 * T * E, "keys_per_image": N, "heads": heads, "d": d}
    for compute in ("f32", "f16"):
        def tall():
            hip.set_edit_batch(E)
            try:
                return hip.attention_tokens(q, k, v, heads, scale, compute=compute, tiles=(idx, E * LATENT, LATENT))
            finally:
                hip.set_edit_batch(1)

        def each():
            outs = []
            for e in range(E):
                rows = slice(16 * T * e, 16 * T * (e + 1))
                outs.append(hip.attention_tokens(q[:, rows], k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N], heads, scale, compute=compute))
            return outs

        gt, out_tall = capture_fn(tall)
        ge, out_each = capture_fn(each)
        tt, te = [], []
        for i in range(7):
            for name in (("t", "e") if i % 2 == 0 else ("e", "t")):
                (tt if name == "t" else te).append(events_ms(gt if name == "t" else ge, a.steps, 3) * 1e3)
        ut, mmt = _stat(tt)
        ue, mme = _stat(te)
        row[compute] = {"one_launch_us": ut, "one_launch_us_min_max": mmt, "E_single_launches_us": ue, "E_single_launches_us_min_max": mme,
                        "E_single_over_one": round(ue / ut, 3),
                        "max_abs_one_minus_E_single": float((out_tall - torch.cat(out_each, 1)).abs().max())}
        del gt, ge
    print(TAG + json.dumps(row), flush=True)


def child_stacked(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip, stacked
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet

    hip.lib()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731

    def make_model():
        torch.manual_seed(0)
        m = SDUNet(SDConfig()).eval().to(dev).to(memory_format=torch.channels_last)
        m.set_scatter_inplace(True)
        return m

    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, 4, LATENT, LATENT, generator=g)
    noises = [torch.randn(1, 4, LATENT, LATENT, generator=g) for _ in range(8)]
    ctx = torch.randn(1, 77, 768, generator=g).to(dev)
    ts = torch.full((1,), 500.0, device=dev)
    mask = square_mask(IMAGE, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    run = lambda m, x: m(x, ts, context=ctx)  # noqa: E731

    with torch.no_grad():
        single, tall_model = make_model(), make_model()
        masks = downsample_mask(mask.to(dev), min_res=8, dilation=1)
        for m in (single, tall_model):
            m.set_mode("full")
            run(m, cl(x0))
            m.set_masks(masks)
            m.set_mode("sparse")
        inside = masks[(LATENT, LATENT)].cpu()
        edits = [cl(x0 + n * inside) for n in noises]
        row["tiles_64x64"] = int(single.input_blocks[1][1].gather.active_indices.shape[0])
        x1 = edits[0].clone()
        run(single, x1)
        n0 = hip.launch_count()
        run(single, x1)
        row["single_edit_library_launches"] = hip.launch_count() - n0
        g1, out1 = capture_fn(lambda: run(single, x1))
        row["E"] = {}
        for E in (2, 4, 8):
            xs = cl(torch.cat(edits[:E], 0))
            stacked.stack_caches(tall_model, E)
            try:
                stacked.set_masks(tall_model, [masks] * E)
                with stacked.edit_batch(tall_model, E):
                    run(tall_model, xs)
                    n0 = hip.launch_count()
                    run(tall_model, xs)
                    launches = hip.launch_count() - n0
                    gE, outE = capture_fn(lambda: run(tall_model, xs))
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


def main_parent(a):
    from sige_amd import build

    res = {"workload": "SD v1 U-Net (SDConfig(): 860 M parameters), latent [E,4,64,64], one prompt [1,77,768], one timestep, B = 1; exact "
                       "fp32, channels-last, in-place Scatters, hipGraph replay, default-initialised weights (seed 0); stacked edits: E "
                       "edited versions of one original under one square mask each, another noise per edit",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    common = ["--steps", str(a.steps), "--batches", str(a.batches)]
    jobs = [("attention", ["--attention"])] + [(r, ["--ratio", r]) for r in a.ratios.split(",")]
    for tag, extra in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), *extra, *common]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": tag, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        if tag == "attention":
            res["self_attention_alone_64x64_E8"] = json.loads(line[len(TAG):])
        else:
            res["rows"].append(json.loads(line[len(TAG):]))
        print("sd_stacked_bench.py: %s done" % tag, file=sys.stderr, flush=True)
    out = a.out or OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child, seconds")
    ap.add_argument("--out", default=None, help="default: profiles/sd_unet_stacked_bench.json")
    ap.add_argument("--ratio", type=float, default=None, help="(child) one edit size, on the GPU")
    ap.add_argument("--attention", action="store_true", help="(child) the self-attention launch alone at E = 8, on the GPU")
    a = ap.parse_args()
    if a.attention:
        return attention_alone(a) or 0
    if a.ratio is not None:
        return child_stacked(a) or 0
    return main_parent(a)


if __name__ == "__main__":
    sys.exit(main())
