#!/usr/bin/env python3
"""The SD VAE decoder (configs/sige.yaml's ddconfig, latent 64 x 64 -> 512 x 512) on the MI355X: fp32, channels-last, hipGraph replay.

    python tools/vae_bench.py            -> profiles/sd_vae_decoder_bench.json
    python tools/vae_bench.py --stacked  -> profiles/sd_vae_stacked_bench.json ("decoder"): stacked edits, tools/vae_stacked.py
    python tools/vae_bench.py --dtype f16 -> profiles/sd_vae_f16_bench.json ("decoder"): the f16 compute mode, see child_f16()

Per square edit of 1.2 / 5 / 15 % of the 512 x 512 image, in ONE child process so that the comparison stays inside one session:
  (a) the sparse forward;
  (b) the same forward with the attention block on the torch chain (sd_vae.NATIVE_ATTENTION = False): bmm, softmax over a
      [1, Nq, 4096] score tensor, bmm, with the reference's reshapes and copies -- (b) - (a) is what the one-launch attention is worth;
  (c) the dense forward of the same decoder on MIOpen (set_plain_dense, cudnn.benchmark) on the edited latent.
Timing: HIP events around `--steps` replays, after warm-up replays; (a) and (b) alternate batch by batch, the edited latent in the
graphs' input buffer changes from batch to batch, the medians over `--batches` batches are reported.  Also: the library launches
of (a) and (b), max |a - b| over the outputs after the graphs have replayed on the same latent, and the attention launch ALONE
(hip.attention_wide: Nq = 16 x active tiles, 4 096 keys, one 512-wide head, k | v the halves of one [1,4096,1024] tensor) against
the torch chain (bmm / softmax / bmm on contiguous q, k, v) at the same shape, each as a graph of `--reps` launches, with the
FLOP the algorithm needs (4 Nq Nk d) over the time.

The parent process never touches the GPU: it starts one child per ratio under `timeout -k 10` and stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import vae_stacked  # noqa: E402  (--stacked)

PEAK_F32_MFMA = 157.3e12
LATENT = 64


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


def attention_alone(tiles, reps, steps):
    """hip.attention_wide and the torch chain at the decoder's shape for `tiles` active 4x4 tiles, alternating, medians of 7."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip

    Nq, Nk, d = 16 * tiles, LATENT * LATENT, 512
    g = torch.Generator().manual_seed(tiles)
    q = (torch.randn(1, Nq, d, generator=g) * 2.0).cuda()
    kv = torch.randn(1, Nk, 2 * d, generator=g).cuda()
    k, v = kv[:, :, :d], kv[:, :, d:]
    kc, vc = k.contiguous(), v.contiguous()
    scale = d ** -0.5
    out = torch.empty(1, Nq, d, device="cuda")

    def native():
        for _ in range(reps):
            hip.attention_wide(q, k, v, 1, scale, out=out)
        return out

    def chain():
        for _ in range(reps):
            o = torch.bmm(torch.softmax(torch.bmm(q, kc.transpose(1, 2)) * scale, dim=2), vc)
        return o

    gn, on = capture_fn(native)
    gc, oc = capture_fn(chain)
    tn, tc = [], []
    for i in range(7):
        for name in (("n", "c") if i % 2 == 0 else ("c", "n")):
            (tn if name == "n" else tc).append(events_ms(gn if name == "n" else gc, steps, 3) * 1e3 / reps)
    flop = 4.0 * Nq * Nk * d
    un, uc = statistics.median(tn), statistics.median(tc)
    return {"tiles": tiles, "Nq": Nq, "Nk": Nk, "d": d, "kernel_us": round(un, 2), "kernel_us_min_max": [round(min(tn), 2), round(max(tn), 2)],
            "torch_chain_us": round(uc, 2), "torch_chain_us_min_max": [round(min(tc), 2), round(max(tc), 2)],
            "kernel_not_slower": bool(un <= uc), "flop": flop, "kernel_tflops": round(flop / (un * 1e-6) / 1e12, 2),
            "kernel_of_f32_mfma_peak": round(flop / (un * 1e-6) / PEAK_F32_MFMA, 4),
            "max_abs_kernel_minus_chain": float((on - oc).abs().max())}


def attention_forms_alone(tiles, reps, steps):
    """hip.attention_wide in both arithmetic forms and the torch chain at the decoder's shape for `tiles` active 4x4 tiles: three graphs
    of `reps` launches, rotated, medians of 7."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip

    Nq, Nk, d = 16 * tiles, LATENT * LATENT, 512
    g = torch.Generator().manual_seed(tiles)
    q = (torch.randn(1, Nq, d, generator=g) * 2.0).cuda()
    kv = torch.randn(1, Nk, 2 * d, generator=g).cuda()
    k, v = kv[:, :, :d], kv[:, :, d:]
    kc, vc = k.contiguous(), v.contiguous()
    scale = d ** -0.5
    outs = {c: torch.empty(1, Nq, d, device="cuda") for c in ("f32", "f16")}

    def native(compute):
        def run():
            for _ in range(reps):
                hip.attention_wide(q, k, v, 1, scale, out=outs[compute], compute=compute)
            return outs[compute]
        return run

    def chain():
        for _ in range(reps):
            o = torch.bmm(torch.softmax(torch.bmm(q, kc.transpose(1, 2)) * scale, dim=2), vc)
        return o

    graphs = {"f32": capture_fn(native("f32")), "f16": capture_fn(native("f16")), "torch_chain": capture_fn(chain)}
    names = list(graphs)
    us = {n: [] for n in names}
    for i in range(7):
        for n in names[i % 3:] + names[:i % 3]:
            us[n].append(events_ms(graphs[n][0], steps, 3) * 1e3 / reps)
    flop = 4.0 * Nq * Nk * d
    row = {"tiles": tiles, "Nq": Nq, "Nk": Nk, "d": d, "flop": flop}
    for n in names:
        row[n + "_us"] = round(statistics.median(us[n]), 2)
        row[n + "_us_min_max"] = [round(min(us[n]), 2), round(max(us[n]), 2)]
    row["f16_not_slower_than_f32"] = bool(row["f16_us"] <= row["f32_us"])
    row["f16_tflops"] = round(flop / (row["f16_us"] * 1e-6) / 1e12, 2)
    row["max_abs_f16_minus_f32"] = float((graphs["f16"][1] - graphs["f32"][1]).abs().max())
    return row


def child_f16(a):
    """--dtype f16, one ratio: the sparse forward in f16 mode (a), in f32 mode (b: a second model with its own caches), in f16 mode
    with sd_vae.ATTENTION_COMPUTE = "f32" (c), as graphs that alternate batch by batch; the library launches of each; the attention
    launch alone in both forms beside the torch chain."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import sd_vae
    from tests.golden import vae_inputs

    hip.lib()
    dev = torch.device("cuda")
    cfg = sd_vae.VAEDecoderConfig()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    z0 = torch.randn(1, cfg.z_channels, LATENT, LATENT, generator=g)
    noises = [torch.randn(1, cfg.z_channels, LATENT, LATENT, generator=g) for _ in range(4)]
    size = LATENT * 2 ** (len(cfg.ch_mult) - 1)
    mask = vae_inputs.square_mask(size, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    models = {}
    with torch.no_grad():
        for dtype in ("f16", "f32"):
            torch.manual_seed(0)
            m = sd_vae.SparseVAEDecoder(cfg).eval().to(dev).to(memory_format=torch.channels_last)
            m.set_scatter_inplace(True)
            m.set_compute_dtype(dtype)
            m.set_mode("full")
            m(cl(z0))
            masks = downsample_mask(dilate_mask(mask.to(dev), 2), LATENT)
            m.set_masks(masks)
            m.set_mode("sparse")
            models[dtype] = m
        m64 = masks[(LATENT, LATENT)].cpu()
        edits = [cl(z0 + n * m64) for n in noises]
        z1 = edits[0].clone()
        tiles = int(models["f16"].mid.attn_1.gather.active_indices.shape[0])
        row["attention_tiles"] = tiles
        graphs, outs = {}, {}
        for name, dtype, attention in (("a_f16", "f16", "f16"), ("b_f32", "f32", "f32"), ("c_f16_attention_f32", "f16", "f32")):
            sd_vae.ATTENTION_COMPUTE = attention
            m = models[dtype]
            m(z1)
            n0 = hip.launch_count()
            m(z1)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture_fn(lambda m=m: m(z1))
        sd_vae.ATTENTION_COMPUTE = None
        ms = {k: [] for k in graphs}
        names = list(graphs)
        for batch in range(a.batches):
            z1.copy_(edits[batch % len(edits)])
            for name in names[batch % 3:] + names[:batch % 3]:
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        row["a_minus_b_max_abs"] = float((outs["a_f16"] - outs["b_f32"]).abs().max())
        row["a_minus_c_max_abs"] = float((outs["a_f16"] - outs["c_f16_attention_f32"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["f16_over_f32"] = round(row["a_f16_ms"] / row["b_f32_ms"], 3)
        del graphs
        row["attention_alone"] = attention_forms_alone(tiles, a.reps, a.steps)
    print("VAE_BENCH_ROW " + json.dumps(row), flush=True)


def child(a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import sd_vae
    from tests.golden import vae_inputs

    hip.lib()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = sd_vae.VAEDecoderConfig()
    model = sd_vae.SparseVAEDecoder(cfg).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    z0 = torch.randn(1, cfg.z_channels, LATENT, LATENT, generator=g)
    noises = [torch.randn(1, cfg.z_channels, LATENT, LATENT, generator=g) for _ in range(4)]
    size = LATENT * 2 ** (len(cfg.ch_mult) - 1)
    mask = vae_inputs.square_mask(size, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    with torch.no_grad():
        model.set_mode("full")
        model(cl(z0))
        masks = downsample_mask(dilate_mask(mask.to(dev), 2), LATENT)
        model.set_masks(masks)
        model.set_mode("sparse")
        m64 = masks[(LATENT, LATENT)].cpu()
        edits = [cl(z0 + n * m64) for n in noises]
        z1 = edits[0].clone()
        tiles = int(model.mid.attn_1.gather.active_indices.shape[0])
        row["attention_tiles"] = tiles
        graphs, outs = {}, {}
        for name, native in (("a_sparse", True), ("b_sparse_torch_attention", False)):
            sd_vae.NATIVE_ATTENTION = native
            model(z1)
            n0 = hip.launch_count()
            model(z1)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture_fn(lambda: model(z1))
        sd_vae.NATIVE_ATTENTION = True
        ms = {k: [] for k in graphs}
        for batch in range(a.batches):
            z1.copy_(edits[batch % len(edits)])  # (another edited latent in the graphs' input buffer)
            for name in (list(graphs) if batch % 2 == 0 else list(graphs)[::-1]):
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        # (a capture runs nothing: the outputs hold values only after a replay -- both graphs last ran on the same latent)
        row["a_minus_b_max_abs"] = float((outs["a_sparse"] - outs["b_sparse_torch_attention"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["a_not_slower_than_b"] = bool(row["a_sparse_ms"] <= row["b_sparse_torch_attention_ms"])
        del graphs
        row["attention_alone"] = attention_alone(tiles, a.reps, a.steps)
        # (c) the stock dense decoder on MIOpen, on the edited latent
        model.set_mode("full")
        model.set_plain_dense(True)
        gd, _ = capture_fn(lambda: model(z1))
        kd = max(5, a.steps // 8)
        row["c_dense_miopen_ms"] = round(statistics.median(events_ms(gd, kd, 2) for _ in range(5)), 4)
        row["dense_over_sparse"] = round(row["c_dense_miopen_ms"] / row["a_sparse_ms"], 3)
    print("VAE_BENCH_ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--ratio", type=float, default=None, help="(child) one ratio, on the GPU")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None, help="default: profiles/sd_vae_decoder_bench.json; --dtype f16: profiles/sd_vae_f16_bench.json")
    ap.add_argument("--dtype", choices=("f32", "f16"), default="f32", help="f16: the f16 compute mode beside f32, child_f16()")
    vae_stacked.add_arguments(ap)
    a = ap.parse_args()
    if a.stacked:
        return vae_stacked.dispatch("decoder", a, __file__)
    if a.ratio is not None:
        return child_f16(a) if a.dtype == "f16" else child(a)
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "sd_vae_f16_bench.json" if a.dtype == "f16" else "sd_vae_decoder_bench.json")
    from sige_amd import build

    res = {"workload": "SD VAE decoder (configs/sige.yaml ddconfig), latent [1,4,64,64] -> 512 x 512, fp32, channels-last, hipGraph replay, "
                       "default-initialised weights (seed 0)",
           "context": "the reference quotes 235.0 ms dense / 48.0 ms sparse on an RTX 3090 (BASELINE.md 2): context only",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    for r in a.ratios.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ratio", r, "--steps", str(a.steps),
               "--batches", str(a.batches), "--reps", str(a.reps)] + (["--dtype", "f16"] if a.dtype == "f16" else [])
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith("VAE_BENCH_ROW ")), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"ratio": r, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        res["rows"].append(json.loads(line[len("VAE_BENCH_ROW "):]))
    if a.dtype == "f16":
        # one file for both models: this tool owns its "decoder" key (tools/vae_encoder_bench.py: "encoder")
        res["workload"] = res["workload"].replace("fp32, ", "f16 compute mode beside fp32, ")
        whole = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                whole = json.load(f)
        whole["decoder"] = res
        with open(a.out, "w") as f:
            json.dump(whole, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return 1 if "failed" in res else 0
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
