#!/usr/bin/env python3
"""The SD VAE encoder (configs/sige.yaml's ddconfig, image 512 x 512 -> moments [1,8,64,64]) on the MI355X: exact fp32, channels-last,
hipGraph replay.

    python tools/vae_encoder_bench.py            -> profiles/sd_vae_encoder_bench.json
    python tools/vae_encoder_bench.py --stacked  -> profiles/sd_vae_stacked_bench.json ("encoder"): stacked edits, tools/vae_stacked.py
    python tools/vae_encoder_bench.py --dtype f16 -> profiles/sd_vae_f16_bench.json ("encoder"): the f16 compute mode, see child_f16()

Per square edit of 1.2 / 5 / 15 % of the image, in ONE child process so that the comparison stays inside one session:
  (a) the sparse forward through moments(): the tail is group_norm_affine + ONE launch of hip.conv3x3_latent_head_cl with quant_conv
      folded into conv_out's weights;
  (b) the same forward with the tail on the torch chain (sd_vae.NATIVE_HEAD = False): F.group_norm, SiLU, MIOpen's conv_out,
      quant_conv -- (b) - (a) is what the one-launch tail is worth;
  (c) the dense forward of the same encoder on MIOpen (set_plain_dense, cudnn.benchmark) on the edited image, quant_conv behind it.
Timing: HIP events around `--steps` replays, after warm-up replays; (a) and (b) alternate batch by batch, the edited image in the
graphs' input buffer changes from batch to batch, the medians over `--batches` batches are reported.  Also: the library launches
of (a) and (b), max |a - b| over the moments after the graphs have replayed on the same image, and -- once, in a child of its own --
the head launch ALONE at [1,512,64,64] (affine + SiLU + conv + folded quant_conv) against the torch chain on the ALREADY ACTIVATED
tensor (MIOpen's conv_out + quant_conv: the chain is not charged for GroupNorm and SiLU), each as a graph of `--reps` launches,
alternating, medians of 9; with the FLOP (2 H W 9 C Cout) and bytes (x + weights + out) the algorithm needs over the time, as
fractions of the fp32 MFMA peak and of the HBM bandwidth (the larger of the two bounds the launch).

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
from tools import vae_stacked  # noqa: E402  (--stacked)

PEAK_F32_MFMA = 157.3e12  # 256 CUs x 4 SIMDs x 64 FLOP / clk x 2.4 GHz
PEAK_HBM = 8.0e12         # bytes / s
IMAGE, LATENT = 512, 64


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


def head_alone(a):
    """hip.conv3x3_latent_head_cl and the torch chain at the encoder's real tail shape, alternating."""
    import torch
    from torch.nn import functional as F

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.workloads import sd_vae

    hip.lib()
    torch.backends.cudnn.benchmark = True
    C, H, W, Cout = 512, LATENT, LATENT, 8
    torch.manual_seed(0)
    enc = sd_vae.SparseVAEEncoder().eval()
    conv_out = enc.conv_out.cuda().to(memory_format=torch.channels_last)
    quant = torch.nn.Conv2d(Cout, Cout, 1).cuda().to(memory_format=torch.channels_last)
    enc.conv_out = conv_out
    w, b = enc.folded_head(quant)
    g = torch.Generator().manual_seed(2)
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
    xs = [cl(torch.randn(1, C, H, W, generator=g)) for _ in range(4)]  # (4 x 8 MB: below the 256 MB last-level cache, as in the forward)
    sc, sh = (1.0 + 0.1 * torch.randn(1, C, 1, 1, generator=g)).cuda(), (0.1 * torch.randn(1, C, 1, 1, generator=g)).cuda()
    acts = [cl(F.silu(x * sc + sh)) for x in xs]
    out = torch.empty(1, Cout, H, W, device="cuda").contiguous(memory_format=torch.channels_last)

    def native():
        for i in range(a.reps):
            hip.conv3x3_latent_head_cl(xs[i % len(xs)], w, b, sc, sh, "swish", out=out)
        return out

    def chain():
        with torch.no_grad():
            for i in range(a.reps):
                o = quant(conv_out(acts[i % len(acts)]))
        return o

    assert native() is not None
    gn, on = capture_fn(native)
    gc, oc = capture_fn(chain)
    tn, tc = [], []
    for i in range(9):
        for name in (("n", "c") if i % 2 == 0 else ("c", "n")):
            (tn if name == "n" else tc).append(events_ms(gn if name == "n" else gc, a.steps, 3) * 1e3 / a.reps)
    flop = 2.0 * H * W * 9 * C * Cout
    nbytes = 4.0 * (H * W * C + 9 * C * Cout + H * W * Cout)
    un, uc = statistics.median(tn), statistics.median(tc)
    spread = max(max(tn) - min(tn), max(tc) - min(tc))
    row = {"shape": [1, C, H, W], "Cout": Cout, "reps_per_graph": a.reps, "kernel_us": round(un, 2),
           "kernel_us_min_max": [round(min(tn), 2), round(max(tn), 2)], "torch_chain_us": round(uc, 2),
           "torch_chain_us_min_max": [round(min(tc), 2), round(max(tc), 2)],
           "torch_chain": "MIOpen conv_out on the activated tensor + quant_conv (GroupNorm and SiLU not charged)",
           "run_to_run_spread_us": round(spread, 2), "kernel_not_slower_beyond_spread": bool(un <= uc + spread),
           "flop": flop, "bytes": nbytes, "kernel_tflops": round(flop / (un * 1e-6) / 1e12, 2),
           "kernel_of_f32_mfma_peak": round(flop / (un * 1e-6) / PEAK_F32_MFMA, 4),
           "kernel_of_hbm_bandwidth": round(nbytes / (un * 1e-6) / PEAK_HBM, 4),
           "bound": "fp32 MFMA (%.2f us at peak) over HBM (%.2f us)" % (flop / PEAK_F32_MFMA * 1e6, nbytes / PEAK_HBM * 1e6),
           "max_abs_kernel_minus_chain": float((on - oc).abs().max())}
    print("VAE_ENC_BENCH_ROW " + json.dumps(row), flush=True)


def child_f16(a):
    """--dtype f16, one ratio: the sparse forward through moments() in f16 mode (a), in f32 mode (b: a second model with its own
    caches), in f16 mode with sd_vae.ATTENTION_COMPUTE = "f32" (c), as graphs that alternate batch by batch; the library launches of
    each; the attention launch alone in both forms beside the torch chain (tools/vae_bench.attention_forms_alone: the middle block
    is the decoder's -- 4 096 keys, one 512-wide head)."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import sd_vae
    from tests.golden import vae_inputs
    from tools.vae_bench import attention_forms_alone

    hip.lib()
    dev = torch.device("cuda")
    cfg = sd_vae.VAEEncoderConfig()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, cfg.in_channels, IMAGE, IMAGE, generator=g)
    noises = [torch.randn(1, cfg.in_channels, IMAGE, IMAGE, generator=g) for _ in range(4)]
    mask = vae_inputs.square_mask(IMAGE, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    models = {}
    with torch.no_grad():
        for dtype in ("f16", "f32"):
            torch.manual_seed(0)
            m = sd_vae.SparseVAEEncoder(cfg).eval().to(dev).to(memory_format=torch.channels_last)
            quant = torch.nn.Conv2d(2 * cfg.z_channels, 2 * cfg.z_channels, 1).to(dev).to(memory_format=torch.channels_last)
            m.set_scatter_inplace(True)
            m.set_compute_dtype(dtype)
            m.set_mode("full")
            m(cl(x0))
            m.set_masks(downsample_mask(dilate_mask(mask.to(dev), 2), LATENT))
            m.set_mode("sparse")
            models[dtype] = (m, quant)
        edits = [cl(x0 + n * mask.float()) for n in noises]
        x1 = edits[0].clone()
        tiles = int(models["f16"][0].mid.attn_1.gather.active_indices.shape[0])
        row["attention_tiles"] = tiles
        graphs, outs = {}, {}
        for name, dtype, attention in (("a_f16", "f16", "f16"), ("b_f32", "f32", "f32"), ("c_f16_attention_f32", "f16", "f32")):
            sd_vae.ATTENTION_COMPUTE = attention
            m, quant = models[dtype]
            m.moments(x1, quant)
            n0 = hip.launch_count()
            m.moments(x1, quant)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture_fn(lambda m=m, quant=quant: m.moments(x1, quant))
        sd_vae.ATTENTION_COMPUTE = None
        ms = {k: [] for k in graphs}
        names = list(graphs)
        for batch in range(a.batches):
            x1.copy_(edits[batch % len(edits)])
            for name in names[batch % 3:] + names[:batch % 3]:
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        row["a_minus_b_max_abs"] = float((outs["a_f16"] - outs["b_f32"]).abs().max())
        row["a_minus_c_max_abs"] = float((outs["a_f16"] - outs["c_f16_attention_f32"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["f16_over_f32"] = round(row["a_f16_ms"] / row["b_f32_ms"], 3)
        del graphs
        row["attention_alone"] = attention_forms_alone(tiles, 4, a.steps)
    print("VAE_ENC_BENCH_ROW " + json.dumps(row), flush=True)


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
    cfg = sd_vae.VAEEncoderConfig()
    model = sd_vae.SparseVAEEncoder(cfg).eval().to(dev).to(memory_format=torch.channels_last)
    quant = torch.nn.Conv2d(2 * cfg.z_channels, 2 * cfg.z_channels, 1).to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, cfg.in_channels, IMAGE, IMAGE, generator=g)
    noises = [torch.randn(1, cfg.in_channels, IMAGE, IMAGE, generator=g) for _ in range(4)]
    mask = vae_inputs.square_mask(IMAGE, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}
    with torch.no_grad():
        model.set_mode("full")
        model(cl(x0))
        masks = downsample_mask(dilate_mask(mask.to(dev), 2), LATENT)
        model.set_masks(masks)
        model.set_mode("sparse")
        edits = [cl(x0 + n * mask.float()) for n in noises]
        x1 = edits[0].clone()
        row["first_level_tiles"] = int(model.down[0].block[0].main_gather.active_indices.shape[0])
        row["attention_tiles"] = int(model.mid.attn_1.gather.active_indices.shape[0])
        graphs, outs = {}, {}
        for name, native in (("a_sparse", True), ("b_sparse_torch_head", False)):
            sd_vae.NATIVE_HEAD = native
            model.moments(x1, quant)
            n0 = hip.launch_count()
            model.moments(x1, quant)
            row[name + "_library_launches"] = hip.launch_count() - n0
            graphs[name], outs[name] = capture_fn(lambda: model.moments(x1, quant))
        sd_vae.NATIVE_HEAD = True
        ms = {k: [] for k in graphs}
        for batch in range(a.batches):
            x1.copy_(edits[batch % len(edits)])  # (another edited image in the graphs' input buffer)
            for name in (list(graphs) if batch % 2 == 0 else list(graphs)[::-1]):
                ms[name].append(events_ms(graphs[name], a.steps, 5))
        # (a capture runs nothing: the outputs hold values only after a replay -- both graphs last ran on the same image)
        row["a_minus_b_max_abs"] = float((outs["a_sparse"] - outs["b_sparse_torch_head"]).abs().max())
        for name, v in ms.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["a_not_slower_than_b"] = bool(row["a_sparse_ms"] <= row["b_sparse_torch_head_ms"])
        del graphs
        # (c) the stock dense encoder on MIOpen, on the edited image
        model.set_mode("full")
        model.set_plain_dense(True)
        gd, _ = capture_fn(lambda: model.moments(x1, quant))
        kd = max(5, a.steps // 8)
        row["c_dense_miopen_ms"] = round(statistics.median(events_ms(gd, kd, 2) for _ in range(5)), 4)
        row["dense_over_sparse"] = round(row["c_dense_miopen_ms"] / row["a_sparse_ms"], 3)
    print("VAE_ENC_BENCH_ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--ratio", type=float, default=None, help="(child) one ratio, on the GPU")
    ap.add_argument("--head", action="store_true", help="(child) the head launch alone, on the GPU")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None, help="default: profiles/sd_vae_encoder_bench.json; --dtype f16: profiles/sd_vae_f16_bench.json")
    ap.add_argument("--dtype", choices=("f32", "f16"), default="f32", help="f16: the f16 compute mode beside f32, child_f16()")
    vae_stacked.add_arguments(ap)
    a = ap.parse_args()
    if a.stacked:
        return vae_stacked.dispatch("encoder", a, __file__)
    if a.head:
        return head_alone(a)
    if a.ratio is not None:
        return child_f16(a) if a.dtype == "f16" else child(a)
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "sd_vae_f16_bench.json" if a.dtype == "f16" else "sd_vae_encoder_bench.json")
    from sige_amd import build

    res = {"workload": "SD VAE encoder (configs/sige.yaml ddconfig), image [1,3,512,512] -> moments [1,8,64,64] through quant_conv, "
                       "exact fp32, channels-last, hipGraph replay, default-initialised weights (seed 0)",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    common = ["--steps", str(a.steps), "--batches", str(a.batches), "--reps", str(a.reps)]
    jobs = [("head", ["--head"])] + [(r, ["--ratio", r]) for r in a.ratios.split(",")]
    if a.dtype == "f16":
        jobs = [(r, ["--ratio", r, "--dtype", "f16"]) for r in a.ratios.split(",")]  # (the latent head has no fp16 form: not measured again)
    for tag, extra in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), *extra, *common]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith("VAE_ENC_BENCH_ROW ")), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": tag, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        row = json.loads(line[len("VAE_ENC_BENCH_ROW "):])
        if tag == "head":
            res["head_alone"] = row
        else:
            res["rows"].append(row)
    if a.dtype == "f16":
        # one file for both models: this tool owns its "encoder" key (tools/vae_bench.py: "decoder")
        res["workload"] = res["workload"].replace("exact fp32, ", "f16 compute mode beside exact fp32, ")
        whole = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                whole = json.load(f)
        whole["encoder"] = res
        res = whole
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res.get("encoder", res) else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
