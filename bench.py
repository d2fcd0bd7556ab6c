#!/usr/bin/env python3
"""bench.py -- the reference's headline benchmark on MI355X.

Metric (BASELINE.json): U-Net forward ms + active-block conv TFLOP/s vs
edit-ratio on the 256x256 DDPM (LSUN-Church) U-Net, fp32, synthetic activations,
random-init weights.  Workload at N=1: BASELINE.json configs[1] -- one sparse
(SIGE) forward of the DDPM-256 U-Net at a 1.2 % square edit.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

`python bench.py --gpus N` launches its own N ranks (torch.distributed.run, one process per GPU, RCCL);
under a torchrun environment it joins it.

A plain run does only what the headline figure needs: set-up, W warm-up replays, the K timed steps, the outputs of the
last timed step (--dump-outputs DIR: DIR/output.npy, float32) and the result line.  Everything else described below
(dense baseline, per-kernel accounting and rooflines, the edit-ratio / f16 / f16x3 sweeps, mask-change latencies,
stacked edits, GauGAN, the SD transformer, the CPU baseline and the parity against the reference's CPU path) runs
only with --full.

A "step" = one sparse U-Net forward per GPU (each rank edits its own region of the shared original image).
N = 1: the timed region is K hipGraph replays of that forward.  N > 1: the timed region is one JOB -- the
activation cache of the original image, computed by rank 0, is distributed to the other ranks as one flat buffer
(one RCCL collective; what a rank derives from the cache is rebuilt locally) and every rank then runs K sparse
forwards -- so `value` counts the distribution inside the job; the steady-state rate (cache already resident)
and the cache-per-step rate are reported next to it (`multi_gpu`).  Barrier + synchronize on both sides, max over ranks.

One JSON line on rank 0, with (--full) `roofline` (dominant hot-path kernel, HIP events on the launch stream, rotating
buffers), `roofline_gather` / `roofline_scatter_gather` / `roofline_hbm` + the `data_movement` table (the HBM-bound
kernels, standalone), `parity_max_abs` (the benchmarked artefact's outputs against the reference's CPU path on the
same weights / inputs / masks, per edit ratio) and `cpu_baseline` (the reference's own sige/cpu backend --
oracle/_ref -- under the same U-Net on the host cores; the C restatement, kind "port", if _ref is absent).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from benchlib.common import (CAPTURE_MODE, PEAK_F16_MFMA_TFS, PEAK_F32_MFMA_TFS, PEAK_HBM_GBS, _hip, _replay_ms, capture,  # noqa: E402,F401
                             capture_fn, eager_ms, square_mask, time_graph_of, timed_replays)
from benchlib.gaugan import gaugan_section  # noqa: E402
from benchlib.sd_transformer import sd_transformer_section  # noqa: E402

# ------------------------------------------------------------------ op trace --
TRACED = ("gather", "scatter_gather", "scatter_fused", "scatter_with_block_residual_fused", "block_conv",
          "block_conv_direct", "gather_conv", "scatter_gather_conv", "gather_conv_nchw",
          # channels-last forms (the layout the benchmark runs in)
          "gather_cl", "scatter_gather_cl", "scatter_cl", "scatter_with_block_residual_cl", "block_conv_cl",
          "gather_conv_cl", "scatter_gather_conv_cl", "scatter_gather_conv_scatter_cl", "wide_conv_cl", "attention_tokens")


class Tracer:
    """Wraps the sige_amd.hip entry points the modules call; while `log` is a list
    every call is recorded as (name, args, kwargs) holding the live tensors."""

    def __init__(self, hip):
        self.log = None
        for name in TRACED:
            orig = getattr(hip, name)

            def wrapped(*a, _orig=orig, _name=name, **k):
                if self.log is not None:
                    self.log.append((_name, a, k, _orig))
                return _orig(*a, **k)

            setattr(hip, name, wrapped)


def op_cost(name, a, k=None):
    """(family, algorithmic bytes, algorithmic flops) of one traced call --
    SURVEY.md 8(d): reference out-of-place semantics, fp32.  In-place scatters
    (`out=` given) are accounted with the cache-preserving minimum (tile bytes only)
    under their own family name, never mixed with the out-of-place figure."""
    e = 4
    k = k or {}
    if name in ("gather_cl", "scatter_gather_cl"):
        name = name[:-3]
    if name == "block_conv_cl":
        name = "block_conv"
    if name == "scatter_cl":
        x, y, idx = a[0], a[1], a[4]
        res = a[6] if len(a) > 6 else k.get("residual")
        inplace = (a[7] if len(a) > 7 else k.get("out")) is not None
        tiles = e * y.shape[0] * idx.shape[0] * y.shape[1] * x.shape[2] * x.shape[3] * (2 + (1 if res is not None else 0))
        return ("scatter_inplace", tiles, 0) if inplace else ("scatter", 2 * e * y.numel() + tiles, 0)
    if name == "scatter_with_block_residual_cl":
        x0, y0, x1, i0, i1 = a[0], a[1], a[2], a[6], a[8]
        inplace = (a[10] if len(a) > 10 else k.get("out")) is not None
        B, C = y0.shape[:2]
        tiles = 3 * e * B * i0.shape[0] * C * x0.shape[2] * x0.shape[3] + 4 * e * B * i1.shape[0] * C * x1.shape[2] * x1.shape[3]
        return ("scatter_block_residual_inplace", tiles, 0) if inplace else ("scatter_block_residual", 2 * e * y0.numel() + tiles, 0)
    if name in ("gather_conv_cl", "gather_conv_nchw"):
        x, x2, block, idx = a[0], a[1], a[2], a[3]
        cout, kernel, stride = a[9], a[10], a[11]
        T, cin = x.shape[0] * idx.shape[0], x.shape[1] + (0 if x2 is None else x2.shape[1])
        ro, so = (block[0] - kernel[0]) // stride[0] + 1, (block[1] - kernel[1]) // stride[1] + 1
        dense = True
        if name == "gather_conv_cl":
            full = k.get("full")
            # dense layer = every output pixel covered by a tile; a sparse tile list written into a full tensor is
            # the conv -> Scatter fusion of a SIGE layer
            dense = full is not None and idx.shape[0] * ro * so >= full["out_res"][0] * full["out_res"][1]
        return ("dense_conv_mfma" if dense else "block_conv_mfma"), 0, 2 * T * ro * so * cout * cin * kernel[0] * kernel[1]
    if name == "attention_tokens":  # q [B,Nq,C], k / v [B,Nk,C]: QK^T and PV, 2 flop per multiply-add each
        q, kk = a[0], a[1]
        return "attention_tokens", 0, 4 * q.shape[0] * q.shape[1] * kk.shape[1] * q.shape[2]
    if name == "wide_conv_cl":  # dense layer on the fp16 matrix cores (conv_wide.hpp): algorithmic flops of the conv
        x, x2, cout, kernel = a[0], a[1], a[7], a[8]
        cin = x.shape[1] + (0 if x2 is None else x2.shape[1])
        up = 4 if k.get("upsample2x") else 1
        return "dense_conv_wide", 0, 2 * x.shape[0] * x.shape[2] * x.shape[3] * up * cout * cin * kernel[0] * kernel[1]
    if name == "scatter_gather_conv_cl":
        name = "scatter_gather_conv"
    if name == "scatter_gather_conv_scatter_cl":
        y, block, idx, cout, kernel = a[1], a[2], a[3], a[10], a[11]
        T, cin = y.shape[0] * idx.shape[0], y.shape[1]
        ro, so = block[0] - kernel[0] + 1, block[1] - kernel[1] + 1
        return "block_conv_mfma", 0, 2 * T * ro * so * cout * cin * kernel[0] * kernel[1]
    if name == "gather":
        x, bH, bW, idx = a[0], a[1], a[2], a[3]
        B, C = x.shape[:2]
        return "gather", 2 * e * B * idx.shape[0] * C * bH * bW, 0
    if name == "scatter_gather":
        x, y, bH, bW, idx = a[0], a[1], a[2], a[3], a[4]
        B, C = y.shape[:2]
        n = idx.shape[0]
        return "scatter_gather", 2 * e * B * n * C * bH * bW + 12 * n * bH * bW, 0
    if name == "scatter_fused":
        x, y, n = a[0], a[1], a[3]
        res = a[4] if len(a) > 4 else None
        full = 2 * e * y.numel()
        o2 = x.shape[2] * x.shape[3]
        return "scatter", full + e * y.shape[0] * n * y.shape[1] * o2 * (2 + (1 if res is not None else 0)), 0
    if name == "scatter_with_block_residual_fused":
        x0, y0, x1, n0, n1 = a[0], a[1], a[2], a[5], a[7]
        B, C = y0.shape[:2]
        return ("scatter_block_residual",
                2 * e * y0.numel() + 3 * e * B * n0 * C * x0.shape[2] * x0.shape[3]
                + 4 * e * B * n1 * C * x1.shape[2] * x1.shape[3], 0)
    if name == "block_conv":
        x, cout, kernel, stride = a[0], a[3], a[4], a[5]
        T, cin, R, S = x.shape
        ro, so = (R - kernel[0]) // stride[0] + 1, (S - kernel[1]) // stride[1] + 1
        return "block_conv_mfma", 0, 2 * T * ro * so * cout * cin * kernel[0] * kernel[1]
    if name in ("gather_conv", "scatter_gather_conv"):
        # fused producer + conv: MFMA-bound; flops of the conv only (the gather adds no flops worth counting)
        if name == "gather_conv":
            x, block, idx, cout, kernel, stride = a[0], a[1], a[2], a[8], a[9], a[10]
            T, cin = x.shape[0] * idx.shape[0], x.shape[1]
        else:
            y, block, idx, cout, kernel, stride = a[1], a[2], a[3], a[10], a[11], a[12]
            T, cin = y.shape[0] * idx.shape[0], y.shape[1]
        ro, so = (block[0] - kernel[0]) // stride[0] + 1, (block[1] - kernel[1]) // stride[1] + 1
        return "block_conv_mfma", 0, 2 * T * ro * so * cout * cin * kernel[0] * kernel[1]
    if name == "block_conv_direct":
        x, w, stride, groups = a[0], a[1], a[3], a[4]
        T, cin, R, S = x.shape
        cout, cig, kh, kw = w.shape
        ro, so = (R - kh) // stride[0] + 1, (S - kw) // stride[1] + 1
        return "block_conv_direct", 0, 2 * T * ro * so * cout * cig * kh * kw
    raise KeyError(name)


def a_numel(t):
    return t.numel()


def shape_key(name, a):
    parts = [name]
    for v in a:
        if isinstance(v, torch.Tensor):
            parts.append(tuple(v.shape))
        elif isinstance(v, (int, str, bool, tuple)) or v is None:
            parts.append(v)
    return tuple(parts)


def pmc_data_movement():
    """Counter bytes per launch of the data-movement rows (profiles/pmc_data_movement.json: rocprofv3 FETCH_SIZE / WRITE_SIZE passes
    over tools/profile_data_movement.py --pmc-manifest, reduced by tools/pmc_data_movement.py), if measured on THESE kernel sources."""
    try:
        with open(os.path.join(REPO, "profiles", "pmc_data_movement.json")) as f:
            d = json.load(f)
    except Exception:
        return {}
    if d.get("source_hash") != source_hash():
        return {}
    return {(r["op"], r["layout"], r["edit_ratio"]): r for r in d.get("rows", [])}


def data_movement_rooflines(hip, dev, pmc_manifest=None):
    """HBM roofline of the data-movement kernels that replace sige/cuda/gather_kernel.cu:7-67, scatter_gather_kernel.cu:8-67 and
    scatter_kernel.cu:8-44, standalone (the forward fuses most of them away), NCHW and channels-last, at a bandwidth-bound size
    (15 % edit, C = 256, B = 2, 256 x 256) and at the headline's launch-bound size (1.2 %, C = 128, B = 1).  Algorithmic bytes =
    SURVEY.md 8(d), reference out-of-place semantics; the in-place scatter is listed under its own name with the
    cache-preserving minimum.  HIP events on the launch stream, rotating buffer sets larger than the 256 MiB Infinity Cache.
    Next to the algorithmic bytes every row carries the COUNTER bytes of its launch (fabric-side reads, gfx950-corrected, + writes)
    when a PMC pass on these kernel sources is committed.  `pmc_manifest` (a list): the profiling mode of that pass -- no timing,
    three eager launches per row, their positions in the library's launch sequence appended to the list."""
    from sige_amd.utils import reduce_mask

    rows = []
    counters = {} if pmc_manifest is not None else pmc_data_movement()
    for ratio, B, C in ((0.15, 2, 256), (0.012, 1, 128)):
        mask = square_mask(ratio).to(dev)
        idx6 = reduce_mask(mask, 6, 4, 1)
        n6 = idx6.shape[0]
        smap = hip.get_scatter_map(256, 256, 6, 6, 3, 3, 1, 1, 1, 1, idx6)
        table = hip.tile_table(idx6, (1, 1), (1, 1), (4, 4), (256, 256))
        full_bytes = 4 * B * C * 256 * 256
        nsets = max(3, min(8, int(1.2e9 // (2 * full_bytes)) + 1))
        for layout in ("nhwc", "nchw"):
            fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
            ys = [torch.randn(B, C, 256, 256, device=dev).contiguous(memory_format=fmt) for _ in range(nsets)]
            rs = [torch.randn(B, C, 256, 256, device=dev).contiguous(memory_format=fmt) for _ in range(nsets)]
            t4 = [torch.randn(B * n6, C, 4, 4, device=dev).contiguous(memory_format=fmt) for _ in range(nsets)]
            sc, sh = torch.randn(1, C, 1, 1, device=dev), torch.randn(1, C, 1, 1, device=dev)
            e = 4
            gbytes = 2 * e * B * n6 * C * 36
            tile_bytes = e * B * n6 * C * 16
            cl = layout == "nhwc"
            ops = {
                "gather (6x6, affine + SiLU)": (gbytes, (lambda i: hip.gather_cl(ys[i], 6, 6, idx6, sc, sh, "swish")) if cl else
                                                (lambda i: hip.gather(ys[i], 6, 6, idx6, sc, sh, "swish", False))),
                "gather (6x6, raw)": (gbytes, (lambda i: hip.gather_cl(ys[i], 6, 6, idx6)) if cl else
                                      (lambda i: hip.gather(ys[i], 6, 6, idx6))),
                "scatter_gather (4x4 -> 6x6, affine + SiLU)": (gbytes + 12 * n6 * 36,
                                                               (lambda i: hip.scatter_gather_cl(t4[i], ys[i], 6, 6, idx6, smap, sc, sh, "swish")) if cl else
                                                               (lambda i: hip.scatter_gather(t4[i], ys[i], 6, 6, idx6, smap, sc, sh, "swish", False))),
                "scatter (out-of-place, + full residual)": (2 * full_bytes + 3 * tile_bytes,
                                                            (lambda i: hip.scatter_cl(t4[i], ys[i], (1, 1), (1, 1), idx6, table, rs[i])) if cl else
                                                            (lambda i: hip.scatter_fused(t4[i], ys[i], table, n6, rs[i]))),
            }
            if cl:
                ops["scatter (in-place persistent output, + full residual)"] = (
                    3 * tile_bytes, lambda i: hip.scatter_cl(t4[i], ys[i], (1, 1), (1, 1), idx6, table, rs[i], out=ys[(i + 1) % nsets]))
            for name, (nbytes, f) in ops.items():
                if pmc_manifest is not None:
                    f(0)
                    torch.cuda.synchronize()
                    n0 = hip.launch_count()
                    for i in range(3):
                        f((i + 1) % nsets)
                    torch.cuda.synchronize()
                    pmc_manifest.append({"op": name, "layout": layout, "edit_ratio": ratio, "alg_MB": round(nbytes / 1e6, 2),
                                         "first_launch": n0, "launches": hip.launch_count() - n0, "calls": 3})
                    continue
                it = [0]

                def rot():
                    f(it[0] % nsets)
                    it[0] += 1

                us = time_graph_of(rot, reps=nsets * 2)
                gbs = nbytes / us / 1e3
                row = {"op": name, "layout": layout, "edit_ratio": ratio, "B": B, "C": C, "active_tiles": int(n6),
                       "alg_MB": round(nbytes / 1e6, 2), "us": round(us, 2), "GBps": round(gbs, 1),
                       "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 4),
                       "regime": "bandwidth-bound" if nbytes / 6.3e6 > 10.0 else "launch-bound (< 10 us of traffic at the measured copy ceiling)"}
                cnt = counters.get((name, layout, ratio))
                if cnt is not None:  # what the launch moved according to the memory counters, and the rate that gives
                    row["counter_MB"] = cnt["counter_MB"]
                    row["counter_GBps"] = round(cnt["counter_MB"] * 1e3 / us, 1)
                    row["counter_frac_of_hbm_peak"] = round(cnt["counter_MB"] * 1e3 / us / PEAK_HBM_GBS, 4)
                rows.append(row)
            del ys, rs, t4
    if pmc_manifest is not None:
        return {}
    pick = lambda op, lay, r: next(x for x in rows if x["op"].startswith(op) and x["layout"] == lay and x["edit_ratio"] == r)  # noqa: E731
    g = pick("gather (6x6, affine", "nhwc", 0.15)
    sg = pick("scatter_gather", "nhwc", 0.15)
    so = pick("scatter (out-of-place", "nhwc", 0.15)

    def roof(x):
        return {"kernel": x["op"], "layout": x["layout"], "shape": "[%d,%d,256,256], %d active tiles (%.0f %% edit)"
                % (x["B"], x["C"], x["active_tiles"], x["edit_ratio"] * 100), "bound": "hbm", "alg_MB": x["alg_MB"], "us": x["us"],
                "achieved": x["GBps"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": x["frac_of_hbm_peak"],
                "traffic": int(x["counter_MB"] * 1e6) if "counter_MB" in x else None,
                "frac_on_counter_bytes": x.get("counter_frac_of_hbm_peak")}

    return {"data_movement": rows, "roofline_gather": roof(g), "roofline_scatter_gather": roof(sg), "roofline_hbm": roof(so)}


def kernel_families(trace):
    """Per-kernel accounting of one traced forward (warm, in-situ tensors): every distinct call shape is timed as a
    hipGraph of back-to-back launches; returns (families, per-shape records, JSON table, SIGE-conv TFLOP/s, total us)."""
    fam = {}
    per_cfg = {}
    for name, a, k, orig in trace:
        key = shape_key(name, a)  # (packed weights of the two matrix paths differ in size: distinct keys)
        if key not in per_cfg:
            family, nbytes, flops = op_cost(name, a, k)
            us = time_graph_of(lambda: orig(*a, **k), reps=8)
            per_cfg[key] = dict(family=family, bytes=nbytes, flops=flops, us=us, count=0, call=(orig, a, k))
        per_cfg[key]["count"] += 1
    for c in per_cfg.values():
        f = fam.setdefault(c["family"], dict(us=0.0, bytes=0, flops=0, launches=0))
        f["us"] += c["us"] * c["count"]
        f["bytes"] += c["bytes"] * c["count"]
        f["flops"] += c["flops"] * c["count"]
        f["launches"] += c["count"]
    kernels = {}
    for name, f in fam.items():
        kernels[name] = {"launches": f["launches"], "us_total": round(f["us"], 1)}
        if f["bytes"]:
            kernels[name]["alg_MB"] = round(f["bytes"] / 1e6, 1)
            kernels[name]["alg_GBps"] = round(f["bytes"] / f["us"] / 1e3, 1)
        if f["flops"]:
            kernels[name]["GFLOP"] = round(f["flops"] / 1e9, 2)
            kernels[name]["TFLOPs"] = round(f["flops"] / f["us"] / 1e6, 2)
    conv = [f for n, f in fam.items() if n.startswith("block_conv")]  # the active-block (SIGE) convs
    conv_tflops = sum(f["flops"] for f in conv) / max(1e-9, sum(f["us"] for f in conv)) / 1e6
    hot_us = sum(f["us"] for f in fam.values())
    return fam, per_cfg, kernels, conv_tflops, hot_us


def flop_by_compute(trace):
    """Conv FLOPs of one traced forward by the arithmetic they ran in ("f32" exact, "f16" operands, "f16x3" split operands): how
    the packed weights of each conv call were laid out (hip.PackedWeights.compute)."""
    by = {}
    for name, a, k, orig in trace:
        fam, nbytes, flops = op_cost(name, a, k)
        if not flops:
            continue
        comp = next((getattr(v, "compute", "f32") for v in list(a) + list((k or {}).values())
                     if isinstance(v, torch.Tensor) and type(v).__name__ == "PackedWeights"), "f32")
        comp = comp[:-1] if comp.endswith("w") else comp  # (wide packs are tagged "f16w" / "f16x3w" / "f32w")
        by[comp] = by.get(comp, 0.0) + flops
    tot = sum(by.values()) or 1.0
    return {c: round(v / tot, 4) for c, v in sorted(by.items())}


# ------------------------------------------------------ inputs shared by both legs --
def make_inputs():
    """The original image and the edit noise, on the CPU (both legs start from exactly these)."""
    gen = torch.Generator(device="cpu").manual_seed(1)
    x0 = torch.randn(1, 3, 256, 256, generator=gen)
    noise = torch.randn(1, 3, 256, 256, generator=gen)
    return x0, noise


def edit_mask(ratio, rank=0):
    """Each rank edits its own region of the shared original."""
    return square_mask(ratio, top=100 - 6 * rank, left=90 + 6 * rank)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, arrays, rank=0):
    """--dump-outputs: every array as <directory>/<name>.npy, float32, NCHW (rank r > 0: <name>_rank<r>.npy).  Weights, inputs
    and masks are seeded, so two builds run with the same arguments can be compared output for output."""
    import numpy as np

    host = {name: a.detach().float().contiguous().cpu().numpy() for name, a in arrays.items()}
    total = sum(v.nbytes for v in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError("--dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(directory, exist_ok=True)
    for name, v in host.items():
        np.save(os.path.join(directory, name + ("_rank%d" % rank if rank else "") + ".npy"), v)


# ---------------------------------------------------------------- cpu baseline --
CPU_THREADS_CAP = 32
CPU_THREADS_CAP_REASON = ("OpenMP over all 256 hardware threads of the GPU box is slower than 16-32 threads on loops this small "
                          "(124 tiles per layer at a 1.2 % edit; measured in round 2); SIGE_CPU_THREADS overrides")
REPO_MODEL = "repo workload on reference natives"
REFERENCE_MODEL = "reference sige.nn + diffusion/models/ddpm_arch/sige_fused_unet.py (unmodified) on oracle/_ref"


def cpu_threads():
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, int(os.environ.get("SIGE_CPU_THREADS", str(CPU_THREADS_CAP)))))


def reference_root():
    """The mounted reference (build container only; absent on the GPU box), or None."""
    root = os.environ.get("SIGE_REFERENCE", "/root/reference")
    ok = os.path.isfile(os.path.join(root, "diffusion", "models", "ddpm_arch", "sige_fused_unet.py")) and os.path.isdir(os.path.join(root, "sige", "nn"))
    return root if ok else None


def cpu_reference_unmodified(root, ratios, headline_ratio, seconds, cores):
    """BASELINE.md 3 to the letter: the reference's OWN `sige.nn` and `sige_fused_unet.py`, unmodified, on its
    compiled sige/cpu (oracle/_ref), in a process of its own (benchlib/ref_cpu_leg.py) with this run's weights / image / noise /
    masks.  Returns (times, {ratio: sparse output}) or None when that stack cannot be set up."""
    import subprocess
    import tempfile

    from oracle import build_ref
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    try:
        build_ref.load()
    except Exception:
        return None
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval()
    x0, noise = make_inputs()
    with tempfile.TemporaryDirectory() as d:
        job, out = os.path.join(d, "job.pt"), os.path.join(d, "out.pt")
        torch.save({"state": model.state_dict(), "x0": x0, "noise": noise, "masks": {r: edit_mask(r) for r in ratios},
                    "headline": headline_ratio}, job)
        cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "benchlib", "ref_cpu_leg.py"),
               "--reference", root, "--job", job, "--seconds", str(seconds), "--threads", str(cores), "--out", out]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=max(600.0, 20 * seconds))
        except subprocess.TimeoutExpired:
            return None
        if res.returncode != 0:
            sys.stderr.write("cpu_baseline: the unmodified reference stack failed, falling back to the repo workload:\n" + res.stderr[-1500:] + "\n")
            return None
        info = json.loads(res.stdout.strip().splitlines()[-1])
        return info["times"], torch.load(out)


def cpu_reference(ratios, headline_ratio, seconds):
    """The same weights, original image, noise and masks as the GPU run (rank 0's edit) on the host cores.  Returns
    (cpu_baseline dict, {ratio: sparse output}).
    * the reference is mounted (build container): its unmodified `sige.nn` + `sige_fused_unet.py` on oracle/_ref --
      `"model": REFERENCE_MODEL` (cpu_reference_unmodified);
    * otherwise (the GPU box: /root/reference does not exist there): this repo's DDPMSparseUNet / sige_amd.nn on the natives of
      oracle/_ref (the reference's own compiled sige/cpu backend, shipped as a .so) or, if that is absent, of the C restatement --
      `"model": REPO_MODEL`; the workload is pinned to the reference model by tests/test_reference_models.py
      (test_workload_unet_equals_reference_model); the tile convs are the reference's own F.conv2d call either way.
    Timing protocol: 5 warm-up + up to 20 timed sparse forwards at the headline ratio, bounded by
    `seconds`; `value` is quoted on the MEDIAN."""
    import statistics

    from oracle import build_ref, oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    cores = cpu_threads()
    outs, times, model_name, kind = {}, [], REPO_MODEL, None
    root = reference_root()
    if root is not None and seconds > 0:
        got = cpu_reference_unmodified(root, ratios, headline_ratio, seconds, cores)
        if got is not None:
            times, outs = got
            model_name, kind = REFERENCE_MODEL, "reference"
    if kind is None:
        ref = None
        try:
            ref = build_ref.load()
        except Exception:
            ref = None
        kind = "reference" if ref is not None else "port"
        # threads actually used: the affinity mask, capped (CPU_THREADS_CAP_REASON)
        torch.set_num_threads(cores)
        oracle.set_num_threads(cores)
        os.environ["OMP_NUM_THREADS"] = str(cores)
        runtime.register_backend("cpu", oracle.as_backend(ref) if ref is not None else oracle)
        try:
            torch.manual_seed(0)
            model = DDPMSparseUNet(DDPMConfig()).eval()
            x0, noise = make_inputs()
            t = torch.zeros(1)
            with torch.no_grad():
                model.set_mode("full")
                model(x0, t)
                for r in ratios:
                    mask = edit_mask(r)
                    model.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
                    model.set_mode("sparse")
                    outs[r] = model(x0 + noise * mask, t)
                if seconds > 0:
                    mask = edit_mask(headline_ratio)
                    x1 = x0 + noise * mask
                    model.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
                    t_begin = time.perf_counter()
                    for i in range(25):
                        t0 = time.perf_counter()
                        model(x1, t)
                        if i >= 5:
                            times.append(time.perf_counter() - t0)
                        if time.perf_counter() - t_begin > seconds and len(times) >= 3:
                            break
        finally:
            runtime.unregister_backend("cpu")
        natives = "oracle/_ref (reference sige/cpu)" if ref is not None else "oracle C restatement"
    else:
        natives = "oracle/_ref (reference sige/cpu)"
    base = None
    if times:
        med = statistics.median(times)
        base = {"value": round(1.0 / med, 3), "unit": "forward/s", "ms_per_forward": round(med * 1e3, 2),
                "ms_per_forward_mean": round(sum(times) / len(times) * 1e3, 2), "statistic": "median", "cores": cores,
                "host_cpus": os.cpu_count(), "kind": kind, "model": model_name, "threads_cap_reason": CPU_THREADS_CAP_REASON,
                "sample": "%d timed sparse DDPM-256 U-Net forwards at %.1f%% edit after 5 warm-ups (same weights, original "
                          "image, noise and masks as the GPU run; model = %s; native ops = %s, tile convs = torch CPU F.conv2d "
                          "as in sige/nn/base.py:88-89)" % (len(times), headline_ratio * 100, model_name, natives)}
    return base, outs


# ------------------------------------------------- BASELINE configs[2] / [3] sections --
def main_sd(args, world, rank, dev):
    """--workload sd: BASELINE.json configs[3] -- the Stable Diffusion v1 U-Net (860 M parameters, random init) on a 64 x 64
    latent with classifier-free-guidance batch 2, a 15 % square edit of the 512 x 512 image; N different edits of ONE original
    image, one per GPU, the original's activation cache distributed from rank 0 (same job definition as the DDPM headline)."""
    from sige_amd import hip, parallel
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet

    hip.lib()
    # the token GEMMs (nn.Linear as in the reference) on the fp32 solutions TunableOp measured fastest for these shapes on gfx950
    # (sige_amd/workloads/gemm_tuning.py); dense and sparse forwards alike
    from sige_amd.workloads import gemm_tuning

    tuned_gemms = False if args.no_tuned_gemms else gemm_tuning.enable_tuned_gemms()
    # MIOpen picks its convs (the dense baseline's, and the sparse forward's four plain ones) by measurement, as in the DDPM job: the
    # dense forward is 8 % faster for it (25.0 -> 23.0 ms: speedup_vs_dense is quoted against the better baseline), the sparse 0.5 %
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    model = SDUNet(SDConfig()).eval()
    n_params = sum(p.numel() for p in model.parameters())
    model = model.to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    model.set_compute_dtype(args.dtype)
    gen = torch.Generator().manual_seed(1)
    cl = lambda t_: t_.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    x0, noise = cl(torch.randn(2, 4, 64, 64, generator=gen)), cl(torch.randn(2, 4, 64, 64, generator=gen))
    ctx = torch.randn(2, 77, 768, generator=gen).to(dev)
    ts = torch.full((2,), 500.0, device=dev)
    mask512 = torch.zeros(512, 512, dtype=torch.bool, device=dev)
    mask512[150 - 8 * rank:348 - 8 * rank, 120 + 8 * rank:318 + 8 * rank] = True  # 15 %, every rank its own region
    masks = downsample_mask(mask512, min_res=8, dilation=1)  # stable-diffusion/runners/inpainting_runner.py:50-54
    x1 = cl(x0 + noise * masks[(64, 64)])
    run = lambda x: model(x, ts, context=ctx)  # noqa: E731
    res = {}
    with torch.no_grad():
        model.set_mode("full")
        dense_ms = None
        if rank == 0 and args.full:
            dense_ms, _, gd = _replay_ms(lambda: run(x1), k=10, warm=2)
            del gd
        run(x0 if rank == 0 else torch.zeros_like(x0))
        flat = parallel.pack_caches(model)
        n_cached = len(parallel.cache_slots(model))
        method, dist_info = None, {}
        if world > 1:
            names = ["broadcast", "scatter_allgather"] if args.distribute in ("auto", "recompute") else [args.distribute]
            cands = {m_: (lambda m_=m_: parallel.distribute_cache(flat, src=0, method=m_, model=model)) for m_ in names}
            choice = parallel.choose_distribution(cands, recompute=None, device=dev)  # (same selection + watchdog as the DDPM job)
            method = choice["method_chosen"]
            dist_info.update(method_chosen=method, methods_ms=choice["methods_ms"], watchdog_s=choice["watchdog_s"])
            if choice["errors"]:
                dist_info["errors"] = choice["errors"]
            cands[method]()
            chk = flat.double().sum().reshape(1)
            lo, hi = chk.clone(), chk.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist_info["cache_identical_on_all_ranks"] = bool(lo.item() == hi.item())
        model.set_masks(masks)
        model.set_mode("sparse")
        # the attention core / the token linears of the spatial transformers: the reference's rearrange / bmm / softmax / nn.Linear
        # chain against the library's kernels (sige_amd/workloads/sd_transformer.py: NATIVE_ATTENTION, NATIVE_LINEAR)
        from sige_amd.workloads import sd_transformer as _sdt

        routing, kernels_sd, roof_sd = {}, None, None
        if rank == 0 and args.full and world == 1:
            keep_flags = (_sdt.NATIVE_ATTENTION, _sdt.NATIVE_LINEAR, _sdt.BATCHED_QKV)
            ref_out = None
            for tag, att, lin, form, bq in (("reference_chain", False, False, 0, False), ("native_attention", True, False, 0, True),
                                            ("native_attention_separate_qkv_projections", True, False, 0, False),
                                            ("native_attention_32_queries_per_workgroup", True, False, 2, True),
                                            ("native_attention_and_linears", True, True, 0, False)):
                _sdt.NATIVE_ATTENTION, _sdt.NATIVE_LINEAR, _sdt.BATCHED_QKV = att, lin, bq
                if form and not hip.lib().has_tuning:
                    continue  # (a kernel-form comparison: only in the measurement build, SIGE_HIP_LIB=.../libsige_hip_tuning.so)
                if hip.lib().has_tuning:
                    hip.tuning_set("attention_form", form)
                run(x1)
                n0 = hip.launch_count()
                run(x1)
                nl = hip.launch_count() - n0
                ms_v, o_v, g_v = _replay_ms(lambda: run(x1), k=10, warm=2)
                if ref_out is None:
                    ref_out = o_v.float().clone()
                routing[tag] = {"forward_ms": round(ms_v, 3), "library_launches": nl, "max_abs_vs_reference_chain": round(float((o_v.float() - ref_out).abs().max()), 8)}
                del g_v
            _sdt.NATIVE_ATTENTION, _sdt.NATIVE_LINEAR, _sdt.BATCHED_QKV = keep_flags
            if hip.lib().has_tuning:
                hip.tuning_set("attention_form", 0)
            # per-kernel accounting of the library's launches in one forward (the same accounting as the DDPM headline's table)
            tracer = Tracer(hip)
            run(x1)
            tracer.log = []
            run(x1)
            tr_sd, tracer.log = tracer.log, None
            fam_sd, _, kernels_sd, conv_tf_sd, hot_sd = kernel_families(tr_sd)
            peak_sd = PEAK_F16_MFMA_TFS if args.dtype in ("f16", "f16x3") else PEAK_F32_MFMA_TFS
            dom = max(fam_sd, key=lambda n_: fam_sd[n_]["us"])
            ach = fam_sd[dom]["flops"] / max(1e-9, fam_sd[dom]["us"]) / 1e6
            roof_sd = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": peak_sd, "unit": "TFLOP/s", "frac": round(ach / peak_sd, 4),
                       "traffic": None, "launches_per_forward": fam_sd[dom]["launches"], "us_per_forward": round(fam_sd[dom]["us"], 1),
                       "library_kernel_us_per_forward": round(hot_sd, 1),
                       "note": "the library kernel family with the most time in one SD forward (warm in-situ tensors, every distinct call "
                               "shape timed as a hipGraph of back-to-back launches); the forward also runs torch kernels (LayerNorm, GEGLU, "
                               "adds, and the token linears unless NATIVE_LINEAR): forward_ms - library_kernel_us is theirs + launch gaps"}
            del tr_sd, tracer
        n0 = hip.launch_count()
        run(x1)
        launches = hip.launch_count() - n0
        g, out = capture_fn(lambda: run(x1))
        settle()
        for _ in range(args.warmup):
            g.replay()

        def job(with_distribution):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t_d = 0.0
            if with_distribution:
                if args.no_pipeline:
                    parallel.distribute_cache(flat, src=0, method=method, model=model)
                else:
                    parallel.distribute_cache_pipelined(flat, model, src=0, method=method, n_chunks=args.chunks)
                torch.cuda.synchronize()
                t_d = time.perf_counter() - t0
            for _ in range(args.steps):
                g.replay()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            return parallel.max_over_ranks(time.perf_counter() - t0, device=dev), parallel.max_over_ranks(t_d, device=dev)

        dt_steady, _ = job(False)
        dt, dist_s = job(True) if world > 1 else (dt_steady, 0.0)
        if args.dump_outputs:  # (the graph's output buffer still holds the last timed step)
            dump_outputs(args.dump_outputs, {"output": out}, rank)
        assert torch.isfinite(out).all()
        if args.full:
            g.replay()
            torch.cuda.synchronize()
            gpu_sparse = out.float().cpu()
    parity = None
    if rank == 0 and args.full and args.cpu_seconds > 0:
        # configs[3] AT ITS OWN SIZE against the reference's CPU path: the same 860 M-parameter U-Net (same seed), latent,
        # context and masks on the host cores, native ops from oracle/_ref (the reference's compiled sige/cpu) or the C
        # restatement, convs = torch CPU; one full + one sparse forward, outside every timed region
        from oracle import build_ref, oracle
        from sige_amd import runtime

        try:
            ref = build_ref.load()
        except Exception:
            ref = None
        n_thr = max(1, min(len(os.sched_getaffinity(0)), int(os.environ.get("SIGE_CPU_THREADS", "32"))))
        torch.set_num_threads(n_thr)
        oracle.set_num_threads(n_thr)
        runtime.register_backend("cpu", oracle.as_backend(ref) if ref is not None else oracle)
        try:
            torch.manual_seed(0)
            cpu_model = SDUNet(SDConfig()).eval()
            with torch.no_grad():
                t0 = time.perf_counter()
                cpu_model.set_mode("full")
                cpu_model(x0.cpu().contiguous(), ts.cpu(), context=ctx.cpu())
                cpu_model.set_masks(downsample_mask(mask512.cpu(), min_res=8, dilation=1))
                cpu_model.set_mode("sparse")
                t1 = time.perf_counter()
                cpu_sparse = cpu_model(x1.cpu().contiguous(), ts.cpu(), context=ctx.cpu())
                t2 = time.perf_counter()
            err = float((gpu_sparse - cpu_sparse).abs().max())
            tol = 1e-3 if args.dtype in ("f32", "f16x3") else None
            parity = {"parity_max_abs": round(err, 7), "parity_max_ref": round(float(cpu_sparse.abs().max()), 4),
                      "parity_against": ("oracle/_ref (reference sige/cpu)" if ref is not None else "oracle C restatement")
                                        + " + torch CPU convs, the same 860 M-parameter U-Net / latent / context / masks",
                      "cpu_baseline": {"value": round(1.0 / (t2 - t1), 4), "unit": "forward/s", "ms_per_forward": round((t2 - t1) * 1e3, 1),
                                       "cores": n_thr, "host_cpus": os.cpu_count(), "kind": "reference" if ref is not None else "port",
                                       "sample": "ONE sparse SD U-Net forward (CFG batch 2) after one full forward (%.1f s)" % (t1 - t0)}}
            if tol is not None:
                parity.update(parity_tolerance=tol, parity_ok=bool(err <= tol))
            del cpu_model
        finally:
            runtime.unregister_backend("cpu")
    if rank == 0:
        ms_steady = dt_steady * 1e3 / args.steps
        line = {"metric": "Stable Diffusion v1 U-Net sparse (SIGE) forwards/s", "value": round(world * args.steps / dt, 2),
                "unit": "forward/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(dt * 1e3 / args.steps, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": args.dtype, "data": "synthetic",
                "config": {"workload": "Stable Diffusion v1 U-Net (320 ch, mult 1-2-4-4, %.0fM params, random init), latent [2,4,64,64] "
                                       "(CFG batch 2), text context [2,77,768], 15%% square edit of the 512x512 image, %d different edits of "
                                       "one original image, one per GPU, hipGraph replay, NHWC, in-place scatter buffers%s"
                                       % (n_params / 1e6, world, "; the timed job = distribute the original's cache from rank 0 (%s) + %d "
                                          "sparse forwards per rank" % (method, args.steps) if world > 1 else ""),
                           "edit_ratio": 0.15, "batch_per_gpu": 2, "parallelism": "dp%d" % world},
                "forward_ms": round(ms_steady, 4)}
        if dense_ms is not None:
            line.update(dense_forward_ms=round(dense_ms, 3), speedup_vs_dense=round(dense_ms / ms_steady, 2))
        line.update({
            "hip_kernel_launches_per_forward": launches, "cache_bytes": int(flat.numel() * 4), "cached_tensors": n_cached,
            "active_token_ratio_64": round(float(masks[(64, 64)].float().mean()), 4),
            "native_attention": bool(_sdt.NATIVE_ATTENTION), "native_linear": bool(_sdt.NATIVE_LINEAR), "batched_qkv": bool(_sdt.BATCHED_QKV),
            "tuned_token_gemms": bool(tuned_gemms)})
        if routing:
            line["attention_routing"] = routing
        if roof_sd is not None:
            line["roofline"] = roof_sd
            line["kernels"] = kernels_sd
        if world > 1:
            step_s = dt_steady / args.steps
            line["multi_gpu"] = dict(dist_info, method=method, cache_distribution_ms=round(dist_s * 1e3, 3),
                                     value_steady_state_cache_resident=round(world * args.steps / dt_steady, 2),
                                     value_cache_refreshed_every_step=round(world / (dist_s + step_s), 2),
                                     efficiency=round(dt_steady / dt, 4))
        if parity is not None:
            line.update(parity)
        from benchlib.line import emit

        emit(line, name="bench_detail_sd.json")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ---------------------------------------------------------------- launching --
def settle():
    """Before the warm-up of a timed region: host buffers of earlier pageable uploads are freed NOW (their driver registration goes
    with them), and the queue eviction that causes -- restored tens of ms later, DESIGN 3.15 -- has passed before anything is timed.
    Outside every timed region; nothing the measured work depends on."""
    import gc

    torch.cuda.synchronize()
    gc.collect()
    time.sleep(0.3)
    torch.cuda.synchronize()


def self_launch(args):
    """`python bench.py --gpus N` without a torchrun environment: run under torch.distributed.run, one rank per GPU, in a child
    process (this one has initialised the GPU already), and exit with its status."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    n_vis = torch.cuda.device_count()
    if n_vis < args.gpus and not args.oversubscribe:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (args.gpus, n_vis))
    import socket

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    sys.stdout.flush()
    import subprocess

    raise SystemExit(subprocess.call(cmd, env=env))


def source_hash():
    from sige_amd import build

    return build.source_hash()


def pmc_traffic(family, dtype="f32"):
    """HBM-side bytes per launch of a kernel family from the committed rocprofv3 PMC pass -- bench.py cannot run the
    profiler on itself -- but ONLY if that pass was taken on exactly these kernel sources (hash of sige_amd/csrc +
    include/, recorded by tools/pmc_traffic.py) and under THIS compute dtype (the f16 forward runs other kernels:
    profiles/pmc_traffic_f16.json); otherwise (None, why)."""
    name = "pmc_traffic.json" if dtype == "f32" else "pmc_traffic_%s.json" % dtype
    path = os.path.join(REPO, "profiles", name)
    try:
        with open(path) as f:
            d = json.load(f)
    except Exception:
        return None, "no profiles/%s" % name
    if d.get("source_hash") != source_hash():
        return None, "profiles/%s was measured on different kernel sources (stale): not reported" % name
    fam = d.get("families", {}).get(family)
    if fam is None:
        return None, "family %s not in profiles/%s" % (family, name)
    return int(fam["traffic_MB_per_launch"] * 1e6), d.get("provenance", "profiles/" + name)


# ------------------------------------------------------------------------ main --
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also run every section besides the headline timing: dense baseline, per-kernel accounting and rooflines, "
                         "sweeps, other precisions, mask-change latencies, stacked edits, GauGAN / SD transformer, CPU baseline and "
                         "parity (the options below that tune those sections apply only with --full)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write the output of the last timed step as DIR/output.npy (float32, NCHW; "
                         "rank r > 0: output_rank<r>.npy)")
    ap.add_argument("--ratio", type=float, default=0.012, help="edit ratio of the headline workload")
    ap.add_argument("--sweep", default="0.012,0.05,0.15", help="edit ratios for the sweep section ('' = skip)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline timing (0 = skip the CPU leg)")
    ap.add_argument("--dump-calls", default="", help="write the per-call-shape table of the headline forward (us, GFLOP) to this JSON file")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--layout", default="nhwc", choices=["nhwc", "nchw"],
                    help="memory format of the activations: nhwc = torch.channels_last (default), nchw = the reference's")
    ap.add_argument("--no-inplace-scatter", action="store_true",
                    help="Scatter modules return a fresh full tensor per call (reference semantics) instead of "
                         "updating a persistent output buffer")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16", "f16x3"],
                    help="arithmetic of the tile convs: f32 = exact fp32 products (BASELINE configs[1], the headline); f16 = fp16 "
                         "operands on the fp16 matrix cores, fp32 accumulation and storage (BASELINE configs[4])")
    ap.add_argument("--f16-sweep", default="0.01,0.02,0.05,0.1,0.2",
                    help="edit ratios of the f16-compute section a default (f32) run appends ('' = skip)")
    ap.add_argument("--x3-sweep", default="0.012,0.05,0.15",
                    help="edit ratios of the split-fp16-operand (f16x3) section a default (f32) run appends ('' = skip)")
    ap.add_argument("--no-dynamic", action="store_true", help="skip the mask-change / multi-step section")
    ap.add_argument("--no-extras", action="store_true", help="skip the GauGAN (configs[2]) and SD transformer (configs[3]) sections")
    ap.add_argument("--no-tuned-gemms", action="store_true", help="--workload sd: the token GEMMs on the libraries' default solutions "
                    "instead of the table of sige_amd/workloads/gemm_tuning.py")
    ap.add_argument("--workload", default="ddpm", choices=["ddpm", "sd"],
                    help="ddpm = BASELINE configs[1] (the headline; what a plain `bench.py` measures); sd = configs[3], the Stable "
                         "Diffusion v1 U-Net, N different edits of one original image one per GPU")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (nccl = RCCL; gloo only to "
                    "exercise the multi-rank code path without N GPUs)")
    ap.add_argument("--oversubscribe", action="store_true", help="debugging: all ranks on GPU 0 (with --backend gloo): runs the "
                    "multi-rank code path on a one-GPU box; the numbers mean nothing")
    ap.add_argument("--distribute", default="auto", choices=["auto", "broadcast", "scatter_allgather", "recompute"],
                    help="N > 1: collective that distributes the original image's cache")
    ap.add_argument("--no-pipeline", action="store_true", help="N > 1: one collective over the whole cache, then the local refresh "
                    "(default: chunks in module order, refresh of chunk k overlapped with the transfer of chunk k+1)")
    ap.add_argument("--chunks", type=int, default=8, help="N > 1: chunks of the pipelined cache distribution")
    ap.add_argument("--wire-dtype", default="f32", choices=["f32", "f16"],
                    help="N > 1: the cached activations travel as fp16 (half the bytes; every rank, the source included, ends up with "
                         "the same fp16-rounded cache; the cached affines stay fp32).  Only with --dtype f16: the rounding costs up to "
                         "1.6e-3 of output error at 15 %% edit (profiles/r3_f16_cache_trace.json) -- inside the f16 criterion, outside "
                         "the fp32 path's 1e-3")
    ap.add_argument("--batched-ratios", default="0.05,0.15", help="stacked edits also at these edit ratios (E = 1 and 8), '' = skip")
    ap.add_argument("--batched-edits", default="1,2,4,8,16",
                    help="stacked edits (sige_amd/stacked.py): batch sizes E of the throughput section, '' = skip")
    ap.add_argument("--cache-dtype", default="auto", choices=["auto", "f32", "f16"],
                    help="how the full pass's cached activations are STORED (SIGEModel.set_cache_dtype): auto = f16 with --dtype f16 "
                         "(half the resident cache and half the bytes of its distribution, no conversion passes; cached affines stay "
                         "fp32), f32 otherwise (the reference; the fp32 path's 1e-3 needs it)")
    args = ap.parse_args()
    if args.cache_dtype == "auto":
        args.cache_dtype = "f16" if args.dtype == "f16" else "f32"
    if args.cache_dtype == "f16" and args.dtype != "f16":
        ap.error("--cache-dtype f16 goes with --dtype f16 (an fp16-rounded cache does not keep the fp32 path's 1e-3)")
    if args.wire_dtype == "f16" and args.dtype != "f16":
        ap.error("--wire-dtype f16 goes with --dtype f16 (an fp16-rounded cache does not keep the fp32 path's 1e-3)")
    if args.dump_calls and not args.full:
        ap.error("--dump-calls goes with --full (the per-call table comes from the per-kernel accounting)")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path; see DESIGN.md)")
    self_launch(args)
    from benchlib.line import reserve_stdout

    reserve_stdout()  # (whatever a library prints to stdout -- RCCL's banner, at exit -- goes to stderr: the contract line stays the last line)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d "
                         "(or plain `python bench.py --gpus %d`, which does that itself)" % (args.gpus, world, args.gpus, args.gpus))
    if args.oversubscribe:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime

        limit = datetime.timedelta(seconds=300)  # (a collective that hangs fails the run in minutes, not after the default 10-30)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=limit)
        else:
            dist.init_process_group("gloo", timeout=limit)
        from benchlib.line import flush_c_stdio

        flush_c_stdio()  # (RCCL's banner, written through C stdio when the communicator is created: out now, not at exit)

    if args.workload == "sd":
        return main_sd(args, world, rank, dev)

    from sige_amd import hip, parallel
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    hip.lib()
    tracer = Tracer(hip)
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).to(dev).eval()  # random init: no checkpoints offline
    n_params = sum(p.numel() for p in model.parameters())
    x0_cpu, noise_cpu = make_inputs()
    x0, noise = x0_cpu.to(dev), noise_cpu.to(dev)
    if args.layout == "nhwc":
        model = model.to(memory_format=torch.channels_last)
        x0, noise = x0.contiguous(memory_format=torch.channels_last), noise.contiguous(memory_format=torch.channels_last)
    inplace = args.layout == "nhwc" and not args.no_inplace_scatter
    model.set_scatter_inplace(inplace)
    model.set_compute_dtype(args.dtype, edit_ratio=args.ratio)  # (the f16 precision policy depends on the edited area)
    if args.layout == "nhwc":
        model.set_cache_dtype(args.cache_dtype)
    mfma_peak = PEAK_F16_MFMA_TFS if args.dtype in ("f16", "f16x3") else PEAK_F32_MFMA_TFS
    t = torch.zeros(1, device=dev)

    def edited(ratio):
        m = edit_mask(ratio, rank).to(dev)
        return m, x0 + noise * m

    result = {}
    gpu_out = {}  # edit ratio -> sparse output of the benchmarked artefact (rank 0), for the parity check
    with torch.no_grad():
        # ---- dense baseline: the stock U-Net forward on the same GPU (rank 0) ------
        dense_ms = None
        if rank == 0 and args.full:
            model.set_mode("full")
            model.set_plain_dense(True)
            mask, x1 = edited(args.ratio)
            kd = max(10, args.steps // 10)
            gd, _ = capture(model, x1, t)
            dense_ms = timed_replays(gd, kd, 3, 1) * 1e3 / kd
            del gd
            dense_by_layout = {args.layout: round(dense_ms, 3)}
            if args.layout == "nhwc":
                # the stock model in the reference's own layout too; the baseline is the faster of the two
                model.to(memory_format=torch.contiguous_format)
                gd, _ = capture(model, x1.contiguous(), t)
                d2 = timed_replays(gd, kd, 3, 1) * 1e3 / kd
                del gd
                model.to(memory_format=torch.channels_last)
                dense_by_layout["nchw"] = round(d2, 3)
                dense_ms = min(dense_ms, d2)
            result["dense_forward_ms_by_layout"] = dense_by_layout
            model.set_plain_dense(False)

        # ---- the alternative to distributing the cache: every rank recomputes it (the full pass on the library's kernels,
        #      split fp16 operands: fp32-level, deterministic -- the same bits on every rank; no communication) ----
        recompute_ms = None
        gf, gf_caches = None, None
        if world > 1 and args.layout == "nhwc":
            try:
                model.set_compute_dtype("f16x3")
                model.set_mode("full")
                gf, _ = capture(model, x0, t)
                # the cache tensors this graph writes (static: they live in the graph's pool); the model is re-pointed at views of
                # the packed buffer below, so a recompute = replay + one copy per cache tensor into those views
                gf_caches = [parallel._get(s) for s in parallel.cache_slots(model)]
                recompute_ms = round(parallel.max_over_ranks(timed_replays(gf, 5, 2, 1) * 1e3 / 5, device=dev), 3)
            except Exception as e:  # (never the reason a scaling run dies)
                recompute_ms = repr(e)[:200]
                gf, gf_caches = None, None
            model.set_compute_dtype(args.dtype)

        # ---- cache of the original image: rank 0 computes it, one collective distributes it ----
        model.set_mode("full")
        model(x0 if rank == 0 else torch.zeros_like(x0), t)  # ranks > 0 only need the cache SLOTS (shapes) here
        flat = parallel.pack_caches(model)  # every ORIGINAL cache tensor is now a view of `flat`
        n_cached = len(parallel.cache_slots(model))
        torch.cuda.synchronize()
        dist_info = {}
        distribute = None
        wire = torch.float16 if args.wire_dtype == "f16" else None
        recompute_cache = None
        if world > 1:
            cache_views = [parallel._get(s) for s in parallel.cache_slots(model)]
            if gf is not None and len(gf_caches) == len(cache_views) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(gf_caches, cache_views)):
                def recompute_cache():
                    """No communication: this rank's own full pass (library kernels, split fp16 operands: the same bits on every
                    rank), copied into the packed cache the sparse graph reads, derived buffers refreshed."""
                    gf.replay()
                    torch._foreach_copy_(cache_views, gf_caches)
                    parallel.refresh_derived(model)
            # measured ONCE at start-up, the same decision on every rank: broadcast | scatter + all-gather | recompute; a
            # collective that takes longer than parallel.WATCHDOG_S (or raises) on any rank is dropped
            names = ["broadcast", "scatter_allgather"] if args.distribute == "auto" else ([] if args.distribute == "recompute" else [args.distribute])
            cands = {m_: (lambda m_=m_: parallel.distribute_cache(flat, src=0, method=m_, model=model, wire_dtype=wire)) for m_ in names}
            choice = parallel.choose_distribution(cands, recompute=recompute_cache if args.distribute in ("auto", "recompute") else None, device=dev)
            distribute = choice["method_chosen"]
            dist_info.update(method_chosen=distribute, methods_ms=choice["methods_ms"], fallback=choice["fallback"], watchdog_s=choice["watchdog_s"])
            if choice["errors"]:
                dist_info["errors"] = choice["errors"]
            # one more run of the winner, so that what the ranks hold now is what the timed job will hand them: rank 0's cache (a
            # collective) or each rank's own recomputation (deterministic: the checksum comparison below covers it)
            (recompute_cache if distribute == "recompute" else cands[distribute])()
            # every rank now holds rank 0's cache: compare checksums
            chk = torch.tensor([parallel.checksum(flat)], dtype=torch.int64, device=dev)
            lo, hi = chk.clone(), chk.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist_info["cache_identical_on_all_ranks"] = bool(lo.item() == hi.item())

        def prepare(ratio):
            if args.dtype == "f16":  # (the f16 precision policy of the model depends on the edited area)
                model.set_compute_dtype("f16", edit_ratio=ratio)
            m, xe = edited(ratio)
            model.set_masks(downsample_mask(dilate_mask(m, 5), 8))  # diffusion/runner.py:157-165
            model.set_mode("sparse")
            return xe

        # ---- headline: sparse forward at --ratio ----------------------------------
        x1 = prepare(args.ratio)
        model(x1, t)  # packs weights, builds tile tables, registers the activated twins
        model(x1, t)  # builds the twins' persistent buffers (library launches since round 4: not part of a steady-state forward)
        trace, e_ms = None, None
        if args.full:
            tracer.log = []
            n0, p0 = hip.launch_count(), hip.conv_pairs_fused()
            model(x1, t)
            launches_per_forward = hip.launch_count() - n0  # kernels libsige_hip.so launched for one sparse forward
            pairs_per_forward = hip.conv_pairs_fused() - p0  # (shortcut, conv1) pairs that shared a launch
            trace, tracer.log = tracer.log, None
            e_ms = eager_ms(model, x1, t, 20)
        g, out = capture(model, x1, t)
        settle()
        for _ in range(args.warmup):
            g.replay()

        # timed region.  N = 1: K graph replays.  N > 1: ONE job = the original image's cache distributed from rank 0
        # (one collective + the local refresh of what is derived from it) followed by K sparse forwards per rank.
        def timed_job(with_distribution):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t_d = 0.0
            if with_distribution:
                # chunks in module order, issued asynchronously; what a rank derives from the cache is refreshed chunk by
                # chunk while later chunks still move (in place: the captured graph's buffers keep their addresses)
                if distribute == "recompute":
                    recompute_cache()
                elif args.no_pipeline:
                    parallel.distribute_cache(flat, src=0, method=distribute, model=model, wire_dtype=wire)
                else:
                    parallel.distribute_cache_pipelined(flat, model, src=0, method=distribute, n_chunks=args.chunks, wire_dtype=wire)
                torch.cuda.synchronize()
                t_d = time.perf_counter() - t0
            for _ in range(args.steps):
                g.replay()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            dt_ = time.perf_counter() - t0
            return parallel.max_over_ranks(dt_, device=dev), parallel.max_over_ranks(t_d, device=dev)

        dt_steady, _ = timed_job(False)
        if world > 1:
            dt, dist_s = timed_job(True)
        else:
            dt, dist_s = dt_steady, 0.0
        ms_per_step = dt * 1e3 / args.steps
        ms_steady = dt_steady * 1e3 / args.steps
        if args.dump_outputs:  # (the graph's output buffer still holds the last timed step)
            dump_outputs(args.dump_outputs, {"output": out}, rank)
        assert torch.isfinite(out).all()
        if args.full:
            g.replay()
            torch.cuda.synchronize()
            gpu_out[args.ratio] = out.float().cpu()

        if rank == 0 and args.full:
            # ---- per-kernel accounting of the hot path (warm, in-situ tensors) ----
            fam, per_cfg, kernels, conv_tflops, hot_us = kernel_families(trace)
            if args.dump_calls:  # the per-call-shape table behind `kernels` (which layers are furthest from the matrix rate)
                rows = [{"call": repr(key)[:400], "family": c["family"], "count": c["count"], "us": round(c["us"], 2),
                         "GFLOP": round(c["flops"] / 1e9, 4), "TFLOPs": round(c["flops"] / max(1e-9, c["us"]) / 1e6, 2),
                         "MB": round(c["bytes"] / 1e6, 3)} for key, c in per_cfg.items()]
                with open(args.dump_calls, "w") as f:
                    json.dump(sorted(rows, key=lambda r: -r["us"] * r["count"]), f, indent=1)
            result.update(kernels=kernels, hot_path_us=round(hot_us, 1), block_conv_tflops=round(conv_tflops, 2),
                          launches_per_forward=launches_per_forward, conv_pairs_per_forward=pairs_per_forward,
                          launches_note="conv calls = launches + pairs; K-split convs finish inside their launch (no second pass)")

            # ---- roofline of the dominant hot-path kernel family ---------------------
            if not args.no_roofline:
                dom = max((n for n in fam if n != "dense_conv_mfma"), key=lambda n: fam[n]["us"])  # hot path = the SIGE ops
                cfgs = [c for c in per_cfg.values() if c["family"] == dom]
                # cold measurement: clone the inputs into >= 6 rotating sets so that the
                # 256 MiB Infinity Cache does not serve them
                tot_us, tot_work, launches = 0.0, 0.0, 0
                for c in cfgs:
                    orig, a, k = c["call"]
                    nbytes_in = sum(v.numel() * v.element_size() for v in a if isinstance(v, torch.Tensor))
                    nsets = max(2, min(8, int(600e6 // max(1, nbytes_in)) + 1))
                    sets = [tuple(v.clone() if isinstance(v, torch.Tensor) and v.is_floating_point() and v.numel() > 4096
                                  else v for v in a) for _ in range(nsets)]
                    it = [0]

                    def rot():
                        orig(*sets[it[0] % nsets], **k)
                        it[0] += 1

                    us = time_graph_of(rot, reps=nsets * 2)
                    tot_us += us * c["count"]
                    tot_work += (c["flops"] if c["flops"] else c["bytes"]) * c["count"]
                    launches += c["count"]
                    del sets
                is_mfma = fam[dom]["flops"] > 0
                achieved = tot_work / tot_us / (1e6 if is_mfma else 1e3)
                peak = mfma_peak if is_mfma else PEAK_HBM_GBS
                traffic, traffic_note = pmc_traffic(dom, args.dtype)
                result["roofline"] = {
                    "kernel": dom, "bound": "mfma" if is_mfma else "hbm",
                    "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s" if is_mfma else "GB/s",
                    "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_note,
                    "launches_per_forward": launches, "avg_launch_us": round(tot_us / launches, 2),
                    "work_per_launch": round(tot_work / launches / (1e9 if is_mfma else 1e6), 4),
                    "work_unit": "GFLOP" if is_mfma else "MB",
                    "note": "algorithmic work of all %d launches of this kernel family in one forward / their summed "
                            "duration (hipGraph of back-to-back launches, HIP events on the launch stream, "
                            "rotating input sets); traffic = fabric-side bytes per launch from a rocprofv3 PMC pass "
                            "(FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE, separate runs; Infinity-Cache hits "
                            "included), printed only when that pass was taken on these exact kernel sources" % launches}
                result.update(data_movement_rooflines(hip, dev))
        del trace

        # ---- the same forward with the reference's out-of-place Scatter semantics (a fresh tensor per call) ----
        if rank == 0 and inplace and args.full:
            model.set_scatter_inplace(False)
            model(x1, t)
            g2, out2 = capture(model, x1, t)
            k2 = max(20, args.steps // 4)
            result["forward_ms_out_of_place"] = round(timed_replays(g2, k2, 5, 1) * 1e3 / k2, 4)
            # (same values up to fp32 summation order: the unfused tile convs may split K across workgroups)
            result["out_of_place_vs_in_place_max_abs"] = round(float((out2 - out).abs().max()), 8)
            del g2, out2
            model.set_scatter_inplace(True)
        del g

        # ---- edit-ratio sweep (rank 0 only, short) -----------------------------------
        sweep = []
        if rank == 0 and args.full and args.sweep and world == 1:  # (at N > 1 the other ranks would idle in the final barrier)
            for r in [float(v) for v in args.sweep.split(",")]:
                xs = prepare(r)
                model(xs, t)
                tracer.log = []
                model(xs, t)
                tr, tracer.log = tracer.log, None
                costs = [op_cost(n, a, k) for n, a, k, o in tr]
                flops = sum(c[2] for c in costs if c[0] != "dense_conv_mfma")
                _, _, kern_r, conv_tf_r, _ = kernel_families(tr)  # the metric: active-block conv TFLOP/s vs edit ratio
                gs, outs = capture(model, xs, t)
                k = max(20, args.steps // 4)
                ms = timed_replays(gs, k, 5, 1) * 1e3 / k
                gpu_out[r] = outs.float().cpu()
                n256 = max([a[3].shape[0] for n, a, kk, o in tr if n in ("gather", "gather_cl", "gather_conv_cl") and a[0].shape[2] == 256]
                           + [a[2].shape[0] for n, a, kk, o in tr if n == "gather_conv" and a[0].shape[2] == 256] + [0])
                sweep.append({"edit_ratio": r, "forward_ms": round(ms, 3), "speedup_vs_dense": round(dense_ms / ms, 2),
                              "active_tiles_256": n256, "block_conv_GFLOP": round(flops / 1e9, 2),
                              "block_conv_TFLOPs": round(conv_tf_r, 2), "block_conv_frac_of_mfma_peak": round(conv_tf_r / mfma_peak, 4),
                              "block_conv_us": kern_r.get("block_conv_mfma", {}).get("us_total"),
                              "dense_remainder_us": kern_r.get("dense_conv_mfma", {}).get("us_total")})
                del gs, tr, outs

        # ---- the tile conv v3 (csrc/conv_tile3.hpp): routed by the library from sige_amd.hip.TILE3_MIN_BLOCKS = 512 v3 workgroups on
        #      (decided in C per launch); the same forward with the router off, at the edit ratios where launches reach the threshold ----
        tile3 = None
        if rank == 0 and args.full and world == 1 and args.dtype == "f32" and args.layout == "nhwc" and args.sweep and not args.no_extras:
            rows3 = []
            keep3 = hip.TILE3_MIN_BLOCKS
            try:
                for r in (0.15, 0.20):
                    xs = prepare(r)
                    row = {"edit_ratio": r}
                    for tag, th in (("router_off", 1 << 30), ("default", keep3)):
                        hip.TILE3_MIN_BLOCKS = th
                        model(xs, t)
                        model(xs, t)
                        gs, outs = capture(model, xs, t)
                        row[tag + "_ms"] = round(timed_replays(gs, 20, 5, 1) * 1e3 / 20, 4)
                        if tag == "router_off":
                            base3 = outs.clone()
                        else:
                            row["max_abs_vs_router_off"] = round(float((outs - base3).abs().max()), 8)
                        del gs, outs
                    rows3.append(row)
                tile3 = {"min_blocks": keep3, "rows": rows3,
                         "note": "launch by launch: profiles/r5h_tile3_bench.json; in the forward: profiles/r5j_sequence_15pct_*.csv"}
            except Exception as e:
                tile3 = {"error": repr(e)[:300]}
            finally:
                hip.TILE3_MIN_BLOCKS = keep3
            prepare(args.ratio)

        # ---- f16 compute (BASELINE.json configs[4]): the same forward with fp16 operands on the fp16 matrix cores ----
        f16 = None
        gpu_out_f16 = {}
        if rank == 0 and args.full and world == 1 and args.dtype == "f32" and args.f16_sweep and args.layout == "nhwc":
            rows = []
            for r in [float(v) for v in args.f16_sweep.split(",")]:
                model.set_compute_dtype("f16", edit_ratio=r)  # (the model's precision policy depends on the edited area)
                xs = prepare(r)
                model(xs, t)
                tracer.log = []
                model(xs, t)
                tr16, tracer.log = tracer.log, None
                _, _, _, conv_tf_r, _ = kernel_families(tr16)
                frac16 = flop_by_compute(tr16)
                gs, outs = capture(model, xs, t)
                k = max(20, args.steps // 4)
                ms = timed_replays(gs, k, 5, 1) * 1e3 / k
                gpu_out_f16[r] = outs.float().cpu()
                rows.append({"edit_ratio": r, "forward_ms": round(ms, 3), "speedup_vs_dense_fp32": round(dense_ms / ms, 2),
                             "block_conv_TFLOPs": round(conv_tf_r, 2), "kept_at_higher_precision": list(model.compute_policy["keep"]),
                             "conv_flop_fraction_by_arithmetic": frac16, "fp16_flop_fraction": frac16.get("f16", 0.0)})
                del tr16
                del gs, outs
            model.set_compute_dtype("f16", edit_ratio=args.ratio)
            xs = prepare(args.ratio)
            model(xs, t)
            tracer.log = []
            model(xs, t)
            tr, tracer.log = tracer.log, None
            _, _, kern16, conv_tf16, _ = kernel_families(tr)
            gs, outs = capture(model, xs, t)
            k = max(20, args.steps // 2)
            ms16 = timed_replays(gs, k, 5, 1) * 1e3 / k
            gpu_out_f16[args.ratio] = outs.float().cpu()
            del gs, outs, tr
            f16 = {"what": "convs with fp16 operands (v_mfma_f32_32x32x16_f16 / 16x16x32_f16), fp32 accumulation; activations, "
                           "caches and every other kernel fp32; GroupNorm affine + SiLU fused in fp32 before the down-convert; "
                           "for edits above the model's F16_KEEP_ABOVE (5 % of the image) the convs named in F16_KEEP (from the "
                           "per-layer error trace profiles/r3a_f16_error_trace.json; `kept_at_higher_precision` per sweep row) run "
                           "split fp16 operands (f16x3: fp32-level) or, below 2 GFLOP per launch, exact fp32; the 4 stride-2 "
                           "downsample convs are always exact fp32",
                   "keep_higher_precision_above_edit_ratio": getattr(model, "F16_KEEP_ABOVE", None),
                   "keep_higher_precision": list(getattr(model, "F16_KEEP", ())),
                   "forward_ms": round(ms16, 4), "edit_ratio": args.ratio, "speedup_vs_dense_fp32": round(dense_ms / ms16, 2),
                   "speedup_vs_f32_sparse": round(ms_steady / ms16, 2), "sweep": rows, "kernels": kern16,
                   "block_conv_tflops": round(conv_tf16, 2),
                   "roofline": {"kernel": "block_conv_mfma (f16 compute)", "bound": "mfma", "achieved": round(conv_tf16, 2),
                                "peak": PEAK_F16_MFMA_TFS, "unit": "TFLOP/s", "frac": round(conv_tf16 / PEAK_F16_MFMA_TFS, 4),
                                "note": "launch / latency-bound: at the fp16 rate the matrix work of a launch is 0.1-0.5 us, the "
                                        "rest of its ~5 us is the kernel boundary, the index -> gather -> LDS prologue chain and "
                                        "the epilogue (warm in-situ tensors, hipGraph of back-to-back launches)"}}
            model.set_compute_dtype("f32")

        # ---- split fp16 operands ("f16x3"): fp32-level results on the fp16 matrix cores -- dense remainder + the full pass ----
        x3 = None
        gpu_out_x3 = {}
        if rank == 0 and args.full and world == 1 and args.dtype == "f32" and args.x3_sweep and args.layout == "nhwc":
            model.set_compute_dtype("f16x3")
            rows = []
            kern_x3 = None
            for r in [float(v) for v in args.x3_sweep.split(",")]:
                xs = prepare(r)
                model(xs, t)
                model(xs, t)
                n0 = hip.launch_count()
                tracer.log = []
                model(xs, t)
                trx, tracer.log = tracer.log, None
                nl = hip.launch_count() - n0
                if kern_x3 is None:
                    kern_x3 = kernel_families(trx)[2]
                del trx
                gs, outs = capture(model, xs, t)
                k = max(20, args.steps // 4)
                ms = timed_replays(gs, k, 5, 1) * 1e3 / k
                gpu_out_x3[r] = outs.float().cpu()
                rows.append({"edit_ratio": r, "forward_ms": round(ms, 4), "speedup_vs_dense_fp32": round(dense_ms / ms, 2), "launches": nl})
                del gs, outs
            # the cache-producing full pass (sige/nn/base.py:85-86; one per denoising step in the reference's sampler,
            # diffusion/samplers/ddim_ddpm_sampler.py:60-66): stock torch / MIOpen in fp32 against the library's kernels
            from sige_amd.nn import dense as _dense

            full = {}
            for cdt in ("f32", "f16x3", "f32_native"):
                model.set_compute_dtype("f32" if cdt == "f32_native" else cdt)
                _dense.FULL_PASS_F32_NATIVE = cdt == "f32_native"  # exact fp32 products on the library's dense-layer kernel
                model.set_mode("full")
                gf, outf = capture(model, x0, t)
                kf = max(10, args.steps // 10)
                full[cdt] = timed_replays(gf, kf, 3, 1) * 1e3 / kf
                full[cdt + "_out"] = outf.float().clone()
                del gf, outf
            _dense.FULL_PASS_F32_NATIVE = False
            full_delta_native = float((full["f32_out"] - full.pop("f32_native_out")).abs().max())
            full_delta = float((full.pop("f32_out") - full.pop("f16x3_out")).abs().max())
            # restore the fp32 cache of the original for everything that follows
            model.set_compute_dtype("f32")
            model.set_mode("full")
            model(x0, t)
            flat = parallel.pack_caches(model)
            base = rows[0]["forward_ms"] if rows else None
            x3 = {"what": "every fp32 operand of a dense-layer conv split into fp16 hi + lo, products hi*hi + lo*hi + hi*lo on "
                          "v_mfma_f32_32x32x16_f16, fp32 accumulation (22-bit operands; weights pre-scaled by a power of two): "
                          "the dense remainder of the sparse pass (layers >= 1 GFLOP) and the cache-producing full pass; tile convs "
                          "stay exact fp32",
                  "forward_ms": base, "sweep": rows, "kernels": kern_x3,
                  "full_pass_ms": {"torch_miopen_f32": round(full["f32"], 3), "library_f16x3": round(full["f16x3"], 3),
                                   "speedup": round(full["f32"] / full["f16x3"], 2),
                                   "max_abs_output_delta": round(full_delta, 7),
                                   "library_f32_exact": round(full["f32_native"], 3),
                                   "library_f32_exact_max_abs_output_delta": round(full_delta_native, 7),
                                   "note": "library = the dense-layer conv (conv_wide.hpp) with cat / nearest upsampling / residual sum "
                                           "inside the launch, GroupNorm affines from the per-channel statistics the convs leave (no pass "
                                           "over the tensor), small convs and downsamples on the tile kernels; no torch conv / norm / "
                                           "elementwise op left except the timestep embedding"},
                  "step_ms_full_plus_sparse": {"f32": round(full["f32"] + ms_steady, 3),
                                               "f32_exact_library_full_pass": round(full["f32_native"] + ms_steady, 3),
                                               "f16x3": round(full["f16x3"] + (base or ms_steady), 3),
                                               "note": "one denoising step of the reference's sampler = full pass on the original + "
                                                       "sparse pass on the edit (ddim_ddpm_sampler.py:60-73)"}}

        # ---- a new edit arrives (mask change), and one cache per denoising step (cache_id) ----
        dyn = None
        if rank == 0 and args.full and world == 1 and not args.no_dynamic and args.layout == "nhwc":
            import statistics

            model.set_compute_dtype(args.dtype)
            tms = {"set_masks": [], "first_forward_eager": [], "recapture": []}
            for i in range(4):
                m, xe = edited(0.012 + 0.004 * i)  # (a different mask every time: nothing is memoised)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                model.set_mode("sparse")
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                model(xe, t)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                gm, _ = capture_fn(lambda: model(xe, t), warm=0)  # (capture only: the eager forward above was the warm-up)
                gm.replay()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                del gm
                tms["set_masks"].append((t1 - t0) * 1e3)
                tms["first_forward_eager"].append((t2 - t1) * 1e3)
                tms["recapture"].append((t3 - t2) * 1e3)
            med = {k: round(statistics.median(v), 3) for k, v in tms.items()}
            # (b) what a host that re-captures per mask does (sige_amd/graphs.py): one capture stream + one memory pool for every
            #     capture, and the capture IS the first forward under the new mask
            from sige_amd.graphs import GraphPool

            gp = GraphPool(dev, CAPTURE_MODE)
            tcf = {"set_masks": [], "capture": [], "first_replay": []}
            gprev = None
            cf_equal = True
            for i in range(6):
                # (two edit sizes in turn, the first visit of each warms the pool up: a steady interactive session -- a LARGER edit
                #  than any before grows the pool once, by hipMalloc inside the capture, which is not what is timed here)
                m, xe = edited((0.013, 0.021)[i % 2])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                model.set_mode("sparse")
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                del gprev  # (its blocks are what this capture reuses)
                gprev, oc = gp.capture(lambda: model(xe, t))
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                gprev.replay()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                if i >= 2:
                    tcf["set_masks"].append((t1 - t0) * 1e3)
                    tcf["capture"].append((t2 - t1) * 1e3)
                    tcf["first_replay"].append((t3 - t2) * 1e3)
                    cf_equal = cf_equal and bool(torch.equal(oc, model(xe, t)))
            del gprev, gp
            # (c) a launch plan (sige_amd/plan.py, include/sige_hip.h sige_hip_plan_*): the library calls of the mask pipeline and of
            #     the forward recorded ONCE, replayed from C with the new mask's tile counts -- no Python per launch, no re-capture
            plan_info = None
            try:
                from sige_amd.plan import FORWARD as P_FWD, MASKS as P_MASKS, LaunchPlan

                def build_masks(mk):
                    return downsample_mask(dilate_mask(mk, 5), 8)

                m0, xe0 = edited(0.012)
                xs = xe0.clone()  # (the plan's static input)
                plan = LaunchPlan(model, dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan.record(m0, build_masks, lambda: model(xs, t))
                torch.cuda.synchronize()
                record_ms = (time.perf_counter() - t0) * 1e3
                tp = {"bind_mask": [], "run_from_c": [], "capture": [], "first_replay": []}
                plan_equal, counts_seen = True, []
                for i in range(8):
                    m, xe = edited((0.013, 0.021, 0.05, 0.012)[i % 4])
                    xs.copy_(xe)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    plan.bind_mask(m)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    got = plan.run()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    got = got.clone()
                    plan.capture()
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    rep = plan.replay()
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    plan_equal = plan_equal and bool(torch.equal(rep, got))
                    if i >= 4:
                        tp["bind_mask"].append((t1 - t0) * 1e3)
                        tp["run_from_c"].append((t2 - t1) * 1e3)
                        tp["capture"].append((t3 - t2) * 1e3)
                        tp["first_replay"].append((t4 - t3) * 1e3)
                    # the reference for this mask: the module-level (Python) path, twins warm
                    model.set_masks(build_masks(m))
                    model.set_mode("sparse")
                    model(xe, t)
                    plan_equal = plan_equal and bool(torch.equal(model(xe, t), got))
                    counts_seen.append(sum(plan.counts))
                # steady state of the C-issued eager forward (no graph at all) and of the plan's own graph
                kp = max(20, args.steps)
                plan.bind_mask(m0)
                xs.copy_(xe0)
                torch.cuda.synchronize()

                def batches(fn, n=5):
                    # median of n batches of kp calls: ONE batch is what a queue eviction (a freed host buffer of an
                    # earlier upload, restored tens of ms later) lands in -- r5's last run printed 2.58 ms for a 1.41 ms forward
                    out_ = []
                    for _ in range(n):
                        t0_ = time.perf_counter()
                        for _ in range(kp):
                            fn()
                        torch.cuda.synchronize()
                        out_.append((time.perf_counter() - t0_) * 1e3 / kp)
                    return statistics.median(out_), out_

                run_ms, run_all = batches(plan.run)
                plan.capture()
                plan.replay()
                torch.cuda.synchronize()
                replay_ms, replay_all = batches(plan.replay)
                medp = {k: round(statistics.median(v), 3) for k, v in tp.items()}
                plan_info = dict(
                    medp, record_once_ms=round(record_ms, 2), to_first_output_ms=round(medp["bind_mask"] + medp["run_from_c"], 3),
                    to_first_output_with_graph_ms=round(medp["bind_mask"] + medp["capture"] + medp["first_replay"], 3),
                    forward_ms_issued_from_c=round(run_ms, 4), forward_ms_plan_graph=round(replay_ms, 4),
                    forward_ms_batches={"issued_from_c": [round(v, 4) for v in run_all], "plan_graph": [round(v, 4) for v in replay_all],
                                        "statistic": "median of 5 batches of %d" % kp},
                    calls={"masks": plan.calls(P_MASKS), "forward": plan.calls(P_FWD)}, shape_bound=plan.shape_bound,
                    output_equals_module_forward_bit_for_bit=plan_equal, tile_counts_seen=sorted(set(counts_seen)),
                    note="ONE recording serves every later mask: bind_mask = copy the mask, replay the recorded mask pipeline (dilate, "
                         "pyramid, compaction, one count read-back, scatter maps, tile tables, in-place refresh of the persistent outputs "
                         "and twins); run = the recorded forward issued from C with the new counts; capture = the same calls into a "
                         "hipGraph for the steady state")
                del plan
            except Exception as e:  # (never the reason the headline dies)
                plan_info = {"error": repr(e)[:300]}
            model.set_masks(downsample_mask(dilate_mask(edit_mask(args.ratio, rank).to(dev), 5), 8))
            # K denoising steps with one cache per step (set_cache_id(k), sige/nn/scatter.py:59-60, diffusion_demo/runner.py:134-164)
            K = 4
            x1m = prepare(args.ratio)
            graphs = []
            for cid in range(K):
                model.set_cache_id(cid)
                model.set_mode("full")
                model(x0 * (1.0 - 0.05 * cid), t)  # (a different "x_t" per step)
                model.set_mode("sparse")
                model(x1m, t)
                graphs.append(capture(model, x1m, t)[0])
            reps = max(5, args.steps // K)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                for g_ in graphs:
                    g_.replay()
            torch.cuda.synchronize()
            per_step = (time.perf_counter() - t0) * 1e3 / (reps * K)
            del graphs
            model.set_cache_id(0)
            medc = {k: round(statistics.median(v), 3) for k, v in tcf.items()}
            dyn = {"mask_change_ms": round(med["set_masks"] + med["first_forward_eager"], 3), "mask_change_parts_ms": med,
                   "mask_change_capture_first": dict(
                       medc, to_first_output_with_graph_ms=round(sum(medc.values()), 3),
                       eager_then_recapture_to_graph_ms=round(sum(med.values()), 3), output_equals_eager=cf_equal,
                       note="sige_amd.graphs.GraphPool: one capture stream + one memory pool for every capture (torch.cuda.graph gives "
                            "each capture a new pool and empties the allocator cache first), and the capture itself is the first "
                            "forward under the new mask: new mask -> first output AND the steady-state graph"),
                   "mask_change_plan": plan_info,
                   "mask_change_note": "new edit -> first sparse output: set_masks (device mask pyramid, every index list, ONE device->host "
                                       "read) + the first eager forward (tile tables, scatter maps); `recapture` = capturing and "
                                       "replaying a hipGraph for the new mask (what a multi-step loop on that mask then amortises)",
                   "multi_step": {"steps": K, "caches": K, "sparse_ms_per_step_one_cache_per_step": round(per_step, 4),
                                  "note": "K hipGraphs, one per cache_id, replayed round-robin: every step reads a DIFFERENT 673 MB "
                                          "cache (no cross-step cache residency); parity of cache_id > 0 is a -m gpu test"}}
            prepare(args.ratio)

    # ---- stacked edits ("throughput mode"): E edits of ONE original, each with its own mask, through one set of launches ----
    batched = None
    if rank == 0 and args.full and world == 1 and not args.no_dynamic and args.layout == "nhwc" and args.batched_edits:
        from sige_amd import stacked
        from sige_amd.nn import dense as _dense

        def build_pyr(mk):
            return downsample_mask(dilate_mask(mk, 5), 8)

        def place(e):  # (eight different places: the masks of a batch do not overlap much)
            r_ = batch_ratio[0]
            mod = 208 if r_ == args.ratio else 256 - int(round(r_ ** 0.5 * 256))  # (the whole square inside the image)
            return square_mask(r_, top=(16 + 61 * e) % mod, left=(24 + 97 * e) % mod).to(dev)

        batch_ratio = [args.ratio]

        try:
            with torch.no_grad():
                model.set_compute_dtype(args.dtype)
                model.clear_cache()  # (the multi-step section left one cache per cache id)
                model.set_cache_id(0)
                model.set_mode("full")
                model(x0, t)  # (a fresh, unpacked cache of the original: stacking replaces the cache tensors)
                Es = [int(v) for v in args.batched_edits.split(",")]
                emax = max(Es)
                mks = [place(e) for e in range(emax)]
                singles = []
                for mk in mks:
                    model.set_masks(build_pyr(mk))
                    model.set_mode("sparse")
                    xi = x0 + noise * mk
                    model(xi, t)
                    singles.append(model(xi, t).clone())
                rows = []
                wide_keep = dict(_dense.WIDE_MIN_FLOP_F32_STACKED)
                for E in Es:
                    routes = ("tile",) if E == 1 else (("tile", "wide", "wide2", "f16x3") if E == emax and args.dtype == "f32" else ("tile", "wide"))
                    for route in routes:
                        # `wide` / `wide2`: dense 3x3 layers of at least 8 / 2 GFLOP on the dense-layer kernel in its exact-fp32 form
                        # (stacking makes the dense remainder E times as many pixels: matrix-bound there, 0.7-0.8 of the fp32 MFMA peak:
                        # DESIGN 3.7); `f16x3`: split fp16 operands (fp32-level results) wherever a launch is matrix-bound
                        # (the library's stacked-mode default is the `wide` route; `tile` switches it off for the comparison)
                        _dense.WIDE_MIN_FLOP_F32_STACKED = ({3: 2.0e9, 1: 1.0e30} if route == "wide2" else {3: 1.0e30, 1: 1.0e30} if route == "tile"
                                                            else {3: 8.0e9, 1: 1.0e30})
                        model.set_compute_dtype("f16x3" if route == "f16x3" else args.dtype)
                        xe = torch.cat([x0 + noise * mk for mk in mks[:E]], 0).contiguous(memory_format=torch.channels_last)
                        if E > 1:
                            stacked.stack_caches(model, E)
                        try:
                            if E > 1:
                                stacked.set_masks(model, [build_pyr(mk) for mk in mks[:E]])
                            else:
                                model.set_masks(build_pyr(mks[0]))
                            model.set_mode("sparse")
                            with stacked.edit_batch(model, E):
                                gb, ob = capture(model, xe, t)
                                kb = max(20, args.steps // 2)
                                ms = timed_replays(gb, kb, 5, 1) * 1e3 / kb
                                err = max(float((ob[e] - singles[e][0]).abs().max()) for e in range(E))
                                n0 = hip.launch_count()
                                tracer.log = []
                                model(xe, t)
                                trb, tracer.log = tracer.log, None
                                nl = hip.launch_count() - n0
                                _, _, kern_b, conv_tf_b, _ = kernel_families(trb)
                                del trb, gb, ob
                        finally:
                            if E > 1:
                                stacked.unstack_caches(model)
                        rows.append({"edits": E, "dense_route": route, "ms_per_launch_set": round(ms, 4), "ms_per_edit": round(ms / E, 4),
                                     "forwards_per_s": round(E / ms * 1e3, 1), "launches": nl,
                                     "max_abs_vs_single_edit_forward": round(err, 8),
                                     "block_conv_TFLOPs": round(conv_tf_b, 2), "block_conv_frac_of_mfma_peak": round(conv_tf_b / mfma_peak, 4),
                                     "dense_conv_TFLOPs": kern_b.get("dense_conv_mfma", {}).get("TFLOPs"),
                                     "block_conv_us": kern_b.get("block_conv_mfma", {}).get("us_total"),
                                     "dense_remainder_us": kern_b.get("dense_conv_mfma", {}).get("us_total"),
                                     "dense_conv_wide": kern_b.get("dense_conv_wide")})
                        if E == emax:
                            rows[-1]["kernels"] = kern_b
                _dense.WIDE_MIN_FLOP_F32_STACKED = wide_keep
                model.set_compute_dtype(args.dtype)
                # the same at the sweep's larger edits: E = 1 and 8, the library's own routing
                other = []
                for ratio in [float(v) for v in args.batched_ratios.split(",") if v]:
                    batch_ratio[0] = ratio
                    mks_r = [place(e) for e in range(8)]
                    for E in (1, 8):
                        xe = torch.cat([x0 + noise * mk for mk in mks_r[:E]], 0).contiguous(memory_format=torch.channels_last)
                        if E > 1:
                            stacked.stack_caches(model, E)
                        try:
                            if E > 1:
                                stacked.set_masks(model, [build_pyr(mk) for mk in mks_r[:E]])
                            else:
                                model.set_masks(build_pyr(mks_r[0]))
                            model.set_mode("sparse")
                            with stacked.edit_batch(model, E):
                                gb, ob = capture(model, xe, t)
                                ms = timed_replays(gb, 20, 5, 1) * 1e3 / 20
                                tracer.log = []
                                model(xe, t)
                                trb, tracer.log = tracer.log, None
                                _, _, kern_b, conv_tf_b, _ = kernel_families(trb)
                                del trb, gb, ob
                        finally:
                            if E > 1:
                                stacked.unstack_caches(model)
                        other.append({"edit_ratio": ratio, "edits": E, "ms_per_launch_set": round(ms, 4), "ms_per_edit": round(ms / E, 4),
                                      "forwards_per_s": round(E / ms * 1e3, 1), "block_conv_TFLOPs": round(conv_tf_b, 2),
                                      "block_conv_frac_of_mfma_peak": round(conv_tf_b / mfma_peak, 4),
                                      "dense_conv_wide": kern_b.get("dense_conv_wide")})
                batch_ratio[0] = args.ratio
                base = next(r for r in rows if r["edits"] == 1)["forwards_per_s"]
                best = {}
                for r in rows:
                    if r["edits"] not in best or r["forwards_per_s"] > best[r["edits"]]["forwards_per_s"]:
                        best[r["edits"]] = r
                batched = {"edit_ratio": args.ratio, "rows": rows, "rows_at_other_edit_ratios": other,
                           "speedup_forwards_per_s_vs_one_edit": {str(e): round(best[e]["forwards_per_s"] / base, 2) for e in sorted(best)},
                           "note": "sige_amd/stacked.py + sige_hip_set_edit_batch: E edited versions of one original, each with its OWN mask at "
                                   "its own place, stacked along H into one tall image (the same bytes as [E,C,H,W] channels-last; masks, "
                                   "index lists, maps and the original's cache stacked alike): every layer is still ONE launch, which now "
                                   "sees the active tiles of all E edits; halo rows across an image seam are zero padding inside the "
                                   "kernels; first / last conv, attention and the output GroupNorm run per image with batch E.  "
                                   "ms_per_edit = time of one stacked forward / E; parity against each edit's own single-edit forward "
                                   "(fp32 summation order only).  The reference batches only under a SHARED mask (sige/cpu/gather.cpp:17-21)"}
                # restore the single-edit state the sections below expect
                model.clear_cache()
                model.set_mode("full")
                model(x0, t)
                flat = parallel.pack_caches(model)
                prepare(args.ratio)
        except Exception as e:  # (never the reason the headline dies)
            batched = {"error": repr(e)[:400]}
            try:
                stacked.unstack_caches(model)
                hip.set_edit_batch(1)
            except Exception:
                pass

    extras = {}
    if rank == 0 and args.full and world == 1 and not args.no_extras and args.layout == "nhwc":
        for key, fn in (("gaugan", lambda: gaugan_section(dev, cpu_parity=args.cpu_seconds > 0)), ("sd_transformer", lambda: sd_transformer_section(dev))):
            try:
                extras[key] = fn()
            except Exception as e:  # the headline must not die with an auxiliary section
                extras[key] = {"error": repr(e)[:300]}
            torch.cuda.empty_cache()

    if world > 1:
        dist.barrier()
    if rank == 0:
        cpu = None
        parity = None
        if args.full and args.cpu_seconds > 0:
            # the benchmarked artefact (this layout, in-place buffers, hipGraph replay) against the reference's CPU path on
            # the SAME weights / image / noise / masks: max |gpu - cpu| per edit ratio, outside every timed region
            ratios = sorted(set(gpu_out) | set(gpu_out_f16) | set(gpu_out_x3))
            cpu, cpu_out = cpu_reference(ratios, args.ratio, args.cpu_seconds if world == 1 else 0.0)
            parity = {("%g" % r): round(float((gpu_out[r] - cpu_out[r]).abs().max()), 7) for r in sorted(gpu_out)}
            if f16 is not None:
                from sige_amd import tolerance

                chk = {("%g" % r): tolerance.f16_check(gpu_out_f16[r], cpu_out[r]) for r in sorted(gpu_out_f16)}
                f16["parity_vs_fp32_reference"] = chk
                f16["parity_max_abs_vs_fp32_reference"] = {k: v["max_abs"] for k, v in chk.items()}
                f16["parity_tolerance"] = tolerance.F16_CRITERION + " (the same criterion in tests/test_gpu_round3.py)"
                f16["parity_ok"] = bool(all(v["ok"] for v in chk.values()))
            if x3 is not None:
                x3["parity_max_abs_vs_fp32_reference"] = {("%g" % r): round(float((gpu_out_x3[r] - cpu_out[r]).abs().max()), 7)
                                                          for r in sorted(gpu_out_x3)}
                x3["parity_tolerance"] = 1e-3
                x3["parity_ok"] = bool(max(x3["parity_max_abs_vs_fp32_reference"].values()) <= 1e-3)
        line = {
            "metric": "DDPM-256 U-Net sparse (SIGE) forwards/s",
            "value": round(world * args.steps / dt, 2),
            "unit": "forward/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "DDPM 256x256 church U-Net (ch128, mult 1-1-2-2-4-4, %.1fM params, random init), "
                                   "%.1f%% square edit, one edited image per GPU, hipGraph replay, %s activations%s%s%s"
                                   % (n_params / 1e6, args.ratio * 100, args.layout.upper(),
                                      ", f16-compute tile convs (fp16 MFMA operands, fp32 accumulate / storage)" if args.dtype == "f16" else "",
                                      ", in-place scatter buffers" if inplace else "",
                                      "; the timed job = distribute the original image's cache from rank 0 (%s) + %d sparse "
                                      "forwards per rank" % (distribute, args.steps) if world > 1 else ""),
                       "edit_ratio": args.ratio, "batch_per_gpu": 1, "resolution": 256,
                       "parallelism": "dp%d" % world},
            "rccl_ranks": dist.get_world_size() if world > 1 else 1, "backend": args.backend if world > 1 else None,
            "devices": [torch.cuda.get_device_name(i) for i in range(min(world, torch.cuda.device_count()))],
            "forward_ms": round(ms_steady, 4),
        }
        if args.full:
            line.update(forward_ms_eager=round(e_ms, 3), dense_forward_ms=round(dense_ms, 3), speedup_vs_dense=round(dense_ms / ms_steady, 2))
        line.update(cache_bytes=int(flat.numel() * flat.element_size()), cache_dtype=args.cache_dtype, cached_tensors=n_cached)
        if args.full:
            line["sweep"] = sweep
        if world > 1:
            step_s = dt_steady / args.steps
            line["multi_gpu"] = dict(
                dist_info, method=distribute, pipelined=not args.no_pipeline, chunks=None if args.no_pipeline else args.chunks,
                rccl_ranks_seen=dist.get_world_size(),
                wire_dtype=args.wire_dtype, wire_bytes=int(flat.numel() * (2 if (wire is not None or flat.dtype == torch.float16) else 4)),
                cache_distribution_ms=round(dist_s * 1e3, 3),
                recompute_full_pass_ms=recompute_ms,
                value_cache_distribution_inside_job=round(world * args.steps / dt, 2),
                value_steady_state_cache_resident=round(world * args.steps / dt_steady, 2),
                value_cache_refreshed_every_step=round(world / (dist_s + step_s), 2),
                efficiency=round(dt_steady / dt, 4),
                efficiency_note="value(N) / (N x steady-state value of one rank): the timed job (one cache distribution + K forwards per "
                                "rank, max over ranks) against the same K forwards with the cache resident -- what the distribution "
                                "costs a %d-step job; the north_star asks >= 0.85 at 8 GPUs" % args.steps,
                note="`value` counts ONE cache distribution (collective + local refresh of derived buffers) inside the timed "
                     "job of %d steps; steady_state = the same replays with the cache already resident; every_step = a fresh "
                     "cache per step (SDEdit-style), computed from the two measured times; recompute_full_pass_ms = what every rank "
                     "would spend recomputing the cache itself instead (library full pass, split fp16 operands, hipGraph), max over "
                     "ranks" % args.steps)
        line.update(result)
        # the >= 6x target of north_star is quoted against the stock dense forward (MIOpen: SURVEY.md 8d); the same forward on this
        # library's own dense-layer kernels is faster than MIOpen, so both ratios are printed
        fp = (x3 or {}).get("full_pass_ms") or {}
        if dense_ms is not None:
            line["speedup_vs_dense_detail"] = {
                "vs_miopen": round(dense_ms / ms_steady, 2),
                "vs_library_full_pass_f32_exact": round(fp["library_f32_exact"] / ms_steady, 2) if fp.get("library_f32_exact") else None,
                "vs_library_full_pass_f16x3": round(fp["library_f16x3"] / ms_steady, 2) if fp.get("library_f16x3") else None,
                "note": "dense forward of the same U-Net on the same GPU / this sparse forward: MIOpen fp32 (best of NCHW / NHWC; the "
                        "contract of SURVEY.md 8d), the library's own exact-fp32 full pass, the library's full pass on split fp16 operands"}
        if parity is not None:
            line["parity_max_abs"] = parity
            if args.dtype == "f16":
                from sige_amd import tolerance

                chk = {("%g" % r): tolerance.f16_check(gpu_out[r], cpu_out[r]) for r in sorted(gpu_out)}
                line["parity_vs_fp32_reference"] = chk
                line["parity_tolerance"] = tolerance.F16_CRITERION
                line["parity_ok"] = bool(all(v["ok"] for v in chk.values()))
            else:
                line["parity_tolerance"] = 1e-3
                line["parity_ok"] = bool(max(parity.values()) <= 1e-3)
            line["parity_against"] = "oracle/_ref (reference sige/cpu) + torch CPU convs, same weights / inputs / masks"
        if f16 is not None:
            line["f16_compute"] = f16
        if x3 is not None:
            line["f16x3_compute"] = x3
        if dyn is not None:
            line["dynamic"] = dyn
            plan_row = dyn.get("mask_change_plan") or {}
            if plan_row.get("forward_ms_issued_from_c") is not None:
                # the forward WITHOUT a graph, issued by the launch plan from C (what a caller that cannot capture pays), beside
                # forward_ms_eager = the same launches issued one by one from Python through ctypes
                line["forward_ms_eager_launch_plan"] = plan_row["forward_ms_issued_from_c"]
        if tile3 is not None:
            line["tile_conv3"] = tile3
        if batched is not None:
            line["batched_edits"] = batched
        line.update(extras)
        if cpu is not None:
            line["cpu_baseline"] = cpu
        from benchlib.line import emit

        emit(line)  # the detail file + an earlier stdout line carry everything; the LAST line is the <= 4 KB contract line
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
