#!/usr/bin/env python3
"""The library's token linear (csrc/token_linear.hip) against what it replaces, per launch, at every (tokens M, width C) of the SD
U-Net's sparse forward (bench.py --workload sd: same model, latent, context; the token counts are read off the transformer blocks of one
sparse forward under the mask).  Per transformer block six launches:

    qkv        LayerNorm -> [q | k | v]          vs  add_layer_norm_tokens (LayerNorm only) + the strided-batched matmul of BATCHED_QKV
    to_out     x . W^T + bias + residual   (x 2) vs  F.linear (its add is the next row's helper)
    attn2.q    LayerNorm -> q                    vs  add_layer_norm_tokens (add + bias + LayerNorm) + F.linear
    ff.proj    LayerNorm -> GEGLU projection     vs  add_layer_norm_tokens + F.linear (bias) + geglu_tokens
    ff.out     h . W^T + bias + residual         vs  F.linear + add_bias_tokens

each timed as a hipGraph of back-to-back repeats (benchlib.common.time_graph_of: us per call including the launch boundary; the
smaller of two timings), the GEMM
side once on the libraries' default solutions and once with the shipped TunableOp table on (sige_amd/workloads/gemm_tuning.py).
`--forms`: also both row-block forms of the token linear (measurement build, SIGE_HIP_TUNE_TOKEN_LINEAR_FORM), not only the one the
library picks.  Two masks: the benchmarked one and one whose token counts the TunableOp table does not hold.

    python tools/token_linear_bench.py --out out/token_linear_bench.json
"""
import argparse
import collections
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from benchlib.common import PEAK_F32_MFMA_TFS, time_graph_of  # noqa: E402

MASKS = {"bench": (150, 348, 120, 318), "other": (100, 260, 200, 440)}  # rows, columns of the 512 x 512 edit mask


def table_token_counts():
    """The M of every GEMM row of the shipped TunableOp table (tn_<N>_<M>_<K>_...)."""
    from sige_amd.workloads.gemm_tuning import TABLE

    ms = set()
    for line in open(TABLE):
        f = line.strip().split(",")
        if len(f) > 1 and f[0] != "Validator":
            ms.add(int(f[1].split("_")[2]))
    return ms


def block_shapes(mask_box, dev):
    """{(M, C, on the switch's path): transformer blocks per forward} of the SD U-Net's sparse forward under the mask.  A block whose
    transformer is not tiled (the middle block's 8 x 8 level) gets no K / V scatter and keeps its path whatever TOKEN_LINEAR says."""
    from sige_amd.utils import downsample_mask
    from sige_amd.workloads.sd_transformer import TransformerBlock
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet

    torch.manual_seed(0)
    model = SDUNet(SDConfig()).eval().to(dev).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    gen = torch.Generator().manual_seed(1)
    cl = lambda t_: t_.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    x0, noise = cl(torch.randn(2, 4, 64, 64, generator=gen)), cl(torch.randn(2, 4, 64, 64, generator=gen))
    ctx = torch.randn(2, 77, 768, generator=gen).to(dev)
    ts = torch.full((2,), 500.0, device=dev)
    shapes = {}
    with torch.no_grad():
        for name, (r0, r1, c0, c1) in mask_box.items():
            model.set_mode("full")
            model(x0, ts, context=ctx)
            mask512 = torch.zeros(512, 512, dtype=torch.bool, device=dev)
            mask512[r0:r1, c0:c1] = True
            masks = downsample_mask(mask512, min_res=8, dilation=1)
            model.set_masks(masks)
            model.set_mode("sparse")
            seen = collections.Counter()
            note = lambda mod, a, kw, seen=seen: seen.update([(a[0].shape[0] * a[0].shape[1], a[0].shape[2], kw.get("kv_scatter") is not None)])  # noqa: E731
            hooks = [m.register_forward_pre_hook(note, with_kwargs=True) for m in model.modules() if isinstance(m, TransformerBlock)]
            model(cl(x0 + noise * masks[(64, 64)]), ts, context=ctx)
            for h in hooks:
                h.remove()
            shapes[name] = dict(seen)
    del model
    torch.cuda.empty_cache()
    return shapes


def rows_of(M, C, dev, hip, forms, reps):
    """The six launches of one block at (M, C): library us, GEMM-library us on the default and on the tuned solutions."""
    from sige_amd.workloads import gemm_tuning

    g = torch.Generator().manual_seed(M * 7 + C)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x, d, o, h = rn(1, M, C), rn(1, M, C), rn(1, M, C), rn(1, M, 4 * C)
    norm = torch.nn.LayerNorm(C).to(dev)
    w = lambda n, k: (rn(n, k) * k ** -0.5)  # noqa: E731
    wq, wk, wv, wo, w0, w2 = w(C, C), w(C, C), w(C, C), w(C, C), w(8 * C, C), w(C, 4 * C)
    bo, b0, b2 = rn(C), rn(8 * C), rn(C)
    qkv_w = torch.stack([t.t() for t in (wq, wk, wv)]).contiguous()
    p_qkv, p_o, p_q = hip.token_linear_pack([wq, wk, wv]), hip.token_linear_pack(wo), hip.token_linear_pack(wq)
    p_0, p_2 = hip.token_linear_pack(w0, geglu=True), hip.token_linear_pack(w2)
    spec = [
        ("qkv", 3 * C, C, "ln+parts3", 1,
         lambda: hip.token_linear(x, p_qkv, 3 * C, norm=norm, parts=3),
         lambda: torch.matmul(hip.add_layer_norm_tokens(x, None, None, norm)[1].reshape(1, M, C), qkv_w)),
        ("to_out", C, C, "bias+residual", 2,
         lambda: hip.token_linear(o, p_o, C, bias=bo, residual=x),
         lambda: F.linear(o, wo)),
        ("attn2.q", C, C, "ln", 1,
         lambda: hip.token_linear(x, p_q, C, norm=norm),
         lambda: F.linear(hip.add_layer_norm_tokens(x, d, bo, norm)[1], wq)),
        ("ff.proj", 8 * C, C, "ln+geglu", 1,
         lambda: hip.token_linear(x, p_0, 8 * C, bias=b0, norm=norm, geglu=True),
         lambda: hip.geglu_tokens(F.linear(hip.add_layer_norm_tokens(x, d, bo, norm)[1], w0, b0))),
        ("ff.out", C, 4 * C, "bias+residual", 1,
         lambda: hip.token_linear(h, p_2, C, bias=b2, residual=x),
         lambda: hip.add_bias_tokens(x, F.linear(h, w2), b2)),
    ]
    out = []
    # (every figure the smaller of two timings: the first graph after host-side set-up runs while the clock still ramps)
    timed = lambda fn: min(time_graph_of(fn, reps) for _ in range(2))  # noqa: E731
    with torch.no_grad():
        for name, N, K, form, per_block, lib_fn, base_fn in spec:
            assert lib_fn() is not None, (name, M, N, K)
            row = {"launch": name, "M": M, "N": N, "K": K, "form": form, "per_block": per_block, "gflop": 2e-9 * M * N * K}
            row["library_us"] = timed(lib_fn)
            if forms:
                for key, knob in (("library_16tok_us", 1), ("library_64tok_us", 2)):
                    with hip.tuning_build():
                        hip.tuning_set("token_linear_form", knob)
                        row[key] = timed(lib_fn)
            row["default_us"] = timed(base_fn)
            row["tuned_us"] = None
            if gemm_tuning.enable_tuned_gemms():
                try:
                    row["tuned_us"] = timed(base_fn)
                finally:
                    gemm_tuning.disable_tuned_gemms()
            row["library_tflops"] = row["gflop"] * 1e-3 / (row["library_us"] * 1e-6)
            row["library_frac_of_f32_mfma_peak"] = row["library_tflops"] / PEAK_F32_MFMA_TFS
            out.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", default="bench,other")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forms", action="store_true", help="also time both row-block forms (needs the measurement build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sige_amd import hip

    dev = torch.device("cuda:0")
    hip.lib()
    in_table = table_token_counts()
    shapes = block_shapes({m: MASKS[m] for m in args.masks.split(",")}, dev)
    res = {"workload": "bench.py --workload sd (SD v1 U-Net, latent [2,4,64,64]); us per call from a hipGraph of %d back-to-back calls" % args.reps,
           "f32_mfma_peak_tflops": PEAK_F32_MFMA_TFS, "masks": {}}
    done = {}
    for mask, sh in shapes.items():
        entry = {"box": MASKS[mask], "levels": []}
        for (M, C, on_path), blocks in sorted(sh.items(), key=lambda kv: -kv[0][0]):
            if (M, C) not in done:
                done[(M, C)] = rows_of(M, C, dev, hip, args.forms, args.reps)
            rows = done[(M, C)]
            tot = lambda key: (None if any(r[key] is None for r in rows) else round(sum(r[key] * r["per_block"] for r in rows), 2))  # noqa: E731
            entry["levels"].append({"M": M, "C": C, "blocks_per_forward": blocks, "on_switch_path": on_path, "M_in_tunableop_table": M in in_table,
                                    "per_block_us": {"library": tot("library_us"), "default": tot("default_us"), "tuned": tot("tuned_us")},
                                    "rows": rows})
            print(json.dumps({k: v for k, v in entry["levels"][-1].items() if k != "rows"}), flush=True)
        on = [l for l in entry["levels"] if l["on_switch_path"]]  # (what the switch changes: the other blocks are listed, not summed)
        per_fwd = lambda key: (None if any(l["per_block_us"][key] is None for l in on)  # noqa: E731
                               else round(sum(l["per_block_us"][key] * l["blocks_per_forward"] for l in on), 1))
        entry["per_forward_us"] = {k: per_fwd(k) for k in ("library", "default", "tuned")}
        print(json.dumps({"mask": mask, "per_forward_us": entry["per_forward_us"]}), flush=True)
        res["masks"][mask] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
