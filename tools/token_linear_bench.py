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
`--compute f16`: the library columns are the token linear on fp16 operands (csrc/token_linear_f16.hip), the exact-fp32 form of the same
run is the column `f32_library_us`, and `max_abs_vs_fp64` is max |out - fp64| of the launch's outputs (the formula evaluated in fp64 on
the same inputs).

    python tools/token_linear_bench.py --out out/token_linear_bench.json
    python tools/token_linear_bench.py --compute f16 --forms --out profiles/token_linear_f16_bench.json

`--ksplit`: instead of the columns above, the K split inside the launch (hip.token_linear(ksplit=...)) at the same shapes, in both
computes: the launch at ksplit 1 -- the unsplit 16-token instance -- and forced at 2 / 4 / 8 in the same run, `library_us` (the entry
without a split argument: the form the library picks) next to them, each figure [smallest, largest] of three timings, and the split the
library's rule picks.  A captured split launch keeps its workspace slice for the life of its graph, so a graph holds as many
back-to-back calls (at most --reps) as the pool's graph region has slices for: `reps` of the row.

    python tools/token_linear_bench.py --ksplit --out profiles/token_linear_ksplit_bench.json
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


def rows_of(M, C, dev, hip, forms, reps, compute="f32"):
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
    packs = {c: (hip.token_linear_pack([wq, wk, wv], compute=c), hip.token_linear_pack(wo, compute=c), hip.token_linear_pack(wq, compute=c),
                 hip.token_linear_pack(w0, geglu=True, compute=c), hip.token_linear_pack(w2, compute=c)) for c in {"f32", compute}}
    f64 = lambda t: t.double()  # noqa: E731
    ln64 = lambda t: F.layer_norm(f64(t), (C,), f64(norm.weight), f64(norm.bias), norm.eps)  # noqa: E731

    def geglu64(t):
        v, gate = t.chunk(2, dim=-1)
        return v * F.gelu(gate)

    # (name, N, K, form, launches per block, the library launch for a compute, what it replaces, the same formula in fp64)
    spec = [
        ("qkv", 3 * C, C, "ln+parts3", 1,
         lambda c: hip.token_linear(x, packs[c][0], 3 * C, norm=norm, parts=3, compute=c),
         lambda: torch.matmul(hip.add_layer_norm_tokens(x, None, None, norm)[1].reshape(1, M, C), qkv_w),
         lambda: ln64(x) @ f64(torch.cat([wq, wk, wv])).t()),
        ("to_out", C, C, "bias+residual", 2,
         lambda c: hip.token_linear(o, packs[c][1], C, bias=bo, residual=x, compute=c),
         lambda: F.linear(o, wo),
         lambda: f64(x) + F.linear(f64(o), f64(wo), f64(bo))),
        ("attn2.q", C, C, "ln", 1,
         lambda c: hip.token_linear(x, packs[c][2], C, norm=norm, compute=c),
         lambda: F.linear(hip.add_layer_norm_tokens(x, d, bo, norm)[1], wq),
         lambda: ln64(x) @ f64(wq).t()),
        ("ff.proj", 8 * C, C, "ln+geglu", 1,
         lambda c: hip.token_linear(x, packs[c][3], 8 * C, bias=b0, norm=norm, geglu=True, compute=c),
         lambda: hip.geglu_tokens(F.linear(hip.add_layer_norm_tokens(x, d, bo, norm)[1], w0, b0)),
         lambda: geglu64(F.linear(ln64(x), f64(w0), f64(b0)))),
        ("ff.out", C, 4 * C, "bias+residual", 1,
         lambda c: hip.token_linear(h, packs[c][4], C, bias=b2, residual=x, compute=c),
         lambda: hip.add_bias_tokens(x, F.linear(h, w2), b2),
         lambda: f64(x) + F.linear(f64(h), f64(w2), f64(b2))),
    ]
    out = []
    # (every figure the smaller of two timings: the first graph after host-side set-up runs while the clock still ramps)
    timed = lambda fn: min(time_graph_of(fn, reps) for _ in range(2))  # noqa: E731
    with torch.no_grad():
        for name, N, K, form, per_block, lib_c, base_fn, ref_fn in spec:
            lib_fn = lambda lib_c=lib_c: lib_c(compute)  # noqa: E731
            got = lib_fn()
            assert got is not None, (name, M, N, K)
            row = {"launch": name, "M": M, "N": N, "K": K, "form": form, "per_block": per_block, "gflop": 2e-9 * M * N * K, "compute": compute}
            row["max_abs_vs_fp64"] = float((torch.cat(got, dim=-1) if isinstance(got, tuple) else got).double().sub(ref_fn()).abs().max())
            row["library_us"] = timed(lib_fn)
            if compute != "f32":
                row["f32_library_us"] = timed(lambda: lib_c("f32"))
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
            out.append({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()})
            print(json.dumps(out[-1]), flush=True)
    return out


def ksplit_rows_of(M, C, dev, hip, reps):
    """The five launches of one block at (M, C), both computes: us at ksplit 1 | 2 | 4 | 8 (None: refused), [smallest, largest] of three."""
    g = torch.Generator().manual_seed(M * 7 + C)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x, o, h = rn(1, M, C), rn(1, M, C), rn(1, M, 4 * C)
    norm = torch.nn.LayerNorm(C).to(dev)
    w = lambda n, k: (rn(n, k) * k ** -0.5)  # noqa: E731
    wq, wk, wv, wo, w0, w2 = w(C, C), w(C, C), w(C, C), w(C, C), w(8 * C, C), w(C, 4 * C)
    bo, b0, b2 = rn(C), rn(8 * C), rn(C)
    out = []
    for c in ("f32", "f16"):
        pk = (hip.token_linear_pack([wq, wk, wv], compute=c), hip.token_linear_pack(wo, compute=c), hip.token_linear_pack(wq, compute=c),
              hip.token_linear_pack(w0, geglu=True, compute=c), hip.token_linear_pack(w2, compute=c))
        # (name, N, K, LayerNorm, GEGLU, parts, the launch at a ksplit)
        spec = [("qkv", 3 * C, C, True, False, 3, lambda ks: hip.token_linear(x, pk[0], 3 * C, norm=norm, parts=3, compute=c, ksplit=ks)),
                ("to_out", C, C, False, False, 1, lambda ks: hip.token_linear(o, pk[1], C, bias=bo, residual=x, compute=c, ksplit=ks)),
                ("attn2.q", C, C, True, False, 1, lambda ks: hip.token_linear(x, pk[2], C, norm=norm, compute=c, ksplit=ks)),
                ("ff.proj", 8 * C, C, True, True, 1, lambda ks: hip.token_linear(x, pk[3], 8 * C, bias=b0, norm=norm, geglu=True, compute=c, ksplit=ks)),
                ("ff.out", C, 4 * C, False, False, 1, lambda ks: hip.token_linear(h, pk[4], C, bias=b2, residual=x, compute=c, ksplit=ks))]
        with torch.no_grad():
            for name, N, K, ln, geglu, parts, fn in spec:
                units = -(-M // 16) * -(-N // 64)
                row = {"launch": name, "compute": c, "M": M, "N": N, "K": K, "grid16": units, "chunks": -(-K // (64 if c == "f32" else 128)),
                       "rule_ksplit": hip.token_linear_ksplit(M, N, K, ln, geglu, parts, compute=c), "us": {}, "reps": {}}
                for key, ks in (("library", None), ("1", 1), ("2", 2), ("4", 4), ("8", 8)):
                    if ks is not None and fn(ks) is None:  # (more splits than chunks)
                        row["us"][key] = None
                        continue
                    # the graph region of the workspace pool: 24 Mi floats, units * ks * 1024 per captured launch (and its warm-up)
                    n = reps if ks in (None, 1) else max(1, min(reps, (24 << 20) // (units * ks * 1024) - 1))
                    ts = []
                    for _ in range(3):
                        ts.append(time_graph_of(lambda: fn(ks), n))
                        hip.release_graph_tickets()  # (the graph is gone: its slices start over)
                    row["us"][key], row["reps"][key] = [float("%.4g" % min(ts)), float("%.4g" % max(ts))], n
                out.append(row)
                print(json.dumps(row), flush=True)
    return out


def main_ksplit(args, hip, dev):
    shapes = block_shapes({m: MASKS[m] for m in args.masks.split(",")}, dev)
    res = {"workload": "bench.py --workload sd (SD v1 U-Net, latent [2,4,64,64]); us per call from a hipGraph of `reps` back-to-back calls, "
                       "[smallest, largest] of three graphs; ksplit 1 = the unsplit 16-token instance, library = the entry without a split",
           "masks": {}}
    done = {}
    for mask, sh in shapes.items():
        levels = []
        for (M, C, on_path), blocks in sorted(sh.items(), key=lambda kv: -kv[0][0]):
            if (M, C) not in done:
                done[(M, C)] = ksplit_rows_of(M, C, dev, hip, args.reps)
            levels.append({"M": M, "C": C, "blocks_per_forward": blocks, "on_switch_path": on_path, "rows": done[(M, C)]})
        res["masks"][mask] = {"box": MASKS[mask], "levels": levels}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", default="bench,other")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forms", action="store_true", help="also time both row-block forms (needs the measurement build)")
    ap.add_argument("--compute", default="f32", choices=("f32", "f16"), help="the operands of the library columns")
    ap.add_argument("--ksplit", action="store_true", help="time the K split inside the launch at ksplit 1 / 2 / 4 / 8, both computes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sige_amd import hip

    dev = torch.device("cuda:0")
    hip.lib()
    if args.ksplit:
        return main_ksplit(args, hip, dev)
    in_table = table_token_counts()
    shapes = block_shapes({m: MASKS[m] for m in args.masks.split(",")}, dev)
    res = {"workload": "bench.py --workload sd (SD v1 U-Net, latent [2,4,64,64]); us per call from a hipGraph of %d back-to-back calls" % args.reps,
           "f32_mfma_peak_tflops": PEAK_F32_MFMA_TFS, "library_compute": args.compute, "masks": {}}
    done = {}
    for mask, sh in shapes.items():
        entry = {"box": MASKS[mask], "levels": []}
        for (M, C, on_path), blocks in sorted(sh.items(), key=lambda kv: -kv[0][0]):
            if (M, C) not in done:
                done[(M, C)] = rows_of(M, C, dev, hip, args.forms, args.reps, args.compute)
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
