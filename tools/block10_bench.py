#!/usr/bin/env python3
"""Block size 10 against the default 6 / 4, on the MI355X.

Launch by launch: the two 3x3 convs of a DDPM ResBlock -- gather + affine + SiLU -> tiles (conv1) and scatter_gather -> full tensor with
block residual (conv2) -- at the 256^2 / 128-channel and 128^2 / 256-channel shapes under bench.py's 5 % and 15 % masks: the 6x6 list
on the kernel the router picks for it against the 10x10 list on the one-window form of the tile conv v3 (csrc/conv_tile3.hpp:
Tile3GeoE10).  Each as a hipGraph of 20 back-to-back launches (weights L2-warm in both), the two lists alternating three
times (minimum reported, every run kept); microseconds per launch and TFLOP/s on the output pixels the list computes (10x10 lists
compute more pixels for the same edit: coarser coverage).

The forward: DDPM-256 sparse, main_block = 10 with shortcut_block = 8 and with the default 4 against the default 6 / 4, at 1.2 / 5 / 15 % edits, as captured graphs
timed alternately; launches per forward and how many of them are sige_hip_block_conv_direct_f32 (the 9x9 tiles of the Downsamples).

    python tools/block10_bench.py [--out profiles/block10_bench.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402


REPEATS = 3  # alternating repeats of every per-launch timing (the minimum is reported, every run kept)


def layer_rows(hip, dev, ratios):
    from sige_amd.utils import dilate_mask, downsample_mask, reduce_mask

    cl = lambda t_: t_.contiguous(memory_format=torch.channels_last)  # noqa: E731
    rows = []
    for ratio in ratios:
        pyr = downsample_mask(dilate_mask(bench.square_mask(ratio).to(dev), 5), 8)
        for (R, C) in ((256, 128), (128, 256)):
            m = pyr[(R, R)]
            x, y = cl(torch.randn(1, C, R, R, device=dev)), cl(torch.randn(1, C, R, R, device=dev))
            w = torch.randn(C, C, 3, 3, device=dev) / (3 * C ** 0.5)
            bias = torch.randn(C, device=dev)
            sc, sh = torch.randn(1, C, 1, 1, device=dev), torch.randn(1, C, 1, 1, device=dev)
            y1, out = cl(torch.randn(1, C, R, R, device=dev)), cl(torch.randn(1, C, R, R, device=dev))
            row = {"edit_ratio": ratio, "resolution": R, "C": C}
            calls, keep = {}, []
            for tag, block, o, short in (("b6", 6, 4, 4), ("b10", 10, 8, 8)):
                idx, idx1 = reduce_mask(m, block, o, 1), reduce_mask(m, short, short, 0)
                N = idx.shape[0]
                packed = hip.conv_pack_weights(w, block, block, (1, 1))
                smap = hip.get_scatter_map(R, R, block, block, 3, 3, 1, 1, 1, 1, idx)
                tin = cl(torch.randn(N, C, o, o, device=dev))
                x1 = cl(torch.randn(idx1.shape[0], C, short, short, device=dev))
                table1 = hip.tile_table(idx1, (0, 0), (1, 1), (short, short), (R, R))
                flop = 2.0 * N * o * o * C * C * 9

                def conv1(block=block, idx=idx, packed=packed):
                    return hip.gather_conv_cl(x, None, (block, block), idx, sc, sh, "swish", packed, bias, C, (3, 3), (1, 1))

                def conv2(block=block, idx=idx, packed=packed, tin=tin, smap=smap, x1=x1, table1=table1):
                    return hip.scatter_gather_conv_scatter_cl(tin, y, (block, block), idx, smap, None, None, "identity", packed, bias, C,
                                                              (3, 3), (1, 1), out, residual=y1, x1=x1, table1=table1)

                assert conv1() is not None and conv2() is not None
                calls[tag] = (conv1, conv2, flop)
                keep.append((idx, idx1, packed, smap, tin, x1, table1))
                row[tag] = {"tiles": N, "staged_px": N * block * block, "computed_px": N * o * o, "GFLOP": round(flop / 1e9, 3),
                            "workgroups": (-(-N // 2) if block == 6 else N) * (C // 64)}
            runs = {tag: ([], []) for tag in calls}
            for _ in range(REPEATS):  # (the two lists alternate: other work shares the host; the spread is kept)
                for tag, (conv1, conv2, _) in calls.items():
                    runs[tag][0].append(bench.time_graph_of(conv1, 20))
                    runs[tag][1].append(bench.time_graph_of(conv2, 20))
            for tag, (_, _, flop) in calls.items():
                us1, us2 = min(runs[tag][0]), min(runs[tag][1])
                row[tag].update({"gather_affine_swish_to_tiles_us": round(us1, 2), "gather_us_runs": [round(v, 2) for v in runs[tag][0]],
                                 "gather_TFLOPs": round(flop / us1 / 1e6, 1),
                                 "scatter_gather_to_full_block_residual_us": round(us2, 2),
                                 "scatter_gather_us_runs": [round(v, 2) for v in runs[tag][1]],
                                 "scatter_gather_TFLOPs": round(flop / us2 / 1e6, 1)})
            rows.append(row)
    return rows


class _direct_calls:
    def __init__(self, hip):
        self.lib, self.n = hip.lib(), 0

    def __enter__(self):
        self.real = self.lib.sige_hip_block_conv_direct_f32

        def spy(*args):
            self.n += 1
            return self.real(*args)

        self.lib.sige_hip_block_conv_direct_f32 = spy
        return self

    def __exit__(self, *exc):
        self.lib.sige_hip_block_conv_direct_f32 = self.real
        return False


def forward_rows(hip, dev, ratios):
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    cl = lambda t_: t_.contiguous(memory_format=torch.channels_last)  # noqa: E731
    x0, noise = bench.make_inputs()
    x0, noise, t = cl(x0.to(dev)), cl(noise.to(dev)), torch.zeros(1, device=dev)
    models = {}
    for tag, cfg in (("blocks_6_4", DDPMConfig()), ("blocks_10_8", DDPMConfig(main_block=10, shortcut_block=8)),
                     ("blocks_10_4", DDPMConfig(main_block=10))):
        torch.manual_seed(0)
        model = DDPMSparseUNet(cfg).eval().to(dev).to(memory_format=torch.channels_last)
        model.set_scatter_inplace(True)
        with torch.no_grad():
            model.set_mode("full")
            model(x0, t)
        models[tag] = model
    rows = []
    with torch.no_grad():
        for ratio in ratios:
            mask = bench.square_mask(ratio).to(dev)
            x1 = x0 + noise * mask
            row, graphs, outs = {"edit_ratio": ratio}, {}, {}
            for tag, model in models.items():
                model.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
                model.set_mode("sparse")
                model(x1, t)
                model(x1, t)
                n0 = hip.launch_count()
                with _direct_calls(hip) as spy:
                    outs[tag] = model(x1, t).clone()
                row[tag] = {"launches": hip.launch_count() - n0, "block_conv_direct_calls": spy.n}
                graphs[tag] = bench.capture(model, x1, t)
            times = {tag: [] for tag in graphs}
            for _ in range(3):  # (alternating: other work shares the host)
                for tag, (g, _) in graphs.items():
                    times[tag].append(bench.timed_replays(g, 30, 5, 1) * 1e3 / 30)
            for tag in graphs:
                row[tag]["forward_ms"] = round(min(times[tag]), 4)
                row[tag]["forward_ms_runs"] = [round(v, 4) for v in times[tag]]
            row["max_abs_diff_between_configs"] = float((outs["blocks_6_4"] - outs["blocks_10_8"]).abs().max())
            del graphs
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    a = ap.parse_args()
    from sige_amd import hip

    if not torch.cuda.is_available():
        raise SystemExit("block10_bench: needs the GPU (no timing is taken anywhere else)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "compute": "f32"}
    if not a.skip_layers:
        res["layers"] = layer_rows(hip, dev, (0.05, 0.15))
    if not a.skip_forward:
        res["forward"] = forward_rows(hip, dev, (0.012, 0.05, 0.15))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
