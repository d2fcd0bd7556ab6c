#!/usr/bin/env python3
"""The Upsample phase convs on the tile conv v3 against what the same call takes today, on the MI355X.
Writes profiles/upsample_phase_tile3_bench.json.

(a) Launch alone, exact fp32 and fp16 operands: every Upsample conv of the SD VAE decoder (512 ch -> 128^2, 512 ch -> 256^2, 256 ch ->
512^2 under square edits of 1.2 / 5 / 15 % of the 512^2 image) and of DDPM-256 (its five, at 5 / 15 / 20 %) as
hip.gather_conv_cl(..., phase3=pack) with hip.PHASE_TILE3_MIN_BLOCKS = 1 beside the same call with phase3=None -- the launch the call
takes today: the phase form of conv_mfma.hpp below the v3 router's threshold (fp32), the 9-tap v3 or conv_mfma.hpp launch otherwise.
Each a hipGraph of 20 back-to-back launches between HIP events, the two alternating `--batches` times; median and [min, max].

(b) Whole forward with Gather.PHASE_UPSAMPLE_TILE3 on and off (hip.PHASE_TILE3_MIN_BLOCKS = `--min-blocks`, default the shipped
value): two hipGraphs of one model, HIP events around `--steps` replays after warm-up replays, alternating batch by batch over
rotating edited inputs; medians and [min, max] of both, and max |on - off| of the outputs.  SD VAE decoder fp32 and f16 at 1.2 / 5 /
15 %; DDPM-256 fp32 at 15 / 20 %; stacked E = 8: DDPM-256 at 1.2 / 5 %, SD VAE decoder at 5 %.

The parent never touches the GPU: one child per job under `timeout -k 10`, and it stops at the first child that fails.

    python tools/upsample_phase_tile3_bench.py [--jobs launch_f32,launch_f16,vae_f32,...] [--min-blocks N]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "upsample_phase_tile3_bench.json")
TAG = "PHASE_TILE3_ROW "
JOBS = ["launch_f32", "launch_f16", "vae_f32", "vae_f16", "ddpm", "ddpm_stacked", "vae_stacked"]
VAE_UPS = [(512, 64), (512, 128), (256, 256)]                       # (channels, low-res edge) of the decoder's three Upsample convs
DDPM_UPS = [(512, 8), (512, 16), (256, 32), (256, 64), (128, 128)]  # DDPM-256's five


def _stat(v):
    return round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]


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


def child_launch(a, compute):
    import torch

    from benchlib.common import square_mask, time_graph_of
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, reduce_mask
    from tests.golden import vae_inputs

    hip.lib()
    dev = torch.device("cuda")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    rows = []
    shapes = [("sd_vae_decoder", C, r, 512, 2, ratio) for (C, r) in VAE_UPS for ratio in (0.012, 0.05, 0.15)]
    shapes += [("ddpm256", C, r, 256, 5, ratio) for (C, r) in DDPM_UPS for ratio in (0.05, 0.15, 0.20)]
    for workload, C, r, image, dil, ratio in shapes:
        g = torch.Generator().manual_seed(C + r)
        mask = vae_inputs.square_mask(image, ratio) if image == 512 else square_mask(ratio)
        m = dilate_mask(mask.to(dev), dil)
        H = 2 * r
        if H != image:  # the level's mask: any edited pixel under a cell
            m = torch.nn.functional.max_pool2d(m[None, None].float(), image // H)[0, 0] > 0
        idx = reduce_mask(m, 6, 4, 1)
        N = int(idx.shape[0])
        x, out = cl(torch.randn(1, C, r, r, generator=g)), cl(torch.randn(1, C, H, H, generator=g))
        w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
        bias = torch.randn(C, generator=g).to(dev)
        packed = hip.conv_pack_weights(w, 6, 6, (1, 1), compute)
        phase = hip.upsample_phase_pack(w) if compute == "f32" else None
        p3 = hip.upsample_phase_tile3_pack(w, compute)
        full = dict(offset=(1, 1), out_res=(H, H), residual=None)

        def call(pk):
            return hip.gather_conv_cl(x, None, (6, 6), idx, None, None, "identity", packed, bias, C, (3, 3), (1, 1), full=full,
                                      upsample2x=True, out=out, phase=phase, phase3=pk)

        new, old = [], []
        hip.PHASE_TILE3_MIN_BLOCKS = 1
        # what today's call asks of the routing entry point, OBSERVED: (upsample2x, status) of every sige_hip_gather_conv_nhwc call
        real, asked = hip.lib().sige_hip_gather_conv_nhwc, []

        def spy(*args):
            status = real(*args)
            asked.append([int(args[37]), int(status)])
            return status

        hip.lib().sige_hip_gather_conv_nhwc = spy
        try:
            call(None)
        finally:
            hip.lib().sige_hip_gather_conv_nhwc = real
        for i in range(a.batches):
            for name in (("n", "o") if i % 2 == 0 else ("o", "n")):
                (new if name == "n" else old).append(time_graph_of((lambda: call(p3)) if name == "n" else (lambda: call(None)), 20))
        un, mmn = _stat(new)
        uo, mmo = _stat(old)
        v3_today = -(-N // 2) * (C // 64)
        # which kernel the entry point then launches is decided in C (block_conv.hip: tile3_takes) and is NOT observed here: the label
        # repeats the router's rule from the thresholds the binding hands over
        today = ("9 taps, tile conv v3" if v3_today >= (hip.TILE3_MIN_BLOCKS if compute == "f32" else min(hip.TILE3_MIN_BLOCKS_F16, 128))
                 else "phase form, conv_mfma.hpp" if compute == "f32" else "9 taps, conv_mfma.hpp")
        flop9 = 2.0 * N * 16 * C * C * 9
        rows.append({"workload": workload, "compute": compute, "C": C, "out_res": H, "ratio": ratio, "tiles": N,
                     "workgroups_new": -(-N // 8) * (C // 64) * 4, "v3_workgroups_of_the_9_tap_call": v3_today, "today_inferred": today,
                     "today_gather_conv_calls_upsample2x_status": asked,
                     "new_us": un, "new_us_min_max": mmn, "today_us": uo, "today_us_min_max": mmo, "new_over_today": round(un / uo, 3),
                     "new_TFLOPs_of_the_9_tap_flop": round(flop9 / un / 1e6, 1), "today_TFLOPs_of_the_9_tap_flop": round(flop9 / uo / 1e6, 1)})
        print("launch %s %s C%d -> %d^2 %.3f: %d tiles  new %.2f us  today %.2f us (%s)" % (compute, workload, C, H, ratio, N, un, uo, today),
              file=sys.stderr, flush=True)
    print(TAG + json.dumps(rows), flush=True)


def _ab(a, run, rotate, note):
    """Two graphs of `run()` -- the switch on, then off -- alternating over `--batches` batches; `rotate(batch)` changes the inputs."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.nn import Gather

    seen = []
    real = hip.lib().sige_hip_upsample_phase_tile3_nhwc

    def spy(*args):
        status = real(*args)
        seen.append(int(status))
        return status

    graphs, outs, launches = {}, {}, {}
    for on in (True, False):
        Gather.PHASE_UPSAMPLE_TILE3 = on
        try:
            run()
            run()
            if on:
                hip.lib().sige_hip_upsample_phase_tile3_nhwc = spy
            n0 = hip.launch_count()
            run()
            launches[on] = hip.launch_count() - n0
            hip.lib().sige_hip_upsample_phase_tile3_nhwc = real
            graphs[on], outs[on] = capture_fn(run)
        finally:
            hip.lib().sige_hip_upsample_phase_tile3_nhwc = real
            Gather.PHASE_UPSAMPLE_TILE3 = False
    t = {True: [], False: []}
    for batch in range(a.batches):
        rotate(batch)
        for on in ((True, False) if batch % 2 == 0 else (False, True)):
            t[on].append(events_ms(graphs[on], a.steps, 5))
    rotate(0)
    graphs[True].replay()
    got = outs[True].clone()
    graphs[False].replay()
    torch.cuda.synchronize()
    m1, mm1 = _stat(t[True])
    m0, mm0 = _stat(t[False])
    row = dict(note)
    row.update({"on_ms": m1, "on_ms_min_max": mm1, "off_ms": m0, "off_ms_min_max": mm0, "on_minus_off_us": round((m1 - m0) * 1e3, 2),
                "on_over_off": round(m1 / m0, 4), "launches_on": launches[True], "launches_off": launches[False],
                "upsample_calls_taken": seen.count(0), "upsample_calls_refused": len(seen) - seen.count(0),
                "max_abs_on_minus_off": float((got - outs[False]).abs().max()), "max_abs_out": float(outs[False].abs().max())})
    print("forward %s: on %.4f off %.4f ms (%d taken, %d refused)" % (note, m1, m0, row["upsample_calls_taken"], row["upsample_calls_refused"]),
          file=sys.stderr, flush=True)
    return row


def child_forward(a, job):
    import torch

    import bench
    from sige_amd import hip, stacked
    from sige_amd.utils import dilate_mask, downsample_mask
    from tests.golden import vae_inputs

    hip.lib()
    if a.min_blocks is not None:
        hip.PHASE_TILE3_MIN_BLOCKS = hip.PHASE_TILE3_MIN_BLOCKS_F16 = a.min_blocks
    dev = torch.device("cuda")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    vae = job.startswith("vae")
    E = 8 if job.endswith("stacked") else 1
    f16 = job == "vae_f16"
    ratios = {"vae_f32": (0.012, 0.05, 0.15), "vae_f16": (0.012, 0.05, 0.15), "ddpm": (0.15, 0.20), "ddpm_stacked": (0.012, 0.05),
              "vae_stacked": (0.05,)}[job]
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    if vae:
        from sige_amd.workloads import sd_vae

        cfg = sd_vae.VAEDecoderConfig()
        model = sd_vae.SparseVAEDecoder(cfg).eval().to(dev).to(memory_format=torch.channels_last)
        x0 = torch.randn(1, cfg.z_channels, 64, 64, generator=g)
        noises = [torch.randn(x0.shape, generator=g) for _ in range(8)]
        fwd = lambda x: model(x)  # noqa: E731
    else:
        from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

        model = DDPMSparseUNet(DDPMConfig()).eval().to(dev).to(memory_format=torch.channels_last)
        x0, _ = bench.make_inputs()
        noises = [torch.randn(x0.shape, generator=g) for _ in range(8)]
        t = torch.zeros(1, device=dev)
        fwd = lambda x: model(x, t)  # noqa: E731
    model.set_scatter_inplace(True)
    if f16:
        model.set_compute_dtype("f16")
    rows = []
    with torch.no_grad():
        model.set_mode("full")
        fwd(cl(x0))
        for ratio in ratios:
            if vae:
                mask = vae_inputs.square_mask(512, ratio)
                masks = downsample_mask(dilate_mask(mask.to(dev), 2), 64)
                inside = masks[(64, 64)].cpu()
            else:
                mask = bench.square_mask(ratio)
                masks = downsample_mask(dilate_mask(mask.to(dev), 5), 8)
                inside = mask
            edits = [cl(x0 + n * inside) for n in noises]
            note = {"workload": "sd_vae_decoder" if vae else "ddpm256", "compute": "f16" if f16 else "f32", "E": E, "ratio": ratio,
                    "min_blocks": int(min(hip.PHASE_TILE3_MIN_BLOCKS, hip.PHASE_TILE3_MIN_BLOCKS_F16) if f16 else hip.PHASE_TILE3_MIN_BLOCKS)}
            if E == 1:
                model.set_masks(masks)
                model.set_mode("sparse")
                x1 = edits[0].clone()
                rows.append(_ab(a, lambda: fwd(x1), lambda b: x1.copy_(edits[b % len(edits)]), note))
            else:
                xs = cl(torch.cat(edits[:E], 0))

                def rotate(b):
                    for e in range(E):
                        xs[e].copy_(edits[(b + e) % len(edits)][0])

                stacked.stack_caches(model, E)
                try:
                    stacked.set_masks(model, [masks] * E)
                    model.set_mode("sparse")
                    with stacked.edit_batch(model, E):
                        rows.append(_ab(a, lambda: fwd(xs), rotate, note))
                finally:
                    stacked.unstack_caches(model)
    print(TAG + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default=",".join(JOBS))
    ap.add_argument("--child", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--min-blocks", type=int, default=None, help="hip.PHASE_TILE3_MIN_BLOCKS of the forwards (default: the shipped value)")
    ap.add_argument("--limit", type=int, default=420, help="seconds per child")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("upsample_phase_tile3_bench: needs the GPU (no timing is taken anywhere else)")
        if a.child.startswith("launch_"):
            return child_launch(a, a.child[len("launch_"):]) or 0
        return child_forward(a, a.child) or 0
    from sige_amd import build

    res = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"today_inferred": "the form of the baseline launch is inferred from the router's thresholds (hip.TILE3_MIN_BLOCKS, "
                                  "hip.TILE3_MIN_BLOCKS_F16, the 128-workgroup rule for sparse fp16 lists), not observed; the calls the "
                                  "binding made are observed (today_gather_conv_calls_upsample2x_status)",
                "method": "hipGraph replay between HIP events; the two forms alternate batch by batch, medians and [min, max] over "
                          "%d batches; launches: graphs of 20 back-to-back launches, weights L2-warm; forwards: %d replays per batch after "
                          "5 warm-up replays, edited inputs rotating" % (a.batches, a.steps),
                "source_hash": build.source_hash()})
    code = 0
    for job in a.jobs.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", job, "--steps", str(a.steps),
               "--batches", str(a.batches)] + ([] if a.min_blocks is None else ["--min-blocks", str(a.min_blocks)])
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-6000:])
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": job, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            code = 1
            break
        res.pop("failed", None)
        key = job if a.min_blocks is None or job.startswith("launch_") else "%s_min_blocks_%d" % (job, a.min_blocks)
        res[key] = json.loads(line[len(TAG):])
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return code


if __name__ == "__main__":
    sys.exit(main())
