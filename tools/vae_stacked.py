#!/usr/bin/env python3
"""Stacked edits (sige_amd/stacked.py) through the SD VAE decoder and encoder on the MI355X: what `tools/vae_bench.py --stacked` and
`tools/vae_encoder_bench.py --stacked` run, in the protocol of `tools/sub_mobile_bench.py --stacked`.  Both write their half of
profiles/sd_vae_stacked_bench.json ("decoder" / "encoder").

Per square edit of 1.2 / 5 / 15 % of the 512 x 512 image, in ONE child process: two models with the same weights (seed 0), one stays
on single edits, the other is stacked for E = 2, 4, 8 in turn (E edited versions of the same original under the same square, another
noise per edit).  Both forwards are hipGraphs; HIP events around `--steps` replays after warm-up replays; the stacked and the
single-edit graph alternate batch by batch and the edited inputs in the graphs' buffers change from batch to batch; medians over
`--batches` batches.  `speedup` = E x the single-edit time OF THE SAME RUN over the stacked time.  Also: library launches, and
max |stacked - single| per edit after both graphs replayed on the same inputs.  The decoder is forward(), the encoder encode() with
quant_conv and one posterior noise per edit.

Once per run, in a child of its own: the attention launch ALONE at E = 8 -- hip.attention_wide(tiles=...) on the tall K | V
([1, 8 x 4096, 1024], one 512-wide head), the tiles of a 5 % edit in every image -- beside E single launches of hip.attention_wide on
the same rows, each as one graph, alternating, medians of 7.

No threshold hangs on any figure.  The parent process never touches the GPU: it starts one child per measurement under
`timeout -k 10` and stops at the first that fails."""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
IMAGE, LATENT = 512, 64
TAG = "VAE_STACKED_ROW "
OUT = os.path.join(REPO, "profiles", "sd_vae_stacked_bench.json")
OUT_F16 = os.path.join(REPO, "profiles", "sd_vae_f16_bench.json")  # (--dtype f16: "decoder_stacked" / "encoder_stacked")
SCALE_FACTOR = 0.18215


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
    """E = 8: one per-image launch for the tiles of all edits beside eight single launches, on the same q and K | V rows."""
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip
    from sige_amd.utils import dilate_mask, downsample_mask, reduce_mask
    from tests.golden import vae_inputs

    hip.lib()
    E, d, N = 8, 512, LATENT * LATENT
    m64 = downsample_mask(dilate_mask(vae_inputs.square_mask(IMAGE, 0.05).cuda(), 2), LATENT)[(LATENT, LATENT)]
    one = reduce_mask(m64, 4, 4, 0).to(torch.int32)  # the attention block's 4x4 tiles of ONE edit
    T = int(one.shape[0])
    idx = torch.cat([one + torch.tensor([e * LATENT, 0], dtype=torch.int32, device=one.device) for e in range(E)]).contiguous()
    g = torch.Generator().manual_seed(T)
    q = (torch.randn(1, 16 * T * E, d, generator=g) * 2.0).cuda()
    kv = torch.randn(1, E * N, 2 * d, generator=g).cuda()
    k, v = kv[:, :, :d], kv[:, :, d:]
    out_tall, out_each = torch.empty_like(q), torch.empty_like(q)
    scale = d ** -0.5

    def tall():
        hip.set_edit_batch(E)
        try:
            return hip.attention_wide(q, k, v, 1, scale, out=out_tall, tiles=(idx, E * LATENT, LATENT))
        finally:
            hip.set_edit_batch(1)

    def each():
        for e in range(E):
            rows = slice(16 * T * e, 16 * T * (e + 1))
            hip.attention_wide(q[:, rows], k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N], 1, scale, out=out_each[:, rows])
        return out_each

    gt, _ = capture_fn(tall)
    ge, _ = capture_fn(each)
    tt, te = [], []
    for i in range(7):
        for name in (("t", "e") if i % 2 == 0 else ("e", "t")):
            (tt if name == "t" else te).append(events_ms(gt if name == "t" else ge, a.steps, 3) * 1e3)
    ut, mmt = _stat(tt)
    ue, mme = _stat(te)
    row = {"E": E, "tiles_per_edit": T, "Nq": 16 * T * E, "keys_per_image": N, "d": d,
           "one_launch_us": ut, "one_launch_us_min_max": mmt, "E_single_launches_us": ue, "E_single_launches_us_min_max": mme,
           "E_single_over_one": round(ue / ut, 3),
           # (the key split follows the launch's tile count: another summation order, not another result)
           "max_abs_one_minus_E_single": float((out_tall - out_each).abs().max())}
    print(TAG + json.dumps(row), flush=True)


def child_stacked(kind, a):
    import torch

    from benchlib.common import capture_fn
    from sige_amd import hip, stacked
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads import sd_vae
    from tests.golden import vae_inputs

    hip.lib()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)  # noqa: E731
    decoder = kind == "decoder"
    cfg = sd_vae.VAEDecoderConfig() if decoder else sd_vae.VAEEncoderConfig()

    def make_model():
        torch.manual_seed(0)
        m = (sd_vae.SparseVAEDecoder if decoder else sd_vae.SparseVAEEncoder)(cfg).eval().to(dev).to(memory_format=torch.channels_last)
        m.set_scatter_inplace(True)
        if getattr(a, "dtype", "f32") == "f16":
            m.set_compute_dtype("f16")  # (--dtype f16: both the single-edit and the stacked model, every launch in its fp16 form)
        return m

    torch.manual_seed(0)
    quant = None if decoder else torch.nn.Conv2d(2 * cfg.z_channels, 2 * cfg.z_channels, 1).to(dev).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(1)
    shape = (1, cfg.z_channels, LATENT, LATENT) if decoder else (1, cfg.in_channels, IMAGE, IMAGE)
    x0 = torch.randn(shape, generator=g)
    noises = [torch.randn(shape, generator=g) for _ in range(8)]
    post = None if decoder else [cl(torch.randn(1, cfg.z_channels, LATENT, LATENT, generator=g)) for _ in range(8)]
    mask = vae_inputs.square_mask(IMAGE, a.ratio)
    row = {"ratio": a.ratio, "edit_ratio": float(mask.float().mean())}

    def run(m, x, n):
        if decoder:
            return m(x)
        return m.encode(x, quant, noise=n, scale_factor=SCALE_FACTOR)[1]

    with torch.no_grad():
        single, tall_model = make_model(), make_model()
        masks = downsample_mask(dilate_mask(mask.to(dev), 2), LATENT)
        for m in (single, tall_model):
            m.set_mode("full")
            run(m, cl(x0), None if decoder else post[0])
            m.set_masks(masks)
            m.set_mode("sparse")
        inside = masks[(LATENT, LATENT)].cpu() if decoder else mask.float()
        edits = [cl(x0 + n * inside) for n in noises]
        row["attention_tiles"] = int(single.mid.attn_1.gather.active_indices.shape[0])
        x1 = edits[0].clone()
        n1 = None if decoder else post[0].clone()
        run(single, x1, n1)
        n0 = hip.launch_count()
        run(single, x1, n1)
        row["single_edit_library_launches"] = hip.launch_count() - n0
        g1, out1 = capture_fn(lambda: run(single, x1, n1))
        row["E"] = {}
        for E in (2, 4, 8):
            xs = cl(torch.cat(edits[:E], 0))
            ns = None if decoder else cl(torch.cat(post[:E], 0))
            stacked.stack_caches(tall_model, E)
            try:
                stacked.set_masks(tall_model, [masks] * E)
                with stacked.edit_batch(tall_model, E):
                    run(tall_model, xs, ns)
                    n0 = hip.launch_count()
                    run(tall_model, xs, ns)
                    launches = hip.launch_count() - n0
                    gE, outE = capture_fn(lambda: run(tall_model, xs, ns))
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
                    if n1 is not None:
                        n1.copy_(post[e])
                    g1.replay()
                    worst = max(worst, float((outE[e] - out1[0]).abs().max()))
                if n1 is not None:
                    n1.copy_(post[0])
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


def main_stacked(kind, a, script):
    """The parent of `script --stacked`: one child per job; its half of profiles/sd_vae_stacked_bench.json."""
    from sige_amd import build

    what = ("SD VAE decoder (configs/sige.yaml ddconfig), latents [E,4,64,64] -> E images of 512 x 512" if kind == "decoder" else
            "SD VAE encoder (configs/sige.yaml ddconfig), E images [E,3,512,512] -> posterior samples [E,4,64,64] through quant_conv")
    res = {"workload": what + "; exact fp32, channels-last, hipGraph replay, default-initialised weights (seed 0); stacked edits: E "
                              "edited versions of one original under one square mask each, another noise per edit",
           "source_hash": build.source_hash(), "steps": a.steps, "batches": a.batches, "rows": []}
    f16 = getattr(a, "dtype", "f32") == "f16"
    common = ["--stacked", "--steps", str(a.steps), "--batches", str(a.batches)] + (["--dtype", "f16"] if f16 else [])
    jobs = ([("attention", ["--attention"])] if kind == "decoder" and not f16 else []) + [(r, ["--ratio", r]) for r in a.ratios.split(",")]
    if f16:
        res["workload"] = res["workload"].replace("exact fp32, ", "f16 compute mode (set_compute_dtype), ")
    for tag, extra in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(script), *extra, *common]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
        if p.returncode != 0 or line is None:
            # (a fault, an abort or a time limit: nothing more is started on the GPU)
            res["failed"] = {"job": tag, "returncode": p.returncode, "stderr_tail": p.stderr[-2000:]}
            break
        if tag == "attention":
            res["attention_alone_E8"] = json.loads(line[len(TAG):])
        else:
            res["rows"].append(json.loads(line[len(TAG):]))
        print("%s --stacked: %s done" % (os.path.basename(script), tag), file=sys.stderr, flush=True)
    out = a.stacked_out or (OUT_F16 if f16 else OUT)
    both = {}
    if os.path.isfile(out):
        with open(out) as f:
            both = json.load(f)
    both[kind + "_stacked" if f16 else kind] = res
    with open(out, "w") as f:
        json.dump(both, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "failed" in res else 0


def add_arguments(ap):
    ap.add_argument("--stacked", action="store_true", help="stacked edits E = 2, 4, 8 against single edits -> profiles/sd_vae_stacked_bench.json")
    ap.add_argument("--attention", action="store_true", help="(child of --stacked) the attention launch alone at E = 8, on the GPU")
    ap.add_argument("--stacked-out", default=None)


def dispatch(kind, a, script):
    """What `script` does under --stacked (None: not asked for)."""
    if not a.stacked:
        return None
    if a.attention:
        return attention_alone(a) or 0
    if a.ratio is not None:
        return child_stacked(kind, a) or 0
    return main_stacked(kind, a, script)
