#!/usr/bin/env python3
"""What accepting an edit costs: DDPM-256 in the benchmarked configuration (channels-last, set_scatter_inplace(True), twins warmed by
one forward), at 1.2 / 5 / 15 % edits, the ms of
  (a) the plain sparse forward,
  (b) the `sparse_update` forward (the edit becomes the new original),
  (c) the first forward under a NEW mask after (b),
the commit launches of (b) alone, and hip.launch_count() per forward.  EAGER forwards (a `sparse_update` forward is not captured in
a graph), otherwise the method of DESIGN.md 4: inputs resident in HBM, a synchronise on both sides of exactly K forwards, HIP
events, the median over the batches.  Public API only, so the same file runs on the commit before the commit path existed -- what
that commit cannot do is recorded as an "error" string.

    python tools/commit_bench.py --tag result --out profiles/ddpm_commit_bench.json      (rows are appended under the tag)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from sige_amd import hip  # noqa: E402
from sige_amd.utils import dilate_mask, downsample_mask  # noqa: E402
from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet  # noqa: E402

DEV = torch.device("cuda")
CL = torch.channels_last


def timed(fn, k, batches, before=None):
    """Median (min, max) ms of one call of fn over `batches` batches of k calls.  `before`: runs, untimed, in front of EVERY call
    (each call is then timed on its own and the batch is their mean)."""
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before is None:
            torch.cuda.synchronize()
            a.record()
            for _ in range(k):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / k)
        else:
            total = 0.0
            for _ in range(k):
                before()
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                total += a.elapsed_time(b)
            out.append(total / k)
    return dict(ms=round(statistics.median(out), 4), min=round(min(out), 4), max=round(max(out), 4))


def launches(fn):
    n0 = hip.launch_count()
    fn()
    torch.cuda.synchronize()
    return hip.launch_count() - n0


def guarded(row, key, fn):
    try:
        row[key] = fn()
    except Exception as e:  # (a commit that cannot run this step: say so, go on)
        row[key] = dict(error="%s: %s" % (type(e).__name__, str(e)[:200]))
        torch.cuda.synchronize()
        return False
    return True


def one_ratio(ratio, k, batches, opt_in):
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=CL)
    if opt_in is not None and hasattr(type(model), "COMMIT_TILES"):
        model.COMMIT_TILES = opt_in
    model.set_scatter_inplace(True)
    x0, noise = bench.make_inputs()
    m1, m2 = bench.edit_mask(ratio), bench.edit_mask(ratio, rank=3)
    t = torch.zeros(1, device=DEV)
    x0d = x0.to(DEV).contiguous(memory_format=CL)
    x1 = (x0 + noise * m1).to(DEV).contiguous(memory_format=CL)
    x2 = (x0 + noise * m1 + noise.flip(-1) * m2).to(DEV).contiguous(memory_format=CL)
    p1, p2 = (downsample_mask(dilate_mask(m.to(DEV), 5), 8) for m in (m1, m2))
    row = dict(ratio=ratio, commit_tiles=getattr(model, "COMMIT_TILES", None))

    def plain():
        model(x1, t)

    def accept():
        model.set_sparse_update(True)
        try:
            model(x1, t)
        finally:
            model.set_sparse_update(False)

    def to_m1_and_accept():
        model.set_masks(p1)
        model(x1, t)
        accept()
        model.set_masks(p2)

    with torch.no_grad():
        model.set_mode("full")
        model(x0d, t)
        model.set_masks(p1)
        model.set_mode("sparse")
        for _ in range(3):
            plain()  # (registers and warms the twins; every kernel loaded)
        row["a_plain"] = dict(timed(plain, k, batches), launches=launches(plain))
        if guarded(row, "b_sparse_update", lambda: dict(timed(accept, k, batches), launches=launches(accept))):
            seen = []
            if hasattr(hip, "commit_tiles"):
                inner = hip.commit_tiles
                hip.commit_tiles = lambda recs: (seen.append(list(recs)), inner(recs))[1]
                try:
                    accept()
                finally:
                    hip.commit_tiles = inner
            if seen:
                recs = seen[-1]
                row["commit_alone"] = dict(timed(lambda: hip.commit_tiles(recs), k, batches), launches=launches(lambda: hip.commit_tiles(recs)),
                                           records=len(recs))
            guarded(row, "c_new_mask_first_forward", lambda: dict(
                timed(lambda: model(x2, t), 3, max(3, batches // 2), before=to_m1_and_accept),
                launches=(to_m1_and_accept(), launches(lambda: model(x2, t)))[1]))
        # (a) again, behind everything: the plain forward is what it was
        model.set_masks(p1)
        for _ in range(2):
            plain()
        row["a_plain_after"] = dict(timed(plain, k, batches), launches=launches(plain))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ddpm_commit_bench.json"))
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--ratios", default="0.012,0.05,0.15")
    ap.add_argument("--opt-in", choices=("default", "on", "off"), default="default")
    args = ap.parse_args()
    opt_in = {"default": None, "on": True, "off": False}[args.opt_in]
    rows = [one_ratio(float(r), args.k, args.batches, opt_in) for r in args.ratios.split(",")]
    doc = {}
    if os.path.isfile(args.out):
        doc = json.load(open(args.out))
    doc[args.tag] = dict(rows=rows, device=torch.cuda.get_device_name(0), k=args.k, batches=args.batches, opt_in=args.opt_in,
                         when=time.strftime("%Y-%m-%d %H:%M:%S"), method="eager forwards, HIP events, synchronise on both sides of k forwards, median over batches")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
