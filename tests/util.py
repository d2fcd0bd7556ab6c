"""Helpers shared by the tests: golden loading, seeded inputs as torch tensors."""
import os

import numpy as np
import torch

from tests.golden_cases import CASES, make_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def golden(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN, name + ".npz"))
    return _cache[name]


def case_ids():
    return [c["name"] for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def tensors(case, device="cpu"):
    """Seeded inputs of a case as torch tensors on `device` (None stays None)."""
    d = make_inputs(case)
    out = {}
    for k, v in d.items():
        if isinstance(v, np.ndarray) and v.dtype != np.int64:
            out[k] = torch.from_numpy(v).to(device)
        else:
            out[k] = v
    return out


def ref(case, key, device="cpu"):
    return torch.from_numpy(golden("ops")["%s/%s" % (case["name"], key)]).to(device)


def x1_tiles(case, d, n1, device="cpu"):
    rs = np.random.RandomState(int(d["x1_seed"]))
    a = rs.standard_normal((case["B"] * n1, case["cout"], 4, 4)).astype(np.float32)
    return torch.from_numpy(a).to(device)


def shortcut_mask(case, d):
    g = case["geom"]
    Ho, Wo = d["out_res"]
    m = d["mask"].cpu().numpy()[:: g.stride[0], :: g.stride[1]][:Ho, :Wo]
    m = np.ascontiguousarray(np.pad(m, ((0, Ho - m.shape[0]), (0, Wo - m.shape[1]))))
    return torch.from_numpy(m)


def unpack(bits, shape):
    n = int(shape[0]) * int(shape[1])
    return torch.from_numpy(np.unpackbits(bits)[:n].reshape(int(shape[0]), int(shape[1])).astype(bool))


SWISH_RTOL = 1e-6  # swish <= 1e-6 rel (reference computes it in mixed float/double)
SWISH_ATOL = 1e-7
CONV_ATOL = 1e-3   # north_star: activations within 1e-3 fp32 on conv-containing paths


# ---- the benchmark network on the CPU with the oracle as native backend: what model-level GPU tests are pinned to ----------
_ddpm_oracle = {}


def cpu_backend():
    """The reference's own sige/cpu (oracle/_ref, built in the container from /root/reference and shipped as a .so) when it is
    there, else the C restatement -- the same choice as bench.py's parity leg."""
    from oracle import oracle

    try:
        from oracle import build_ref

        return oracle.as_backend(build_ref.load()), "oracle/_ref"
    except Exception:
        return oracle, "oracle (C restatement)"


def ddpm_cpu_oracle(masks, flip=False):
    """bench.py's DDPM-256 network (seed-0 weights, bench.make_inputs) on the CPU with the oracle natives
    (/root/reference/sige/cpu/gather.cpp:4-58, scatter.cpp:4-68, scatter_gather.cpp:5-84 restated / compiled): the full pass on
    the original (`flip`: its mirror image) and one sparse forward per mask in `masks` ([256,256] bool, CPU).  Returns
    (full, [sparse per mask]) as CPU tensors; memoised per process, so every model-level GPU test of one run compares with the
    SAME reference outputs.  A HIP-vs-HIP self-check is only a statement about two HIP paths; this is the row-defining one."""
    import bench
    from oracle import oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    keys = [(bool(flip), m.numpy().tobytes()) for m in masks]
    if ("full", bool(flip)) not in _ddpm_oracle or any(k not in _ddpm_oracle for k in keys):
        torch.manual_seed(0)
        model = DDPMSparseUNet(DDPMConfig()).eval()
        x0, noise = bench.make_inputs()
        if flip:
            x0 = x0.flip(-1).contiguous()
        t = torch.zeros(1)
        n_thr = min(32, os.cpu_count() or 1)
        torch.set_num_threads(n_thr)
        oracle.set_num_threads(n_thr)
        backend, _ = cpu_backend()
        runtime.register_backend("cpu", backend)
        try:
            with torch.no_grad():
                model.set_mode("full")
                _ddpm_oracle[("full", bool(flip))] = model(x0, t).clone()
                for k, m in zip(keys, masks):
                    if k in _ddpm_oracle:
                        continue
                    model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                    model.set_mode("sparse")
                    _ddpm_oracle[k] = model(x0 + noise * m, t).clone()
        finally:
            runtime.unregister_backend("cpu")
    return _ddpm_oracle[("full", bool(flip))], [_ddpm_oracle[k] for k in keys]


class native_full_pass:
    """Model-level GPU tests produce their caches with the library's exact-fp32 full pass (sige_amd/nn/dense.py
    FULL_PASS_F32_NATIVE): fixed kernels, fixed summation order -> the same caches bit for bit on every MI355X.  torch's conv
    goes through MIOpen's find mode, whose algorithm choice (and with it the last bits of every cache) may differ per box."""

    def __enter__(self):
        from sige_amd.nn import dense

        self._dense, self._keep = dense, dense.FULL_PASS_F32_NATIVE
        dense.FULL_PASS_F32_NATIVE = True
        return self

    def __exit__(self, *exc):
        self._dense.FULL_PASS_F32_NATIVE = self._keep
        return False


GAUGAN_SELF_ATOL = 1e-5  # the SPADE generator's output is a tanh: no amplification; measured 2e-7 (profiles/r6a_test_margins.jsonl)
SELF_ATOL = 1e-3   # two HIP forms of one forward against EACH OTHER: never tighter than the row's own tolerance (CONV_ATOL)


def record_margin(test, what, value, tol):
    """Append (measured difference, tolerance) of a model-level comparison to gpurun_out/test_margins.jsonl (when that scratch
    directory exists: the GPU sessions copy it to profiles/), so tolerances are set from a recorded distribution over boxes
    instead of one run's margin (VERDICT r5 next #1a)."""
    import json

    out = os.path.join(os.path.dirname(GOLDEN), os.pardir, "gpurun_out")
    if os.path.isdir(out):
        try:
            with open(os.path.join(out, "test_margins.jsonl"), "a") as f:
                f.write(json.dumps({"test": test, "what": what, "value": float(value), "tol": float(tol)}) + "\n")
        except OSError:  # (a read-only scratch directory must not fail a parity test)
            pass
    return float(value)


# ---- poisoned allocations: what a kernel leaves unwritten, or reads from memory nobody wrote, must show ----------------------
class poisoned:
    """Inside `with poisoned(value) as p:` every floating-point tensor that aten.empty / empty_like / new_empty / empty_strided /
    new_empty_strided returns (any device, any memory format; fp64 / fp32 / fp16 / bf16) is filled with `value` before anyone
    sees it, so an output a kernel never stores to, or a workspace it reads before writing, carries NaN (or a huge finite value,
    for the reads a NaN slips through: max, ReLU, `x > tol`).  torch.empty hands back freed blocks of the same size, which in a
    test often still hold the right answer; poisoning is what makes a missed store visible.  Integer and bool tensors (index
    lists, tables, maps) are left alone on purpose: an out-of-range index turns an over-read into an out-of-bounds address; they
    are compared bit-exactly instead.  Inside a CUDA graph capture the fill is captured too, so every replay re-poisons.
    A finite value beyond a narrow type's range becomes that type's largest finite value.  `p.n` counts the tensors poisoned.  (Not torch.utils.deterministic.fill_uninitialized_memory: that fills integers with
    INT_MAX and, through use_deterministic_algorithms, changes algorithm choice everywhere.)"""

    def __init__(self, value=float("nan")):
        self.value = float(value)
        self.n = 0
        self._mode = None

    def __enter__(self):
        from torch.utils._python_dispatch import TorchDispatchMode

        aten = torch.ops.aten
        empties = {aten.empty.memory_format, aten.empty_like.default, aten.new_empty.default, aten.empty_strided.default,
                   aten.new_empty_strided.default}
        owner = self

        class _Poison(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                if (func in empties and isinstance(out, torch.Tensor) and out.is_floating_point()
                        and out.device.type != "meta" and out.numel() > 0):
                    v = owner.value
                    if abs(v) != float("inf") and abs(v) > torch.finfo(out.dtype).max:  # (1e30 in an fp16 buffer: its largest finite)
                        v = torch.finfo(out.dtype).max if v > 0 else -torch.finfo(out.dtype).max
                    out.fill_(v)
                    owner.n += 1
                return out

        self._mode = _Poison()
        self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        mode, self._mode = self._mode, None
        mode.__exit__(*exc)
        return False


def assert_finite(t, what):
    """`t` holds no NaN / Inf; else name the first non-finite element (multi-index into t's logical shape) and its value."""
    ok = torch.isfinite(t)
    if bool(ok.all()):
        return
    flat = (~ok).reshape(-1).nonzero()
    first = int(flat[0])
    index = tuple(int(i) for i in np.unravel_index(first, tuple(t.shape)))
    raise AssertionError("%s: %d non-finite of %d, first at %s = %r" % (what, int(flat.numel()), t.numel(), index,
                                                                        float(t.reshape(-1)[first])))
