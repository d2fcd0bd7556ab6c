"""CPU tests of tests/mask_zoo.py: the masks of the model-level GPU tests (tests/test_gpu_masks.py) are pinned tile count for
tile count, every one is a real edit, and every one is WELL CONDITIONED -- measured on the reference alone (the network on the CPU
with the oracle natives), never on the code under test: a legitimate change of fp32 rounding or of fp16 operand rounding moves
its output by a small fraction of the tolerance the GPU tests apply.  A mask that does not meet that is replaced, not excused."""
import os

import pytest
import torch
from torch import nn

from tests import mask_zoo, util

NAMES = list(mask_zoo.COUNTS)
F32_JITTER_BOUND = 1e-4  # a tenth of util.CONV_ATOL; measured worst 6.9e-6 (assets_mask)
F16_EMULATED_BOUND = 0.5  # of tolerance.f16_check's allowance; measured worst 0.18


def test_zoo_is_what_the_table_says():
    from oracle import oracle

    zoo = mask_zoo.zoo()
    assert list(zoo) == NAMES and len(zoo) == 9
    assert set(mask_zoo.SEQUENCE) == set(NAMES) and len(mask_zoo.SEQUENCE) == 9
    assert set(mask_zoo.STACK) == set(NAMES) - {"diagonal"} and len(mask_zoo.STACK) == 8
    for name, m in zoo.items():
        assert m.dtype == torch.bool and tuple(m.shape) == (256, 256) and m.device.type == "cpu" and not m.all(), name
        pyr = oracle.downsample_mask(oracle.dilate_mask(m, 5), 8)
        assert sorted(pyr, reverse=True) == [(r, r) for r in mask_zoo.LEVELS], name
        got6 = tuple(oracle.reduce_mask(pyr[(r, r)], 6, 4, 1).shape[0] for r in mask_zoo.LEVELS)
        got4 = tuple(oracle.reduce_mask(pyr[(r, r)], 4, 4, 0).shape[0] for r in mask_zoo.LEVELS)
        assert (got6, got4) == mask_zoo.COUNTS[name], (name, got6, got4)
    # what the names promise
    assert abs(float(zoo["assets_mask"].float().mean()) - 0.155) < 1e-3 and zoo["assets_mask"][0].any() and zoo["assets_mask"][:, 255].any()
    assert int(zoo["specks"].sum()) == 48 and int(zoo["corners"].sum()) == 4 and int(zoo["last_pixel"].sum()) == 1
    assert float(zoo["full_grid"].float().mean()) == 0.0625
    assert mask_zoo.COUNTS["full_grid"][0] == tuple((r // 4 + 1) ** 2 for r in mask_zoo.LEVELS)
    assert mask_zoo.COUNTS["full_grid"][1] == tuple((r // 4) ** 2 for r in mask_zoo.LEVELS)
    # the seams of the stacked forward: the (dilated) mask is active in the last row of the upper image and in the first row of
    # the lower one
    for up, low in mask_zoo.SEAMS_ACTIVE_ON_BOTH_SIDES:
        assert mask_zoo.STACK.index(low) == mask_zoo.STACK.index(up) + 1
        assert oracle.dilate_mask(zoo[up], 5)[255].any() and oracle.dilate_mask(zoo[low], 5)[0].any(), (up, low)


@pytest.fixture(scope="module")
def conditioning():
    """Per mask, on the CPU oracle network alone: |sparse - full|, the largest move of the output under two draws of a one-rounding
    fp32 jitter of every conv's input and output, and the f16 criterion of the emulated fp16 forward (operands; operands + storage)."""
    import bench
    from oracle import oracle
    from sige_amd import runtime, tolerance
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet
    from tests.f16_error_trace import Emulator

    zoo = mask_zoo.zoo()
    full, sparse = util.ddpm_cpu_oracle(list(zoo.values()))
    res = {n: {"edit": float((o - full).abs().max())} for n, o in zip(zoo, sparse)}

    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval()
    emus = {False: Emulator(model, storage=False), True: Emulator(model, storage=True)}
    keep = tuple(model.F16_KEEP)
    f16_names = [n for n in emus[False].convs if not any(n == k or n.startswith(k) for k in keep)]
    assert 0 < len(f16_names) < len(emus[False].convs)
    jitter_on = [False]
    gen = torch.Generator().manual_seed(3)

    def jit(t):
        return t * (1.0 + (torch.rand(t.shape, generator=gen) * 2 - 1) * 2.0 ** -23)

    def pre(mod, args):
        if jitter_on[0] and isinstance(args[0], torch.Tensor) and args[0].dtype == torch.float32:
            return (jit(args[0]),) + tuple(args[1:])
        return None

    def post(mod, args, out):
        if jitter_on[0] and isinstance(out, torch.Tensor):
            return jit(out)
        return None

    n_convs = 0
    for mod in model.modules():
        if isinstance(mod, nn.Conv2d):
            mod.register_forward_pre_hook(pre)
            mod.register_forward_hook(post)
            n_convs += 1
    assert n_convs > 60
    x0, noise = bench.make_inputs()
    t = torch.zeros(1)
    n_thr = min(32, os.cpu_count() or 1)
    torch.set_num_threads(n_thr)
    oracle.set_num_threads(n_thr)
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            model.set_mode("full")
            model(x0, t)
            for (name, m), want in zip(zoo.items(), sparse):
                x1 = x0 + noise * m
                model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
                model.set_mode("sparse")
                ref = model(x1, t).clone()
                assert torch.equal(ref, want), name  # (hooks idle: the memoised reference of the GPU tests, bit for bit)
                worst = 0.0
                for _ in range(2):
                    jitter_on[0] = True
                    try:
                        got = model(x1, t).clone()
                    finally:
                        jitter_on[0] = False
                    worst = max(worst, float((got - ref).abs().max()))
                res[name]["f32_jitter"] = worst
                for storage, emu in emus.items():
                    emu.set_active(f16_names)
                    try:
                        got = model(x1, t).clone()
                    finally:
                        emu.set_active(())
                    res[name]["f16_storage" if storage else "f16"] = tolerance.f16_check(got, ref)["worst_over_allowed"]
                print("%-12s %s" % (name, res[name]), flush=True)
    finally:
        runtime.unregister_backend("cpu")
    return res


@pytest.mark.parametrize("name", NAMES)
def test_every_mask_is_a_real_and_well_conditioned_edit(conditioning, name):
    r = conditioning[name]
    assert r["edit"] > 1e-2, r  # (smallest measured: last_pixel, 0.047)
    assert 0.0 < r["f32_jitter"] <= F32_JITTER_BOUND, r
    assert 0.0 < r["f16"] <= F16_EMULATED_BOUND and 0.0 < r["f16_storage"] <= F16_EMULATED_BOUND, r
