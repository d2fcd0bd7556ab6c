"""The Progressive Distillation U-Net workload on the GPU against tests/golden/pd_unet.npz (the REAL reference's SIGEUNet,
tests/golden/make_pd_golden.py): the reference's NCHW layout through the module chain, channels-last through the fused path
(hip.resample_tiles for the blocks that resample inside the block), persistent shortcut buffers poisoned, a second mask
without a new full pass, graph replay, and what the sparse forward launches at the tiled levels."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import pd_inputs  # noqa: E402
from tests.golden.model_init import init_by_name  # noqa: E402
from tests.test_pd_unet import GOLDEN, check_pd128, check_small, pd_config, run_pd  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]  # (pinned to the real reference's outputs, or to the CPU oracle backend)


def _record(test):
    return lambda what, value, tol: util.record_margin(test, what, value, tol)


@pytest.mark.parametrize("channels_last,inplace", [(False, False), (True, False), (True, True)])
def test_small_configuration_on_the_gpu_matches_the_reference_fixture(channels_last, inplace):
    """Both cached steps: NCHW (module chain), channels-last (fused path), channels-last with in-place persistent outputs
    (conv2 + scatter + residual in one launch, the residual being the kernel's shortcut buffer)."""
    _, outs, counts, ratio = run_pd(pd_inputs.SMALL, "cuda", channels_last, 2, inplace)
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    check_small(outs, util.CONV_ATOL, _record("test_gpu_pd_unet small cl=%d inplace=%d" % (channels_last, inplace)))


def test_small_configuration_with_poisoned_shortcut_buffers():
    """The persistent shortcut buffers hold NaN in front of every sparse forward: whatever the forward reads of them, the
    kernel wrote in that forward."""
    seen = []

    def poison(model):
        bufs = model.res_buffers()
        seen.append(len(bufs))
        for b in bufs:
            b.fill_(float("nan"))

    _, outs, _, _ = run_pd(pd_inputs.SMALL, "cuda", True, 2, True, prepare=poison)
    assert seen == [3, 3]  # two tiled "down" blocks, one tiled "up" block; allocated by set_masks, not by the forward
    for _, sparse in outs:
        util.assert_finite(sparse, "sparse output over poisoned shortcut buffers")
    check_small(outs, util.CONV_ATOL, _record("test_gpu_pd_unet small poisoned"))


def _two_masks(device, channels_last):
    """full(x0), mask A, sparse(x0 + noise * A), mask B (no new full pass), sparse(x0 + noise * B)."""
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.pd_unet import PDSparseUNet

    cfg = pd_inputs.SMALL
    model = PDSparseUNet(pd_config(cfg)).eval()
    init_by_name(model)
    x0, noise = pd_inputs.images(cfg["image_size"])
    model, x0, noise = model.to(device), x0.to(device), noise.to(device)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
        x0, noise = x0.contiguous(memory_format=torch.channels_last), noise.contiguous(memory_format=torch.channels_last)
        model.set_scatter_inplace(True)
    logsnr = torch.full((1,), pd_inputs.LOGSNR[0], device=device)
    outs = []
    with torch.no_grad():
        model.set_mode("full")
        model(x0, logsnr)
        for second in (False, True):
            mask = pd_inputs.edit_mask(cfg["image_size"], second).to(device)
            model.set_masks(pd_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask))
            model.set_mode("sparse")
            outs.append(model(x0 + noise * mask, logsnr).clone().cpu())
    return outs


def test_second_mask_without_a_new_full_pass_vs_cpu_oracle():
    """The shortcut buffers keep the previous mask's cells; the second mask's forward must read none of them."""
    from oracle import oracle
    from sige_amd import runtime

    runtime.register_backend("cpu", oracle)
    try:
        want = _two_masks("cpu", False)
    finally:
        runtime.unregister_backend("cpu")
    got = _two_masks("cuda", True)
    assert float((want[0] - want[1]).abs().max()) > 1e-2
    for k in range(2):
        err = float((got[k] - want[k]).abs().max())
        util.record_margin("test_gpu_pd_unet two masks", "mask %d" % k, err, util.CONV_ATOL)
        assert err <= util.CONV_ATOL, "mask %d: max |diff| %.3e" % (k, err)


def _sparse_model():
    """(model, edited image, logsnr) of the small configuration in sparse mode, channels-last, in-place outputs."""
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.pd_unet import PDSparseUNet

    cfg = pd_inputs.SMALL
    model = PDSparseUNet(pd_config(cfg)).eval()
    init_by_name(model)
    x0, noise = pd_inputs.images(cfg["image_size"])
    mask = pd_inputs.edit_mask(cfg["image_size"]).cuda()
    model = model.cuda().to(memory_format=torch.channels_last)
    x0, noise = (t.cuda().contiguous(memory_format=torch.channels_last) for t in (x0, noise))
    model.set_scatter_inplace(True)
    logsnr = torch.full((1,), pd_inputs.LOGSNR[0], device="cuda")
    with torch.no_grad():
        model.set_mode("full")
        model(x0, logsnr)
        model.set_masks(pd_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask))
        model.set_mode("sparse")
    return model, (x0 + noise * mask).contiguous(memory_format=torch.channels_last), logsnr


def test_sparse_forward_graph_replay_is_bit_identical():
    model, x1, logsnr = _sparse_model()
    with torch.no_grad():
        eager = model(x1, logsnr).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(x1, logsnr)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(x1, logsnr)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    want = GOLDEN["small/sparse0"]
    assert float(np.abs(out.cpu().numpy() - want).max()) <= util.CONV_ATOL


class _AtenOps(torch.utils._python_dispatch.TorchDispatchMode):
    """Every aten op of a forward with the shape of its first tensor output."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else (out,)
        first = next((o for o in outs if isinstance(o, torch.Tensor)), None)
        self.seen.append((func._schema.name.split("::")[-1], None if first is None else tuple(first.shape)))
        return out


_ELEMENTWISE = {"avg_pool2d", "upsample_nearest2d", "silu", "silu_", "sigmoid", "mul", "mul_", "add", "add_"}


def _tiled_level_ops(model, x1, logsnr, dense_res):
    """The forbidden aten ops of one sparse forward whose result is a 4-D activation above the dense levels, or a tile tensor."""
    with torch.no_grad(), _AtenOps() as rec:
        model(x1, logsnr)
    bad = []
    for name, shape in rec.seen:
        if shape is None or len(shape) != 4 or name not in _ELEMENTWISE:
            continue
        if shape[2] not in dense_res:  # (everything that is not a tensor of a dense level: the tiled levels and the tile slabs)
            bad.append((name, shape))
    return bad


def test_no_whole_tensor_elementwise_or_pooling_kernel_at_the_tiled_levels():
    """Between conv_in and norm_out the channels-last sparse forward runs no avg_pool2d / upsample_nearest2d / silu / mul / add aten
    kernel on a tensor of a tiled level (64x64, 32x32) nor on a tile slab; with the resampling blocks forced onto the torch-op
    chain the same probe sees exactly those."""
    from sige_amd.workloads import pd_unet

    model, x1, logsnr = _sparse_model()
    dense = (16,)  # the small configuration's only dense level
    with torch.no_grad():
        model(x1, logsnr)
    assert _tiled_level_ops(model, x1, logsnr, dense) == []
    keep = pd_unet.FUSED_RESAMPLE
    pd_unet.FUSED_RESAMPLE = False
    try:
        bad = _tiled_level_ops(model, x1, logsnr, dense)
    finally:
        pd_unet.FUSED_RESAMPLE = keep
    names = {n for n, _ in bad}
    assert {"avg_pool2d", "upsample_nearest2d", "silu"} <= names, bad


def test_pd128_on_the_gpu_matches_the_reference_fixture():
    """church_pd128-sige.yml (139.6 M parameters), channels-last, in-place outputs: full and sparse against the fixture, and the
    masks rebuilt on the device give the reference's tile counts."""
    _, outs, counts, ratio = run_pd(pd_inputs.PD128, "cuda", True, 1, True)
    assert abs(ratio - float(GOLDEN["pd128/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["pd128/tiles"])
    check_pd128(*outs[0], util.CONV_ATOL, _record("test_gpu_pd_unet pd128"))
