"""The GAN-Compression GauGAN generator (sige_amd.workloads.gaugan_sub_mobile) through the HIP kernels, pinned to
tests/golden/gaugan_sub_mobile.npz (the REAL reference's outputs): the reference's NCHW layout, channels-last with the separable
convs as the reference's module chain, channels-last with ONE hip.spade_separable_cl launch per SPADE layer; the two channels-last
forms against each other; the launch count; and a second cached original.

Tolerances: 1e-3 against the fixture (the row's own, tests/test_models_golden.py).  Native against chain: util.SELF_ATOL; the two
differ by the summation order of exact fp32 products behind a tanh (~1e-6 expected; the measured margins are recorded through
util.record_margin -> profiles/spade_separable_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import sub_mobile_inputs as inputs  # noqa: E402
from tests.test_gaugan_sub_mobile import build_model, check, run_model  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
ATOL = 1e-3  # north_star: activations within 1e-3 fp32 on conv-containing paths
SPADE_LAYERS = 3 * 2 + 4 * 3  # head_0, G_middle_0, G_middle_1: norm_0, norm_1; up_0 .. up_3: norm_0, norm_1, norm_s


class separable_native:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sige_amd.workloads import gaugan_sub_mobile as m

        self.m, self.keep = m, m.SEPARABLE_NATIVE
        m.SEPARABLE_NATIVE = self.on

    def __exit__(self, *exc):
        self.m.SEPARABLE_NATIVE = self.keep
        return False


_memo = {}


def outputs(group, form):
    """(full, sparse) of `form` in nchw_chain | cl_chain | cl_native, computed once per process."""
    if (group, form) not in _memo:
        cl = form != "nchw_chain"
        with separable_native(form == "cl_native"):
            full, sparse, _ = run_model(group, "cuda", cl, fused=cl)
        _memo[(group, form)] = (full.cpu(), sparse.cpu())
    return _memo[(group, form)]


@pytest.mark.parametrize("form", ["nchw_chain", "cl_chain", "cl_native"])
@pytest.mark.parametrize("group", list(inputs.GROUPS))
def test_generator_on_the_gpu_matches_the_reference_fixture(group, form):
    full, sparse = outputs(group, form)
    util.assert_finite(sparse, "sparse output")
    ef = check(group, "full", full, ATOL)
    es = check(group, "sparse", sparse, ATOL)
    util.record_margin("test_gpu_gaugan_sub_mobile vs fixture", "%s %s full" % (group, form), ef, ATOL)
    util.record_margin("test_gpu_gaugan_sub_mobile vs fixture", "%s %s sparse" % (group, form), es, ATOL)


@pytest.mark.parametrize("group", ["small7", "readme"])
def test_native_equals_the_module_chain(group):
    _, chain = outputs(group, "cl_chain")
    _, native = outputs(group, "cl_native")
    diff = float((native - chain).abs().max())
    print("sub-mobile %s: max |native - chain| %.3e" % (group, diff))
    util.record_margin("test_gpu_gaugan_sub_mobile native vs chain", group, diff, util.SELF_ATOL)
    assert diff <= util.SELF_ATOL


def test_one_separable_launch_per_spade_layer():
    """small7/: every block is tiled.  Each hip.spade_separable_cl call is one library launch, and there is one per SPADE layer."""
    from sige_amd import hip

    with separable_native(True):
        _, _, model = run_model("small7", "cuda", True, fused=True)
        x1 = inputs.labels("small7")[1].cuda().contiguous(memory_format=torch.channels_last)
        launches, orig = [], hip.spade_separable_cl

        def counted(*a, **kw):
            n0 = hip.launch_count()
            out = orig(*a, **kw)
            launches.append((hip.launch_count() - n0, out is not None, bool(kw.get("tiled"))))
            return out

        hip.spade_separable_cl = counted
        try:
            with torch.no_grad():
                model(x1)
        finally:
            hip.spade_separable_cl = orig
    assert launches == [(1, True, True)] * SPADE_LAYERS
    with separable_native(False):
        n_chain0 = hip.launch_count()
        with torch.no_grad():
            model(x1)
        n_chain = hip.launch_count() - n_chain0
    with separable_native(True):
        n0 = hip.launch_count()
        with torch.no_grad():
            model(x1)
        n_native = hip.launch_count() - n0
    print("small7 sparse forward: %d library launches native, %d with the module chain" % (n_native, n_chain))
    assert n_chain - n_native >= 3 * SPADE_LAYERS  # (the chain: two grouped and two 1x1 tile convs per layer, torch ops not counted)


def test_second_original_rereads_the_cached_affine():
    """A full pass on ANOTHER original, then a sparse pass: equal to a fresh model's -- the stacked InstanceNorm affine is rebuilt by
    every full pass, and no stale stacked operand survives."""
    with separable_native(True):
        _, _, model = run_model("small7", "cuda", True, fused=True)
        first = [t.clone() for t in model.up_3.norm_0._sep_affine]
        _, again, _ = run_model("small7", "cuda", True, variant=1, model=model)
        moved = max(float((a - b).abs().max()) for a, b in zip(first, model.up_3.norm_0._sep_affine))
        assert moved > 1e-2  # (the two originals have different statistics: a stale affine would show)
        _, fresh, _ = run_model("small7", "cuda", True, fused=True, variant=1)
    diff = float((again - fresh).abs().max())
    util.record_margin("test_gpu_gaugan_sub_mobile second original", "small7", diff, util.SELF_ATOL)
    assert diff <= util.SELF_ATOL
    # ... and an in-place weight update is seen by the stacked operand copies
    with separable_native(True):
        model = build_model("small7").cuda().to(memory_format=torch.channels_last)
        _, before, _ = run_model("small7", "cuda", True, model=model)
        with torch.no_grad():
            model.up_3.norm_0.mlp_gamma.conv[2].bias.add_(0.5)
        _, after, _ = run_model("small7", "cuda", True, model=model)
        with separable_native(False):
            _, chain, _ = run_model("small7", "cuda", True, model=model)
    assert float((after - before).abs().max()) > 1e-2
    assert float((after - chain).abs().max()) <= util.SELF_ATOL
