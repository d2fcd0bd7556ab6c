"""Stacked edits (sige_amd/stacked.py) through the GAN-Compression GauGAN generator (sige_amd.workloads.gaugan_sub_mobile): E = 4
edits of one original, each with its own mask, in ONE forward on the GPU; every edit's slice against THAT edit's own sparse forward
of the same network on the CPU with the oracle as native back end (the workload there is pinned to the real reference by
tests/test_gaugan_sub_mobile.py), and against the same model's single-edit GPU forward.

Configuration: ngf 16, widths 8_8_8_12_8_8_8_8, crop 512 on 256x512 label maps -> 4x8 at the smallest level, the smallest size that
stacks (one image's height must be a power of two >= 4).  num_sparse_layers 4: head_0, G_middle_0 and G_middle_1 are dense (label
widths 16 / 16 / 24, at 4x8, 8x16, 16x32), each of their six SPADE layers recomputes its InstanceNorm per edit; 7: every block tiled.
The edits relabel a 51x128 rectangle each ((label + 5) % 36; 4.98 % of the image): one in the middle, one on rows 0.., one on rows
..255 and one on columns 0.. -- in the tall tensor edit 1's first rows lie under edit 0's last ones and edit 2's last rows over
edit 3's first ones.

Tolerances: util.CONV_ATOL against the oracle; util.GAUGAN_SELF_ATOL stacked against single (fp32 summation order behind a tanh;
with SEPARABLE_STATS_NATIVE off the single forward takes the dense layers' statistics from torch's var_mean instead of the library's
two-pass launch: ~1e-6 relative on the scales).  The measured margins go through util.record_margin
(profiles/spade_separable_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import sub_mobile_inputs as inputs  # noqa: E402
from tests.golden.model_init import gaugan_labels  # noqa: E402
from tests.test_gaugan_sub_mobile import check, run_model  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
CL = torch.channels_last
PLACES = [(85, 128), (0, 28), (205, 328), (125, 0)]  # (top, left) of the 51 x 128 rectangle of edit e
TILED_SPADE = {4: 4 * 3, 7: 3 * 2 + 4 * 3}           # SPADE layers of the tiled blocks (up_*: norm_0, norm_1, norm_s)
DENSE_SPADE = {4: 3 * 2, 7: 0}                        # ... and of the dense ones (head_0, G_middle_*: norm_0, norm_1)


def _model(k, fused):
    from sige_amd.workloads.gaugan_sub_mobile import SubMobileSPADEConfig, SubMobileSpadeGenerator

    cfg = SubMobileSPADEConfig(ngf=16, crop_size=512, channels=(8, 8, 8, 12, 8, 8, 8, 8), num_sparse_layers=k, fused=fused)
    model = SubMobileSpadeGenerator(cfg).eval()
    inputs.init_weights(model)
    assert (model.sh, model.sw) == (4, 8)
    return model


def _labels():
    """(original, [edit 0 .. 3]) one-hot [1,36,256,512] on the CPU."""
    x0 = gaugan_labels(256, 512)[0]
    lab0 = x0.argmax(1)
    edits = []
    for top, left in PLACES:
        lab = lab0.clone()
        lab[:, top:top + 51, left:left + 128] = (lab0[:, top:top + 51, left:left + 128] + 5) % 36
        edits.append(torch.nn.functional.one_hot(lab, 36).permute(0, 3, 1, 2).float().contiguous())
    return x0, edits


def _pyramid(model, x0, xi):
    from sige_amd.utils import compute_difference_mask, dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(compute_difference_mask(x0, xi), 1), (model.sh, model.sw), dilation=2)


_oracle = {}


def oracle_outputs(k):
    """Each edit's own sparse forward on the CPU, oracle back end: computed once per process and left unchanged."""
    if k not in _oracle:
        from oracle import oracle
        from sige_amd import runtime

        model = _model(k, fused=False)
        x0, edits = _labels()
        torch.set_num_threads(8)
        runtime.register_backend("cpu", oracle)
        try:
            with torch.no_grad():
                model.set_mode("full")
                full = model(x0).clone()
                model.set_mode("sparse")
                outs = []
                for xi in edits:
                    model.set_masks(_pyramid(model, x0, xi))
                    outs.append(model(xi)[0].clone())
        finally:
            runtime.unregister_backend("cpu")
        assert float(full.std()) > 0.1 and float((full.abs() > 0.99).float().mean()) <= 0.01  # (unsaturated: the tanh pins something)
        _oracle[k] = outs
    return _oracle[k]


class counted:
    """hip.spade_separable_stats_cl / hip.spade_separable_cl with the library launches of every call written down."""

    def __init__(self, hip):
        self.hip, self.log = hip, []

    def __enter__(self):
        hip, log = self.hip, self.log
        self.keep = (hip.spade_separable_stats_cl, hip.spade_separable_cl)
        stats, sep = self.keep

        def c_stats(*a, **kw):
            n0 = hip.launch_count()
            out = stats(*a, **kw)
            log.append(("stats", hip.launch_count() - n0, out is not None))
            return out

        def c_sep(*a, **kw):
            n0 = hip.launch_count()
            out = sep(*a, **kw)
            log.append(("tiled" if kw.get("tiled") else "dense", hip.launch_count() - n0, out is not None))
            return out

        hip.spade_separable_stats_cl, hip.spade_separable_cl = c_stats, c_sep
        return self.log

    def __exit__(self, *exc):
        self.hip.spade_separable_stats_cl, self.hip.spade_separable_cl = self.keep
        return False


@pytest.mark.parametrize("k", [4, 7])
def test_stacked_edits_vs_cpu_oracle_and_single_edits(k):
    from sige_amd import hip, stacked

    want = oracle_outputs(k)
    E = len(PLACES)
    model = _model(k, fused=True).cuda().to(memory_format=CL)
    x0, edits = _labels()
    x0 = x0.cuda().contiguous(memory_format=CL)
    edits = [x.cuda().contiguous(memory_format=CL) for x in edits]
    with torch.no_grad():
        model.set_mode("full")
        model(x0)
        model.set_mode("sparse")
        pyrs, singles = [], []
        for xi in edits:
            pyrs.append(_pyramid(model, x0, xi))
            model.set_masks(pyrs[-1])
            model(xi)  # (the first forward under a mask packs weights and sizes buffers: not the steady state)
            singles.append(model(xi).clone())
        n0 = hip.launch_count()
        model(edits[-1])
        single_launches = hip.launch_count() - n0
        xs = torch.cat(edits, 0).contiguous(memory_format=CL)
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                model(xs)
                n0 = hip.launch_count()
                with counted(hip) as log:
                    got = model(xs).clone()
                launches = hip.launch_count() - n0
        finally:
            stacked.unstack_caches(model)
        assert hip.get_edit_batch() == 1
        assert tuple(got.shape) == (E, 3, 256, 512)
        util.assert_finite(got, "stacked output")
        # one launch per layer whatever E is: the single forward's, a few for blocks routed differently at E times the tiles, and
        # one statistics launch per dense SPADE layer (which a single forward with SEPARABLE_STATS_NATIVE off leaves to torch kernels)
        print("sub-mobile k=%d: %d library launches stacked (E=%d), %d single" % (k, launches, E, single_launches))
        assert launches <= single_launches + 8 + DENSE_SPADE[k], (launches, single_launches)
        # every dense SPADE layer: one statistics launch, then one separable launch; every tiled one: one launch
        assert all(n == 1 and ok for _, n, ok in log), log
        kinds = [kind for kind, _, _ in log]
        assert kinds.count("stats") == kinds.count("dense") == DENSE_SPADE[k] and kinds.count("tiled") == TILED_SPADE[k], kinds
        assert all(kinds[i + 1] == "dense" for i, kind in enumerate(kinds) if kind == "stats"), kinds
        for e in range(E):
            err = float((got[e].cpu() - want[e]).abs().max())
            own = float((got[e] - singles[e][0]).abs().max())
            print("sub-mobile k=%d edit %d %s: vs oracle %.3e, vs single %.3e" % (k, e, PLACES[e], err, own))
            util.record_margin("gaugan_sub_mobile_stacked vs oracle", "k=%d edit %d" % (k, e), err, util.CONV_ATOL)
            util.record_margin("gaugan_sub_mobile_stacked vs single", "k=%d edit %d" % (k, e), own, util.GAUGAN_SELF_ATOL)
            assert err <= util.CONV_ATOL, (e, PLACES[e], err)
            assert own <= util.GAUGAN_SELF_ATOL, (e, PLACES[e], own)
        assert float((got[0] - got[1]).abs().max()) > 1e-3  # (the edits do differ)
        # back to single edits: the caches are the original's again
        model.set_masks(pyrs[1])
        model(edits[1])
        assert torch.equal(model(edits[1]), singles[1])


def test_a_level_of_two_rows_does_not_stack():
    """small5: crop 256 with six up-samplings is 2 x 4 at the top -- below the four rows the seam shift needs."""
    from sige_amd import hip, stacked

    _, _, model = run_model("small5", "cuda", True, fused=True)
    x1 = inputs.labels("small5")[1].cuda().contiguous(memory_format=CL)
    with stacked.edit_batch(model, 2):
        with torch.no_grad(), pytest.raises(RuntimeError, match="stacked"):
            model(torch.cat([x1, x1]).contiguous(memory_format=CL))
    assert hip.get_edit_batch() == 1


def test_statistics_launch_in_a_single_edit_forward():
    """SEPARABLE_STATS_NATIVE at E = 1: the dense layers' InstanceNorm from the statistics launch instead of the torch prologue."""
    from sige_amd import hip
    from sige_amd.workloads import gaugan_sub_mobile as m

    assert m.SEPARABLE_NATIVE
    keep = m.SEPARABLE_STATS_NATIVE
    outs = {}
    try:
        for on in (False, True):
            m.SEPARABLE_STATS_NATIVE = on
            _, sparse, model = run_model("small5", "cuda", True, fused=True)
            if on:
                x1 = inputs.labels("small5")[1].cuda().contiguous(memory_format=CL)
                with counted(hip) as log, torch.no_grad():
                    model(x1)
                assert [kind for kind, _, _ in log].count("stats") == 2 * 2 and all(n == 1 and ok for _, n, ok in log), log
            outs[on] = sparse.cpu()
    finally:
        m.SEPARABLE_STATS_NATIVE = keep
    util.assert_finite(outs[True], "sparse output")
    diff = float((outs[True] - outs[False]).abs().max())
    print("sub-mobile small5: max |statistics launch - torch prologue| %.3e" % diff)
    util.record_margin("gaugan_sub_mobile stats native vs torch prologue", "small5", diff, util.SELF_ATOL)
    assert diff <= util.SELF_ATOL
    check("small5", "sparse", outs[True], 1e-3)
