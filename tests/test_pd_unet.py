"""The Progressive Distillation U-Net workload (sige_amd/workloads/pd_unet.py) on the CPU with the oracle as native backend,
against tests/golden/pd_unet.npz -- the outputs of the REAL reference's SIGEUNet (tests/golden/make_pd_golden.py) -- and the
argument checks of sige_hip_resample_tiles_nhwc_f32, which are made before anything touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden import pd_inputs  # noqa: E402
from tests.golden.model_init import init_by_name, summarize  # noqa: E402

pytestmark = pytest.mark.oracle_parity  # (pinned to tests/golden/pd_unet.npz = the real reference's outputs)
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "pd_unet.npz"))
ATOL = 1e-3  # tests/util.py CONV_ATOL: activations within 1e-3 fp32 on conv-containing paths


def pd_config(cfg: dict):
    from sige_amd.workloads.pd_unet import PDConfig

    return PDConfig(**cfg)


def run_pd(cfg: dict, device: str, channels_last: bool, steps: int, inplace: bool = False, prepare=None):
    """[(full, sparse) per step] of PDSparseUNet on the fixture's inputs, as the generator ran the reference.  `prepare(model)`
    runs in front of every sparse forward."""
    from sige_amd.utils import dilate_mask, downsample_mask, reduce_mask
    from sige_amd.workloads.pd_unet import PDSparseUNet

    model = PDSparseUNet(pd_config(cfg)).eval()
    init_by_name(model)
    size = cfg["image_size"]
    x0, noise = pd_inputs.images(size)
    mask = pd_inputs.edit_mask(size)
    x1 = x0 + noise * mask
    model, x0, x1, mask = model.to(device), x0.to(device), x1.to(device), mask.to(device)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
        x0, x1 = x0.contiguous(memory_format=torch.channels_last), x1.contiguous(memory_format=torch.channels_last)
    model.set_scatter_inplace(inplace)
    masks = pd_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)
    outs = []
    with torch.no_grad():
        for step in range(steps):
            logsnr = torch.full((1,), pd_inputs.LOGSNR[step], device=device)
            model.set_cache_id(step)
            model.set_mode("full")
            full = model(x0, logsnr).clone()
            model.set_masks(masks)
            model.set_mode("sparse")
            if prepare is not None:
                prepare(model)
            outs.append((full, model(x1, logsnr).clone()))
    counts = pd_inputs.tile_counts({k: v.cpu() for k, v in masks.items()}, reduce_mask)
    return model, outs, counts, float(mask.float().mean())


def check_small(outs, atol=ATOL, record=None):
    for step, (full, sparse) in enumerate(outs):
        for name, t in (("full", full), ("sparse", sparse)):
            want = GOLDEN["small/%s%d" % (name, step)]
            err = float(np.abs(t.float().cpu().numpy() - want).max())
            if record is not None:
                record("small/%s%d" % (name, step), err, atol)
            assert err <= atol, "small/%s%d: max |diff| %.3e > %.1e" % (name, step, err, atol)


def check_pd128(full, sparse, atol=ATOL, record=None):
    for name, t in (("full", full), ("sparse", sparse)):
        s = summarize(t)
        assert list(GOLDEN["pd128/%s/shape" % name]) == s["shape"]
        err = float(np.abs(s["sub"] - GOLDEN["pd128/%s/sub" % name]).max())
        if record is not None:
            record("pd128/%s" % name, err, atol)
        assert err <= atol, "pd128/%s: max |diff| %.3e > %.1e" % (name, err, atol)
        n = float(np.prod(s["shape"]))
        assert abs(s["sum"] - GOLDEN["pd128/%s/sums" % name][0]) <= atol * n * 0.05  # (errors are signed: the sum moves far less)
        assert abs(s["abs_sum"] - GOLDEN["pd128/%s/sums" % name][1]) <= atol * n * 0.05


def _on_oracle(cfg, steps):
    from oracle import oracle
    from sige_amd import runtime

    torch.set_num_threads(8)
    runtime.register_backend("cpu", oracle)
    try:
        return run_pd(cfg, "cpu", False, steps)
    finally:
        runtime.unregister_backend("cpu")


def test_small_configuration_on_the_oracle_backend_matches_the_reference_fixture():
    """Two cached steps (cache_id 0 / 1): every block in the reference's expression order, border tiles with zero padding."""
    _, outs, counts, ratio = _on_oracle(pd_inputs.SMALL, 2)
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    assert float((outs[0][1] - outs[1][1]).abs().max()) > 1e-2  # (the two steps differ: each read its own cache)
    check_small(outs)


def test_pd128_on_the_oracle_backend_matches_the_reference_fixture():
    _, outs, counts, ratio = _on_oracle(pd_inputs.PD128, 1)
    assert abs(ratio - float(GOLDEN["pd128/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["pd128/tiles"])
    check_pd128(*outs[0])


@pytest.mark.parametrize("group,cfg", [("small", pd_inputs.SMALL), ("pd128", pd_inputs.PD128)])
def test_state_dict_has_the_reference_key_set(group, cfg):
    """A reference checkpoint loads as it stands: the reference's keys, and a strict load of a dict that has exactly them."""
    from sige_amd.workloads.pd_unet import PDSparseUNet

    with torch.device("meta"):  # (names and shapes only: the real configuration has 139.6 M parameters)
        keys = sorted(PDSparseUNet(pd_config(cfg)).state_dict().keys())
    assert keys == list(GOLDEN[group + "/keys"])
    if group == "small":
        model, other = PDSparseUNet(pd_config(cfg)), PDSparseUNet(pd_config(cfg))
        init_by_name(other, seed=1)
        ckpt = {k: other.state_dict()[k].clone() for k in GOLDEN[group + "/keys"]}
        model.load_state_dict(ckpt, strict=True)
        assert all(torch.equal(model.state_dict()[k], v) for k, v in ckpt.items())


def test_pd_configs():
    from sige_amd.workloads.pd_unet import PDConfig

    c = PDConfig()
    assert {k: getattr(c, k) for k in pd_inputs.PD128} == pd_inputs.PD128 and (c.main_block, c.shortcut_block) == (6, 4)
    c = PDConfig.pd256()
    assert (c.image_size, c.ch, c.ch_mult, c.temb_ch) == (256, 128, (1, 1, 2, 2, 4, 4), 1024)


# ---- sige_hip_resample_tiles_nhwc_f32: argument checks, no device -------------------------------------------------------------------
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def entry():
    from sige_amd import build, hip

    build.build(verbose=False)
    fn = ctypes.CDLL(hip.LIB_PATH).sige_hip_resample_tiles_nhwc_f32  # (the raw ctypes function: no device guard)
    fn.restype, fn.argtypes = hip._SIGNATURES["sige_hip_resample_tiles_nhwc_f32"]
    return fn


def _call(fn, x=0x1000, B=1, C=8, H=16, W=16, mode=0, idx=0x2000, N=3, bH=6, bW=6, scale=0x3000, shift=0x4000, tiles=0x5000,
          off=(1, 1), stride=(1, 1), cells=(4, 4), res=0x6000):
    """Fake, 16-byte aligned addresses: every call below must return before a launch."""
    p = lambda v: None if not v else v  # noqa: E731
    return fn(p(x), B, C, H, W, mode, p(idx), N, bH, bW, p(scale), p(shift), p(tiles), off[0], off[1], stride[0], stride[1],
              cells[0], cells[1], p(res), None)


def test_resample_tiles_rejects_bad_arguments_before_touching_the_device(entry):
    # non-positive dims, null pointers with work to do
    for kw in (dict(C=0), dict(H=0), dict(W=-2), dict(B=-1), dict(N=-1), dict(bH=0), dict(bW=-1), dict(cells=(0, 4)),
               dict(stride=(0, 1)), dict(x=0), dict(idx=0, tiles=0, N=3)):
        assert _call(entry, **kw) == EINVAL, kw
    # shapes and forms that are not built
    for kw in (dict(C=6), dict(H=15), dict(W=17), dict(mode=2), dict(mode=1), dict(idx=0, N=0), dict(scale=0), dict(shift=0),
               dict(stride=(2, 2)), dict(x=0x1004), dict(tiles=0x5008), dict(res=0x6004), dict(scale=0x3004), dict(N=70000)):
        assert _call(entry, **kw) == EUNSUPPORTED, kw
    # odd sizes are fine in UP mode (no tiles there); their rejection is a DOWN rule
    assert _call(entry, mode=1, tiles=0, H=15, W=17, N=0) == OK


def test_resample_tiles_with_nothing_to_do_launches_nothing(entry):
    from sige_amd import hip

    before = hip.lib().sige_hip_launch_count()
    assert _call(entry, N=0) == OK
    assert _call(entry, B=0) == OK
    assert _call(entry, N=0, x=0) == OK            # (no work: the pointers are not looked at)
    assert _call(entry, tiles=0, res=0) == OK
    assert hip.lib().sige_hip_launch_count() == before
    assert hip.lib().sige_hip_version() == 310     # an addition, not a break
