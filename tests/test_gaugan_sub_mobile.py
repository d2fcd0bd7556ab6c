"""The GAN-Compression GauGAN generator (sige_amd.workloads.gaugan_sub_mobile) on the CPU, pinned to tests/golden/gaugan_sub_mobile.npz
(the REAL reference's SIGEFusedSubMobileSPADEGenerator, produced by tests/golden/make_sub_mobile_golden.py): the workload on the
oracle back end with the same name-keyed weights, the state-dict keys, and the host-side refusals.  Bounds: full 1e-5, sparse 1e-4
-- what test_models_golden.py uses for the other GauGAN generator on the oracle back end."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden import sub_mobile_inputs as inputs  # noqa: E402
from tests.golden.model_init import summarize  # noqa: E402

pytestmark = pytest.mark.oracle_parity
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "gaugan_sub_mobile.npz"))


def stored(group, name, field):
    prefix = "%s/%s" % (group, name)
    if prefix + "/alias" in GOLDEN.files:
        prefix = str(GOLDEN[prefix + "/alias"])
    return GOLDEN["%s/%s" % (prefix, field)]


def check(group, name, t, atol):
    """test_models_golden.py::_check on this fixture's layout."""
    s = summarize(t, step=int(stored(group, name, "step")[0]))
    assert list(stored(group, name, "shape")) == s["shape"]
    err = float(np.abs(s["sub"] - stored(group, name, "sub")).max())
    print("%s/%s: max |got - reference| %.3e (bound %.0e)" % (group, name, err, atol))
    np.testing.assert_allclose(s["sub"], stored(group, name, "sub"), rtol=0, atol=atol)
    n = float(np.prod(s["shape"]))
    assert abs(s["sum"] - stored(group, name, "sums")[0]) <= atol * n * 0.05       # (errors are signed: the sum moves far less)
    assert abs(s["abs_sum"] - stored(group, name, "sums")[1]) <= atol * n * 0.05
    return err


def build_model(group, **cfg_kw):
    from sige_amd.workloads.gaugan_sub_mobile import SubMobileSPADEConfig, SubMobileSpadeGenerator

    config_str, ngf, crop, _, k, _ = inputs.GROUPS[group]
    cfg = SubMobileSPADEConfig(ngf=ngf, crop_size=crop, num_sparse_layers=k, channels=inputs.channels(config_str), **cfg_kw)
    model = SubMobileSpadeGenerator(cfg).eval()
    inputs.init_weights(model)
    return model


def run_model(group, device="cpu", channels_last=False, fused=True, variant=0, model=None):
    """(full on the original, sparse on the edited label map, model) with the gaugan/test.py mask recipe."""
    from sige_amd.utils import compute_difference_mask, dilate_mask, downsample_mask

    if model is None:
        model = build_model(group, fused=fused).to(device)
        if channels_last:
            model = model.to(memory_format=torch.channels_last)
    x0, x1 = (t.to(device) for t in inputs.labels(group, variant))
    if channels_last:
        x0, x1 = x0.contiguous(memory_format=torch.channels_last), x1.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        model.set_mode("full")
        full = model(x0)
        diff = compute_difference_mask(x0, x1)
        model.set_masks(downsample_mask(dilate_mask(diff, 1), (model.sh, model.sw), dilation=2))
        model.set_mode("sparse")
        sparse = model(x1)
    if variant == 0:
        assert abs(float(diff.float().mean()) - float(GOLDEN[group + "/edit_ratio"][0])) < 1e-9
    return full, sparse, model


@pytest.mark.parametrize("group", list(inputs.GROUPS))
def test_fixture_is_not_saturated(group):
    """A condition on the FIXTURE (checked on the reference when it was made): a tanh output of +-1 pins nothing."""
    for name in ("full", "sparse"):
        sub = stored(group, name, "sub")
        assert float((np.abs(sub) > 0.99).mean()) <= 0.01
        assert float(sub.std()) >= 0.1


@pytest.mark.parametrize("group", list(inputs.GROUPS))
def test_state_dict_keys_are_the_references(group):
    model = build_model(group)
    keys = sorted(model.state_dict().keys())
    assert len(keys) == 248
    assert keys == [str(k) for k in GOLDEN[group + "/keys"]]
    assert "up_1.norm_s.mlp_gamma.conv.0.weight" in keys and "up_1.norm_s.mlp_beta.conv.2.bias" in keys
    assert "head_0.norm_0.param_free_norm.running_mean" in keys and "up_0.conv_s.weight" in keys
    twin = build_model(group)
    twin.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)


@pytest.mark.parametrize("group", list(inputs.GROUPS))
def test_workload_on_the_oracle_backend_matches_the_reference_fixture(group):
    from oracle import oracle
    from sige_amd import runtime

    torch.set_num_threads(8)
    runtime.register_backend("cpu", oracle)
    try:
        full, sparse, _ = run_model(group, "cpu", False, False)
    finally:
        runtime.unregister_backend("cpu")
    check(group, "full", full, 1e-5)
    check(group, "sparse", sparse, 1e-4)


def test_default_config_is_the_readme_configuration():
    from sige_amd.workloads.gaugan_sub_mobile import SubMobileSPADEConfig

    cfg = SubMobileSPADEConfig()
    assert cfg.channels == (32, 32, 32, 48, 32, 24, 24, 32) and cfg.num_sparse_layers == 4 and cfg.ngf == 64
    assert SubMobileSPADEConfig.decode("8_8_8_12_8_8_8_8", ngf=16).channels == (8, 8, 8, 12, 8, 8, 8, 8)
    model = build_model("readme")
    widths_in = [getattr(model, b).conv_0.in_channels for b in ("head_0", "G_middle_0", "G_middle_1", "up_0", "up_1", "up_2", "up_3")]
    widths_out = [getattr(model, b).conv_1.out_channels for b in ("head_0", "G_middle_0", "G_middle_1", "up_0", "up_1", "up_2", "up_3")]
    hidden = [getattr(model, b).nhidden for b in ("head_0", "G_middle_0", "G_middle_1", "up_0", "up_1", "up_2", "up_3")]
    assert widths_in == [512, 512, 512, 512, 256, 96, 48]
    assert widths_out == [512, 512, 512, 256, 96, 48, 32]
    assert hidden == [64, 64, 96, 64, 48, 48, 64]


def test_batch_of_two_raises():
    model = build_model("small5")
    x0, _ = inputs.labels("small5")
    with torch.no_grad(), pytest.raises(RuntimeError, match="batch"):
        model(torch.cat([x0, x0]))


def test_stacked_edits_are_refused_off_the_gpu():
    model = build_model("small5")
    x0, _ = inputs.labels("small5")
    model.edit_batch = 2
    with torch.no_grad(), pytest.raises(RuntimeError, match="stacked"):
        model(torch.cat([x0, x0]))
