"""The SD VAE encoder workload (sige_amd/workloads/sd_vae.py, SparseVAEEncoder) on the CPU with the oracle as native backend,
against tests/golden/sd_vae_encoder.npz -- the outputs of the REAL reference's SIGEEncoder and of a plain quant_conv behind it
(tests/golden/make_vae_encoder_golden.py) --, the derived conv_out / quant_conv fold, and the posterior of encode()."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden import vae_encoder_inputs as enc_inputs  # noqa: E402
from tests.golden.model_init import init_by_name, summarize  # noqa: E402

pytestmark = pytest.mark.oracle_parity  # (pinned to tests/golden/sd_vae_encoder.npz = the real reference's outputs)
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "sd_vae_encoder.npz"))
ATOL = 1e-3  # tests/util.py CONV_ATOL: activations within 1e-3 fp32 on conv-containing paths
SMALL_IMAGE = 64
KINDS = ("full", "sparse", "full_moments", "sparse_moments")


def encoder_config(cfg: dict):
    from sige_amd.workloads.sd_vae import VAEEncoderConfig

    return VAEEncoderConfig(**cfg)


def build_model(cfg: dict, device: str, channels_last: bool, inplace: bool = False):
    """(encoder, quant_conv), weights by name as the generator's."""
    from sige_amd.workloads.sd_vae import SparseVAEEncoder

    model = SparseVAEEncoder(encoder_config(cfg)).eval()
    init_by_name(model)
    model = model.to(device)
    quant = enc_inputs.quant_conv(cfg).to(device)
    if channels_last:
        model, quant = model.to(memory_format=torch.channels_last), quant.to(memory_format=torch.channels_last)
    model.set_scatter_inplace(inplace)
    return model, quant


def make_masks(cfg: dict, image: int, device: str, second: bool = False):
    from sige_amd.utils import dilate_mask, downsample_mask

    mask = enc_inputs.edit_mask(image, second).to(device)
    return mask, enc_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)


def inputs(cfg: dict, image: int, step: int, mask, device: str, channels_last: bool):
    x0, noise = enc_inputs.images(cfg, image, step)
    x0, noise = x0.to(device), noise.to(device)
    x1 = enc_inputs.edited(x0, noise, mask)
    if channels_last:
        x0, x1 = x0.contiguous(memory_format=torch.channels_last), x1.contiguous(memory_format=torch.channels_last)
    return x0, x1


def run_encoder(cfg: dict, image: int, device: str, channels_last: bool, steps: int, inplace: bool = False, prepare=None):
    """[{full, sparse, full_moments, sparse_moments} per step] of SparseVAEEncoder on the fixture's inputs, as the generator ran
    the reference: the outputs through forward(), the moments through moments() -- a forward of its own, quant_conv folded into the
    head on the fused path.  `prepare(model)` runs in front of every sparse forward."""
    from sige_amd.utils import reduce_mask

    model, quant = build_model(cfg, device, channels_last, inplace)
    mask, masks = make_masks(cfg, image, device)
    outs = []
    with torch.no_grad():
        for step in range(steps):
            x0, x1 = inputs(cfg, image, step, mask, device, channels_last)
            model.set_cache_id(step)
            model.set_mode("full")
            got = {"full_moments": model.moments(x0, quant).clone(), "full": model(x0).clone()}
            model.set_masks(masks)
            model.set_mode("sparse")
            for name, fn in (("sparse", model), ("sparse_moments", lambda x: model.moments(x, quant))):
                if prepare is not None:
                    prepare(model)
                got[name] = fn(x1).clone()
            outs.append(got)
    counts = enc_inputs.tile_counts({k: v.cpu() for k, v in masks.items()}, reduce_mask)
    return model, quant, outs, counts, float(mask.float().mean())


def check_small(outs, atol=ATOL, record=None):
    for step, got in enumerate(outs):
        for name in KINDS:
            want = GOLDEN["small/%s%d" % (name, step)]
            assert tuple(got[name].shape) == want.shape
            err = float(np.abs(got[name].float().cpu().numpy() - want).max())
            if record is not None:
                record("small/%s%d" % (name, step), err, atol)
            assert err <= atol, "small/%s%d: max |diff| %.3e > %.1e" % (name, step, err, atol)


def check_sd(got, atol=ATOL, record=None):
    for name in KINDS:
        s = summarize(got[name], step=1)
        assert list(GOLDEN["sd/%s/shape" % name]) == s["shape"]
        err = float(np.abs(s["sub"] - GOLDEN["sd/%s/sub" % name]).max())
        if record is not None:
            record("sd/%s" % name, err, atol)
        assert err <= atol, "sd/%s: max |diff| %.3e > %.1e" % (name, err, atol)
        n = float(np.prod(s["shape"]))
        assert abs(s["sum"] - GOLDEN["sd/%s/sums" % name][0]) <= atol * n * 0.05  # (errors are signed: the sum moves far less)
        assert abs(s["abs_sum"] - GOLDEN["sd/%s/sums" % name][1]) <= atol * n * 0.05


def on_oracle(fn):
    from oracle import oracle
    from sige_amd import runtime

    torch.set_num_threads(8)
    runtime.register_backend("cpu", oracle)
    try:
        return fn()
    finally:
        runtime.unregister_backend("cpu")


def test_small_configuration_on_the_oracle_backend_matches_the_reference_fixture():
    """Two cached images (cache_id 0 / 1): every block in the reference's expression order, border tiles with zero padding, the two
    tiled Downsamples, the 192-channel attention block on the bmm chain; outputs and moments; the tile counts."""
    _, _, outs, counts, ratio = on_oracle(lambda: run_encoder(enc_inputs.SMALL, SMALL_IMAGE, "cpu", False, 2))
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    assert int(counts[-1][3]) > 0 and int(counts[0][2]) > 0
    assert float((outs[0]["sparse"] - outs[1]["sparse"]).abs().max()) > 1e-2  # (the two steps differ: each read its own cache)
    assert float((outs[0]["sparse"] - outs[0]["full"]).abs().max()) > 1e-2     # (and the edit shows in the latent)
    check_small(outs)


@pytest.mark.parametrize("group,cfg", [("small", enc_inputs.SMALL), ("sd", enc_inputs.SD)])
def test_state_dict_has_the_reference_key_set(group, cfg):
    """A reference checkpoint's first_stage_model.encoder.* loads as it stands: the reference's keys, and a strict load of a dict
    that has exactly them."""
    from sige_amd.workloads.sd_vae import SparseVAEEncoder

    with torch.device("meta"):  # (names and shapes only: the real configuration has 34.2 M parameters)
        keys = sorted(SparseVAEEncoder(encoder_config(cfg)).state_dict().keys())
    assert keys == list(GOLDEN[group + "/keys"])
    if group == "small":
        model, other = SparseVAEEncoder(encoder_config(cfg)), SparseVAEEncoder(encoder_config(cfg))
        init_by_name(other, seed=1)
        ckpt = {k: other.state_dict()[k].clone() for k in GOLDEN[group + "/keys"]}
        model.load_state_dict(ckpt, strict=True)
        assert all(torch.equal(model.state_dict()[k], v) for k, v in ckpt.items())
        model.folded_head(enc_inputs.quant_conv(cfg))  # (derived weights: the state dict keeps its keys)
        model.mid.attn_1.folded_kv()
        assert sorted(model.state_dict().keys()) == keys


def test_encoder_config_defaults_are_the_reference_ddconfig():
    from sige_amd.workloads.sd_vae import VAEEncoderConfig

    c = VAEEncoderConfig()
    assert {k: getattr(c, k) for k in enc_inputs.SD} == enc_inputs.SD
    assert c.double_z and (c.main_block, c.shortcut_block, c.attn_block) == (6, 4, 4)


def _small_encoder():
    from sige_amd.workloads.sd_vae import SparseVAEEncoder

    model = SparseVAEEncoder(encoder_config(enc_inputs.SMALL)).eval()
    init_by_name(model)
    return model, enc_inputs.quant_conv(enc_inputs.SMALL)


def test_folded_head_equals_the_unfolded_chain_and_follows_its_parameters():
    """W' = Wq Wc, b' = Wq bc + bq: conv3x3 with the folded weights against quant_conv(conv_out(.)) in fp64 -- the fold rounds each
    fp32 weight once (2^-24 relative), so the outputs (O(1) here) agree to a few 1e-7; rebuilt when quant_conv.weight is edited
    in place."""
    from torch.nn import functional as F

    model, quant = _small_encoder()
    C = model.conv_out.in_channels
    x = torch.randn(1, C, 9, 7, generator=torch.Generator().manual_seed(3), dtype=torch.float64)

    def chain():
        m = F.conv2d(x, model.conv_out.weight.double(), model.conv_out.bias.double(), padding=1)
        return F.conv2d(m, quant.weight.double(), quant.bias.double())

    for p in list(model.parameters()) + list(quant.parameters()):
        p.requires_grad_(False)
    w, b = model.folded_head(quant)
    assert model.folded_head(quant)[0] is w
    assert tuple(w.shape) == (8, C, 3, 3) and w.dtype == torch.float32
    want = chain()
    err = float((F.conv2d(x, w.double(), b.double(), padding=1) - want).abs().max())
    assert float(want.abs().max()) > 0.1 and err <= 1e-6, err
    with torch.no_grad():
        quant.weight.mul_(-1.5)
    w2, b2 = model.folded_head(quant)
    assert w2 is not w and float((w2 + 1.5 * w).abs().max()) <= 1e-6
    assert float((F.conv2d(x, w2.double(), b2.double(), padding=1) - chain()).abs().max()) <= 1e-6
    assert sorted(k for k in model.state_dict() if "fold" in k) == []


def test_encode_returns_the_posterior_sample_and_the_mode():
    """encode() = (moments, scale_factor * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise)); noise=None: the mode."""
    model, quant = _small_encoder()
    with torch.no_grad():
        quant.bias[4:].copy_(torch.tensor([-40.0, 30.0, 0.5, -2.0]))  # (logvar planes beyond both clamp bounds)
    x0, _ = enc_inputs.images(enc_inputs.SMALL, SMALL_IMAGE, 0)
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        model.set_mode("full")
        want_m = quant(model(x0))
        m, z = model.encode(x0, quant, noise=noise, scale_factor=0.18215)
        m2, mode = model.encode(x0, quant)
    assert torch.equal(m, want_m) and torch.equal(m2, want_m) and torch.equal(model.moments(x0, quant), want_m)
    mean, logvar = want_m.double()[:, :4], want_m.double()[:, 4:]
    assert float(logvar[:, 0].max()) < -30 and float(logvar[:, 1].min()) > 20
    want_z = 0.18215 * (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise.double())
    assert float(((z.double() - want_z).abs() / (1e-6 + want_z.abs())).max()) <= 1e-5
    assert float((mode.double() - 0.18215 * mean).abs().max()) <= 1e-6
