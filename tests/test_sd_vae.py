"""The SD VAE decoder workload (sige_amd/workloads/sd_vae.py) on the CPU with the oracle as native backend, against
tests/golden/sd_vae_decoder.npz -- the outputs of the REAL reference's SIGEDecoder (tests/golden/make_vae_golden.py) -- and the
argument checks of sige_hip_attention_wide_f32, which are made before anything touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.golden import vae_inputs  # noqa: E402
from tests.golden.model_init import init_by_name, summarize  # noqa: E402

pytestmark = pytest.mark.oracle_parity  # (pinned to tests/golden/sd_vae_decoder.npz = the real reference's outputs)
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "sd_vae_decoder.npz"))
ATOL = 1e-3  # tests/util.py CONV_ATOL: activations within 1e-3 fp32 on conv-containing paths
SD_LATENT = 64


def vae_config(cfg: dict):
    from sige_amd.workloads.sd_vae import VAEDecoderConfig

    return VAEDecoderConfig(**cfg)


def build_model(cfg: dict, device: str, channels_last: bool, inplace: bool = False):
    from sige_amd.workloads.sd_vae import SparseVAEDecoder

    model = SparseVAEDecoder(vae_config(cfg)).eval()
    init_by_name(model)
    model = model.to(device)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    model.set_scatter_inplace(inplace)
    return model


def inputs(cfg: dict, latent: int, step: int, masks, device: str, channels_last: bool):
    z0, noise = vae_inputs.latents(cfg, latent, step)
    z0, noise = z0.to(device), noise.to(device)
    z1 = vae_inputs.edited(z0, noise, masks)
    if channels_last:
        z0, z1 = z0.contiguous(memory_format=torch.channels_last), z1.contiguous(memory_format=torch.channels_last)
    return z0, z1


def make_masks(cfg: dict, latent: int, device: str, second: bool = False):
    from sige_amd.utils import dilate_mask, downsample_mask

    mask = vae_inputs.edit_mask(vae_inputs.image_size(cfg, latent), second).to(device)
    return mask, vae_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)


def run_vae(cfg: dict, latent: int, device: str, channels_last: bool, steps: int, inplace: bool = False, prepare=None):
    """[(full, sparse) per step] of SparseVAEDecoder on the fixture's inputs, as the generator ran the reference.
    `prepare(model)` runs in front of every sparse forward."""
    from sige_amd.utils import reduce_mask

    model = build_model(cfg, device, channels_last, inplace)
    mask, masks = make_masks(cfg, latent, device)
    outs = []
    with torch.no_grad():
        for step in range(steps):
            z0, z1 = inputs(cfg, latent, step, masks, device, channels_last)
            model.set_cache_id(step)
            model.set_mode("full")
            full = model(z0).clone()
            model.set_masks(masks)
            model.set_mode("sparse")
            if prepare is not None:
                prepare(model)
            outs.append((full, model(z1).clone()))
    counts = vae_inputs.tile_counts({k: v.cpu() for k, v in masks.items()}, reduce_mask)
    return model, outs, counts, float(mask.float().mean())


def check_small(outs, atol=ATOL, record=None):
    for step, (full, sparse) in enumerate(outs):
        for name, t in (("full", full), ("sparse", sparse)):
            want = GOLDEN["small/%s%d" % (name, step)]
            err = float(np.abs(t.float().cpu().numpy() - want).max())
            if record is not None:
                record("small/%s%d" % (name, step), err, atol)
            assert err <= atol, "small/%s%d: max |diff| %.3e > %.1e" % (name, step, err, atol)


def sd_has_outputs() -> bool:
    return "sd/full/sub" in GOLDEN.files


def check_sd(full, sparse, atol=ATOL, record=None):
    for name, t in (("full", full), ("sparse", sparse)):
        s = summarize(t)
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
    """Two cached latents (cache_id 0 / 1): every block in the reference's expression order, border tiles with zero padding, the
    192-channel attention block on the bmm chain."""
    _, outs, counts, ratio = on_oracle(lambda: run_vae(vae_inputs.SMALL, 16, "cpu", False, 2))
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    assert int(counts[-1][3]) > 0 and int(counts[0][2]) > 0
    assert float((outs[0][1] - outs[1][1]).abs().max()) > 1e-2  # (the two steps differ: each read its own cache)
    check_small(outs)


def test_the_fixture_edit_touches_a_border_tile():
    from sige_amd.utils import reduce_mask

    _, masks = make_masks(vae_inputs.SMALL, 16, "cpu")
    for res, m in masks.items():
        idx = reduce_mask(m, 6, 4, 1)
        assert int(idx.min()) < 0, res  # (a 6x6 window that starts in the zero padding)


@pytest.mark.parametrize("group,cfg", [("small", vae_inputs.SMALL), ("sd", vae_inputs.SD)])
def test_state_dict_has_the_reference_key_set(group, cfg):
    """A reference checkpoint's first_stage_model.decoder.* loads as it stands: the reference's keys, and a strict load of a dict
    that has exactly them."""
    from sige_amd.workloads.sd_vae import SparseVAEDecoder

    with torch.device("meta"):  # (names and shapes only: the real configuration has 49.5 M parameters)
        keys = sorted(SparseVAEDecoder(vae_config(cfg)).state_dict().keys())
    assert keys == list(GOLDEN[group + "/keys"])
    if group == "small":
        model, other = SparseVAEDecoder(vae_config(cfg)), SparseVAEDecoder(vae_config(cfg))
        init_by_name(other, seed=1)
        ckpt = {k: other.state_dict()[k].clone() for k in GOLDEN[group + "/keys"]}
        model.load_state_dict(ckpt, strict=True)
        assert all(torch.equal(model.state_dict()[k], v) for k, v in ckpt.items())
        model.mid.attn_1.folded_kv()  # (a derived conv: the state dict keeps its keys)
        assert sorted(model.state_dict().keys()) == keys


def test_vae_config_defaults_are_the_reference_ddconfig():
    from sige_amd.workloads.sd_vae import VAEDecoderConfig

    c = VAEDecoderConfig()
    assert {k: getattr(c, k) for k in vae_inputs.SD} == vae_inputs.SD
    assert (c.main_block, c.shortcut_block, c.attn_block) == (6, 4, 4)


def test_folded_kv_follows_its_parameters():
    """The derived C -> 2C conv is rebuilt when k / v change (the rebuild key of ddpm_unet.AttnBlock.folded_qv)."""
    from sige_amd.workloads.sd_vae import SparseVAEDecoder

    attn = SparseVAEDecoder(vae_config(vae_inputs.SMALL)).mid.attn_1
    init_by_name(attn)
    conv = attn.folded_kv()
    assert attn.folded_kv() is conv
    assert torch.equal(conv.weight, torch.cat([attn.k.weight, attn.v.weight])) and torch.equal(conv.bias, torch.cat([attn.k.bias, attn.v.bias]))
    with torch.no_grad():
        attn.v.weight.mul_(2.0)
    again = attn.folded_kv()
    assert again is not conv and torch.equal(again.weight[attn.ch:], attn.v.weight)


# ---- sige_hip_attention_wide_f32: argument checks, no device ----------------------------------------------------------------------
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def entry():
    from sige_amd import build, hip

    build.build(verbose=False)
    fn = ctypes.CDLL(hip.LIB_PATH).sige_hip_attention_wide_f32  # (the raw ctypes function: no device guard)
    fn.restype, fn.argtypes = hip._SIGNATURES["sige_hip_attention_wide_f32"]
    return fn


def _call(fn, q=0x1000, k=0x2000, v=0x3000, out=0x4000, B=1, Nq=32, Nk=100, C=512, heads=1, ld=None, scale=0.1):
    """Fake, 16-byte aligned addresses: every call below must return before a launch.  `ld`: (ldq, ldk, ldv, ldo), default C."""
    p = lambda a: None if not a else a  # noqa: E731
    ldq, ldk, ldv, ldo = ld or (C, C, C, C)
    return fn(p(q), ldq, p(k), ldk, p(v), ldv, B, Nq, Nk, C, heads, scale, p(out), ldo, None)


def test_attention_wide_rejects_bad_arguments_before_touching_the_device(entry):
    # non-positive dims, null pointers with work to do
    for kw in (dict(B=-1), dict(Nq=-16), dict(Nk=0), dict(Nk=-3), dict(C=0), dict(heads=0), dict(heads=-1), dict(ld=(256, 512, 512, 512)),
               dict(q=0), dict(k=0), dict(v=0), dict(out=0)):
        assert _call(entry, **kw) == EINVAL, kw
    # shapes and forms that are not built
    for kw in (dict(C=160), dict(C=128), dict(C=528), dict(C=1024), dict(C=200), dict(C=500), dict(C=512, heads=3), dict(C=640, heads=4),
               dict(Nq=24), dict(Nq=8), dict(q=0x1004), dict(k=0x2008), dict(v=0x3004), dict(out=0x4008),
               dict(ld=(514, 512, 512, 512)), dict(ld=(512, 1026, 1024, 512)), dict(ld=(512, 1024, 1025, 512)), dict(ld=(512, 512, 512, 513))):
        assert _call(entry, **kw) == EUNSUPPORTED, kw


def test_attention_wide_supported_shapes():
    from sige_amd import build, hip

    build.build(verbose=False)
    fn = ctypes.CDLL(hip.LIB_PATH).sige_hip_attention_wide_supported
    fn.restype, fn.argtypes = hip._SIGNATURES["sige_hip_attention_wide_supported"]
    assert [fn(16, 5, c, 1) for c in (160, 176, 192, 256, 512, 528, 200)] == [0, 1, 1, 1, 1, 0, 0]
    assert fn(64, 64, 512, 2) == 1 and fn(64, 64, 512, 4) == 0  # (d = 256; d = 128 is attention_tokens')
    assert fn(24, 64, 512, 1) == 0 and fn(0, 64, 512, 1) == 0
    tok = ctypes.CDLL(hip.LIB_PATH).sige_hip_attention_tokens_supported
    tok.restype, tok.argtypes = hip._SIGNATURES["sige_hip_attention_tokens_supported"]
    assert tok(16, 64, 160, 1) == 1 and tok(16, 64, 176, 1) == 0  # (the existing entry keeps its range)


def test_attention_wide_with_nothing_to_do_launches_nothing(entry):
    from sige_amd import hip

    before = hip.lib().sige_hip_launch_count()
    assert _call(entry, B=0) == OK
    assert _call(entry, Nq=0) == OK
    assert _call(entry, B=0, q=0, k=0, v=0, out=0) == OK  # (no work: the pointers are not looked at)
    assert hip.lib().sige_hip_launch_count() == before
    assert hip.lib().sige_hip_version() == 310            # an addition, not a break
