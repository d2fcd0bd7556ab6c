"""Inputs of the SD VAE encoder fixture (tests/golden/sd_vae_encoder.npz), shared by its generator (which feeds them to the
REFERENCE's SIGEEncoder in the build container) and by the tests (which feed them to sige_amd's SparseVAEEncoder)."""
import numpy as np
import torch

from . import vae_inputs

# vae_inputs.SMALL with the encoder's double_z: image 64 (latent 16), ch 32, mult (1,2,6), 1 res block per level -- the middle block
# is 192 channels wide: its attention is above the 160 channels of hip.attention_tokens, and the latent head runs at C = 192 (a
# multiple of 64 that is no power of two); every kind of block of the real encoder once (tiled residual blocks with and without
# a 1x1 shortcut, two tiled Downsamples, the tiled attention block)
SMALL = dict(vae_inputs.SMALL, double_z=True)
# configs/sige.yaml, first_stage_config.params.ddconfig
SD = dict(vae_inputs.SD, double_z=True)
SD_IMAGE = 128  # the real configuration's recorded step: image 128 x 128, latent 16 x 16

edit_mask = vae_inputs.edit_mask
tile_counts = vae_inputs.tile_counts


def pyramid(mask: torch.Tensor, cfg: dict, dilate_mask, downsample_mask):
    """vae_inputs.pyramid: the edit mask at image size, dilated by 2, downsampled to every level down to the latent's."""
    return vae_inputs.pyramid(mask, cfg, dilate_mask, downsample_mask)


def images(cfg: dict, image: int, step: int, seed: int = 23):
    """(original, noise) [1,3,image,image] of cached step `step`; the edited image is original + noise * mask at image size."""
    rs = np.random.RandomState(seed + 101 * step)
    shape = (1, cfg["in_channels"], image, image)
    x0 = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    return x0, noise


def edited(x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """`mask` [image,image] bool: the UNDILATED edit (the masks a model sees are its dilation)."""
    return x0 + noise * mask.to(x0.device).to(x0.dtype)


def quant_conv(cfg: dict) -> torch.nn.Conv2d:
    """The autoencoder's quant_conv (ldm/models/autoencoder.py: Conv2d(2 z, 2 embed_dim, 1) with embed_dim = z), initialised by
    name as every other layer of the fixture."""
    from .model_init import init_by_name

    holder = torch.nn.Module()
    holder.quant_conv = torch.nn.Conv2d(2 * cfg["z_channels"], 2 * cfg["z_channels"], 1)
    init_by_name(holder)
    return holder.quant_conv
