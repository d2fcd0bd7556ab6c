"""Inputs of the SD VAE decoder fixture (tests/golden/sd_vae_decoder.npz), shared by its generator (which feeds them to the
REFERENCE's SIGEDecoder in the build container) and by the tests (which feed them to sige_amd's SparseVAEDecoder)."""
import numpy as np
import torch

from . import pd_inputs

# image 64 (latent 16), ch 32, mult (1,2,6), 1 res block per level: the middle block is 192 channels wide -- its attention
# (256 keys, one 192-wide head) is above the 160 channels of hip.attention_tokens --, every kind of block of the real decoder
# once (tiled residual blocks with and without a 1x1 shortcut, the tiled attention block, two tiled Upsamples)
SMALL = dict(ch=32, out_ch=3, ch_mult=(1, 2, 6), num_res_blocks=1, attn_resolutions=(), in_channels=3, resolution=64,
             z_channels=4)
# configs/sige.yaml, first_stage_config.params.ddconfig (double_z / dropout are the encoder's and the training's)
SD = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), in_channels=3, resolution=256,
          z_channels=4)


def image_size(cfg: dict, latent: int) -> int:
    return latent * 2 ** (len(cfg["ch_mult"]) - 1)


def edit_mask(size: int, second: bool = False) -> torch.Tensor:
    """The ~5 % rectangles of pd_inputs at IMAGE resolution: the first touches the top and left borders once dilated (border tiles
    with zero padding), the second lies over the bottom-right corner."""
    return pd_inputs.edit_mask(size, second)


def square_mask(size: int, ratio: float) -> torch.Tensor:
    """A centred square edit covering `ratio` of the image (tools/vae_bench.py)."""
    a = int(round(size * ratio ** 0.5))
    o = (size - a) // 2
    m = torch.zeros(size, size, dtype=torch.bool)
    m[o:o + a, o:o + a] = True
    return m


def pyramid(mask: torch.Tensor, cfg: dict, dilate_mask, downsample_mask):
    """pd_inputs.pyramid: the edit mask at image size, dilated by 2, downsampled to every level down to the latent's."""
    size = mask.shape[-1]
    return pd_inputs.pyramid(mask, dict(image_size=size, ch_mult=cfg["ch_mult"]), dilate_mask, downsample_mask)


def latents(cfg: dict, latent: int, step: int, seed: int = 17):
    """(original, noise) [1,z,latent,latent] of cached step `step`; the edited latent is original + noise * mask at latent size."""
    rs = np.random.RandomState(seed + 101 * step)
    shape = (1, cfg["z_channels"], latent, latent)
    z0 = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    return z0, noise


def edited(z0: torch.Tensor, noise: torch.Tensor, masks: dict) -> torch.Tensor:
    m = masks[tuple(z0.shape[2:])]
    return z0 + noise * m.to(z0.device)


tile_counts = pd_inputs.tile_counts
