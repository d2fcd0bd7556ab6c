"""Inputs of the Progressive Distillation U-Net fixture (tests/golden/pd_unet.npz), shared by its generator (which feeds them
to the REFERENCE's SIGEUNet in the build container) and by the tests (which feed them to sige_amd's PDSparseUNet)."""
import numpy as np
import torch

# image 64, ch 32, mult (1,2,4), 1 res block per level, attention at 16x16 with 32-wide heads, tiles at 64x64 and 32x32:
# every kind of block of the real network (tiled / dense, plain / down / up, with and without a 1x1 shortcut, attention) once
SMALL = dict(image_size=64, ch=32, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=(16,), head_dim=32, num_heads=None,
             in_ch=3, out_ch=6, temb_ch=128, logsnr_input_type="inv_cos", sparse_resolution_threshold=32)
# church_pd128-sige.yml
PD128 = dict(image_size=128, ch=64, ch_mult=(1, 2, 4, 6, 8), num_res_blocks=3, attn_resolutions=(8, 16, 32), head_dim=64,
             num_heads=None, in_ch=3, out_ch=6, temb_ch=768, logsnr_input_type="inv_cos", sparse_resolution_threshold=64)
BLOCKS = dict(normal=6, instance=4)  # sige_block_size
LOGSNR = (2.0, -1.5)                 # one value per cached step


def edit_mask(size: int, second: bool = False) -> torch.Tensor:
    """A ~5 % rectangle one pixel off the top and left borders: dilated by 2 it touches both, so border tiles with zero
    padding occur.  `second`: another ~5 % rectangle, over the bottom-right corner (the second mask set of the GPU tests)."""
    a = int(round(size * 0.22))
    b = int(round(0.05 * size * size / a))
    m = torch.zeros(size, size, dtype=torch.bool)
    if second:
        m[size - a:, size - b:] = True
    else:
        m[1:1 + a, 1:1 + b] = True
    return m


def images(size: int, seed: int = 11):
    """(original, noise) [1,3,size,size]; the edited image is original + noise * mask."""
    rs = np.random.RandomState(seed)
    x0 = torch.from_numpy(rs.standard_normal((1, 3, size, size)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((1, 3, size, size)).astype(np.float32))
    return x0, noise


def pyramid(mask: torch.Tensor, cfg: dict, dilate_mask, downsample_mask):
    """The runner's recipe (diffusion/runner.py:158-164) with the caller's mask helpers (the reference's or sige_amd's)."""
    return downsample_mask(dilate_mask(mask, 2), cfg["image_size"] // 2 ** (len(cfg["ch_mult"]) - 1))


def tile_counts(masks: dict, reduce_mask) -> np.ndarray:
    """[[h, w, active 6x6 tiles (stride 4, offset 1), active 4x4 tiles (stride 4, offset 0)], ...] by falling resolution."""
    rows = []
    for res in sorted(masks, reverse=True):
        m = masks[res]
        rows.append([res[0], res[1], int(reduce_mask(m, 6, 4, 1).shape[0]), int(reduce_mask(m, 4, 4, 0).shape[0])])
    return np.array(rows, dtype=np.int64)
