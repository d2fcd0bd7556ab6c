"""Shared by tests/test_change_regions.py (CPU) and tests/test_gpu_dense_change_regions.py: the brute-force pixel walk of the change
regions, the smallest network with a dense down level behind a tiled Downsample, and its masks."""
import torch


def brute(idx, stride, offset, wrote, res, tile, pad, depth):
    """Pixel by pixel: (S_1 .. S_depth as sets of (y, x), main lists, flat lists).  S_0 = the `wrote` x `wrote` output pixels at
    (index + offset) / stride of every listed tile, inside the `res` image; S_k = S_(k-1) grown by one pixel, clamped."""
    hp, wp = res
    cur = set()
    for y0, x0 in idx.tolist():
        for dy in range(wrote):
            for dx in range(wrote):
                y, x = (y0 + offset) // stride + dy, (x0 + offset) // stride + dx
                if 0 <= y < hp and 0 <= x < wp:
                    cur.add((y, x))
    sets, mains, flats = [], [], []
    for _ in range(depth):
        grown = set()
        for y, x in cur:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < hp and 0 <= x + dx < wp:
                        grown.add((y + dy, x + dx))
        cur = grown
        sets.append(set(cur))
        cells = sorted({(y // tile, x // tile) for y, x in cur})
        flats.append(torch.tensor([(cy * tile, cx * tile) for cy, cx in cells], dtype=torch.int32).reshape(-1, 2))
        mains.append(torch.tensor([(cy * tile - pad, cx * tile - pad) for cy, cx in cells], dtype=torch.int32).reshape(-1, 2))
    return sets, mains, flats


def same(got, want):
    return len(got) == len(want) and all(g.dtype == torch.int32 and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


def downsample_indices(mask, res=64):
    """The index list of a tiled Downsample's gather (3x3 stride 2: 5x5 blocks, block stride 4, offset 0) over the `res` level of
    bench.py's mask recipe."""
    from oracle import oracle

    pyramid = oracle.downsample_mask(oracle.dilate_mask(mask, 5), 8)
    return oracle.reduce_mask(pyramid[(res, res)], (5, 5), (4, 4), (0, 0))


def small_cfg():
    from sige_amd.workloads.ddpm_unet import DDPMConfig

    # levels 64 / 32 (tiled) and 16 (dense: 16 cells; one paired block 128 -> 256 with its 1x1 shortcut, one unpaired block)
    return DDPMConfig(ch=128, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(), resolution=64, sparse_threshold=32)


def small_masks():
    interior = torch.zeros(64, 64, dtype=torch.bool)
    interior[29:33, 30:35] = True
    corner = torch.zeros(64, 64, dtype=torch.bool)
    corner[:3, :4] = True
    large = torch.zeros(64, 64, dtype=torch.bool)
    large[3:61, 2:62] = True
    return {"interior": interior, "corner": corner, "large": large}


def small_inputs():
    gen = torch.Generator().manual_seed(3)
    return torch.randn(1, 3, 64, 64, generator=gen), torch.randn(1, 3, 64, 64, generator=gen)
