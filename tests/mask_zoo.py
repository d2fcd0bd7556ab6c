"""The masks the model-level GPU tests of tests/test_gpu_masks.py run the DDPM-256 forward under: everything an interior square
is not.  A real brush edit that touches two borders, a frame along all four, isolated pixels the pyramid's 0.3 threshold drops at
the coarse levels, tile rows / columns that alternate between active and cached over the whole image, the smallest tile counts
there are (one pixel in the last corner), a diagonal, and every tile of every level.

Built from seeds and index arithmetic only (`assets_mask` is the reference's own brush mask, already a fixture of
tests/golden/masks.npz).  tests/test_mask_zoo.py (CPU) pins the tile counts below and the conditioning of every mask ON THE
REFERENCE ALONE, so the set cannot drift and a failing GPU comparison is a statement about the kernels, not about the input.

Deliberately absent: the all-True mask.  On the CPU oracle alone its output moves by 3.5e-4 when every conv's input and output is
jittered by one fp32 rounding (the masks here: 5e-7 to 7e-6), and fp16 operand rounding alone takes it to 0.99 of the f16
criterion (here: at most 0.18).  `full_grid` gives the same tile lists on a well-conditioned input."""
from collections import OrderedDict

import torch

from tests import util

RES = 256
LEVELS = (256, 128, 64, 32, 16, 8)

# tiles per pyramid level (256 .. 8) of downsample_mask(dilate_mask(mask, 5), 8): oracle.reduce_mask(level, 6, 4, 1) -- the 3x3
# convs' 6x6 blocks -- and oracle.reduce_mask(level, 4, 4, 0), the shortcuts' 4x4 blocks
COUNTS = {
    "assets_mask": ((964, 288, 102, 40, 16, 6), (869, 248, 74, 23, 10, 4)),
    "frame": ((861, 305, 93, 45, 21, 9), (732, 240, 60, 28, 12, 4)),
    "specks": ((602, 316, 131, 4, 4, 4), (432, 206, 82, 2, 2, 1)),
    "stripes": ((2080, 1023, 272, 72, 25, 9), (2048, 512, 256, 64, 16, 4)),
    "columns": ((1040, 528, 136, 72, 20, 9), (1024, 256, 128, 32, 16, 4)),
    "corners": ((21, 21, 9, 9, 9, 9), (12, 4, 4, 4, 4, 4)),
    "last_pixel": ((8, 8, 4, 4, 4, 4), (3, 1, 1, 1, 1, 1)),
    "diagonal": ((443, 159, 49, 25, 13, 7), (314, 94, 46, 22, 10, 4)),
    "full_grid": ((4225, 1089, 289, 81, 25, 9), (4096, 1024, 256, 64, 16, 4)),
}

# one model through the whole set: large and small footprints in turn; the first step is the shrink from 4225 tiles to 8
SEQUENCE = ("full_grid", "last_pixel", "stripes", "specks", "assets_mask", "corners", "columns", "frame", "diagonal")
# the images of one stacked forward, top to bottom: masks with active last rows directly above masks with active first rows
STACK = ("frame", "assets_mask", "stripes", "corners", "full_grid", "last_pixel", "columns", "specks")
SEAMS_ACTIVE_ON_BOTH_SIDES = (("frame", "assets_mask"), ("corners", "full_grid"), ("last_pixel", "columns"))

_zoo = None


def _blank():
    return torch.zeros(RES, RES, dtype=torch.bool)


def zoo():
    """name -> [256,256] bool CPU tensor, in the order of COUNTS (a fresh dict of the same tensors on every call)."""
    global _zoo
    if _zoo is None:
        out = OrderedDict()
        g = util.golden("masks")
        out["assets_mask"] = util.unpack(g["assets_mask/mask"], g["assets_mask/shape"])
        m = _blank()
        m[:3] = m[-3:] = True
        m[:, :3] = m[:, -3:] = True
        out["frame"] = m
        m = torch.zeros(RES * RES, dtype=torch.bool)
        m[torch.randperm(RES * RES, generator=torch.Generator().manual_seed(7))[:48]] = True
        out["specks"] = m.view(RES, RES)
        m = _blank()
        m[8::32] = True
        out["stripes"] = m
        m = _blank()
        m[:, 16::64] = True
        out["columns"] = m
        m = _blank()
        m[0, 0] = m[0, RES - 1] = m[RES - 1, 0] = m[RES - 1, RES - 1] = True
        out["corners"] = m
        m = _blank()
        m[RES - 1, RES - 1] = True
        out["last_pixel"] = m
        yy, xx = torch.meshgrid(torch.arange(RES), torch.arange(RES), indexing="ij")
        out["diagonal"] = (yy - xx).abs() < 2
        m = _blank()
        m[2::4, 2::4] = True  # (6.25 % of the pixels; dilated by 5 it is every pixel: every tile of every level)
        out["full_grid"] = m
        assert list(out) == list(COUNTS) and sorted(SEQUENCE) == sorted(COUNTS)
        _zoo = out
    return OrderedDict(_zoo)
