"""Shared by the tests of the first conv (csrc/conv_in.hip) at batch > 1 and many workgroups: the cases of
tests/test_gpu_conv_in_batch.py, their seeded CPU inputs, the fp64 reference and the checker.  Nothing here touches a device
(tests/test_conv_in_batch_inputs.py runs it without one).

Two findings of wrong pixels in this kernel were never explained (one launch at batch 8, 3 -> 64 channels, 128 x 128,
wrong in some images; 5.27: the 32- / 64-channel forms with write-through stores at 1 x 3 x 256 x 256).  Both were errors as large as
the values, in a few dwords of some 32-pixel blocks, in some launches.  So every case is several hundred workgroups at batch > 1, the
bound is the 1e-5 of every other test of this kernel, and the checker names the images that hold a bad element."""
import torch

from tests.block10_common import tile_lists

BOUND = 1e-5      # |got - fp64 conv|: tests/test_gpu_channels_last.py, test_gpu_conv_in_full_size.py, test_gpu_data_movement_ragged.py
SEPARATION = 1e-2  # two images of one case differ by more than this at more than 99 % of the output elements

# name -> B, Cin, H, W, Cout, input layout.  Workgroups = ceil(B H W / 128): one 32-pixel block per wave, four waves.
#   nhwc     channels-last
#   nchw     NCHW-contiguous
#   strided  big[::2] of a channels-last [2B, Cin, H, W] tensor: batch stride 2 Cin H W (also run without a bias)
WHOLE = {
    "b8-c3-128x128-64": (8, 3, 128, 128, 64, "nhwc"),      # the launch of DESIGN.md 5.25: 1024 workgroups
    "b8-c3-128x128-32": (8, 3, 128, 128, 32, "nhwc"),      # the other narrow form on the same grid
    "b4-c3-256x256-128": (4, 3, 256, 256, 128, "nhwc"),    # DDPM stacked at E = 4: the write-through form at 2048 workgroups
    "b8-c3-128x128-128": (8, 3, 128, 128, 128, "nhwc"),    # the write-through form at batch 8
    "b5-c2-67x93-64": (5, 2, 67, 93, 64, "nhwc"),          # 6231 pixels per image: no multiple of 32 or 128, images meet inside blocks
    "b3-c1-131x70-32": (3, 1, 131, 70, 32, "nhwc"),        # K = 9 is odd: the padded k column of the weight stage is live
    "b3-c3-67x93-128": (3, 3, 67, 93, 128, "nchw"),
    "b4-c3-64x64-64-strided": (4, 3, 64, 64, 64, "strided"),
}
# name -> B, H, W, Cout: every 6x6 window at stride 4 from origin -1 on (the last row and column are clipped at the far borders),
# evaluated in place in a buffer that starts as random data.  Workgroups = ceil(B N 36 / 128).
TILES = {
    "tiles-b3-128x128-64": (3, 128, 128, 64),
    "tiles-b3-128x128-32": (3, 128, 128, 32),
    "tiles-b2-256x256-128": (2, 256, 256, 128),
}
BLOCK = 6


def workgroups(name):
    if name in WHOLE:
        B, _, H, W, _, _ = WHOLE[name]
        return -(-B * H * W // 128)
    B, H, W, _ = TILES[name]
    return -(-B * window_list(H, W).shape[0] * BLOCK * BLOCK // 128)


def window_list(H, W):
    """[N,2] int32: the origins 4i - 1 of all 6x6 windows that cover an H x W image (H, W multiples of 4)."""
    return tile_lists(H // 4, W // 4, 4, 1)["every"]


def window_mask(idx, res):
    """[H, W] bool: the pixels of the 6x6 windows at `idx`, clipped at all four borders."""
    m = torch.zeros(res, dtype=torch.bool)
    for h0, w0 in idx.tolist():
        m[max(h0, 0):h0 + BLOCK, max(w0, 0):w0 + BLOCK] = True
    return m


_LAST = [None, None]  # (one case at a time: the largest reference is 268 MB of fp64)


def case(name):
    """Seeded CPU inputs and the fp64 conv of one case, never written to: x in the case's layout, w, bias, want (and want_nobias for
    the strided case); for a tile-list case also idx, the window mask `inside` and the buffer's start z."""
    if _LAST[0] == name:
        return _LAST[1]
    tiled = name in TILES
    B, C, H, W, cout, layout = (TILES[name][0], 3) + TILES[name][1:] + ("nhwc",) if tiled else WHOLE[name]
    gen = torch.Generator().manual_seed(sorted(list(WHOLE) + list(TILES)).index(name) + 2525)
    if layout == "strided":
        big = torch.randn(2 * B, C, H, W, generator=gen).contiguous(memory_format=torch.channels_last)
        x = big[::2]
        assert x.stride() == (2 * C * H * W, 1, W * C, C)
    else:
        x = torch.randn(B, C, H, W, generator=gen)
        if layout == "nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, C, 3, 3, generator=gen) / (3 * C ** 0.5)
    bias = torch.randn(cout, generator=gen)
    d = dict(name=name, B=B, C=C, H=H, W=W, cout=cout, layout=layout, x=x, w=w, bias=bias,
             want=torch.nn.functional.conv2d(x.double(), w.double(), bias.double(), 1, 1))
    if layout == "strided":
        d["want_nobias"] = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    if tiled:
        d["idx"] = window_list(H, W)
        d["inside"] = window_mask(d["idx"], (H, W))
        d["z"] = torch.randn(B, cout, H, W, generator=gen).contiguous(memory_format=torch.channels_last)
    _LAST[:] = [name, d]
    return d


def check(got, want, inside=None):
    """(number of elements with |got - want| > BOUND, the worst difference, the sorted image indices that hold such an element), over
    all of [B, C, H, W] or over the pixels of the [H, W] mask `inside`.  A NaN counts as bad and makes the worst difference NaN."""
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    d = (got.double() - want).abs()
    bad = ~(d <= BOUND)
    if inside is not None:
        bad &= inside.to(bad.device)[None, None]
        d = d[:, :, inside.to(d.device)]
    images = [b for b, hit in enumerate(bad.flatten(1).any(1).tolist()) if hit]
    return int(bad.sum()), float(d.max()), images


def message(name, launch, n_bad, worst, images):
    return "%s, launch %d: %d wrong elements in images %s, worst %.3g (bound %.3g)" % (name, launch, n_bad, images, worst, BOUND)
