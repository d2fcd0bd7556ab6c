"""Block size 10, host side (no GPU): the sub-tile expansion that lets the kernels of the default geometries serve 8x8 and 9x9
blocks, and what Gather derives from a block size of 10."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import oracle
from tests import mask_zoo
from tests.block10_common import tile_lists as _lists


def test_subtile_indices_layout():
    from sige_amd import hip

    idx = torch.tensor([[-1, -1], [7, 15], [15, -1]], dtype=torch.int32)
    sub = hip.subtile_indices(idx, n=2, step=4)
    assert sub.dtype == torch.int32 and tuple(sub.shape) == (12, 2) and sub.is_contiguous()
    for t in range(3):
        for i in range(2):
            for j in range(2):
                assert sub[4 * t + 2 * i + j].tolist() == [int(idx[t, 0]) + 4 * i, int(idx[t, 1]) + 4 * j]
    assert hip.subtile_indices(idx, n=2, step=4) is sub                # cached on the list ...
    idx[0, 0] = 3                                                     # ... until it is written in place
    assert hip.subtile_indices(idx, n=2, step=4)[0].tolist() == [3, -1]
    assert tuple(hip.subtile_indices(torch.zeros((0, 2), dtype=torch.int32)).shape) == (0, 2)


# (kernel, stride, big block, sub block, offset, input resolution): the output is 20x28 in both, neither a multiple of 8
GEOMETRIES = {
    "k1_8x8_as_4x4": (1, 1, 8, 4, 0, (20, 28)),
    "k3s2_9x9_as_5x5": (3, 2, 9, 5, 1, (40, 56)),
}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("tiles", ["every", "corners", "interior", "holes", "empty"])
def test_subtiles_compute_what_the_big_tile_computes(geo, tiles):
    """gather -> conv -> scatter over the four sub-tiles of every tile, placed at (offset + idx) / stride, is gather -> conv ->
    scatter over the large tiles: brute force with the oracle's gather / scatter and F.conv2d on the CPU."""
    from sige_amd import hip

    k, s, big, small, off, (H, W) = GEOMETRIES[geo]
    idx = _lists(3, 4, 8 * s, off)[tiles]
    gen = torch.Generator().manual_seed(11)
    B, Cin, Cout = 2, 5, 3
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen)
    bias = torch.randn(Cout, generator=gen)
    y = torch.randn(B, Cout, 20, 28, generator=gen)
    sub = hip.subtile_indices(idx, n=2, step=4)
    assert tuple(sub.shape) == (4 * idx.shape[0], 2)

    def run(index, block):
        t = oracle.gather(x, block, block, index)
        o = F.conv2d(t.double(), w.double(), bias.double(), stride=s).float() if t.shape[0] else t.new_zeros((0, Cout, (block - k) // s + 1, (block - k) // s + 1))
        return oracle.scatter(o, y, off, off, s, s, index)

    want, got = run(idx, big), run(sub, small)
    assert torch.allclose(got, want, rtol=0, atol=1e-5), float((got - want).abs().max())
    if idx.shape[0] == 0:
        assert torch.equal(got, y)


def test_gather_derives_the_block10_geometry():
    from sige_amd.nn import Gather

    g = Gather(nn.Conv2d(4, 4, 3, 1, 1), 10)
    assert (g.block_size, g.block_stride, g.offset, g.out_tile) == ((10, 10), (8, 8), (1, 1), (8, 8))
    g1 = Gather(nn.Conv2d(4, 4, 1, 1, 0), 8)
    assert (g1.block_size, g1.block_stride, g1.offset, g1.out_tile) == ((8, 8), (8, 8), (0, 0), (8, 8))
    with pytest.warns(UserWarning, match=r"\(10, 10\) to \(9, 9\)"):
        g2 = Gather(nn.Conv2d(4, 4, 3, 2, 1), 10)
    assert (g2.block_size, g2.block_stride, g2.offset, g2.out_tile) == ((9, 9), (8, 8), (1, 1), (4, 4))
    zoo = mask_zoo.zoo()
    for name in ("assets_mask", "frame", "specks", "corners", "last_pixel", "diagonal"):
        mask = zoo[name]
        for m in (g, g1, g2):
            m.input_res, m.timestamp = tuple(mask.shape), None
            m.set_mask({tuple(mask.shape): mask}, {}, name)
            want = oracle.reduce_mask(mask, m.block_size, m.block_stride, m.offset)
            assert torch.equal(m.active_indices.to(torch.int32), want), (name, m.block_size)


def test_block_geometry_names():
    from sige_amd import hip

    assert hip.block_geometry((10, 10), (3, 3), (1, 1)) == "b10"
    assert hip.block_geometry((8, 8), (1, 1), (1, 1)) == "k1b8"
    assert hip.block_geometry((9, 9), (3, 3), (2, 2)) == "s2b9"
    for default in (((6, 6), (3, 3), (1, 1)), ((4, 4), (1, 1), (1, 1)), ((5, 5), (3, 3), (2, 2)), ((10, 10), (1, 1), (1, 1))):
        assert hip.block_geometry(*default) is None
