"""hip.kv_rows_store_f16 = sige_hip_kv_rows_store_f16 (csrc/kv_rows_f16.hip) on the GPU: the K and V rows of the active tiles, rounded to
nearest even and stored into the fp16 K / V in one launch -- bit for bit what torch indexing plus .half() gives, every other row left
as it was (a sentinel pattern)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (H, W) -> tile origins: the 8 x 8 grid; a ragged 10 x 6 one with tiles that overhang the bottom and the right edge
GRIDS = {(8, 8): [(0, 0), (4, 4), (0, 4)], (10, 6): [(0, 0), (8, 0), (4, 4), (8, 4)]}


@pytest.mark.parametrize("C", [8, 72, 320])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("grid", list(GRIDS), ids=lambda g: "%dx%d" % g)
def test_rows_land_rounded_and_nothing_else_moves(grid, B, C):
    from sige_amd import hip

    (H, W), tiles = grid, GRIDS[grid]
    T = len(tiles)
    g = torch.Generator().manual_seed(H * W + B + C)
    # values that need rounding in every binade fp16 has between 2^-16 (subnormal) and 2^8
    rows = [(torch.randn(B, 16 * T, C, generator=g) * 2.0 ** torch.randint(-16, 8, (B, 16 * T, C), generator=g).float()).to(DEV)
            for _ in range(2)]
    sentinel = (torch.arange(B * H * W * C, dtype=torch.float32) % 2039.0 - 1000.0).reshape(B, H * W, C).half().to(DEV)
    got, want = [sentinel.clone(), (-sentinel).clone()], [sentinel.clone(), (-sentinel).clone()]
    for w, r in zip(want, rows):
        for t, (y0, x0) in enumerate(tiles):
            for i in range(4):
                for j in range(4):
                    if y0 + i < H and x0 + j < W:
                        w[:, (y0 + i) * W + x0 + j] = r[:, 16 * t + 4 * i + j].half()
    idx = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    n0 = hip.launch_count()
    hip.kv_rows_store_f16(rows[0], rows[1], got[0], got[1], idx, H, W)
    assert hip.launch_count() == n0 + 1
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
    hip.kv_rows_store_f16(rows[0][:, :0], rows[1][:, :0], got[0], got[1], idx[:0], H, W)  # T = 0: nothing launched
    assert hip.launch_count() == n0 + 1
