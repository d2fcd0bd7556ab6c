"""Shared by the block-size-10 tests: named tile lists over a grid of block origins."""
import torch


def _grid(rows, cols, step, pad, keep=None):
    idx = [(step * i - pad, step * j - pad) for i in range(rows) for j in range(cols)]
    if keep is not None:
        idx = [idx[k] for k in keep]
    return torch.tensor(idx, dtype=torch.int32).reshape(-1, 2)


def tile_lists(rows, cols, step, pad):
    """name -> [N,2] int32 origins (step * i - pad, step * j - pad) over a rows x cols grid."""
    n = rows * cols
    return {
        "every": _grid(rows, cols, step, pad),                                     # all four borders, the overhanging last row included
        "corners": _grid(rows, cols, step, pad, [0, cols - 1, n - cols, n - 1]),
        "interior": _grid(rows, cols, step, pad, [cols + 1]),
        "holes": _grid(rows, cols, step, pad, [k for k in range(n) if k % 3 != 1]),
        "empty": _grid(rows, cols, step, pad, []),
    }
