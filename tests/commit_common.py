"""Shared by the tests of sige_hip_commit_tiles (csrc/commit_tiles.hip): the CPU reference of one record and the record sets, on the
geometries, lists and seeded inputs of tests/data_movement_common.py (the ragged 18 x 26 image).  Nothing here touches a device
(tests/test_commit_tiles_inputs.py runs it without one)."""
import torch

from tests import data_movement_common as D

CHUNK = 64                        # csrc/commit_tiles.hip kChunk: channels of one workgroup
CHANNELS = D.CHANNELS + (132,)    # ... and one count above two chunks that is no multiple of one
CAPACITY = 48                     # include/sige_hip.h SIGE_HIP_COMMIT_CAPACITY
GEOS = tuple(D.GEOS)
NAMES = tuple(D.NAMES)


def swish_cpu(z):
    """The reference's SiLU on fp32 values: z / (1.0 + exp(-z)), the sum and the quotient in double (sige/cpu/common_cpu.cpp)."""
    return (z.double() / (1.0 + torch.exp(-z).double())).float()


def affine_swish(v, scale, shift):
    """SiLU(scale[c] * v + shift[c]) on [*, C, h, w]: two separately rounded fp32 operations, then the SiLU."""
    z = scale.reshape(1, -1, 1, 1) * v
    z = shift.reshape(1, -1, 1, 1) + z
    return swish_cpu(z)


def commit_ref(dst, src, geo, idx, tile_source, value=None):
    """What one record leaves in `dst` [1,C,Ho,Wo] (a new tensor): tile n of `idx` writes the pixels (off + origin) / stride +
    [0,t)^2, clipped at the bottom and right, from the same pixels of `src` [1,C,Ho,Wo] or from tile n of `src` [N,C,t,t]; a later
    tile overwrites an earlier one.  `value`: applied to the source first."""
    g = D.GEOS[geo] if isinstance(geo, str) else geo
    t = g["tile"]
    Ho, Wo = g["out_res"]
    out = dst.clone()
    v = src if value is None else value(src)
    for n, (h0, w0) in enumerate(idx.tolist()):
        h, w = D.origin(g, h0, w0)
        h1, w1 = min(h + t, Ho), min(w + t, Wo)
        if h1 <= h or w1 <= w:
            continue
        out[0, :, h:h1, w:w1] = v[n][:, :h1 - h, :w1 - w] if tile_source else v[0, :, h:h1, w:w1]
    return out


def inputs(C, geo, name, which="xa"):
    """(tiles [N,C,t,t], full source [1,C,Ho,Wo], the destination's start [1,C,Ho,Wo], idx) of one geometry and list."""
    g = D.GEOS[geo]
    idx = g["lists"][name]
    d = D.case(C, 1)[g["tile"]]
    return D.tiles_of(d[which], idx.shape[0]), d["y"], d["z"], idx


def record_args(geo):
    g = D.GEOS[geo]
    return dict(offset=(g["offset"],) * 2, stride=(g["stride"],) * 2, tile=(g["tile"],) * 2)


def mixed_specs():
    """The records of the one-call test: (geo, list, tile_source, which tiles) -- all four geometries, both source kinds, every
    list, an empty record in the middle."""
    out = []
    for gi, geo in enumerate(GEOS):
        for ni, name in enumerate(("every", "empty", "corners", "interior", "holes")):
            out.append((geo, name, bool((gi + ni) % 2), "xa" if ni % 2 else "xb"))
    return out


def many_specs(n):
    """n records with a tile each (no `empty`), cycling over geometries, lists and source kinds."""
    names = ("every", "corners", "interior", "holes")
    return [(GEOS[i % 4], names[(i // 4) % 4], bool((i // 2) % 2), "xa" if i % 3 else "xb") for i in range(n)]


# output tiles above 4 x 4 (the kernel's instances with 4 and 16 passes of 16 pixels): 8 x 8 and 12 x 12 tiles on the 18 x 26 image,
# the last of each hanging over the bottom and right border
LARGE_TILES = {8: torch.tensor([[0, 0], [8, 16], [16, 24]], dtype=torch.int32), 12: torch.tensor([[0, 12], [12, 0], [12, 24]], dtype=torch.int32)}


def large_geo(t):
    return dict(tile=t, offset=0, stride=1, out_res=(D.H, D.W))
