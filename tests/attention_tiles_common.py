"""Inputs, truths and bounds of the per-image token attention's tests (sige_hip_attention_tokens_tiles_f32 / _f16c,
hip.attention_tokens(..., tiles=...); tests/test_attention_tokens_tiles_inputs.py on the CPU, tests/test_gpu_attention_tokens_tiles.py
on the GPU).  No test lives here.

Under stacked edits the queries are the tokens of T 4x4 tiles of the tall image of E images of h rows, and tile t attends to the h W
keys of ITS image -- the image its origin row lies in -- and to no others.

Truth: tests.attention_stress.chain(..., float64) PER IMAGE, from the fp32 inputs.  Bounds: tests.attention_stress.bound with e32 the
fp32 chain's error on the same per-image problems; tests.attention_f16.bound16 with e16 the error of the emulation there on that
image's keys.  `mixed` is what "the keys of all E images" gives in fp64: the bug the entry exists for.

Inputs: q = 2 randn (peaked rows: the maxima matter), k = randn, V of image e = randn + 10 e^2 (0, 10, 40: the mean over all images
is no image's own mean, so every image's output moves by units when it reads a neighbour's keys).

The shapes are the smallest at which each thing can go wrong:
    d = 16 one 16-channel unit; 40 a padded last unit (and the f16 form's half-empty 32-channel unit); 80 whole units; 160 the widest
    heads 1 and 4: workgroups in plain order; 8: the heads dealt to the XCDs
    E = 2 and E = 3 (no power of two) at h = 8
    W = 6: 48 keys, exact key blocks; W = 5: 40 keys, a tail block and fewer blocks than the 4 waves (two 32-key steps in the f16 form)
    h = 16, W = 8: 128 keys, more than one block per wave
The tile lists are uneven between the images; each has tiles in the last tile row of an image and the first of the next; one has an
image with no tile."""
import functools

import torch

from tests import attention_f16 as F
from tests import attention_stress as A

# (E, h, W, heads, d) -> the origin row in the TALL image of every tile, in list order (the per-edit lists one after the other)
CASES = {
    (2, 8, 6, 1, 16): [0, 4, 4, 8],
    (3, 8, 5, 4, 40): [0, 4, 16, 20, 20],            # image 1 has no tile
    (2, 8, 6, 8, 80): [4, 8, 12, 12],
    (3, 8, 5, 1, 160): [0, 4, 8, 12, 12, 20],
    (2, 16, 8, 8, 40): [0, 12, 16, 28, 28],
    (3, 8, 6, 4, 16): [4, 8, 8, 12, 16, 20, 20],
}


def case_id(key):
    return "E%d-h%d-W%d-heads%d-d%d" % key


def per_image(key):
    E, h = key[0], key[1]
    return [sum(1 for r in CASES[key] if r // h == e) for e in range(E)]


@functools.lru_cache(maxsize=None)
def case(key):
    """dict of a case, on the CPU, computed once per process and shared (leave the tensors unchanged):
    q [1,16T,C], k, v [1,E h W,C], idx int32 [T,2], want / mixed fp64 [1,16T,C], image [T] (the image of every tile), e32, bound,
    e16, bound16."""
    E, h, W, heads, d = key
    rows = CASES[key]
    T, N, C = len(rows), h * W, heads * d
    g = torch.Generator().manual_seed(100000 * E + 1000 * h + 100 * W + 10 * heads + d)
    q = torch.randn(1, 16 * T, C, generator=g) * 2.0
    k = torch.randn(1, E * N, C, generator=g)
    v = torch.randn(E, N, C, generator=g) + 10.0 * (torch.arange(E, dtype=torch.float32) ** 2).reshape(E, 1, 1)
    v = v.reshape(1, E * N, C)
    idx = torch.tensor([(r, 0 if W < 8 else 4 * (i % 2)) for i, r in enumerate(rows)], dtype=torch.int32)
    image = torch.tensor([r // h for r in rows])
    scale = d ** -0.5
    want = torch.empty(1, 16 * T, C, dtype=torch.float64)
    e32 = e16 = 0.0
    for e in range(E):
        mine = [t for t in range(T) if int(image[t]) == e]
        if not mine:
            continue
        sel = torch.cat([torch.arange(16 * t, 16 * t + 16) for t in mine])
        qs, ks, vs = q[:, sel], k[:, e * N:(e + 1) * N], v[:, e * N:(e + 1) * N]
        w = A.chain(qs, ks, vs, heads, scale, torch.float64)
        want[:, sel] = w
        e32 = max(e32, float((A.chain(qs, ks, vs, heads, scale, torch.float32).double() - w).abs().max()))
        e16 = max(e16, float((F.emulate(qs, ks, vs, heads, scale).double() - w).abs().max()))
    mixed = A.chain(q, k, v, heads, scale, torch.float64)
    return dict(q=q, k=k, v=v, idx=idx, image=image, want=want, mixed=mixed, e32=e32, bound=A.bound(want, e32), e16=e16,
                bound16=F.bound16(want, e16), scale=scale)
