"""Shapes and shared cases of the fp16-operand wide-head attention's tests (sige_hip_attention_wide_f16c / _tiles_f16c,
hip.attention_wide(..., compute="f16"); tests/test_attention_wide_f16_inputs.py on the CPU, tests/test_gpu_attention_wide_f16.py and
tests/test_gpu_attention_wide_f16_stacked.py on the GPU).  No test lives here.

The contract, its emulation and the bound are those of tests/attention_f16.py (the entries share the arithmetic contract of
sige_hip_attention_tokens_f16c): truth = the fp64 chain on the inputs as given, bound16 = max(4 * e16, 2e-5 * (1 + max|want|)) with e16
the CPU emulation's error on the same inputs."""
import functools

from tests import attention_f16 as F
from tests import attention_stress as A

# (B, Nq, Nk, heads, d)
WIDE_F16_SHAPES = A.WIDE_SHAPES + [
    (1, 16, 17, 1, 192),  # one live key in the second 16-key block
    (1, 16, 33, 1, 512),  # one live key in a second 32-key step
    (1, 16, 40, 1, 176),  # d no multiple of 32 or 64: the zero padding of the last unit
]
SPLIT_SHAPE = (2, 32, 256, 1, 512)  # 4 query tiles, 8 steps of 32 keys: two workgroups per tile
DUST_D = 192


def shape_id(s):
    return "B%d_Nq%d_Nk%d_h%d_d%d" % tuple(s)


def cases():
    """[(shape, regime, spike)] over WIDE_F16_SHAPES x A.regimes_for(Nk)."""
    return [(s, r, j) for s in WIDE_F16_SHAPES for r, j in A.regimes_for(s[2])]


@functools.lru_cache(maxsize=None)
def dust_case():
    """F.dust at one 192-wide head: (q, k, v, want, e16, bound16); computed once, left unchanged."""
    q, k, v = F.dust(d=DUST_D)
    return F._judged(q, k, v, 1, DUST_D ** -0.5)
