"""Inputs, the emulation and the bound of the fp16-operand token attention's tests (sige_hip_attention_tokens_f16c,
hip.attention_tokens(..., compute="f16"); tests/test_attention_f16_inputs.py on the CPU, tests/test_gpu_attention_f16.py on the GPU).
No test lives here.

The contract (include/sige_hip.h): q, k, v rounded to nearest even to fp16; fp32 scores, fp32 scale in units of log2, fp32 softmax state;
the probabilities rounded to nearest even to fp16 for the product with v; O, l and the merge fp32.  `emulate` is
tests.attention_stress.online_softmax -- 16-key blocks dealt round-robin to four "waves", merged by 2^(m - M) weights -- with exactly
these roundings added; l is summed from the UNROUNDED probabilities (the looser of the two sound choices: a kernel that sums the rounded
ones is closer to the truth of its own products and passes too).

Truth: A.chain(..., float64) on the inputs AS GIVEN.  Bound per case: bound16 = max(4 * e16, 2e-5 * (1 + max|want|)), e16 the clean
emulation's error against that truth -- the project's rule (A.bound) with the fp16 emulation in the place of the fp32 chain: another
blocking or summation order of the same roundings, never a much worse one.

`dust`: one key with probability ~1 and 2047 keys with probability e^-11 = 1.7e-5 each -- below 2^-14, an fp16 SUBNORMAL -- that carry
3.4 % of the mass and whose values lie 100 away from the heavy key's.  A matrix unit (or a conversion) that flushes subnormal fp16
operands loses them where they meet the large maximum: in the wave that holds the heavy key, a quarter of the key blocks (the other
waves' own maxima are 0, their probabilities 1; the merge scales them in fp32).  `emulate(flush=True)` does exactly that."""
import functools
import math

import torch

from tests import attention_stress as A

# (B, Nq, Nk, heads, d)
F16_SHAPES = A.TOKEN_SHAPES + [
    (2, 32, 77, 8, 40),  # SD's cross-attention as it is: 77 text keys, 8 heads of 40
    (1, 16, 17, 1, 40),  # one live key in the second 16-key block
    (1, 16, 33, 2, 80),  # one live key in a second 32-key step
]


def r16(t):
    """fp32 -> nearest-even fp16 -> fp32."""
    return t.half().float()


def _wave(qh, kh, vh, sl, blocks, Nk, mutant, flush):
    """A._wave with the probabilities rounded to fp16 (and, `flush`, the subnormal ones zeroed) in the product with V."""
    BH, Nq, d = qh.shape
    start = 0.0 if mutant in ("init0", "nomax") else float("-inf")
    m = torch.full((BH, Nq), start)
    l, O = torch.zeros(BH, Nq), torch.zeros(BH, Nq, d)
    for kb in blocks:
        ks, vs = kh[:, 16 * kb:min(Nk, 16 * kb + 16)], vh[:, 16 * kb:min(Nk, 16 * kb + 16)]
        s = torch.bmm(qh, ks.transpose(1, 2)) * sl
        mb = s.max(dim=2).values
        if mutant == "pad0" and ks.shape[1] < 16:
            mb = mb.clamp_min(0.0)
        if mutant == "tilemax":
            mb = mb.reshape(BH, Nq // 16, 16).max(dim=2, keepdim=True).values.expand(BH, Nq // 16, 16).reshape(BH, Nq)
        m_new = m if mutant == "nomax" else torch.maximum(m, mb)
        alpha = torch.ones_like(m) if mutant == "norescale" else torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[:, :, None])
        p16 = r16(p)
        if flush:
            p16 = torch.where(p16 < 2.0 ** -14, torch.zeros_like(p16), p16)
        l = l * alpha + p.sum(dim=2)
        O = O * alpha[:, :, None] + torch.bmm(p16, vs)
        m = m_new
    return m, l, O, len(blocks) > 0


def emulate(q, k, v, heads, scale, mutant=None, flush=False):
    """fp32 CPU emulation of the contract on q [B,Nq,C], k / v [B,Nk,C] -> [B,Nq,C]; `mutant`: one of A.MUTANTS (what a simpler
    kernel would do); `flush`: probabilities below 2^-14 do not arrive in the product with V."""
    assert mutant is None or mutant in A.MUTANTS
    B = q.shape[0]
    Nk = k.shape[1]
    qh, kh, vh = (A._heads(r16(t), heads, torch.float32) for t in (q, k, v))
    sl = torch.tensor(scale * A.LOG2E, dtype=torch.float32)
    nkb = (Nk + 15) // 16
    blocks = list(range(nkb))
    _, L, O, _ = A._merge([_wave(qh, kh, vh, sl, blocks[w::4], Nk, mutant, flush) for w in range(4)], mutant)
    return A._unheads(O / L[:, :, None], B, heads)


def bound16(want, e16):
    return max(4.0 * float(e16), 2e-5 * (1.0 + float(want.abs().max())))


def _judged(q, k, v, heads, scale):
    """(q, k, v, want, e16, bound16): the fp64 truth of the inputs as given, the clean emulation's error, the bound."""
    want = A.chain(q, k, v, heads, scale, torch.float64)
    e16 = float((emulate(q, k, v, heads, scale).double() - want).abs().max())
    return q, k, v, want, e16, bound16(want, e16)


@functools.lru_cache(maxsize=None)
def case(B, Nq, Nk, heads, d, regime, spike=None):
    """A regime of tests.attention_stress with its inputs rounded to fp16 first; computed once per process and shared (leave the
    tensors unchanged).  scale = d ** -0.5."""
    q, k, v = (r16(t) for t in A.make(B, Nq, Nk, heads, d, regime, spike))
    return _judged(q, k, v, heads, d ** -0.5)


@functools.lru_cache(maxsize=None)
def randn_case(B, Nq, Nk, heads, d):
    """UNROUNDED randn inputs: the input rounding is part of what is judged."""
    g = torch.Generator().manual_seed(16 + 31 * Nq + 17 * Nk + 5 * heads + d + B)
    q, k, v = (torch.randn(B, n, heads * d, generator=g) for n in (Nq, Nk, Nk))
    return _judged(q, k, v, heads, d ** -0.5)


def dust(Nq=16, Nk=2048, d=40):
    """(q, k, v), one batch, one head, scale = d ** -0.5: key 7 scores 11, every other key 0."""
    g = torch.Generator().manual_seed(2048 + d)
    q, k = torch.zeros(1, Nq, d), torch.zeros(1, Nk, d)
    q[..., 0] = 11 * math.sqrt(d)
    k[:, 7, 0] = 1
    v = 100 + torch.randn(1, Nk, d, generator=g)
    v[:, 7] = torch.randn(d, generator=g)
    return r16(q), r16(k), r16(v)


@functools.lru_cache(maxsize=None)
def dust_case():
    q, k, v = dust()
    return _judged(q, k, v, 1, 40 ** -0.5)
