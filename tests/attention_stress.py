"""Inputs, references and the bound of the attention softmax stress tests (tests/test_attention_stress_inputs.py on the CPU,
tests/test_gpu_attention_stress.py on the GPU).  No test lives here.

Why: with q, k ~ randn the scaled scores are about N(0, 4) -- the largest of 4096 is near 8 -- and softmax does not change under a
consistent shift, so a kernel that takes its running maximum over the wrong lanes, over a whole tile, from 0 instead of -inf, or not
at all, still gives the right answer.  The regimes below put the scores tens to hundreds apart, where only the maximum the algorithm
claims to take keeps exp2 inside fp32.

Inputs: q, k, v ~ randn ("the rest") except ONE steering channel per head: q[..., h*d] = c_i * sqrt(d), k[..., h*d] = b_j, so that at
scale = d ** -0.5 the score of query i against key j is c_i * b_j plus the rest's N(0, ~1).

    regime    c_i                      b_j               what only it can see
    offset+   1                        +300              no maximum subtracted (exp overflows)
    offset-   1                        -300              a running maximum started at 0; Nk % 16 != 0: tail keys scored 0, not -inf
    rows      ((i % 16) - 7.5) * 40    1                 one maximum for the 16 queries of a tile (row maxima 600 apart in a tile)
    ramp      as rows                  j / (Nk - 1)      half of a tile's rows peak at the last key and rescale at every block (by up
                                                         to 2^70), the other half peak at key 0 and never rescale: both in one wave
    spike     1                        200 at j*, else 0 one-hot rows, out = v[j*]: all mass in one wave's / one split's partial, the
                                                         others underflow in the merge
    flat      q = 0                    -                 all scores exactly 0, v = 100 + randn: the normaliser, equal maxima everywhere

Truth: chain(..., float64) on the CPU from the fp32 inputs.  Bound per case: max(4 * e32, 2e-5 * (1 + max|want|)), e32 the error of
chain(..., float32) against that truth on the same inputs -- the rule of tests/test_gpu_attention_wide.py (another summation order,
never a much worse one) with the project's fp32-level criterion as a floor (in `spike` the fp32 chain is exact: e32 = 0)."""
import functools

import torch

REGIMES = ("offset+", "offset-", "rows", "ramp", "spike", "flat")
MUTANTS = ("nomax", "init0", "tilemax", "pad0", "norescale", "mergeflat")
LOG2E = 1.44269504088896341

# (B, Nq, Nk, heads, d) of the GPU tests: hip.attention_tokens ...
TOKEN_SHAPES = [
    (2, 48, 100, 2, 40),  # tail keys, 7 key blocks on 4 waves, an odd tile count for form 2
    (1, 16, 5, 1, 64),    # fewer key blocks than waves
    (1, 32, 72, 1, 160),  # the widest head
    (1, 16, 40, 8, 8),    # B * heads a multiple of 8: the (batch, head) pairs dealt to the XCDs
    (1, 16, 1, 1, 64),    # one key
]
# ... and hip.attention_wide
WIDE_SHAPES = [
    (1, 48, 100, 1, 192),
    (1, 16, 5, 1, 512),
    (2, 32, 256, 1, 512),  # key blocks split over workgroups
    (1, 64, 64, 2, 256),   # heads as strides
    (1, 16, 1, 1, 192),    # one key
]


def spikes(Nk, qkv=False):
    """The keys a `spike` sits on: one in each of the first four 16-key blocks, a block edge, the last live key of the tail block;
    for the qkv layouts also the fused kernel's 64-key slice edge and the apply kernels' 256-key value chunk edge."""
    cand = [0, 15, 16, 37, 58, Nk - 1] + ([63, 64, 255, 256] if qkv else [])
    return sorted({j for j in cand if 0 <= j < Nk})


def regimes_for(Nk, qkv=False):
    """[(regime, spike)] of a shape: every regime once, `spike` once per position."""
    out = []
    for r in REGIMES:
        out += [(r, j) for j in spikes(Nk, qkv)] if r == "spike" else [(r, None)]
    return out


def regime_id(regime, spike):
    return regime if spike is None else "%s@%d" % (regime, spike)


def steering(regime, Nq, Nk, spike=None):
    """(c [Nq], b [Nk]) in fp64: the score of query i against key j is c_i * b_j + the rest."""
    i, j = torch.arange(Nq, dtype=torch.float64), torch.arange(Nk, dtype=torch.float64)
    rows = ((i % 16) - 7.5) * 40
    one_q, one_k = torch.ones(Nq, dtype=torch.float64), torch.ones(Nk, dtype=torch.float64)
    if regime == "offset+":
        return one_q, 300 * one_k
    if regime == "offset-":
        return one_q, -300 * one_k
    if regime == "rows":
        return rows, one_k
    if regime == "ramp":
        return rows, j / max(Nk - 1, 1)
    if regime == "spike":
        b = torch.zeros(Nk, dtype=torch.float64)
        b[spike] = 200
        return one_q, b
    raise ValueError(regime)


def make(B, Nq, Nk, heads, d, regime, spike=None, layout="tokens"):
    """fp32 (q, k, v) on the CPU from a seeded generator.  layout "tokens": q [B,Nq,C], k / v [B,Nk,C], C = heads * d.  layout "qkv"
    (one head, d = C, Nq = Nk = HW): the three thirds of a [B,3C,H,W] tensor as they lie in it, [B,C,HW] each -- channel 0 of the q
    and k thirds steered, the pixel index as i / j (see qkv_image / tokens_of)."""
    assert regime in REGIMES and (regime == "spike") == (spike is not None)
    C = heads * d
    g = torch.Generator().manual_seed(1000003 * REGIMES.index(regime) + 7919 * (spike or 0) + 31 * Nq + 17 * Nk + 5 * heads + d + B)
    if layout == "qkv":
        assert heads == 1 and Nq == Nk
        q, k, v = (torch.randn(B, C, Nk, generator=g).transpose(1, 2) for _ in range(3))  # (token views of channel-major data)
    else:
        q, k, v = (torch.randn(B, n, C, generator=g) for n in (Nq, Nk, Nk))
    if regime == "flat":
        q.zero_()
        v += 100
    else:
        c, b = steering(regime, Nq, Nk, spike)
        for h in range(heads):
            q[:, :, h * d] = (c * d ** 0.5).float()
            k[:, :, h * d] = b.float()
    if layout == "qkv":
        return tuple(t.transpose(1, 2) for t in (q, k, v))
    return q, k, v


def tokens_of(t):
    """A third [B,C,HW] (or an output [B,C,H,W]) of the qkv layouts as tokens [B,HW,C]."""
    return t.reshape(t.shape[0], t.shape[1], -1).transpose(1, 2)


def qkv_image(q, k, v, H, W):
    """The thirds [B,C,HW] stacked on the channel axis: [B,3C,H,W], contiguous."""
    B, C, HW = q.shape
    assert HW == H * W
    return torch.cat([q, k, v], 1).reshape(B, 3 * C, H, W).contiguous()


def _heads(t, heads, dtype):
    b, n, c = t.shape
    return t.to(dtype).reshape(b, n, heads, c // heads).permute(0, 2, 1, 3).reshape(b * heads, n, c // heads)


def _unheads(t, B, heads):
    bh, n, d = t.shape
    return t.reshape(B, heads, n, d).permute(0, 2, 1, 3).reshape(B, n, heads * d)


def chain(q, k, v, heads, scale, dtype):
    """bmm / softmax / bmm per (batch, head) in `dtype` -> [B,Nq,C]."""
    B, Nq, C = q.shape
    qh, kh, vh = (_heads(t, heads, dtype) for t in (q, k, v))
    att = torch.bmm(torch.softmax(torch.bmm(qh, kh.transpose(1, 2)) * scale, dim=2), vh)
    return att.reshape(B, heads, Nq, C // heads).permute(0, 2, 1, 3).reshape(B, Nq, C)


def bound(want, e32):
    return max(4.0 * float(e32), 2e-5 * (1.0 + float(want.abs().max())))


@functools.lru_cache(maxsize=None)
def case(B, Nq, Nk, heads, d, regime, spike=None, layout="tokens"):
    """(q, k, v, want) of a case, computed once per process and shared (leave them unchanged): the inputs as tokens [B,N,C] and the
    fp64 chain's output [B,Nq,C] at scale = d ** -0.5."""
    q, k, v = make(B, Nq, Nk, heads, d, regime, spike, layout)
    if layout == "qkv":
        q, k, v = (tokens_of(t) for t in (q, k, v))
    return q, k, v, chain(q, k, v, heads, d ** -0.5, torch.float64)


# ---- an fp32 emulation of what the kernels do, and of what a simpler kernel would do ---------------------------------------------
def _wave(qh, kh, vh, sl, blocks, Nk, mutant):
    """One wave's running (m, l, O) over its 16-key blocks, exp2 form; `seen`: it had a block."""
    BH, Nq, d = qh.shape
    start = 0.0 if mutant in ("init0", "nomax") else float("-inf")
    m = torch.full((BH, Nq), start)
    l, O = torch.zeros(BH, Nq), torch.zeros(BH, Nq, d)
    for kb in blocks:
        ks, vs = kh[:, 16 * kb:min(Nk, 16 * kb + 16)], vh[:, 16 * kb:min(Nk, 16 * kb + 16)]
        s = torch.bmm(qh, ks.transpose(1, 2)) * sl
        mb = s.max(dim=2).values
        if mutant == "pad0" and ks.shape[1] < 16:  # (the tail keys enter the block's maximum as 0, not as -inf; their p stays 0)
            mb = mb.clamp_min(0.0)
        if mutant == "tilemax":  # (one maximum for the 16 queries of a tile)
            mb = mb.reshape(BH, Nq // 16, 16).max(dim=2, keepdim=True).values.expand(BH, Nq // 16, 16).reshape(BH, Nq)
        m_new = m if mutant == "nomax" else torch.maximum(m, mb)
        alpha = torch.ones_like(m) if mutant == "norescale" else torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[:, :, None])
        l = l * alpha + p.sum(dim=2)
        O = O * alpha[:, :, None] + torch.bmm(p, vs)
        m = m_new
    return m, l, O, len(blocks) > 0


def _merge(parts, mutant):
    """Partials (m, l, O, seen) merged by 2^(m_w - M) weights; weight 0 for one that saw no block."""
    live = [p for p in parts if p[3]]
    if not live:
        return parts[0]
    M = functools.reduce(torch.maximum, [p[0] for p in live])
    L, O = torch.zeros_like(live[0][1]), torch.zeros_like(live[0][2])
    for m, l, o, _ in live:
        f = torch.ones_like(m) if mutant == "mergeflat" else torch.exp2(m - M)
        L = L + f * l
        O = O + f[:, :, None] * o
    return M, L, O, True


def online_softmax(q, k, v, heads, scale, mutant=None, splits=1):
    """fp32 CPU emulation of the blocked online softmax of attention_tokens.hip / attention_wide.hip: the 16-key blocks of each of
    `splits` ranges dealt round-robin to four "waves", each with a running (m, l, O) in units of log2, the waves and then the splits
    merged by 2^(m - M) weights.  `mutant`: one of MUTANTS --
      nomax      no maximum subtracted (m stays 0)             init0      the running maximum starts at 0, not at -inf
      tilemax    one maximum for the 16 queries of a tile      pad0       the keys past Nk of the tail block enter its maximum as 0
      norescale  l and O are not rescaled when m grows         mergeflat  the partials are merged with weight 1
    (pad0: in the MAXIMUM only, their probability stays 0 -- the mask applied after the row maximum instead of before it.  Tail keys
    that also carried exp(0 - m) of mass would add 12 keys' worth of weight at Nk = 100 and fail on any input; this one is hidden
    by randn scores, whose row maxima are positive anyway.)"""
    assert mutant is None or mutant in MUTANTS
    B, Nq, C = q.shape
    Nk = k.shape[1]
    qh, kh, vh = (_heads(t, heads, torch.float32) for t in (q, k, v))
    sl = torch.tensor(scale * LOG2E, dtype=torch.float32)
    nkb = (Nk + 15) // 16
    per = -(-nkb // splits)
    parts = []
    for s in range(splits):
        blocks = list(range(s * per, min(nkb, (s + 1) * per)))
        parts.append(_merge([_wave(qh, kh, vh, sl, blocks[w::4], Nk, mutant) for w in range(4)], mutant))
    _, L, O, _ = _merge(parts, mutant)
    return _unheads(O / L[:, :, None], B, heads)
