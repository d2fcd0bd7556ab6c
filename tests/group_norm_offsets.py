"""Inputs, the fp64 reference, the two bounds and the emulations of the GroupNorm-statistics tests on OFFSET inputs
(tests/test_group_norm_offset_inputs.py on the CPU, tests/test_gpu_group_norm_offsets.py on the GPU).  No test lives here.

A GroupNorm affine is (scale, shift) [B,C] with GroupNorm(x + channel_bias) == x * scale + shift.  Every route of
sige_amd/csrc/group_norm.hip sums in fp32 and finishes in fp64; a one-pass variance E[x^2] - mean^2 from fp32 sums loses
eps32 * (mean / std)^2 of its relative accuracy, so what is judged here is a group whose mean is 30 ... 3000 times its spread.

Case table (CASES): `kind` says where the offsets sit, `ratio` is |m_g| / s_g of the offset groups.
* "x": x = m_g + s_g * randn.  Groups cycle through (0, 1), (+R, 1), (-R * 1e-2, 1e-2), (-R, 1) and flip the signs every four
  groups: offsets differ from group to group, both signs and both spreads occur, a zero-offset group sits next to an offset one
  (a pivot or a low part taken from the wrong group or channel shows there).
* "edge" (an "x" case): group 0 is exactly 3.0 (variance 0: scale = gamma / sqrt(eps)), group 1 is 1 + 1e-3 * randn (variance
  ~ eps, ratio 1000), group 2 has no offset, group 3 is 300 + randn; then again.
* "bias": x = s_g * randn and the offsets sit in channel_bias.  "bias_split": the channels of one group at different biases
  (m_g and m_g + s_g alternating), so a pivot can not remove the bias of every channel.

Bounds (check): |scale - scale64| <= 4e-6 |scale64| and max|x * scale + shift - want| <= 3 E_ideal + 2e-6, both sides applied
in fp32, E_ideal the same maximum for scale64 / shift64 rounded to fp32 -- what exact statistics would leave.

Emulations of the accumulation order, numpy on the CPU:
* naive: fp32 sums of x + bias and of its square over slices of 128 pixels, the slices combined in fp64.
* pivot (the direct kernels): K_x = the group's first element, K_b = the bias of the group's first channel;
  v = (x - K_x) + (bias - K_b) in fp32, then as naive; mean = K_x + K_b + s / n, var = ss / n - (s / n)^2.  (The kernels add
  only each lane's few dozen values in fp32 and everything beyond in fp64: the emulation's 128-pixel fp32 slices are the
  looser form of the same scheme.)
* pairs (the per-block statistics): per channel and 128-pixel block, sum and sum of squares as unevaluated fp32 pairs
  (TwoSum; the product's residual from fma(x, x, -x * x)); the finisher adds hi + lo in fp64 and folds the bias in there.
  (The kernels form the block's sums in fp64 and split them into such pairs when they store them: the same stored format, the
  pair arithmetic here is the looser way to fill it.)"""
import collections
import functools

import numpy as np
import torch

from tests import util

EPS = 1e-6
SCALE_RTOL = 4e-6
OUT_FACTOR, OUT_FLOOR = 3.0, 2e-6
SLICE = 128  # pixels per fp32 partial sum

Case = collections.namedtuple("Case", "name kind ratio seed")
CASES = [
    Case("x_r0", "x", 0, 1), Case("x_r30", "x", 30, 2), Case("x_r300", "x", 300, 3), Case("x_r3000", "x", 3000, 4),
    Case("edge", "x", 1000, 5),
    Case("bias_r30", "bias", 30, 6), Case("bias_r300", "bias", 300, 7), Case("bias_r3000", "bias", 3000, 8),
    Case("bias_split_r300", "bias_split", 300, 9),
]
X_CASES = [c for c in CASES if c.kind == "x"]
BIAS_CASES = [c for c in CASES if c.kind != "x"]


def group_table(case, groups):
    """(m_g, s_g, special_g) per group; special: None, "const" or "near"."""
    m, s, special = np.zeros(groups), np.ones(groups), [None] * groups
    for g in range(groups):
        k, flip = g % 4, (-1.0 if (g // 4) % 2 else 1.0)
        if case.name == "edge":
            if k == 0:
                m[g], s[g], special[g] = 3.0, 0.0, "const"
            elif k == 1:
                m[g], s[g], special[g] = 1.0, 1e-3, "near"
            elif k == 3:
                m[g] = 300.0 * flip
        else:
            s[g] = 1e-2 if k == 2 else 1.0
            m[g] = (0.0, flip, -flip, -flip)[k] * case.ratio * s[g]
    return m, s, special


def channel_table(case, C, groups):
    """Per-channel (offset m_c, spread s_c) of `case` -- for a producer that sets them channel by channel (a conv's bias and
    weight rows)."""
    m, s, _ = group_table(case, groups)
    cg = C // groups
    return torch.tensor(np.repeat(m, cg), dtype=torch.float32), torch.tensor(np.repeat(s, cg), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def make(case, shape, groups):
    """(x [B,C,H,W] fp32, gamma [C], beta [C], channel_bias [C] or None) on the CPU; computed once per process and shared
    (leave the tensors unchanged)."""
    B, C, H, W = shape
    cg = C // groups
    g = torch.Generator().manual_seed(1000 * case.seed + 31 * C + 7 * H + W + groups)
    m, s = channel_table(case, C, groups)
    z = torch.randn(B, C, H, W, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    if case.kind == "x":
        x = (m.view(1, C, 1, 1).double() + s.view(1, C, 1, 1).double() * z.double()).float()
        return x, gamma, beta, None
    x = (s.view(1, C, 1, 1) * z).contiguous()
    bias = m.clone()
    if case.kind == "bias_split":
        odd = (torch.arange(C) % cg) % 2 == 1
        bias = torch.where(odd, m + s, m)
    return x, gamma, beta, bias


Ref = collections.namedtuple("Ref", "want scale64 shift64 scale32 shift32 e_ideal")


def apply32(x, scale, shift):
    """x * scale + shift the way the affine's consumers apply it: two fp32 operations."""
    B, C = x.shape[:2]
    return x * scale.reshape(B, C, 1, 1) + shift.reshape(B, C, 1, 1)


def reference(x, groups, eps, gamma, beta, bias):
    """fp64: want = GroupNorm(x + bias) [B,C,H,W]; scale64 / shift64 [B,C] with want == x * scale64 + shift64; the ideal fp32
    affine = those two rounded to fp32, and E_ideal = max|x * scale32 + shift32 - want| applied in fp32."""
    x = x.detach().cpu().float()
    B, C, H, W = x.shape
    cg = C // groups
    t = torch.zeros(C, dtype=torch.float64) if bias is None else bias.detach().cpu().double()
    x64 = x.double() + t.view(1, C, 1, 1)
    grouped = x64.reshape(B, groups, cg * H * W)
    mean = grouped.mean(2)
    var = ((grouped - mean[:, :, None]) ** 2).mean(2)  # two-pass
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.detach().cpu().double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.detach().cpu().double()
    scale64 = ga.view(1, C) * rstd.repeat_interleave(cg, 1)
    shift64 = be.view(1, C) - (mean.repeat_interleave(cg, 1) - t.view(1, C)) * scale64
    want = x.double() * scale64.view(B, C, 1, 1) + shift64.view(B, C, 1, 1)
    scale32, shift32 = scale64.float(), shift64.float()
    e_ideal = float((apply32(x, scale32, shift32).double() - want).abs().max())
    return Ref(want, scale64, shift64, scale32, shift32, e_ideal)


@functools.lru_cache(maxsize=None)
def case_reference(case, shape, groups):
    """reference() of make(case, shape, groups): computed once per process and shared among the tests that need it."""
    x, gamma, beta, bias = make(case, shape, groups)
    return reference(x, groups, EPS, gamma, beta, bias)


def figures(x, scale, shift, ref):
    """(worst |scale - scale64| / |scale64|, max|x * scale + shift - want|, its bound); non-finite figures come out as inf."""
    x = x.detach().cpu().float()
    B, C = x.shape[:2]
    scale, shift = scale.detach().cpu().float().reshape(B, C), shift.detach().cpu().float().reshape(B, C)
    denom = ref.scale64.abs().clamp_min(1e-300)
    rel = float(((scale.double() - ref.scale64).abs() / denom).max())
    err = float((apply32(x, scale, shift).double() - ref.want).abs().max())
    if not bool(torch.isfinite(scale).all() and torch.isfinite(shift).all()):
        rel = err = float("inf")
    return rel, err, OUT_FACTOR * ref.e_ideal + OUT_FLOOR


def violations(x, scale, shift, ref, test=None, what=""):
    """The two conditions, recorded through util.record_margin when `test` is given; a list of what is exceeded (empty: fine)."""
    rel, err, bound = figures(x, scale, shift, ref)
    if test is not None:
        util.record_margin(test, what + " scale rel", rel, SCALE_RTOL)
        util.record_margin(test, what + " out", err, bound)
    bad = []
    if not rel <= SCALE_RTOL:
        bad.append("%s: |scale - scale64| / |scale64| = %.3e > %.1e" % (what, rel, SCALE_RTOL))
    if not err <= bound:
        bad.append("%s: max|x * scale + shift - want| = %.3e > %.3e (E_ideal %.3e)" % (what, err, bound, ref.e_ideal))
    return bad


def check(x, scale, shift, ref, test=None, what=""):
    bad = violations(x, scale, shift, ref, test, what)
    assert not bad, "\n".join(bad)


# ---- emulations ---------------------------------------------------------------------------------------------------------------
def _finish(mean, var, eps, gamma, beta, t, cg):
    """fp64 (mean, var) [B,groups] -> fp32 (scale, shift) [B,C] the way the kernels' finishers round them."""
    rstd = 1.0 / np.sqrt(np.maximum(var, 0.0) + eps)
    scale64 = gamma[None, :] * np.repeat(rstd, cg, 1)
    shift64 = beta[None, :] - (np.repeat(mean, cg, 1) - t[None, :]) * scale64
    return torch.from_numpy(scale64.astype(np.float32)), torch.from_numpy(shift64.astype(np.float32))


def _prep(x, groups, gamma, beta, bias):
    B, C, H, W = x.shape
    xp = x.detach().cpu().float().permute(0, 2, 3, 1).reshape(B, H * W, C).numpy()  # [B, pixel, channel]
    ga = np.ones(C) if gamma is None else gamma.double().numpy()
    be = np.zeros(C) if beta is None else beta.double().numpy()
    t32 = np.zeros(C, np.float32) if bias is None else bias.float().numpy()
    return xp, ga, be, t32, C // groups


def _sliced_sums(v, groups):
    """fp32 (sum, sum of squares) of v [B, pixel, C] per group over slices of SLICE pixels, the slices added in fp64."""
    B, HW, C = v.shape
    cg = C // groups
    s, ss = np.zeros((B, groups)), np.zeros((B, groups))
    for lo in range(0, HW, SLICE):
        blk = v[:, lo:lo + SLICE].reshape(B, -1, groups, cg).transpose(0, 2, 1, 3).reshape(B, groups, -1)
        s += np.sum(blk, axis=2, dtype=np.float32).astype(np.float64)
        ss += np.sum(blk * blk, axis=2, dtype=np.float32).astype(np.float64)
    return s, ss, float(HW * cg)


def emulate_naive(x, groups, eps, gamma, beta, bias):
    xp, ga, be, t32, cg = _prep(x, groups, gamma, beta, bias)
    s, ss, n = _sliced_sums(xp + t32[None, None, :], groups)
    mean = s / n
    return _finish(mean, ss / n - mean * mean, eps, ga, be, t32.astype(np.float64), cg)


def emulate_pivot(x, groups, eps, gamma, beta, bias):
    xp, ga, be, t32, cg = _prep(x, groups, gamma, beta, bias)
    kx = np.repeat(xp[:, 0, ::cg], cg, 1)          # [B, C]: the group's first element
    kb = np.repeat(t32[::cg], cg)                  # [C]: the bias of the group's first channel
    v = (xp - kx[:, None, :]) + (t32 - kb)[None, None, :]
    s, ss, n = _sliced_sums(v, groups)
    mean = kx[:, ::cg].astype(np.float64) + kb[::cg].astype(np.float64)[None, :] + s / n
    return _finish(mean, ss / n - (s / n) ** 2, eps, ga, be, t32.astype(np.float64), cg)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def emulate_pairs(x, groups, eps, gamma, beta, bias):
    xp, ga, be, t32, cg = _prep(x, groups, gamma, beta, bias)
    B, HW, C = xp.shape
    a1, a2 = np.zeros((B, C)), np.zeros((B, C))
    for lo in range(0, HW, SLICE):
        sh = sl = qh = ql = np.zeros((B, C), np.float32)
        for p in range(lo, min(HW, lo + SLICE)):
            v = xp[:, p]
            sh, e = _two_sum(sh, v)
            sl = sl + e
            sq = v * v
            r = (v.astype(np.float64) * v.astype(np.float64) - sq.astype(np.float64)).astype(np.float32)  # fma(v, v, -sq): exact
            qh, e = _two_sum(qh, sq)
            ql = ql + (e + r)
        a1 += sh.astype(np.float64) + sl.astype(np.float64)
        a2 += qh.astype(np.float64) + ql.astype(np.float64)
    a1, a2 = a1 / HW, a2 / HW
    t = t32.astype(np.float64)
    a2 = a2 + 2.0 * t[None, :] * a1 + (t * t)[None, :]
    a1 = a1 + t[None, :]
    mean = a1.reshape(B, groups, cg).sum(2) / cg
    var = a2.reshape(B, groups, cg).sum(2) / cg - mean * mean
    return _finish(mean, var, eps, ga, be, t, cg)
