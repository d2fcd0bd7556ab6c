"""GroupNorm statistics on OFFSET inputs: every route of sige_amd/csrc/group_norm.hip (NCHW, channels-last with and without
channel_bias, per-block statistics from hip.channel_stats_cl and from the dense-layer conv's epilogue) against the fp64
GroupNorm, on groups whose mean is up to 3000 times their spread (tests/group_norm_offsets.py: the cases, the reference and the
two bounds; tests/test_group_norm_offset_inputs.py shows on the CPU that one-pass fp32 sums fail every case with ratio >= 30).

Every test walks the case table for one shape and reports ALL cases that exceed a bound; the worst figure per case is recorded
through util.record_margin (profiles/group_norm_offsets_test_margins.jsonl)."""
import pytest
import torch

from tests import group_norm_offsets as G

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]  # (row a9: the reference computes it with torch's GroupNorm; fp64 here)
DEV = torch.device("cuda")
CL = torch.channels_last


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _d(t):
    return None if t is None else t.to(DEV)


def _walk(test, cases, shape, groups, route):
    """route(x, gamma, beta, bias) -> (scale, shift) for every case of `cases` at `shape`; all violations, not the first."""
    bad = []
    for case in cases:
        x, gamma, beta, bias = G.make(case, shape, groups)
        r = route(x, _d(gamma), _d(beta), _d(bias))
        assert r is not None, "%s: no kernel for %s" % (test, shape)
        torch.cuda.synchronize()
        bad += G.violations(x, r[0], r[1], G.case_reference(case, shape, groups), test, "%s %s" % (case.name, "x".join(map(str, shape))))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape,groups", [
    ((2, 64, 17, 23), 16),   # groups not 16-byte aligned: the scalar path and the tail
    ((1, 32, 64, 64), 4),    # 2 splits per group
    ((1, 128, 8, 8), 32),    # one short slice
])
def test_group_norm_affine_nchw_on_offset_inputs(hip, shape, groups):
    _walk("test_group_norm_affine_nchw_on_offset_inputs", G.X_CASES, shape, groups,
          lambda x, ga, be, _: hip.group_norm_affine(x.to(DEV), groups, G.EPS, ga, be))


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "channel_bias"])
@pytest.mark.parametrize("shape,groups", [
    ((2, 64, 17, 23), 16),
    ((1, 128, 32, 32), 32),  # 8 splits
    ((1, 512, 8, 8), 32),    # 2 pixel lanes
    ((1, 16, 8, 8), 4),      # one quad per group, 64 pixel lanes
])
def test_group_norm_affine_cl_on_offset_inputs(hip, shape, groups, with_bias):
    _walk("test_group_norm_affine_cl_on_offset_inputs", G.BIAS_CASES if with_bias else G.X_CASES, shape, groups,
          lambda x, ga, be, cb: hip.group_norm_affine_cl(_cl(x), groups, G.EPS, ga, be, cb))


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "channel_bias"])
@pytest.mark.parametrize("shape,c2,groups", [
    ((1, 128, 32, 32), 0, 32),
    ((2, 256, 24, 40), 128, 32),  # groups of 12 straddling the two parts
    ((1, 36, 10, 6), 0, 4),       # ragged last pixel block
])
def test_channel_stats_route_on_offset_inputs(hip, shape, c2, groups, with_bias):
    """hip.channel_stats_cl -> hip.group_norm_affine_from_stats; with c2 the statistics of two tensors = the norm of their cat."""
    B, C1, H, W = shape

    def route(x, ga, be, cb):
        parts = [hip.channel_stats_cl(_cl(x[:, :C1]))] + ([hip.channel_stats_cl(_cl(x[:, C1:]))] if c2 else [])
        assert all(p is not None for p in parts)
        return hip.group_norm_affine_from_stats(parts, groups, G.EPS, ga, be, cb)

    _walk("test_channel_stats_route_on_offset_inputs", G.BIAS_CASES if with_bias else G.X_CASES, (B, C1 + c2, H, W), groups, route)


@pytest.mark.parametrize("compute", ["f16x3", "f32"])
@pytest.mark.parametrize("k,c1,c2,cout,H,W,B,res,up", [
    (3, 128, 0, 128, 16, 16, 1, True, False),     # a full-pass layer, no K split
    (3, 1024, 0, 512, 16, 16, 1, True, False),    # deep K: the statistics come from the workgroup that finishes the K split
    (3, 128, 128, 256, 40, 24, 2, False, False),  # cat input, batch 2, H not a multiple of 8 (partly empty pixel blocks)
    (1, 256, 256, 128, 32, 32, 1, False, False),  # 1x1
    (3, 128, 0, 64, 32, 32, 1, False, True),      # nearest x2 upsampling fused into the conv
])
def test_wide_conv_stats_route_on_offset_inputs(hip, compute, k, c1, c2, cout, H, W, B, res, up):
    """hip.wide_conv_cl(stats=True) -> hip.group_norm_affine_from_stats.  The offsets enter through the conv's bias and, where
    there is one, the residual (half each); the spread through the weight rows: the group means of the OUTPUT follow the case
    table.  Judged against the fp64 GroupNorm of the tensor the conv actually wrote."""
    test, groups = "test_wide_conv_stats_route_on_offset_inputs", 32
    bad = []
    for case in G.X_CASES:
        g = torch.Generator().manual_seed(100 * case.seed + 31 * k + cout + H)
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        m, s = G.channel_table(case, cout, groups)
        hs, ws = (H // 2, W // 2) if up else (H, W)
        x, x2 = _cl(r(B, c1, hs, ws)), (_cl(r(B, c2, hs, ws)) if c2 else None)
        w = r(cout, c1 + c2, k, k) / (k * (c1 + c2) ** 0.5) * s.view(-1, 1, 1, 1)
        bias = m * 0.5 if res else m
        residual = _cl(m.view(1, -1, 1, 1) * 0.5 + 0.5 * s.view(1, -1, 1, 1) * r(B, cout, H, W)) if res else None
        gamma, beta = r(cout), r(cout)
        packed = hip.wide_conv_pack_weights(w.to(DEV), compute)
        out = hip.wide_conv_cl(x, x2, None, None, "identity", packed, bias.to(DEV), cout, (k, k), residual=residual, upsample2x=up,
                               stats=True)
        st = hip.channel_stats(out)
        assert st is not None and st.channels == cout and st.count == H * W
        rr = hip.group_norm_affine_from_stats([st], groups, G.EPS, gamma.to(DEV), beta.to(DEV))
        assert rr is not None
        torch.cuda.synchronize()
        wrote = out.cpu().contiguous()
        # the output's groups are what the case says: offset / spread within a factor 2 of the table (constant groups: exact)
        grouped = wrote.double().reshape(B, groups, -1)
        mg, sg, special = G.group_table(case, groups)
        for gi in range(groups):
            if special[gi] == "const":
                assert bool((grouped[:, gi] == 3.0).all())
            elif mg[gi] != 0:
                ratio = float(grouped[:, gi].mean().abs() / grouped[:, gi].std())
                assert 0.5 * abs(mg[gi]) / sg[gi] <= ratio <= 2.0 * abs(mg[gi]) / sg[gi], (case.name, gi, ratio)
        ref = G.reference(wrote, groups, G.EPS, gamma, beta, None)
        bad += G.violations(wrote, rr[0], rr[1], ref, test, "%s %s k%d c%d+%d>%d %dx%d" % (case.name, compute, k, c1, c2, cout, H, W))
    assert not bad, "\n".join(bad)
