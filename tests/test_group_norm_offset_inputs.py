"""The reference side of the GroupNorm-statistics tests on offset inputs (tests/group_norm_offsets.py) -- nothing here touches a
device.  The cases must be able to fail a wrong kernel: the emulation of one-pass fp32 sums (what group_norm.hip did before it
subtracted a pivot / carried fp32 pairs) exceeds the bounds on every case with ratio >= 30, the emulations of the two robust
schemes stay inside them on every case, and so does the ideal fp32 affine by construction.

Measured with these inputs, over SHAPES: naive |scale - scale64| / |scale64| 7e-6 ... 1e-4 at ratio 30, 1.7e-4 ... 1.1e-2 at
ratio 300, 4e-2 ... 1e3 at ratio 3000 (bound 4e-6); pivot <= 7.2e-7 and pairs <= 1.6e-7 on every case; the output error of the
pivot scheme reaches 0.8 of its bound 3 x E_ideal + 2e-6 (bias_r300 at (1, 512, 8, 8): 3.9e-6 of 5.0e-6), pairs stay at E_ideal.
The kernels themselves sit closer to E_ideal than the pivot emulation: they add the lanes' fp32 partials in fp64."""
import pytest
import torch

from tests import group_norm_offsets as G

# (shape, groups): the shapes of the GPU tests' direct and statistics routes
SHAPES = [((2, 64, 17, 23), 16), ((1, 32, 64, 64), 4), ((1, 128, 8, 8), 32), ((1, 128, 32, 32), 32), ((1, 512, 8, 8), 32),
          ((1, 16, 8, 8), 4), ((2, 384, 24, 40), 32), ((1, 36, 10, 6), 4)]
EMULATIONS = {"naive": G.emulate_naive, "pivot": G.emulate_pivot, "pairs": G.emulate_pairs}


def _id(v):
    return v.name if isinstance(v, G.Case) else "x".join(str(d) for d in v[0]) + "g%d" % v[1]


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case, shape, groups):
        key = (case, shape, groups)
        if key not in cache:
            x, gamma, beta, bias = G.make(case, shape, groups)
            cache[key] = G.reference(x, groups, G.EPS, gamma, beta, bias)
        return cache[key]

    return get


def test_case_table_holds_what_it_promises():
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names) and {c.ratio for c in G.CASES} >= {0, 30, 300, 3000}
    for case in G.X_CASES:
        if case.ratio == 0:
            continue
        m, s, special = G.group_table(case, 8)
        assert (m > 0).any() and (m < 0).any() and len(set(m.tolist())) >= 4          # both signs, group by group different
        assert any(m[g] == 0 and m[g + 1] != 0 for g in range(7))                    # no offset next to an offset
        if case.name == "edge":
            assert special[0] == "const" and special[1] == "near"
        else:
            assert set(s.tolist()) == {1.0, 1e-2}
            assert all(abs(m[g]) / s[g] == pytest.approx(case.ratio) for g in range(8) if m[g] != 0)
    x, _, _, bias = G.make(G.CASES[4], (1, 16, 8, 8), 4)
    assert bias is None and bool((x[:, 0:4] == 3.0).all()) and abs(float(x[:, 4:8].var()) - 1e-6) < 3e-7
    x, _, _, bias = G.make(G.CASES[-1], (1, 16, 8, 8), 4)
    assert float(x.abs().max()) < 10 and len(set(bias[4:8].tolist())) == 2             # one group's channels at two biases


@pytest.mark.parametrize("shape_groups", SHAPES, ids=_id)
@pytest.mark.parametrize("case", G.CASES, ids=_id)
def test_reference_and_robust_emulations_hold_and_naive_sums_fail(refs, case, shape_groups):
    shape, groups = shape_groups
    x, gamma, beta, bias = G.make(case, shape, groups)
    ref = refs(case, shape, groups)
    # the reference against torch's own GroupNorm in fp64
    t = 0.0 if bias is None else bias.double().view(1, -1, 1, 1)
    torch_want = torch.nn.functional.group_norm(x.double() + t, groups, gamma.double(), beta.double(), G.EPS)
    assert float((ref.want - torch_want).abs().max()) <= 1e-9 * (1.0 + float(torch_want.abs().max()))
    # the ideal fp32 affine: inside both bounds by construction
    rel, err, bound = G.figures(x, ref.scale32, ref.shift32, ref)
    assert rel <= 6e-8 and err == ref.e_ideal and err <= bound
    out = {}
    for name, fn in EMULATIONS.items():
        scale, shift = fn(x, groups, G.EPS, gamma, beta, bias)
        out[name] = (G.figures(x, scale, shift, ref), G.violations(x, scale, shift, ref, None, name))
    print("%s %s g%d: E_ideal %.2e; " % (case.name, shape, groups, ref.e_ideal)
          + "; ".join("%s scale %.2e out %.2e" % (k, v[0][0], v[0][1]) for k, v in out.items()))
    assert not out["pivot"][1], out["pivot"][1]
    assert not out["pairs"][1], out["pairs"][1]
    if case.ratio >= 30:
        assert out["naive"][1], "one-pass fp32 sums pass %s at %s" % (case.name, shape)
    else:
        assert not out["naive"][1]


def test_constant_group_gets_gamma_over_sqrt_eps(refs):
    case, shape, groups = G.CASES[4], (1, 16, 8, 8), 4
    _, gamma, _, _ = G.make(case, shape, groups)
    ref = refs(case, shape, groups)
    torch.testing.assert_close(ref.scale64[0, :4], gamma[:4].double() / G.EPS ** 0.5, rtol=1e-12, atol=0)
