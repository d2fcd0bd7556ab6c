"""CPU checks of tests/attention_stress.py: every regime has the property it is there for; the fp32 emulation of the kernels' blocked
online softmax stays inside the bound on every shape x regime of the GPU tests (unsplit and with two key splits); every mutant of it
falls out of the bound, or out of fp32, in some regime -- and the mutants that a consistent shift hides PASS the input every other
attention test of the suite draws (q * 2, k, v ~ randn): the gap the stress tests close, kept as an assertion."""
import pytest
import torch

from tests import attention_stress as A

SHAPE = (2, 48, 100, 2, 40)
ALL_SHAPES = A.TOKEN_SHAPES + A.WIDE_SHAPES
_sid = lambda s: "B%d_Nq%d_Nk%d_h%d_d%d" % s  # noqa: E731


def _scores(q, k, heads, d):
    """scale * q k^T per (batch, head) in fp64: [B*heads, Nq, Nk]."""
    qh, kh = A._heads(q, heads, torch.float64), A._heads(k, heads, torch.float64)
    return torch.bmm(qh, kh.transpose(1, 2)) * d ** -0.5


def _rest_max(q, k, heads, d):
    """The largest |score| the unsteered channels add (the N(0, ~1) part)."""
    q, k = q.clone(), k.clone()
    q[:, :, ::d] = 0
    k[:, :, ::d] = 0
    return float(_scores(q, k, heads, d).abs().max())


@pytest.mark.parametrize("shape", [SHAPE, (1, 32, 72, 1, 160), (1, 16, 5, 1, 512)], ids=_sid)
def test_every_regime_has_its_property(shape):
    B, Nq, Nk, heads, d = shape
    for regime, spike in A.regimes_for(Nk):
        q, k, v, want = A.case(B, Nq, Nk, heads, d, regime, spike)
        assert q.dtype == k.dtype == v.dtype == torch.float32 and want.dtype == torch.float64
        assert tuple(q.shape) == (B, Nq, heads * d) and tuple(k.shape) == tuple(v.shape) == (B, Nk, heads * d)
        S = _scores(q, k, heads, d)
        noise = _rest_max(q, k, heads, d) if regime != "flat" else 0.0
        assert noise < 8  # (the rest is N(0, ~1): the steering channel decides)
        if regime == "offset+":  # exp(S) overflows fp32 (above 88.8) for every key
            assert S.min() > 290 and S.max() < 310
        elif regime == "offset-":  # exp(S) is 0 in fp32 (below -104) for every key: a maximum of 0 leaves no mass
            assert S.max() < -290 and S.min() > -310
        elif regime == "rows":
            # the steering alone puts the row maxima of a tile exactly 600 apart; the rest moves each by less than `noise`
            c, _ = A.steering("rows", Nq, Nk)
            assert float(c[:16].max() - c[:16].min()) == 600.0
            rmax = S.max(dim=2).values.reshape(-1, Nq // 16, 16)
            spread = rmax.max(dim=2).values - rmax.min(dim=2).values
            assert float(spread.min()) >= 600 - 2 * noise and float(spread.min()) > 590
            # ... and inside a row the scores stay a softmax's width apart: the row maximum matters, not the key
            assert float((S.max(dim=2).values - S.min(dim=2).values).max()) <= 2 * noise
        elif regime == "ramp":
            rows = S.reshape(-1, Nq // 16, 16, Nk)
            up, down = rows[:, :, 15], rows[:, :, 0]  # c = +300 and c = -300 in every tile
            assert float((up[..., -1] - up[..., 0]).min()) > 280 and float((down[..., 0] - down[..., -1]).min()) > 280
            if Nk >= 32:  # the rising rows peak in the last key block (they rescale at every block), the falling ones in the first
                assert bool((up.argmax(dim=-1) // 16 == (Nk - 1) // 16).all()) and bool((down.argmax(dim=-1) // 16 == 0).all())
        elif regime == "spike":
            assert bool((S.argmax(dim=2) == spike).all())
            others = S.clone()
            others[:, :, spike] = float("-inf")
            assert float((S[:, :, spike] - others.max(dim=2).values).min()) > 180 or Nk == 1
            assert float((want - v[:, spike:spike + 1].double()).abs().max()) <= 1e-12  # out = v[j*]
        else:  # flat
            assert not S.any() and not q.any()
            assert float((v.mean() - 100).abs()) < 1
            assert float((want - v.double().mean(dim=1, keepdim=True)).abs().max()) <= 1e-10


def test_spike_positions():
    assert A.spikes(100) == [0, 15, 16, 37, 58, 99]
    assert A.spikes(5) == [0, 4] and A.spikes(1) == [0] and A.spikes(40) == [0, 15, 16, 37, 39]
    assert A.spikes(272, qkv=True) == [0, 15, 16, 37, 58, 63, 64, 255, 256, 271]
    assert A.spikes(16, qkv=True) == [0, 15]


def test_qkv_layout_is_the_token_layout_transposed():
    B, C, H, W = 2, 64, 4, 4
    q, k, v = A.make(B, H * W, H * W, 1, C, "ramp", layout="qkv")
    assert tuple(q.shape) == (B, C, H * W) and q.is_contiguous()
    img = A.qkv_image(q, k, v, H, W)
    assert tuple(img.shape) == (B, 3 * C, H, W)
    c, b = A.steering("ramp", H * W, H * W)
    assert torch.equal(img[:, 0].reshape(B, -1), (c * C ** 0.5).float().expand(B, -1))      # q third, channel 0, pixel i
    assert torch.equal(img[:, C].reshape(B, -1), b.float().expand(B, -1))                   # k third, channel 0, pixel j
    tq, tk, tv, want = A.case(B, H * W, H * W, 1, C, "ramp", None, "qkv")
    assert torch.equal(tq, A.tokens_of(q)) and torch.equal(A.tokens_of(img[:, 2 * C:]), tv)
    assert tuple(want.shape) == (B, H * W, C)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_online_softmax_is_finite_and_within_the_bound(shape):
    """The correct algorithm in fp32, four waves, unsplit and with the key blocks in two split ranges: every regime (`flat` and the
    one-key shapes included) inside max(4 * e32, 2e-5 * (1 + max|want|)), e32 from the fp32 chain on the CPU."""
    B, Nq, Nk, heads, d = shape
    worst = 0.0
    for regime, spike in A.regimes_for(Nk):
        q, k, v, want = A.case(B, Nq, Nk, heads, d, regime, spike)
        e32 = float((A.chain(q, k, v, heads, d ** -0.5, torch.float32).double() - want).abs().max())
        tol = A.bound(want, e32)
        for splits in (1, 2):
            got = A.online_softmax(q, k, v, heads, d ** -0.5, splits=splits)
            assert bool(torch.isfinite(got).all()), (A.regime_id(regime, spike), splits)
            err = float((got.double() - want).abs().max())
            worst = max(worst, err / tol)
            assert err <= tol, "%s splits=%d: err %.3e > bound %.3e (fp32 chain %.3e)" % (A.regime_id(regime, spike), splits, err, tol, e32)
    print("%s: worst err / bound = %.3f" % (_sid(shape), worst))


def _verdict(q, k, v, heads, d, mutant):
    """(ok, err / bound) of a mutant on one input; ok = finite and within the bound, for both split counts."""
    want = A.chain(q, k, v, heads, d ** -0.5, torch.float64)
    tol = A.bound(want, float((A.chain(q, k, v, heads, d ** -0.5, torch.float32).double() - want).abs().max()))
    worst = 0.0
    for splits in (1, 2):
        got = A.online_softmax(q, k, v, heads, d ** -0.5, mutant=mutant, splits=splits)
        if not bool(torch.isfinite(got).all()):
            return False, float("inf")
        worst = max(worst, float((got.double() - want).abs().max()) / tol)
    return worst <= 1.0, worst


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_mutant_fails_a_regime(mutant):
    B, Nq, Nk, heads, d = SHAPE
    failed = []
    for regime, spike in A.regimes_for(Nk):
        q, k, v, _ = A.case(B, Nq, Nk, heads, d, regime, spike)
        if not _verdict(q, k, v, heads, d, mutant)[0]:
            failed.append(A.regime_id(regime, spike))
    print("%s fails: %s" % (mutant, ", ".join(failed)))
    assert failed, "no regime sees the mutant %s" % mutant


def _suite_input(B, Nq, Nk, heads, d):
    """What test_attention_tokens_vs_fp64 and test_attention_wide_vs_fp64 draw."""
    g = torch.Generator().manual_seed(Nq + Nk + d)
    q, k, v = (torch.randn(B, n, heads * d, generator=g) for n in (Nq, Nk, Nk))
    return q * 2.0, k, v


@pytest.mark.parametrize("mutant", ["nomax", "init0", "tilemax", "pad0"])
def test_the_suites_randn_input_does_not_see_these_mutants(mutant):
    """The gap: a kernel without a maximum, with one that starts at 0, with a tile-wide one, or with tail keys that enter the maximum
    as 0 passes the input of every other attention test.  (Do not simplify the stress inputs back to randn.)"""
    B, Nq, Nk, heads, d = SHAPE
    ok, ratio = _verdict(*_suite_input(B, Nq, Nk, heads, d), heads, d, mutant)
    print("%s on q * 2, k, v ~ randn: err / bound = %.3f" % (mutant, ratio))
    assert ok, "%s is out of bound on randn input (err / bound = %.3f): the statement of the gap no longer holds" % (mutant, ratio)
