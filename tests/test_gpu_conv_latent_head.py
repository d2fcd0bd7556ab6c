"""sige_hip_conv3x3_latent_head_nhwc_f32 (sige_amd.hip.conv3x3_latent_head_cl) alone: conv3x3_pad1(act(scale * x + shift)) + bias
for 5..16 output channels, against torch in fp64 on the CPU (F.conv2d of the activated, zero-padded input), and its posterior
epilogue against the fp64 formula.

Tolerances.  Moments: util.CONV_ATOL absolute on O(1) outputs (x ~ N(0,1), weights ~ N(0,1) / sqrt(9 C)); what exact fp32 products
summed in fp32 need is ~1e-6 (measured 3.9e-7 ... 7.6e-7: profiles/conv_latent_head_test_margins.jsonl).  Posterior: z is compared
with the formula evaluated in fp64 on the kernel's OWN moments, so only the epilogue is measured: 1e-5 relative on the exp factor
plus 4 fp32 roundings (2.4e-7) of the sum's terms.  What is actually needed is the rounding term alone -- expf is within ~2 ulp =
2.4e-7 relative on the factor --: the measured worst error / tolerance was 0.38 ... 0.46, set by the cases' elements without a noise
term (same file)."""
import os
import sys

import pytest
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
EPS32 = 2.0 ** -24

# (B, C, H, W, Cout)
SHAPES = [
    (1, 64, 5, 7, 8),       # an image smaller than any tile, ragged in both directions; one chunk: no channel split
    (2, 192, 16, 16, 8),    # [B,C] scale / shift that differ between the images; C = 3 * 64; a 3-way channel split
    (1, 512, 20, 33, 8),    # full depth, edges no multiple of the 6x6 tile; an 8-way channel split of one chunk each
    (1, 128, 16, 16, 6),    # the Cout limits: 4 column blocks ...
    (1, 128, 16, 16, 16),   # ... and 9
]


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as _hip

    return _hip


def _case(B, C, H, W, Cout, affine, shift_value=None):
    g = torch.Generator().manual_seed(1000 * C + 10 * H + Cout)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    sc = sh = None
    if affine:
        sc = 1.0 + 0.3 * torch.randn(B, C, 1, 1, generator=g)  # (per batch: the two images of B = 2 get different affines)
        sh = 0.3 * torch.randn(B, C, 1, 1, generator=g)
        if shift_value is not None:
            sc, sh = sc * 0.05, sh * 0.05 + shift_value
    return x, w, b, sc, sh


def _reference(x, w, b, sc, sh, act):
    """fp64, CPU: zero padding of the ACTIVATED tensor."""
    a = x.double()
    if sc is not None:
        a = a * sc.double() + sh.double()
    if act == "swish":
        a = a * torch.sigmoid(a)
    return F.conv2d(a, w.double(), b.double(), padding=1)


def _run(hip, x, w, b, sc, sh, act, **kw):
    """The launch on NaN-poisoned destinations."""
    B, C, H, W = x.shape
    out = torch.full((B, w.shape[0], H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    got = hip.conv3x3_latent_head_cl(x.to(DEV).contiguous(memory_format=CL), dev(w), dev(b), dev(sc), dev(sh), act, out=out, **kw)
    return out, got


@pytest.mark.parametrize("mode", ["swish_affine", "identity_plain"])
@pytest.mark.parametrize("B,C,H,W,Cout", SHAPES)
def test_latent_head_vs_fp64(hip, B, C, H, W, Cout, mode):
    affine = mode == "swish_affine"
    act = "swish" if affine else "identity"
    x, w, b, sc, sh = _case(B, C, H, W, Cout, affine)
    out, got = _run(hip, x, w, b, sc, sh, act)
    assert got is out
    util.assert_finite(out, "latent head output over a poisoned buffer")
    want = _reference(x, w, b, sc, sh, act)
    err = float((out.cpu().double() - want).abs().max())
    print("latent head B=%d C=%d %dx%d Cout=%d %s: err %.3e (|out| max %.2f)" % (B, C, H, W, Cout, mode, err, float(want.abs().max())))
    util.record_margin("test_gpu_conv_latent_head vs fp64", "B=%d C=%d H=%d W=%d Cout=%d %s" % (B, C, H, W, Cout, mode), err, util.CONV_ATOL)
    assert float(want.abs().max()) > 0.5
    assert err <= util.CONV_ATOL


def test_latent_head_zero_padding_is_of_the_activated_tensor(hip):
    """shift = 1.3: act(shift) ~ 1.0 at every padded position if the padding leaked through the affine -- an error of the order of
    sum |w| over a border tap (~3) against a tolerance of 1e-3."""
    B, C, H, W, Cout = 1, 64, 5, 7, 8
    x, w, b, sc, sh = _case(B, C, H, W, Cout, True, shift_value=1.3)
    out, _ = _run(hip, x, w, b, sc, sh, "swish")
    want = _reference(x, w, b, sc, sh, "swish")
    leak = F.conv2d(F.silu(F.pad(x.double() * sc.double() + sh.double(), (1, 1, 1, 1), value=1.3)), w.double(), b.double())
    assert float((leak - want).abs().max()) > 100 * util.CONV_ATOL  # (the case can see a leak)
    err = float((out.cpu().double() - want).abs().max())
    util.record_margin("test_gpu_conv_latent_head padding", "shift 1.3", err, util.CONV_ATOL)
    assert err <= util.CONV_ATOL


@pytest.mark.parametrize("B,C,H,W,Cout", [SHAPES[0], SHAPES[1]])
@pytest.mark.parametrize("with_noise", [True, False])
def test_latent_head_posterior_epilogue(hip, B, C, H, W, Cout, with_noise):
    """z = latent_scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise); the first logvar plane is scaled to cross both clamp
    bounds.  noise=None: the mode."""
    Z, ls = Cout // 2, 0.18215
    x, w, b, sc, sh = _case(B, C, H, W, Cout, True)
    w[Z] *= 60.0
    g = torch.Generator().manual_seed(7)
    noise = torch.randn(B, Z, H, W, generator=g) if with_noise else None
    zbuf = torch.full((B, Z, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    out, got = _run(hip, x, w, b, sc, sh, "swish", noise=None if noise is None else noise.to(DEV).contiguous(memory_format=CL),
                    latent_scale=ls, z_out=zbuf)
    assert got[0] is out and got[1] is zbuf
    util.assert_finite(out, "moments")
    util.assert_finite(zbuf, "z")
    want = _reference(x, w, b, sc, sh, "swish")
    assert float(want[:, Z].min()) < -30.0 and float(want[:, Z].max()) > 20.0
    merr = float((out.cpu().double() - want).abs().max())
    util.record_margin("test_gpu_conv_latent_head posterior moments", "C=%d noise=%d" % (C, with_noise), merr, util.CONV_ATOL)
    assert merr <= util.CONV_ATOL
    m = out.cpu().double()
    mean, std = m[:, :Z], torch.exp(0.5 * m[:, Z:].clamp(-30.0, 20.0))
    eps = torch.zeros_like(mean) if noise is None else noise.double()
    want_z = ls * (mean + std * eps)
    tol = ls * (1e-5 * std * eps.abs() + 4 * EPS32 * (mean.abs() + std * eps.abs())) + 1e-30
    ratio = float(((zbuf.cpu().double() - want_z).abs() / tol).max())
    print("latent head posterior C=%d noise=%d: worst |z - fp64| / tolerance %.3f" % (C, with_noise, ratio))
    util.record_margin("test_gpu_conv_latent_head posterior z", "C=%d noise=%d" % (C, with_noise), ratio, 1.0)
    assert ratio <= 1.0


def test_latent_head_refuses_unsupported_shapes_without_a_launch(hip):
    def call(C, Cout, noise=False):
        x, w, b, _, _ = _case(1, C, 8, 8, Cout, False)
        kw = dict(noise=torch.randn(1, Cout // 2, 8, 8, device=DEV).contiguous(memory_format=CL), latent_scale=1.0) if noise else {}
        return hip.conv3x3_latent_head_cl(x.to(DEV).contiguous(memory_format=CL), w.to(DEV), b.to(DEV), None, None, "swish", **kw)

    assert call(64, 8) is not None
    torch.cuda.synchronize()
    before = hip.launch_count()
    assert call(64, 4) is None      # (conv3x3_small_cout_cl's range)
    assert call(64, 17) is None
    assert call(96, 8) is None      # C % 64
    assert call(576, 8) is None     # C > 512
    assert call(64, 7, noise=True) is None  # odd Cout with the posterior
    assert hip.launch_count() == before
    assert call(64, 7) is not None and hip.launch_count() == before + 1  # (ONE launch)
    # the existing entry keeps its range
    x, w, b, _, _ = _case(1, 64, 8, 8, 8, False)
    assert hip.conv3x3_small_cout_cl(x.to(DEV).contiguous(memory_format=CL), w.to(DEV), b.to(DEV)) is None


@pytest.mark.parametrize("B,C,H,W,Cout", [SHAPES[1], SHAPES[2]])
def test_latent_head_is_bit_identical_from_run_to_run(hip, B, C, H, W, Cout):
    """The channel split adds its slices in split order inside the launch: two calls on equal inputs are torch.equal."""
    x, w, b, sc, sh = _case(B, C, H, W, Cout, True)
    first, _ = _run(hip, x, w, b, sc, sh, "swish")
    for _ in range(3):
        again, _ = _run(hip, x, w, b, sc, sh, "swish")
        assert torch.equal(first, again)
