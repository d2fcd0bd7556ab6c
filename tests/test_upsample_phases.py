"""Nearest x2 + 3x3 conv as four 2x2 phase convs on the half-resolution tensor, on the CPU: the derived kernels
against the 9-tap definition in fp64, borders included, and the derivation cache of SIGEConv2d."""
import pytest
import torch
import torch.nn.functional as F


def phase_conv(x, wp, bias):
    """The four phase convs of `wp` [4,Cout,Cin,2,2] on the low-res `x`, interleaved into the upsampled output: phase (a, b) reads
    low-res rows {y - 1 + a, y + a} and columns {x - 1 + b, x + b}; what falls outside the image is zero."""
    B, _, H, W = x.shape
    out = x.new_empty(B, wp.shape[1], 2 * H, 2 * W)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in (0, 1):
        for b in (0, 1):
            o = F.conv2d(xp, wp[2 * a + b], bias)  # [B,Cout,H+1,W+1]: entry (y, x) starts at low-res (y - 1, x - 1)
            out[:, :, a::2, b::2] = o[:, :, a:a + H, b:b + W]
    return out


@pytest.mark.parametrize("res", [(1, 1), (2, 3), (6, 5)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_phase_kernels_equal_the_nine_tap_definition_in_fp64(res, with_bias):
    from sige_amd import hip

    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, *res, generator=gen, dtype=torch.float64)
    w = torch.randn(7, 5, 3, 3, generator=gen, dtype=torch.float64)
    bias = torch.randn(7, generator=gen, dtype=torch.float64) if with_bias else None
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)
    wp = hip.upsample_phase_kernels(w)
    assert wp.shape == (4, 7, 5, 2, 2) and wp.dtype == torch.float64 and wp.is_contiguous()
    got = phase_conv(x, wp, bias)
    # 9 products against 4 products of tap sums, all in fp64: a few ulp of the largest partial sum
    assert float((got - want).abs().max()) <= 1e-13 * (1.0 + float(want.abs().max()))


def test_phase_kernels_are_rounded_once():
    """fp32 weights: every phase entry is the fp64 sum of its taps rounded to fp32 once, and the four phases together hold every
    tap exactly once per (row phase, column phase)."""
    from sige_amd import hip

    w = torch.randn(3, 4, 3, 3, generator=torch.Generator().manual_seed(5))
    wp = hip.upsample_phase_kernels(w)
    assert wp.dtype == torch.float32
    d = w.double()
    # phase (0, 0): rows (w0, w1 + w2), columns (w0, w1 + w2)
    want00 = torch.stack([torch.stack([d[:, :, 0, 0], d[:, :, 0, 1] + d[:, :, 0, 2]], -1),
                          torch.stack([d[:, :, 1, 0] + d[:, :, 2, 0], d[:, :, 1:, 1:].sum((2, 3))], -1)], 2)
    assert torch.equal(wp[0], want00.float())
    # phase (1, 1): rows (w0 + w1, w2), columns (w0 + w1, w2)
    want11 = torch.stack([torch.stack([d[:, :, :2, :2].sum((2, 3)), d[:, :, 0, 2] + d[:, :, 1, 2]], -1),
                          torch.stack([d[:, :, 2, 0] + d[:, :, 2, 1], d[:, :, 2, 2]], -1)], 2)
    assert torch.equal(wp[3], want11.float())
    for k in range(4):
        assert float((wp[k].double().sum((2, 3)) - d.sum((2, 3))).abs().max()) <= 4e-7 * float(d.abs().sum((2, 3)).max())
    with pytest.raises(ValueError):
        hip.upsample_phase_kernels(torch.zeros(3, 4, 1, 1))


def test_derivation_cache_follows_the_weight_and_stays_out_of_the_state_dict():
    from sige_amd.nn.base import SIGEConv2d

    torch.manual_seed(0)
    conv = SIGEConv2d(4, 6, 3, padding=1)
    keys = set(conv.state_dict())
    wp = conv.phase_kernels()
    assert wp.shape == (4, 6, 4, 2, 2)
    assert conv.phase_kernels() is wp                      # same weight, same version: not derived again
    assert set(conv.state_dict()) == keys == {"weight", "bias"}
    assert not any(t is wp for t in list(conv.buffers()) + list(conv.parameters()))
    with torch.no_grad():
        conv.weight.mul_(2.0)                              # in place: the version moves, the address does not
    wp2 = conv.phase_kernels()
    assert wp2 is not wp and torch.equal(wp2, wp * 2.0)    # (a power of two: exact)
    conv.clear_cache()
    assert conv._phase is None
    wp3 = conv.phase_kernels()
    assert wp3 is not wp2 and torch.equal(wp3, wp2)
    conv.rebuild_derived_caches()
    assert conv._phase is None                             # (nothing was packed: derived again on demand)
    fresh = SIGEConv2d(4, 6, 3, padding=1)
    fresh.load_state_dict(conv.state_dict())
    assert torch.equal(fresh.phase_kernels(), wp3)


def test_only_the_plain_padded_3x3_conv_has_phase_kernels():
    from sige_amd.nn.base import SIGEConv2d

    assert SIGEConv2d(4, 4, 1).phase_kernels() is None
    assert SIGEConv2d(4, 4, 3, stride=2, padding=1).phase_kernels() is None
    assert SIGEConv2d(4, 4, 3, padding=0).phase_kernels() is None
    assert SIGEConv2d(4, 4, 3, padding=1, groups=2).phase_kernels() is None
    conv = SIGEConv2d(4, 4, 3, padding=1)
    conv.compute_dtype = "f16"
    assert conv.phase_kernels() is None
    conv.compute_dtype = "f32"
    assert conv.phase_kernels() is not None


def test_gather_carries_the_flag():
    from sige_amd.nn import Gather

    assert Gather.PHASE_UPSAMPLE in (True, False)
