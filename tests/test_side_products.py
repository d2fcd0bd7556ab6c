"""conv1 of an up block split at its torch.cat (ResBlock.split_conv1): the two derived convs add up to conv1, for
an even and an uneven split, in fp64 on the CPU; they follow an in-place weight edit after clear_cache()."""
import pytest
import torch
from torch.nn import functional as F


def _block(ch_h, ch_s, cout=24):
    from sige_amd.workloads.ddpm_unet import DDPMConfig, ResBlock

    torch.manual_seed(ch_h + ch_s)
    return ResBlock(DDPMConfig(groups=8), ch_h + ch_s, cout, sparse=False).double().eval()


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("ch_h,ch_s", [(32, 32), (32, 16)])
def test_split_conv1_sums_to_conv1(ch_h, ch_s):
    block = _block(ch_h, ch_s)
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(1, ch_h, 9, 7, generator=gen, dtype=torch.float64)
    b = torch.randn(1, ch_s, 9, 7, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        want = block.conv1(torch.cat([a, b], 1))
        conv_h, conv_s = block.split_conv1(ch_h)
        assert conv_s.bias is None and tuple(conv_h.weight.shape) == (24, ch_h, 3, 3) and tuple(conv_s.weight.shape) == (24, ch_s, 3, 3)
        got = F.conv2d(a, conv_h.weight, conv_h.bias, 1, 1) + F.conv2d(b, conv_s.weight, None, 1, 1)
    assert _rel(got, want) <= 1e-12, _rel(got, want)
    # derived objects: the state dict keeps the reference's keys, and a second call returns the same convs
    assert not any("split" in k for k in block.state_dict())
    assert block.split_conv1(ch_h)[0] is conv_h and block.split_conv1(ch_h)[1] is conv_s


def test_split_conv1_follows_a_weight_edit_after_clear_cache():
    block = _block(32, 16)
    a, b = torch.randn(1, 32, 5, 5, dtype=torch.float64), torch.randn(1, 16, 5, 5, dtype=torch.float64)
    conv_h, conv_s = block.split_conv1(32)
    with torch.no_grad():
        block.conv1.weight.data.mul_(-0.5)  # (through .data: no version counter moves)
        block.conv1.bias.data.add_(1.0)
        block.clear_cache()
        new_h, new_s = block.split_conv1(32)
        assert new_h is not conv_h and new_s is not conv_s
        want = block.conv1(torch.cat([a, b], 1))
        got = F.conv2d(a, new_h.weight, new_h.bias, 1, 1) + F.conv2d(b, new_s.weight, None, 1, 1)
    assert _rel(got, want) <= 1e-12
    # an edit that moves the version counter needs no clear_cache()
    with torch.no_grad():
        block.conv1.weight.mul_(2.0)
    assert block.split_conv1(32)[0] is not new_h
