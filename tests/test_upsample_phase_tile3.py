"""The Upsample phase convs on the tile conv v3, on the CPU: the switch is off, the derived pack exists only for
what the kernel covers, and it leaves the phase-kernel cache of tests/test_upsample_phases.py alone."""
import pytest
import torch


def test_the_switch_is_off():
    from sige_amd.nn import Gather

    assert Gather.PHASE_UPSAMPLE_TILE3 is False


def test_only_a_plain_3x3_conv_of_64_channel_multiples_on_a_gpu_has_the_pack():
    from sige_amd.nn.base import SIGEConv2d

    assert SIGEConv2d(64, 64, 3, padding=1).phase_tile3_packed() is None            # CPU weights
    for conv in (SIGEConv2d(64, 64, 1), SIGEConv2d(64, 64, 3, stride=2, padding=1), SIGEConv2d(64, 64, 3, padding=0),
                 SIGEConv2d(64, 64, 3, padding=1, groups=2), SIGEConv2d(48, 64, 3, padding=1), SIGEConv2d(64, 48, 3, padding=1)):
        assert conv.phase_tile3_packed() is None and conv._phase3 is None
    conv = SIGEConv2d(64, 64, 3, padding=1)
    conv.compute_dtype = "f16x3"
    assert conv.phase_tile3_packed() is None
    # (the same refusals on GPU weights, where the shape decides: tests/test_gpu_upsample_phase_tile3.py)


def test_never_packed_leaves_the_phase_cache_as_it_was():
    from sige_amd.nn.base import SIGEConv2d

    torch.manual_seed(0)
    conv = SIGEConv2d(4, 6, 3, padding=1)
    keys = set(conv.state_dict())
    assert conv.phase_tile3_packed() is None and conv._phase3 is None
    wp = conv.phase_kernels()
    assert conv.phase_kernels() is wp and conv._phase[2] is None
    assert set(conv.state_dict()) == keys == {"weight", "bias"}
    conv.rebuild_derived_caches()
    assert conv._phase is None and conv._phase3 is None      # (nothing was packed: derived again on demand)
    wp2 = conv.phase_kernels()
    assert wp2 is not wp and torch.equal(wp2, wp)
    conv.clear_cache()
    assert conv._phase is None and conv._phase3 is None
    assert set(conv.state_dict()) == keys
    assert not any(n.startswith("_phase") for n, _ in list(conv.named_buffers()) + list(conv.named_parameters()))


def test_pack_refuses_a_weight_that_is_not_3x3():
    from sige_amd import hip

    with pytest.raises(ValueError):
        hip.upsample_phase_tile3_pack(torch.zeros(64, 64, 1, 1))
    with pytest.raises(ValueError):
        hip.upsample_phase_tile3_pack(torch.zeros(64, 64, 3, 3), compute="f16x3")
    assert isinstance(hip.PHASE_TILE3_MIN_BLOCKS, int) and hip.PHASE_TILE3_MIN_BLOCKS > 0
