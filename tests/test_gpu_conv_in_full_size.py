"""The first-layer conv (csrc/conv_in.hip) at the size the networks run it, 1 x 3 x 256 x 256, for every supported width against
torch's conv: the 32- and 64-channel forms gave wrong pixels there, intermittently (profiles/conv_in_narrow_probe.txt), and the
smaller shapes of tests/test_gpu_channels_last.py never showed it.  Four launches per width: the fault was not in every launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("cout", (32, 64, 128))
def test_conv3x3_small_cin_at_256(cout):
    from sige_amd import hip

    torch.manual_seed(cout)
    x = torch.randn(1, 3, 256, 256, device=DEV).contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, 3, 3, 3, device=DEV) / 5
    b = torch.randn(cout, device=DEV)
    want = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), 1, 1).float()
    for rep in range(4):
        got = hip.conv3x3_small_cin_cl(x, w, b)
        assert got is not None
        bad = int(((got - want).abs() > 1e-5).sum())
        assert bad == 0, "launch %d: %d wrong elements, worst %.3g" % (rep, bad, float((got - want).abs().max()))
