"""The first-layer conv (csrc/conv_in.hip, hip.conv3x3_small_cin_cl) at batch > 1 in launches of several hundred workgroups, against
the fp64 conv within 1e-5 (cases, references and checker: tests/conv_in_common.py; what the checker can see:
tests/test_conv_in_batch_inputs.py).  ONE launch at batch 8 (3 -> 64 channels, 128 x 128) once returned wrong pixels in some images
while every single-image launch was right, and the narrow forms left wrong dwords behind write-through stores at 1 x 3 x 256 x 256
(DESIGN.md 5.25, 5.27); neither cause was found, and the shapes of tests/test_gpu_channels_last.py (batch <= 2, at most 19 x 45) and
tests/test_gpu_conv_in_full_size.py (batch 1) cannot show either.  Here: the 5.25 launch itself, both narrow forms and the
write-through 128-channel form at batch 4 ... 8 on up to 2048 workgroups, ragged images whose boundaries fall inside the 32-pixel
blocks, one and two input channels, NCHW and batch-strided inputs, and the tile-list form on every 6x6 window of 128 x 128 and
256 x 256 images.

Every case allocates under util.poisoned() (NaN), asserts ONE library launch per call, launches four times (the faults were not in
every launch) and names the images that hold a wrong element.  Worst margins go through util.record_margin's file (kept as
profiles/conv_in_batch_test_margins.jsonl)."""
import pytest
import torch

from tests import conv_in_common as K
from tests import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CL = torch.channels_last
TEST = "test_gpu_conv_in_batch"
LAUNCHES = 4


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _launch(hip, call):
    n0 = hip.launch_count()
    out = call()
    n = hip.launch_count() - n0
    assert out is not None, "the launch was refused"
    assert n == 1, "expected 1 launch, counted %d" % n
    return out


def _input(c):
    """The case's input on the GPU with the strides it has on the CPU."""
    if c["layout"] == "strided":
        big = torch.zeros(2 * c["B"], c["C"], c["H"], c["W"], device=DEV).contiguous(memory_format=CL)
        big[1::2] = float("nan")  # (the images in between: reading one shows)
        x = big[::2]
        x.copy_(c["x"])
    elif c["layout"] == "nchw":
        x = c["x"].to(DEV).contiguous()
    else:
        x = c["x"].to(DEV).contiguous(memory_format=CL)
    assert x.stride() == c["x"].stride() or c["C"] == 1, (x.stride(), c["x"].stride())
    return x


@pytest.mark.parametrize("name", list(K.WHOLE))
def test_conv3x3_small_cin_whole_image_at_batch(hip, name):
    """The whole-image form.  The batch-strided input (big[::2], batch stride 2 C H W) reaches the kernel as it is:
    hip.conv3x3_small_cin_cl passes x.stride() on and copies nothing, so the kernel's own batch stride is what is tested; that case
    also runs without a bias."""
    c = K.case(name)
    worst_of_all = 0.0
    with util.poisoned():
        x, w, bias = _input(c), c["w"].to(DEV), c["bias"].to(DEV)
        runs = [("", bias, c["want"].to(DEV))]
        if "want_nobias" in c:
            runs.append((" without bias", None, c["want_nobias"].to(DEV)))
        for tag, b, want in runs:
            for rep in range(LAUNCHES):
                got = _launch(hip, lambda: hip.conv3x3_small_cin_cl(x, w, b))
                assert tuple(got.shape) == tuple(want.shape) and got.is_contiguous(memory_format=CL)
                n_bad, worst, images = K.check(got, want)
                print("%s%s launch %d: worst %.3g (bound %.3g)" % (name, tag, rep, worst, K.BOUND))
                assert n_bad == 0 and worst <= K.BOUND, K.message(name + tag, rep, n_bad, worst, images)
                worst_of_all = max(worst_of_all, worst)
    util.record_margin(TEST, "%s: worst |d| of %d launches, %d workgroups" % (name, LAUNCHES * len(runs), K.workgroups(name)),
                       worst_of_all, K.BOUND)


@pytest.mark.parametrize("name", list(K.TILES))
def test_conv3x3_small_cin_tile_list_at_batch(hip, name):
    """The tile-list form in place in a buffer of random data: inside the windows the fp64 conv within 1e-5, outside them the
    buffer's bits.  (The full list of overlapping windows covers the image, so here the second comparison is over no pixel; the
    lists with holes are those of tests/test_gpu_data_movement_ragged.py.)"""
    c = K.case(name)
    worst_of_all = 0.0
    with util.poisoned():
        x, w, bias = _input(c), c["w"].to(DEV), c["bias"].to(DEV)
        idx, inside, want, z = c["idx"].to(DEV), c["inside"].to(DEV), c["want"].to(DEV), c["z"].to(DEV)
        assert z.is_contiguous(memory_format=CL)
        for rep in range(LAUNCHES):
            buf = z.clone(memory_format=torch.preserve_format)
            assert K.check(buf, want, c["inside"])[0] > 0.99 * want.numel()  # (the buffer does not start as the answer)
            out = _launch(hip, lambda: hip.conv3x3_small_cin_cl(x, w, bias, tiles=(idx, (K.BLOCK, K.BLOCK)), out=buf))
            assert out.data_ptr() == buf.data_ptr()
            n_bad, worst, images = K.check(out, want, c["inside"])
            print("%s launch %d: worst %.3g (bound %.3g)" % (name, rep, worst, K.BOUND))
            assert n_bad == 0 and worst <= K.BOUND, K.message(name, rep, n_bad, worst, images)
            assert torch.equal(out[:, :, ~inside].view(torch.int32), z[:, :, ~inside].view(torch.int32)), \
                "%s, launch %d: a pixel outside the windows was written" % (name, rep)
            worst_of_all = max(worst_of_all, worst)
    util.record_margin(TEST, "%s: worst |d| of %d launches, %d workgroups" % (name, LAUNCHES, K.workgroups(name)), worst_of_all, K.BOUND)
