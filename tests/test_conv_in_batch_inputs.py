"""CPU checks of tests/conv_in_common.py, the cases and the checker of tests/test_gpu_conv_in_batch.py: the checker sees what went
wrong in csrc/conv_in.hip before, on the fp64 reference of every case alone.  Nothing is broken on the GPU to
show this.
  * one dword that holds the value of another pixel of the same image ("errors as large as the values") is reported, with its image;
  * the images of a case differ by more than 1e-2 at more than 99 % of the output elements, pair by pair, so a kernel that reads or
    writes the wrong image cannot pass;
  * a tile row stored at the neighbouring pixel (the reference shifted by one pixel along W) is reported in every image;
  * an element nobody stored (NaN under util.poisoned) is reported."""
import pytest
import torch

from tests import conv_in_common as K

NAMES = list(K.WHOLE) + list(K.TILES)


@pytest.fixture(scope="module", params=NAMES)
def c(request):
    return K.case(request.param)


def _right(c):
    """What a correct launch returns: the reference rounded to fp32, channels-last."""
    return c["want"].float().contiguous(memory_format=torch.channels_last)


def test_the_cases_are_the_launches_they_are_meant_to_be():
    assert K.workgroups("b8-c3-128x128-64") == K.workgroups("b8-c3-128x128-32") == K.workgroups("b8-c3-128x128-128") == 1024
    assert K.workgroups("b4-c3-256x256-128") == 2048
    assert (67 * 93) % 32 and (67 * 93) % 128 and (5 * 67 * 93) % 32 and (131 * 70) % 32  # image boundaries inside 32-pixel blocks
    assert all(K.workgroups(n) >= 100 for n in NAMES) and all(K.workgroups(n) >= 300 for n in K.TILES)
    assert sum(K.WHOLE[n][0] > 2 for n in K.WHOLE) == len(K.WHOLE)
    for n in K.TILES:
        B, H, W, _ = K.TILES[n]
        idx = K.window_list(H, W)
        assert idx.min() == -1 and int(idx[:, 0].max()) + K.BLOCK > H and int(idx[:, 1].max()) + K.BLOCK > W  # clipped on all four sides
        assert bool(K.window_mask(idx, (H, W)).all())  # (stride 4, size 6: the windows overlap and cover the image)


def test_the_reference_passes_and_its_layout_is_the_case_s(c):
    assert K.check(_right(c), c["want"], c.get("inside")) == (0, pytest.approx(0, abs=2e-6), [])
    x, B, C, H, W = c["x"], c["B"], c["C"], c["H"], c["W"]
    want_strides = {"nhwc": (C * H * W, 1, W * C, C), "nchw": (C * H * W, H * W, W, 1), "strided": (2 * C * H * W, 1, W * C, C)}[c["layout"]]
    assert tuple(x.shape) == (B, C, H, W) and (C == 1 or x.stride() == want_strides)
    if c["layout"] == "strided":
        d = c["want"] - c["want_nobias"] - c["bias"].double()[None, :, None, None]
        assert float(d.abs().max()) < 1e-12 and float(c["bias"].abs().min()) > K.BOUND  # (a dropped or doubled bias shows)


def test_one_dword_from_another_pixel_of_the_image_is_reported_with_its_image(c):
    B, cout, H, W = c["B"], c["cout"], c["H"], c["W"]
    for b, ch, h, w in ((B - 1, cout - 4, H - 1, W - 2), (B // 2, 16, H // 2, 5), (0, 0, 0, 0)):
        got = _right(c)
        got[b, ch, h, w] = got[b, ch, (h + 7) % H, (w + 3) % W]
        assert abs(float(got[b, ch, h, w]) - float(c["want"][b, ch, h, w])) > 100 * K.BOUND
        n_bad, worst, images = K.check(got, c["want"], c.get("inside"))
        assert (n_bad, images) == (1, [b]) and worst > 100 * K.BOUND
        assert "images [%d]" % b in K.message(c["name"], 0, n_bad, worst, images)


def test_the_images_of_a_case_differ_almost_everywhere(c):
    want = c["want"]
    for b in range(c["B"]):
        for b2 in range(b + 1, c["B"]):
            far = ((want[b] - want[b2]).abs() > K.SEPARATION).double().mean()
            assert float(far) > 0.99, (c["name"], b, b2, float(far))
    # so the output of image b under the name of image b + 1 (a wrong batch offset on either side) fails in every image
    n_bad, _, images = K.check(_right(c).roll(1, 0), want, c.get("inside"))
    assert images == list(range(c["B"])) and n_bad > 0.99 * want.numel()


def test_a_row_stored_at_the_neighbouring_pixel_is_reported(c):
    n_bad, worst, images = K.check(_right(c).roll(1, 3), c["want"], c.get("inside"))
    assert images == list(range(c["B"])) and n_bad > 0.99 * c["want"].numel() and worst > 1


def test_an_element_nobody_stored_is_reported(c):
    got = _right(c)
    got[c["B"] - 1, 3, 2, 1] = float("nan")
    n_bad, worst, images = K.check(got, c["want"], c.get("inside"))
    assert (n_bad, images) == (1, [c["B"] - 1]) and worst != worst


def test_outside_the_mask_nothing_counts():
    """The tile-list form is compared inside its windows only (outside them the buffer's bits are compared, with torch.equal)."""
    c = K.case("tiles-b3-128x128-32")
    inside = torch.zeros(c["H"], c["W"], dtype=torch.bool)
    inside[:6, :6] = True
    got = _right(c)
    got[1, 0, 6, 0] = 7.0
    got[2, 0, 0, 6] = float("nan")
    assert K.check(got, c["want"], inside)[::2] == (0, [])
    got[2, 1, 5, 5] = 7.0
    assert K.check(got, c["want"], inside)[::2] == (1, [2])
