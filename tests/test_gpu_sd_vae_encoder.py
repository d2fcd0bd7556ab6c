"""The SD VAE encoder workload on the GPU against tests/golden/sd_vae_encoder.npz (the REAL reference's SIGEEncoder with a plain
quant_conv behind it, tests/golden/make_vae_encoder_golden.py): the reference's NCHW layout through the module chain, channels-last
through the fused path (the tail on hip.conv3x3_latent_head_cl, quant_conv folded in), the torch-chain switch, what the tail and
the attention block launch, poisoned persistent buffers, a second mask without a new full pass, graph replay, and the real
configuration."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import vae_encoder_inputs as enc_inputs  # noqa: E402
from tests.test_sd_vae_encoder import GOLDEN, SMALL_IMAGE, build_model, check_sd, check_small, inputs, make_masks, run_encoder  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]  # (pinned to the real reference's outputs, or to the CPU oracle backend)
SMALL = enc_inputs.SMALL
LAYOUTS = [(False, False), (True, False), (True, True)]  # (channels_last, in-place scatters)


def _record(test):
    return lambda what, value, tol: util.record_margin(test, what, value, tol)


@pytest.fixture
def torch_head():
    """NATIVE_HEAD = False for the test: the tail on the reference's chain."""
    from sige_amd.workloads import sd_vae

    keep = sd_vae.NATIVE_HEAD
    sd_vae.NATIVE_HEAD = False
    try:
        yield sd_vae
    finally:
        sd_vae.NATIVE_HEAD = keep


def _launches(fn):
    """{entry: [launched?] per call} of hip.conv3x3_latent_head_cl and hip.attention_wide while fn() runs."""
    from sige_amd import hip

    calls = {"conv3x3_latent_head_cl": [], "attention_wide": []}
    orig = {name: getattr(hip, name) for name in calls}

    def counted(name):
        def call(*a, **kw):
            out = orig[name](*a, **kw)
            calls[name].append(out is not None)
            return out
        return call

    for name in calls:
        setattr(hip, name, counted(name))
    try:
        with torch.no_grad():
            fn()
    finally:
        for name in calls:
            setattr(hip, name, orig[name])
    return calls


def _check_launches(model, quant, channels_last, native_head=True):
    mask, masks = make_masks(SMALL, SMALL_IMAGE, "cuda")
    _, x1 = inputs(SMALL, SMALL_IMAGE, 1, mask, "cuda", channels_last)
    fused = [True] if channels_last else []
    for fn in (lambda: model(x1), lambda: model.moments(x1, quant), lambda: model.encode(x1, quant, noise=None)):
        calls = _launches(fn)
        assert calls["conv3x3_latent_head_cl"] == (fused if native_head else [])  # (ONE call per sparse forward, and it launched)
        assert calls["attention_wide"] == fused


@pytest.mark.parametrize("channels_last,inplace", LAYOUTS)
def test_small_configuration_on_the_gpu_matches_the_reference_fixture(channels_last, inplace):
    """Both cached images, outputs and moments: NCHW (module chain), channels-last (fused path: the tiled first conv, the 192-channel
    attention on hip.attention_wide, the tail on the latent-head launch), channels-last with in-place persistent outputs."""
    model, quant, outs, counts, ratio = run_encoder(SMALL, SMALL_IMAGE, "cuda", channels_last, 2, inplace)
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae_encoder small cl=%d inplace=%d" % (channels_last, inplace)))
    _check_launches(model, quant, channels_last)


@pytest.mark.parametrize("channels_last,inplace", LAYOUTS)
def test_small_configuration_on_the_torch_head_matches_the_reference_fixture(torch_head, channels_last, inplace):
    model, quant, outs, _, _ = run_encoder(SMALL, SMALL_IMAGE, "cuda", channels_last, 2, inplace)
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae_encoder small torch head cl=%d inplace=%d" % (channels_last, inplace)))
    _check_launches(model, quant, channels_last, native_head=False)


def test_encode_on_the_fused_path_matches_the_torch_chain(torch_head):
    """(moments, z) of encode() with noise and without: the launch's posterior epilogue against the fallback's torch expression."""
    model, quant, _, _, _ = run_encoder(SMALL, SMALL_IMAGE, "cuda", True, 1, True)
    mask, _ = make_masks(SMALL, SMALL_IMAGE, "cuda")
    _, x1 = inputs(SMALL, SMALL_IMAGE, 0, mask, "cuda", True)
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(5)).to("cuda")
    with torch.no_grad():
        want = [model.encode(x1, quant, noise=noise), model.encode(x1, quant)]
        torch_head.NATIVE_HEAD = True
        got = [model.encode(x1, quant, noise=noise), model.encode(x1, quant)]
    for (wm, wz), (gm, gz) in zip(want, got):
        assert tuple(gz.shape) == (1, 4, 16, 16)
        for what, a, b in (("moments", gm, wm), ("z", gz, wz)):
            err = float((a - b).abs().max())
            util.record_margin("test_gpu_sd_vae_encoder encode", what, err, util.CONV_ATOL)
            assert err <= util.CONV_ATOL, (what, err)
    assert float((got[0][1] - got[1][1]).abs().max()) > 1e-2  # (the sample is not the mode)
    assert float(np.abs(got[0][0].cpu().numpy() - GOLDEN["small/sparse_moments0"]).max()) <= util.CONV_ATOL


def _tile_cells(model, shape):
    """[H,W] bool: the cells of the attention block's active 4x4 tiles."""
    m = torch.zeros(shape, dtype=torch.bool, device="cuda")
    for h0, w0 in model.mid.attn_1.gather.active_indices.tolist():
        m[max(h0, 0):h0 + 4, max(w0, 0):w0 + 4] = True
    return m


def test_small_configuration_with_poisoned_persistent_buffers():
    """In front of every sparse forward: NaN in the attention's output rows and in ALL of conv_in's window buffer (inside the
    active windows the forward rewrites it, outside nobody reads it), and in the persistent K | V tensor on the cells of the
    active tiles.  EXEMPT: K | V outside the active tiles and the Scatter outputs outside theirs -- the cache of the original."""
    seen = []

    def poison(model):
        bufs = model.persistent_buffers()
        seen.append(sorted(name for name, _, _ in bufs))
        for name, buf, rewritten in bufs:
            if rewritten:
                buf.fill_(float("nan"))
            else:
                buf.masked_fill_(_tile_cells(model, tuple(buf.shape[2:]))[None, None], float("nan"))

    model, quant, outs, _, _ = run_encoder(SMALL, SMALL_IMAGE, "cuda", True, 2, True, prepare=poison)
    assert seen == [["attn_out", "conv_in", "kv"]] * 4  # allocated by set_masks / set_mode, not by the forward
    for got in outs:
        util.assert_finite(got["sparse"], "sparse output over poisoned persistent buffers")
        util.assert_finite(got["sparse_moments"], "sparse moments over poisoned persistent buffers")
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae_encoder small poisoned"))


def _two_masks(device, channels_last):
    """full(x0), mask A, sparse(x0 + noise * A), mask B (no new full pass), sparse(x0 + noise * B): the moments."""
    model, quant = build_model(SMALL, device, channels_last, channels_last)
    outs = []
    with torch.no_grad():
        for second in (False, True):
            mask, masks = make_masks(SMALL, SMALL_IMAGE, device, second)
            x0, x1 = inputs(SMALL, SMALL_IMAGE, 0, mask, device, channels_last)
            if not second:
                model.set_mode("full")
                model(x0)
            model.set_masks(masks)
            model.set_mode("sparse")
            outs.append(model.moments(x1, quant).clone().cpu())
    return outs


def test_second_mask_without_a_new_full_pass_vs_cpu_oracle():
    from oracle import oracle
    from sige_amd import runtime

    runtime.register_backend("cpu", oracle)
    try:
        want = _two_masks("cpu", False)
    finally:
        runtime.unregister_backend("cpu")
    got = _two_masks("cuda", True)
    assert float((want[0] - want[1]).abs().max()) > 1e-2
    for k in range(2):
        err = float((got[k] - want[k]).abs().max())
        util.record_margin("test_gpu_sd_vae_encoder two masks", "mask %d" % k, err, util.CONV_ATOL)
        assert err <= util.CONV_ATOL, "mask %d: max |diff| %.3e" % (k, err)


def test_sparse_forward_graph_replay_equals_eager():
    model, quant = build_model(SMALL, "cuda", True, True)
    mask, masks = make_masks(SMALL, SMALL_IMAGE, "cuda")
    x0, x1 = inputs(SMALL, SMALL_IMAGE, 0, mask, "cuda", True)
    with torch.no_grad():
        model.set_mode("full")
        model(x0)
        model.set_masks(masks)
        model.set_mode("sparse")
        eager = model.moments(x1, quant).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.moments(x1, quant)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model.moments(x1, quant)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    assert float(np.abs(out.cpu().numpy() - GOLDEN["small/sparse_moments0"]).max()) <= util.CONV_ATOL


def test_real_configuration_on_the_gpu_matches_the_reference_fixture():
    """configs/sige.yaml's encoder (34.2 M parameters), image 128 x 128 -> latent 16 x 16, channels-last, in-place outputs: full and
    sparse, outputs and moments, against the fixture; the head runs at C = 512."""
    model, quant, outs, counts, ratio = run_encoder(enc_inputs.SD, enc_inputs.SD_IMAGE, "cuda", True, 1, True)
    assert abs(ratio - float(GOLDEN["sd/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["sd/tiles"])
    check_sd(outs[0], util.CONV_ATOL, _record("test_gpu_sd_vae_encoder sd"))
    mask, _ = make_masks(enc_inputs.SD, enc_inputs.SD_IMAGE, "cuda")
    _, x1 = inputs(enc_inputs.SD, enc_inputs.SD_IMAGE, 0, mask, "cuda", True)
    calls = _launches(lambda: model.moments(x1, quant))
    assert calls["conv3x3_latent_head_cl"] == [True] and calls["attention_wide"] == [True]
