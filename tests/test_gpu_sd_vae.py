"""The SD VAE decoder workload on the GPU against tests/golden/sd_vae_decoder.npz (the REAL reference's SIGEDecoder,
tests/golden/make_vae_golden.py): the reference's NCHW layout through the module chain, channels-last through the fused path (the
attention block on hip.attention_wide), the torch-chain switch, poisoned persistent buffers, a second mask without a new full
pass, graph replay, what the attention block launches, and the real configuration."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import vae_inputs  # noqa: E402
from tests.test_sd_vae import GOLDEN, SD_LATENT, build_model, check_sd, check_small, inputs, make_masks, run_vae, sd_has_outputs  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]  # (pinned to the real reference's outputs, or to the CPU oracle backend)
SMALL, LATENT = vae_inputs.SMALL, 16


def _record(test):
    return lambda what, value, tol: util.record_margin(test, what, value, tol)


@pytest.fixture
def torch_chain():
    """NATIVE_ATTENTION = False for the test: the attention block on the reference's bmm / softmax / bmm chain."""
    from sige_amd.workloads import sd_vae

    keep = sd_vae.NATIVE_ATTENTION
    sd_vae.NATIVE_ATTENTION = False
    try:
        yield sd_vae
    finally:
        sd_vae.NATIVE_ATTENTION = keep


def _attention_launches(model, z1):
    """How many hip.attention_wide calls one sparse forward makes."""
    from sige_amd import hip

    calls, orig = [], hip.attention_wide

    def counted(*a, **kw):
        out = orig(*a, **kw)
        calls.append(out is not None)
        return out

    hip.attention_wide = counted
    try:
        with torch.no_grad():
            model(z1)
    finally:
        hip.attention_wide = orig
    return calls


@pytest.mark.parametrize("channels_last,inplace", [(False, False), (True, False), (True, True)])
def test_small_configuration_on_the_gpu_matches_the_reference_fixture(channels_last, inplace):
    """Both cached latents: NCHW (module chain), channels-last (fused path: the 192-channel attention on hip.attention_wide),
    channels-last with in-place persistent outputs (K | V scattered into one persistent tensor by the conv's epilogue)."""
    model, outs, counts, ratio = run_vae(SMALL, LATENT, "cuda", channels_last, 2, inplace)
    assert abs(ratio - float(GOLDEN["small/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["small/tiles"])
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae small cl=%d inplace=%d" % (channels_last, inplace)))
    _, masks = make_masks(SMALL, LATENT, "cuda")
    _, z1 = inputs(SMALL, LATENT, 1, masks, "cuda", channels_last)
    assert _attention_launches(model, z1) == ([True] if channels_last else [])  # (ONE launch, and it is the new kernel's)


@pytest.mark.parametrize("channels_last,inplace", [(False, False), (True, False), (True, True)])
def test_small_configuration_on_the_torch_chain_matches_the_reference_fixture(torch_chain, channels_last, inplace):
    model, outs, _, _ = run_vae(SMALL, LATENT, "cuda", channels_last, 2, inplace)
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae small torch chain cl=%d inplace=%d" % (channels_last, inplace)))
    _, masks = make_masks(SMALL, LATENT, "cuda")
    _, z1 = inputs(SMALL, LATENT, 1, masks, "cuda", channels_last)
    assert _attention_launches(model, z1) == []


def _tile_cells(model, shape):
    """[H,W] bool: the cells of the attention block's active 4x4 tiles."""
    m = torch.zeros(shape, dtype=torch.bool, device="cuda")
    for h0, w0 in model.mid.attn_1.gather.active_indices.tolist():
        m[max(h0, 0):h0 + 4, max(w0, 0):w0 + 4] = True
    return m


def test_small_configuration_with_poisoned_persistent_buffers():
    """In front of every sparse forward: the attention's output rows hold NaN everywhere, the persistent K | V tensor on the cells
    of the active tiles -- what the forward rewrites before it reads.  EXEMPT: K | V outside the active tiles, and the persistent
    outputs of the Scatter modules outside theirs -- those cells legitimately carry the ORIGINAL's values (they are the cache the
    sparse forward exists to reuse; sige_amd.nn.scatter._OutputBuffers); inside the active tiles the Scatter outputs are
    poisoned too."""
    from sige_amd.nn import Scatter, ScatterWithBlockResidual

    seen = []

    def poison(model):
        bufs = model.persistent_buffers()
        seen.append(sorted(name for name, _, _ in bufs))
        for name, buf, rewritten in bufs:
            if rewritten:
                buf.fill_(float("nan"))
            else:
                cells = _tile_cells(model, tuple(buf.shape[2:]))
                buf.masked_fill_(cells[None, None], float("nan"))
        attn = model.mid.attn_1
        for sc in (attn.out_scatter, model.mid.block_1.scatter, model.mid.block_2.scatter):
            assert isinstance(sc, (Scatter, ScatterWithBlockResidual))
            entry = sc._out_bufs.bufs.get(sc.cache_id)
            if entry is not None:  # (built by the first sparse forward of this cache id)
                entry[1].masked_fill_(_tile_cells(model, tuple(entry[1].shape[2:]))[None, None], float("nan"))

    model, outs, _, _ = run_vae(SMALL, LATENT, "cuda", True, 2, True, prepare=poison)
    assert seen == [["attn_out", "kv"], ["attn_out", "kv"]]  # allocated by set_masks / set_mode, not by the forward
    for _, sparse in outs:
        util.assert_finite(sparse, "sparse output over poisoned persistent buffers")
    check_small(outs, util.CONV_ATOL, _record("test_gpu_sd_vae small poisoned"))
    # a second forward under the same mask, poisoned again (now every Scatter output exists)
    _, masks = make_masks(SMALL, LATENT, "cuda")
    _, z1 = inputs(SMALL, LATENT, 1, masks, "cuda", True)
    poison(model)
    with torch.no_grad():
        again = model(z1)
    util.assert_finite(again, "second sparse forward over poisoned persistent buffers")
    assert float(np.abs(again.cpu().numpy() - GOLDEN["small/sparse1"]).max()) <= util.CONV_ATOL


def _two_masks(device, channels_last):
    """full(z0), mask A, sparse(z0 + noise * A), mask B (no new full pass), sparse(z0 + noise * B)."""
    model = build_model(SMALL, device, channels_last, channels_last)
    outs = []
    with torch.no_grad():
        for second in (False, True):
            _, masks = make_masks(SMALL, LATENT, device, second)
            z0, z1 = inputs(SMALL, LATENT, 0, masks, device, channels_last)
            if not second:
                model.set_mode("full")
                model(z0)
            model.set_masks(masks)
            model.set_mode("sparse")
            outs.append(model(z1).clone().cpu())
    return outs


def test_second_mask_without_a_new_full_pass_vs_cpu_oracle():
    """The persistent K | V tensor keeps the first mask's tiles until set_masks() restores it; the second mask's forward must see
    the original's K | V everywhere outside ITS tiles."""
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
        util.record_margin("test_gpu_sd_vae two masks", "mask %d" % k, err, util.CONV_ATOL)
        assert err <= util.CONV_ATOL, "mask %d: max |diff| %.3e" % (k, err)


def _sparse_model(cfg=SMALL, latent=LATENT):
    """(model, edited latent) in sparse mode, channels-last, in-place outputs."""
    model = build_model(cfg, "cuda", True, True)
    _, masks = make_masks(cfg, latent, "cuda")
    z0, z1 = inputs(cfg, latent, 0, masks, "cuda", True)
    with torch.no_grad():
        model.set_mode("full")
        model(z0)
        model.set_masks(masks)
        model.set_mode("sparse")
    return model, z1


def test_sparse_forward_graph_replay_equals_eager():
    model, z1 = _sparse_model()
    with torch.no_grad():
        eager = model(z1).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(z1)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(z1)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    assert float(np.abs(out.cpu().numpy() - GOLDEN["small/sparse0"]).max()) <= util.CONV_ATOL


_CHAIN_OPS = ("bmm", "baddbmm", "softmax", "copy", "clone")


class _AtenOps(torch.utils._python_dispatch.TorchDispatchMode):
    """Every aten op that runs while `active` is set (tests/test_gpu_pd_unet.py's probe, scoped to one module)."""

    def __init__(self):
        super().__init__()
        self.seen, self.active = [], False

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if self.active:
            self.seen.append(func._schema.name.split("::")[-1])
        return func(*args, **(kwargs or {}))


def _attention_block_chain_ops(model, z1):
    """The bmm / baddbmm / softmax / copy (copy_, clone, _to_copy) aten ops -- each one a kernel on GPU tensors -- that one sparse
    forward runs INSIDE mid.attn_1."""
    attn = model.mid.attn_1
    with torch.no_grad(), _AtenOps() as rec:
        pre = attn.register_forward_pre_hook(lambda m, a: setattr(rec, "active", True))
        post = attn.register_forward_hook(lambda m, a, o: setattr(rec, "active", False))
        try:
            model(z1)
        finally:
            pre.remove()
            post.remove()
    return sorted({k for n in rec.seen for k in _CHAIN_OPS if k in n})


def test_attention_block_launches_no_torch_chain_kernel(torch_chain):
    """Channels-last sparse forward: no bmm / baddbmm / softmax / copy aten kernel from the attention block; with
    NATIVE_ATTENTION = False the same probe sees them."""
    torch_chain.NATIVE_ATTENTION = True
    model, z1 = _sparse_model()
    with torch.no_grad():
        model(z1)
    assert _attention_block_chain_ops(model, z1) == []
    torch_chain.NATIVE_ATTENTION = False
    with torch.no_grad():
        model(z1)
    seen = _attention_block_chain_ops(model, z1)
    assert "bmm" in seen and "softmax" in seen and ("copy" in seen or "clone" in seen), seen


def test_real_configuration_on_the_gpu_matches_the_reference_fixture():
    """configs/sige.yaml's decoder (49.5 M parameters), latent 64 x 64 -> 512 x 512, channels-last, in-place outputs: full and sparse
    against the fixture; the attention block is 4 096 keys x one 512-wide head."""
    assert sd_has_outputs()
    model, outs, counts, ratio = run_vae(vae_inputs.SD, SD_LATENT, "cuda", True, 1, True)
    assert abs(ratio - float(GOLDEN["sd/edit_ratio"][0])) < 1e-9
    assert np.array_equal(counts, GOLDEN["sd/tiles"])
    check_sd(*outs[0], util.CONV_ATOL, _record("test_gpu_sd_vae sd"))
    _, masks = make_masks(vae_inputs.SD, SD_LATENT, "cuda")
    _, z1 = inputs(vae_inputs.SD, SD_LATENT, 0, masks, "cuda", True)
    assert _attention_launches(model, z1) == [True]
