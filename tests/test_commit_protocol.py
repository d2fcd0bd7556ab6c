"""The host protocol of a `sparse_update` forward that commits through the queue (sige_amd/nn/commit.py), without a device: the
small DDPM network on the CPU oracle backend with deferred.FORCE_ON_CPU (as tests/test_host_logic.py does for deferral) and
hip.commit_tiles replaced by a torch restatement of what a record means.  What reaches the caches, which records each module
queues, when a non-empty queue raises, and that a model which does not opt in never sees a queue."""
import warnings

import pytest
import torch

from oracle import oracle
from sige_amd import hip, runtime
from sige_amd.nn import Scatter, ScatterGather, deferred
from sige_amd.utils import dilate_mask, downsample_mask
from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet, ResBlock

CFG = DDPMConfig(ch=32, ch_mult=(1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16,), resolution=64, sparse_threshold=32, groups=8)


def fake_commit_tiles(calls):
    """hip.commit_tiles on CPU tensors (NCHW or not): the record's meaning written out, tile by tile."""

    def run(records):
        records = list(records)
        calls.append(records)
        for r in records:
            v = r.src
            if r.scale is not None:
                v = torch.nn.functional.silu(r.scale.reshape(1, -1, 1, 1) * v + r.shift.reshape(1, -1, 1, 1))
            H, W = r.dst.shape[2:]
            for n, (h0, w0) in enumerate(r.idx.tolist()):
                h, w = int((r.offset[0] + h0) / r.stride[0]), int((r.offset[1] + w0) / r.stride[1])
                h1, w1 = min(h + r.tile[0], H), min(w + r.tile[1], W)
                if h1 > h and w1 > w:
                    r.dst[0, :, h:h1, w:w1] = (v[n][:, :h1 - h, :w1 - w] if r.tile_source else v[0, :, h:h1, w:w1]).to(r.dst.dtype)
        return -(-sum(1 for r in records if r.idx.shape[0]) // hip.COMMIT_CAPACITY)

    return run


@pytest.fixture()
def env(monkeypatch):
    calls = []
    runtime.register_backend("cpu", oracle)
    monkeypatch.setattr(deferred, "FORCE_ON_CPU", True)
    monkeypatch.setattr(hip, "commit_tiles", fake_commit_tiles(calls))
    yield calls
    runtime.unregister_backend("cpu")


def _model(opt_in=True):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DDPMSparseUNet(CFG).eval()
    if not opt_in:
        model.COMMIT_TILES = False
    model.set_scatter_inplace(True)
    return model


def _inputs():
    g = torch.Generator().manual_seed(1)
    x0, n1, n2 = (torch.randn(1, 3, 64, 64, generator=g) for _ in range(3))
    m = torch.zeros(64, 64, dtype=torch.bool)
    m[10:22, 14:30] = True
    return x0, x0 + n1 * m, x0 + n1 * m + n2 * m, m, torch.zeros(1)


def _caches(model):
    out = {}
    for name, mod in model.named_modules():
        for attr in ("original_outputs", "original_residuals", "activated_outputs"):
            for cid, t in getattr(mod, attr, {}).items():
                out[(name, attr, cid)] = t
    return out


def _sequence(model):
    """full(x0); the accepted edit x1 under the mask; a plain sparse forward on x2 on top of it."""
    x0, x1, x2, m, t = _inputs()
    with torch.no_grad():
        model.set_mode("full")
        model(x0, t)
        model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
        model.set_mode("sparse")
        model(x1, t)
        model.set_sparse_update(True)
        a = model(x1, t).clone()
        model.set_sparse_update(False)
        b = model(x2, t).clone()
    return a, b


def test_the_commit_leaves_what_the_reference_route_leaves(env):
    calls = env
    new, old = _model(True), _model(False)
    a0, b0 = _sequence(old)
    assert calls == [] and old.__dict__.get("_commit_queue") is None
    # (the generation counters only: without a device a plain sparse forward builds no persistent output -- that they keep their
    #  addresses is tests/test_gpu_ddpm_commit.py's to show)
    bufs = lambda model: {n: dict(mod._out_bufs.gen) for n, mod in model.named_modules() if hasattr(mod, "_out_bufs")}  # noqa: E731
    # (run the new model up to the commit forward by hand, to look at its buffers on both sides of it)
    x0, x1, x2, m, t = _inputs()
    with torch.no_grad():
        new.set_mode("full")
        new(x0, t)
        new.set_masks(downsample_mask(dilate_mask(m, 5), 8))
        new.set_mode("sparse")
        new(x1, t)
        before, ids = bufs(new), {k: id(v) for k, v in _caches(new).items()}
        new.set_sparse_update(True)
        a1 = new(x1, t).clone()
        assert len(calls) == 1 and len(new._commit_queue) == 0  # ONE flush, at the end of the forward
        new.set_sparse_update(False)
        assert bufs(new) == before                                # no generation bumped: nothing was invalidated
        assert {k: id(v) for k, v in _caches(new).items()} == ids  # the cache tensors are the same objects
        b1 = new(x2, t).clone()
    assert len(calls) == 1
    torch.testing.assert_close(a1, a0, rtol=0, atol=1e-5)
    torch.testing.assert_close(b1, b0, rtol=0, atol=1e-5)
    c_new, c_old = _caches(new), _caches(old)
    assert sorted(c_new) == sorted(c_old) and any(k[1] == "activated_outputs" for k in c_new)
    for k in c_new:
        torch.testing.assert_close(c_new[k], c_old[k], rtol=0, atol=1e-5, msg=str(k))


def _records_into(records, tensor):
    return [r for r in records if r.dst is tensor]


def test_record_lists_of_a_resblock_with_and_without_a_tiled_shortcut(env):
    calls = env
    model = _model(True)
    x0, x1, _, m, t = _inputs()
    with torch.no_grad():
        model.set_mode("full")
        model(x0, t)
        model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
        model.set_mode("sparse")
        model.set_sparse_update(True)
        model(x1, t)
        model.set_sparse_update(False)
    (records,) = calls
    tiled = [b for b in model.modules() if isinstance(b, ResBlock) and b.sparse_main]
    with_shortcut = [b for b in tiled if b.sparse_shortcut]
    without = [b for b in tiled if not b.sparse_shortcut]
    assert with_shortcut and without
    seen = 0
    for b in tiled:
        mg, sg_mod = b.main_gather, b.scatter_gather
        s2, t2 = b.affine[0][2:]
        raw, act = sg_mod.original_outputs[0], sg_mod.activated_outputs[0]
        (r_raw,), (r_act,) = _records_into(records, raw), _records_into(records, act)
        assert r_raw.tile_source and r_act.tile_source and r_raw.src is r_act.src and r_raw.scale is None
        assert r_act.scale is s2 and r_act.shift is t2
        for r in (r_raw, r_act):
            assert tuple(r.src.shape) == (mg.active_indices.shape[0], b.cout, 4, 4) and r.idx is mg.active_indices
            assert (r.offset, r.stride, r.tile) == (tuple(mg.offset), (1, 1), (4, 4))
        out = b.scatter._out_bufs.bufs[0][1]
        into_out = _records_into(records, b.scatter.original_outputs[0])
        if b.sparse_shortcut:
            sh = b.shortcut_gather
            main, short = into_out
            assert main.src is out and short.src is out and not main.tile_source and not short.tile_source
            assert main.idx is mg.active_indices and (main.offset, main.tile) == (tuple(mg.offset), (4, 4))
            assert short.idx is sh.active_indices and (short.offset, short.tile) == ((0, 0), (4, 4))
            (res,) = _records_into(records, b.scatter.original_residuals[0])
            assert res.tile_source and tuple(res.src.shape) == (sh.active_indices.shape[0], b.cout, 4, 4) and res.idx is sh.active_indices
            seen += 5
        else:
            (main,) = into_out
            assert main.src is out and not main.tile_source and main.idx is mg.active_indices
            seen += 3
    # ... and the remaining records are the plain Scatters of the Downsample / Upsample / attention layers: one each
    others = [m_ for m_ in model.modules() if isinstance(m_, Scatter) and not any(m_ is getattr(b, "scatter", None) for b in tiled)]
    for sc in others:
        (r,) = _records_into(records, sc.original_outputs[0])
        assert not r.tile_source and r.src is sc._out_bufs.bufs[0][1]
    assert len(records) == seen + len(others)
    assert sum(1 for m_ in model.modules() if isinstance(m_, ScatterGather)) == len(tiled)


def test_a_queue_that_was_not_flushed_raises(env):
    model = _model(True)
    x0, x1, _, m, t = _inputs()
    masks = downsample_mask(dilate_mask(m, 5), 8)
    with torch.no_grad():
        model.set_mode("full")
        model(x0, t)
        model.set_masks(masks)
        model.set_mode("sparse")
        model.set_sparse_update(True)
        blk = model.down[0].block[0]
        blk(model.conv_in(x1), None)  # a block run outside the model's forward: queued, never flushed
        assert len(model._commit_queue) == 3
        for what in (lambda: model.set_masks(masks), lambda: model.set_mode("full"), lambda: model.clear_cache(),
                     lambda: model.set_sparse_update(False), lambda: model.set_sparse_update(True)):
            with pytest.raises(RuntimeError, match="never flushed"):
                what()
        assert model.mode == "sparse" and blk.sparse_update
        assert model.flush_commit() == 1 and len(model._commit_queue) == 0
        model.set_sparse_update(False)
        model.set_mode("full")
        model.set_mode("sparse")
        model.clear_cache()


def test_opt_in_off_means_no_queue(env):
    calls = env
    model = _model(False)
    model.set_sparse_update(True)
    assert model.__dict__.get("_commit_queue") is None
    assert all(getattr(m, "commit_queue", None) is None for m in model.modules())
    model.set_sparse_update(False)
    # any SIGEModel that does not opt in: the reference's behaviour, the tiles materialised (tests/test_host_logic.py:361-365)
    from tests.test_host_logic import ResNet

    net = ResNet(4, 4).eval()
    assert not net.COMMIT_TILES
    net.set_sparse_update(True)
    assert net.__dict__.get("_commit_queue") is None and net.block.scatter.commit_queue is None
    assert net.block.main_gather._no_deferral()
    assert net.flush_commit() == 0 and calls == []


def test_stacked_edits_cannot_be_committed(env):
    model = _model(True)
    model.edit_batch = 2
    with pytest.raises(RuntimeError, match="stacked"):
        model.set_sparse_update(True)
    assert model.__dict__.get("_commit_queue") is None and not any(getattr(m, "sparse_update", False) for m in model.modules())
