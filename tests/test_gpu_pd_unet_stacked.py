"""Stacked edits (sige_amd/stacked.py) through the Progressive Distillation U-Net (sige_amd.workloads.pd_unet): E = 4 edits of one
original, each with its own mask, in ONE forward on the GPU.

Configuration: pd_inputs.SMALL -- 64x64, tiled at 64 and 32 (a tiled "down" block at each, a tiled "up" block 32 -> 64), dense with
attention at 16: every kind of block once.  Edits: x0 + noise_e * mask_e with another noise seed per edit; masks of 14 x 15 pixels:
the fixture's two (bottom-right first, then top-left), a third on the bottom-left, a fourth in the middle -- in the tall tensor
edit 1's top tiles lie under edit 0's bottom tiles, and edit 2's bottom tiles over edit 3's first rows.

Every edit's slice of one stacked forward is compared with THAT edit's own single sparse forward on the CPU with the oracle as
native back end (util.CONV_ATOL; the way of test_second_mask_without_a_new_full_pass_vs_cpu_oracle) and with the same model's
single-edit GPU forward (util.SELF_ATOL).  Margins and launch counts go through util.record_margin's file (kept as
profiles/pd_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.golden import pd_inputs  # noqa: E402
from tests.golden.model_init import init_by_name  # noqa: E402
from tests.test_gpu_pd_unet import _ELEMENTWISE, _AtenOps  # noqa: E402
from tests.test_pd_unet import check_pd128, pd_config  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
CL = torch.channels_last
CFG, SIZE, E = pd_inputs.SMALL, 64, 4
TEST = "test_gpu_pd_unet_stacked"


# ---- the edits ------------------------------------------------------------------------------------------------------------------
def edit_masks():
    """[4 x bool [64,64]], 14 rows x 15 columns each."""
    third = torch.zeros(SIZE, SIZE, dtype=torch.bool)
    third[50:64, 0:15] = True
    fourth = torch.zeros(SIZE, SIZE, dtype=torch.bool)
    fourth[25:39, 30:45] = True
    return [pd_inputs.edit_mask(SIZE, second=True), pd_inputs.edit_mask(SIZE), third, fourth]


def pyramids(device, cfg=CFG, masks=None):
    from sige_amd.utils import dilate_mask, downsample_mask

    return [pd_inputs.pyramid(m.to(device), cfg, dilate_mask, downsample_mask) for m in (masks or edit_masks())]


def edit_inputs(device, size=SIZE, masks=None):
    """(original [1,3,s,s], [edited image of edit e]), NCHW on `device`."""
    x0 = pd_inputs.images(size)[0]
    edits = [x0 + pd_inputs.images(size, seed=100 + e)[1] * m for e, m in enumerate(masks or edit_masks())]
    return x0.to(device), [x.to(device) for x in edits]


def build(device, channels_last=True, cfg=CFG):
    from sige_amd.workloads.pd_unet import PDSparseUNet

    model = PDSparseUNet(pd_config(cfg)).eval()
    init_by_name(model)
    model = model.to(device)
    if channels_last:
        model = model.to(memory_format=CL)
        model.set_scatter_inplace(True)
    return model, torch.full((1,), pd_inputs.LOGSNR[0], device=device)


def _fmt(x, channels_last=True):
    return x.contiguous(memory_format=CL) if channels_last else x.contiguous()


_oracle = {}


def oracle_outputs():
    """Each edit's own sparse forward on the CPU, oracle back end: computed once per process and left unchanged."""
    if "outs" not in _oracle:
        from oracle import oracle
        from sige_amd import runtime

        model, logsnr = build("cpu", False)
        pyrs = pyramids("cpu")
        x0, edits = edit_inputs("cpu")
        torch.set_num_threads(8)
        runtime.register_backend("cpu", oracle)
        try:
            with torch.no_grad():
                model.set_mode("full")
                model(x0, logsnr)
                outs = []
                for e, xe in enumerate(edits):
                    model.set_masks(pyrs[e])
                    model.set_mode("sparse")
                    outs.append(model(xe, logsnr)[0].clone())
        finally:
            runtime.unregister_backend("cpu")
        _oracle["outs"] = outs
    return _oracle["outs"]


def test_the_stacked_list_has_tiles_on_both_sides_of_a_seam():
    """(CPU) the 64-row list of the tall image -- the per-edit lists one after the other, each with its image's row offset
    (stacked.set_masks) -- holds a tile whose first window row is the previous image's last row, and a window that reaches past an
    image's last row."""
    from sige_amd.utils import reduce_mask

    lists = [reduce_mask(p[(SIZE, SIZE)], 6, 4, 1) for p in pyramids("cpu")]
    rows = torch.cat([idx[:, 0] + e * SIZE for e, idx in enumerate(lists)])
    assert bool(((rows % SIZE == SIZE - 1) & (rows != -1)).any())
    assert bool((((rows % SIZE) != SIZE - 1) & ((rows % SIZE) + 6 > SIZE)).any())


def _record_launches(what, E, stacked_launches, single_launches):
    """The library launches of the stacked and of the single forward, beside the margins: a line of util.record_margin whose `value`
    is the stacked count and whose `tol` the single forward's (a record, not a bound: routing may differ at E times the tiles)."""
    util.record_margin(TEST + " library launches", "%s, E=%d: stacked (value) beside single (tol)" % (what, E), stacked_launches,
                       single_launches)


class counted:
    """hip.resample_tiles / hip.attention_tokens with every call written down: (kind, tiled?, query batch, library launches, served?)."""

    def __init__(self, hip):
        self.hip, self.log = hip, []

    def __enter__(self):
        hip, log = self.hip, self.log
        self.keep = (hip.resample_tiles, hip.attention_tokens)
        resample, tokens = self.keep

        def c_resample(x, mode, activeIndices=None, *a, **kw):
            n0 = hip.launch_count()
            out = resample(x, mode, activeIndices, *a, **kw)
            log.append(("resample " + mode, activeIndices is not None, x.shape[0], hip.launch_count() - n0, True))
            return out

        def c_tokens(q, *a, **kw):
            n0 = hip.launch_count()
            out = tokens(q, *a, **kw)
            log.append(("attention", False, q.shape[0], hip.launch_count() - n0, out is not None))
            return out

        hip.resample_tiles, hip.attention_tokens = c_resample, c_tokens
        return log

    def __exit__(self, *exc):
        self.hip.resample_tiles, self.hip.attention_tokens = self.keep
        return False


def _prepared():
    """(model, logsnr, pyramids, x0, edits, singles): behind the full pass on the original, each edit's steady single forward."""
    from sige_amd import hip

    model, logsnr = build("cuda")
    pyrs = pyramids("cuda")
    x0, edits = edit_inputs("cuda")
    x0, edits = _fmt(x0), [_fmt(x) for x in edits]
    with torch.no_grad():
        model.set_mode("full")
        model(x0, logsnr)
        model.set_mode("sparse")
        singles = []
        for e in range(E):
            model.set_masks(pyrs[e])
            model(edits[e], logsnr)  # (the first forward under a mask packs weights and sizes buffers: not the steady state)
            singles.append(model(edits[e], logsnr).clone())
        n0 = hip.launch_count()
        with counted(hip) as single_log:
            model(edits[E - 1], logsnr)
        _prepared.single = (hip.launch_count() - n0, single_log)  # (the steady single forward's launches, for the record)
    return model, logsnr, pyrs, x0, edits, singles


def _check(got, singles, what):
    want = oracle_outputs()
    util.assert_finite(got, what)
    assert got.shape[0] == E and tuple(got.shape[1:]) == tuple(singles[0].shape[1:])
    for e in range(E):
        err = float((got[e].cpu() - want[e]).abs().max())
        own = float((got[e] - singles[e][0]).abs().max())
        print("pd_unet %s edit %d: vs oracle %.3e, vs single %.3e" % (what, e, err, own))
        util.record_margin(TEST + " vs oracle", "%s edit %d" % (what, e), err, util.CONV_ATOL)
        util.record_margin(TEST + " vs single", "%s edit %d" % (what, e), own, util.SELF_ATOL)
        assert err <= util.CONV_ATOL, (what, e, err)
        assert own <= util.SELF_ATOL, (what, e, own)
    for a in range(E):
        for b in range(a + 1, E):
            assert float((got[a] - got[b]).abs().max()) > 1e-2  # (the edits do differ)


def _tall_level_ops(model, xs, logsnr, dense_res):
    """test_gpu_pd_unet._tiled_level_ops under stacked edits: a level is judged by the per-image height of the tall tensor."""
    with torch.no_grad(), _AtenOps() as rec:
        model(xs, logsnr)
    bad = []
    for name, shape in rec.seen:
        if shape is None or len(shape) != 4 or name not in _ELEMENTWISE:
            continue
        hp = shape[2] // E if (shape[0] == 1 and shape[2] == E * shape[3]) else shape[2]
        if hp not in dense_res:
            bad.append((name, shape))
    return bad


class stacked_model:
    """`with stacked_model() as m:` -- the prepared model with its caches stacked, the masks of the E edits set and one stacked
    forward behind it; the edit batch is NOT entered.  Unstacked on the way out."""

    def __enter__(self):
        from sige_amd import stacked

        self.model, self.logsnr, self.pyrs, self.x0, self.edits, self.singles = _prepared()
        self.single = _prepared.single
        self.single_shapes = [tuple(b.shape) for b in self.model.res_buffers()]
        self.xs = _fmt(torch.cat(self.edits, 0))
        stacked.stack_caches(self.model, E)
        try:
            stacked.set_masks(self.model, self.pyrs)
            self.set_masks_ptrs = [b.data_ptr() for b in self.model.res_buffers()]
            with stacked.edit_batch(self.model, E), torch.no_grad():
                self.model(self.xs, self.logsnr)  # (packs weights, sizes buffers)
        except BaseException:
            stacked.unstack_caches(self.model)
            raise
        return self

    def __exit__(self, *exc):
        from sige_amd import hip, stacked

        stacked.unstack_caches(self.model)
        assert hip.get_edit_batch() == 1 and self.model.edit_batch == 1
        return False


def test_stacked_edits_vs_cpu_oracle_and_single_edits_over_poisoned_shortcut_buffers():
    """Parity per edit with the shortcut buffers holding NaN in front of the forward, what the forward launches, and the way back
    to single edits."""
    from sige_amd import hip, stacked
    from sige_amd.utils import reduce_mask

    with stacked_model() as m, torch.no_grad():
        model, logsnr, xs = m.model, m.logsnr, m.xs
        # the shortcut buffers: E times as tall, allocated by stacked.set_masks and not by the forward
        bufs = model.res_buffers()
        assert len(bufs) == 3 and len(m.single_shapes) == 3
        assert [tuple(b.shape) for b in bufs] == [(s[0], s[1], E * s[2], s[3]) for s in m.single_shapes]
        assert [b.data_ptr() for b in bufs] == m.set_masks_ptrs
        # the library's list of the tall image IS the per-edit lists one after the other -- without the candidates at origin row 63
        # that a single-image list ends with (one image row, no cell inside the output): in the tall image that origin is the next
        # image's origin -1, and only that image's mask makes it active
        own = [reduce_mask(p[(SIZE, SIZE)], 6, 4, 1).cpu() for p in m.pyrs]
        want_idx = torch.cat([idx[idx[:, 0] != SIZE - 1] + torch.tensor([e * SIZE, 0], dtype=torch.int32) for e, idx in enumerate(own)])
        got_idx = model.down[0].block[0].main_gather.active_indices.cpu()
        assert sorted(map(tuple, got_idx.tolist())) == sorted(map(tuple, want_idx.tolist()))

        single_launches, single_log = m.single
        with stacked.edit_batch(model, E):
            model(xs, logsnr)
            for b in model.res_buffers():
                b.fill_(float("nan"))
            n0 = hip.launch_count()
            with counted(hip) as log:
                got = model(xs, logsnr).clone()
            launches = hip.launch_count() - n0
        assert hip.get_edit_batch() == 1
        _check(got, m.singles, "E=%d poisoned" % E)

        print("pd_unet small: %d library launches stacked (E=%d), %d single" % (launches, E, single_launches))
        _record_launches("small configuration", E, launches, single_launches)
        tiled = [r for r in log if r[0].startswith("resample") and r[1]]
        assert [r[0] for r in tiled] == ["resample down", "resample down", "resample up"], log
        assert all(n == 1 and b == 1 for _, _, b, n, _ in tiled), log  # ONE launch per tiled resampling block
        attn = [r for r in log if r[0] == "attention"]
        assert len(attn) == 4 and all(b == E and n == 1 and ok for _, _, b, n, ok in attn), log  # ONE launch per block, batch E
        assert [r[0] for r in single_log] == [r[0] for r in log]

    # ---- back to single edits
    model.set_masks(m.pyrs[1])
    assert [tuple(b.shape) for b in model.res_buffers()] == m.single_shapes
    with torch.no_grad():
        model(m.edits[1], logsnr)
        assert torch.equal(model(m.edits[1], logsnr), m.singles[1])


def test_no_whole_tensor_elementwise_or_pooling_kernel_at_the_tiled_levels_under_stacked_edits():
    from sige_amd import stacked

    with stacked_model() as m:
        with stacked.edit_batch(m.model, E):
            assert _tall_level_ops(m.model, m.xs, m.logsnr, (16,)) == []


def test_stacked_forward_graph_replay_is_bit_identical():
    from sige_amd import stacked

    with stacked_model() as m, torch.no_grad():
        model, logsnr, xs = m.model, m.logsnr, m.xs
        with stacked.edit_batch(model, E):
            eager = model(xs, logsnr).clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model(xs, logsnr)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model(xs, logsnr)
            for _ in range(2):
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
        for e in range(E):
            assert float((out[e] - m.singles[e][0]).abs().max()) <= util.SELF_ATOL


def _stacked_forward(channels_last=True, mode="sparse", batch=2):
    from sige_amd import hip, stacked

    model, logsnr = build("cuda", channels_last)
    pyrs = pyramids("cuda")[:2]
    x0, edits = edit_inputs("cuda")
    with torch.no_grad():
        model.set_mode("full")
        model(_fmt(x0, channels_last), logsnr)
        model.set_mode("sparse")
        stacked.stack_caches(model, 2)
        try:
            stacked.set_masks(model, pyrs)
            model.set_mode(mode)
            with stacked.edit_batch(model, 2):
                model(_fmt(torch.cat(edits[:batch], 0), channels_last), logsnr)
        finally:
            stacked.unstack_caches(model)
            assert hip.get_edit_batch() == 1 and model.edit_batch == 1


def test_nchw_refuses_stacked_edits():
    with pytest.raises(RuntimeError, match="stacked"):
        _stacked_forward(channels_last=False)


def test_the_torch_chain_of_the_resampling_blocks_refuses_stacked_edits():
    from sige_amd.workloads import pd_unet

    keep = pd_unet.FUSED_RESAMPLE
    pd_unet.FUSED_RESAMPLE = False
    try:
        with pytest.raises(RuntimeError, match="stacked"):
            _stacked_forward()
    finally:
        pd_unet.FUSED_RESAMPLE = keep


def test_full_mode_and_an_input_batch_that_is_not_the_edit_batch_are_refused():
    with pytest.raises(RuntimeError, match="stacked"):
        _stacked_forward(mode="full")
    with pytest.raises(RuntimeError, match="stacked"):
        _stacked_forward(batch=1)


def test_pd128_two_stacked_edits():
    """church_pd128-sige.yml, E = 2, no CPU run: edit 0 is the fixture's edit (the reference's sparse output), edit 1 the fixture's
    image under the second mask, against its own single-edit forward."""
    from sige_amd import hip, stacked

    cfg, size = pd_inputs.PD128, 128
    masks = [pd_inputs.edit_mask(size), pd_inputs.edit_mask(size, second=True)]
    model, logsnr = build("cuda", True, cfg)
    pyrs = pyramids("cuda", cfg, masks)
    x0, noise = pd_inputs.images(size)
    edits = [_fmt((x0 + noise * m).cuda()) for m in masks]  # (the fixture's noise for both)
    x0 = _fmt(x0.cuda())
    with torch.no_grad():
        model.set_cache_id(0)
        model.set_mode("full")
        full = model(x0, logsnr).clone()
        model.set_mode("sparse")
        model.set_masks(pyrs[1])
        model(edits[1], logsnr)
        n0 = hip.launch_count()
        single = model(edits[1], logsnr).clone()
        single_launches = hip.launch_count() - n0
        stacked.stack_caches(model, 2)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, 2):
                model(_fmt(torch.cat(edits, 0)), logsnr)
                n0 = hip.launch_count()
                got = model(_fmt(torch.cat(edits, 0)), logsnr).clone()
                launches = hip.launch_count() - n0
        finally:
            stacked.unstack_caches(model)
    assert hip.get_edit_batch() == 1
    util.assert_finite(got, "pd128 stacked output")
    print("pd_unet pd128: %d library launches stacked (E=2), %d single" % (launches, single_launches))
    _record_launches("pd128", 2, launches, single_launches)
    check_pd128(full, got[0:1], util.CONV_ATOL, lambda what, value, tol: util.record_margin(TEST + " pd128 E=2 edit 0", what, value, tol))
    own = float((got[1] - single[0]).abs().max())
    print("pd_unet pd128 E=2 edit 1: vs single %.3e" % own)
    util.record_margin(TEST + " pd128 E=2 vs single", "edit 1", own, util.SELF_ATOL)
    assert own <= util.SELF_ATOL, own
    assert float((got[0] - got[1]).abs().max()) > 1e-2
