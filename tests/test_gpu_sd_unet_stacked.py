"""Stacked edits (sige_amd/stacked.py) through the Stable Diffusion U-Net (sige_amd.workloads.sd_unet): E = 2 and 4 edits of one
original under one prompt, each with its own mask, in ONE forward on the GPU.

Configuration: SDConfig(model_channels=64, num_res_blocks=1, num_heads=4, context_dim=96) (tests/ref_runner_models.py) with the weights
of tests/golden/model_init.init_by_name, latent [1,4,64,64] -- every level's per-image height (64, 32, 16, 8) is a power of two >= 4;
the heads are 16 / 32 / 64 channels wide --, context [1,77,96], one timestep.  Edits: four ~5 % masks -- one on the bottom rows, one on
the top rows (in the tall tensor the first lies across a seam from the second), two rectangles; edit e adds (1 + e) x its own noise
inside its mask.

Model level: every edit's slice of one stacked forward against THAT edit's own sparse forward of the same weights on the CPU with the
oracle as native back end (util.CONV_ATOL), and against the same model's single-edit GPU forward (util.SELF_ATOL).  The SD U-Net owns
no persistent buffer that a forward rewrites as a whole (the attention's output is a fresh tensor; the in-place Scatter buffers ARE
the cache outside the tiles), so what a missed store would leave behind is made wrong two ways: the measured forward allocates under
util.poisoned (NaN), and the warm-up forward before it ran on OTHER inputs, so every tile of every persistent buffer holds another
edit's values.  A spy on hip.attention_tokens shows every tiled self-attention went through `tiles=` in one library launch.

Block level: one tiled SpatialTransformer (input_blocks.5.1: 256 channels, 4 heads of 64, 16 x 16 tokens per image) alone on the tall
tensor against the block in fp64 on each edit's own image, on the cells of the active tiles; bound tests/attention_stress.bound.  The
test also computes in fp64 what `the keys of all E images` would give and asserts it is >= 10 bounds away (16 and 30 bounds at E = 2
and 4 in fp64 on the CPU; at 32 x 32 tokens an edit's ~50 changed keys among 1024 move the output by 6 to 9 bounds only, which is why
the block is this one).

Margins go through util.record_margin (kept as profiles/sd_unet_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import util  # noqa: E402
from tests.attention_stress import bound as attention_bound  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
CL = torch.channels_last
LATENT, IMAGE = 64, 512


# ---- the model, the edits ---------------------------------------------------------------------------------------------------------
def build_model(device, inplace=True):
    from sige_amd.workloads.sd_unet import SDConfig, SDUNet
    from tests.golden.model_init import init_by_name

    model = SDUNet(SDConfig(model_channels=64, num_res_blocks=1, num_heads=4, context_dim=96)).eval()
    init_by_name(model)
    if device != "cpu":
        model = model.to(device).to(memory_format=CL)
        model.set_scatter_inplace(inplace)
    return model


def edit_masks():
    """[4 x bool [512,512]]: ~5 % each -- the bottom rows, the top rows, two rectangles."""
    m = [torch.zeros(IMAGE, IMAGE, dtype=torch.bool) for _ in range(4)]
    m[0][IMAGE - 64:, 80:285] = True
    m[1][:64, 250:455] = True
    m[2][100:214, 60:175] = True
    m[3][300:414, 330:445] = True
    return m


def pyramids(device):
    from sige_amd.utils import downsample_mask

    return [downsample_mask(m.to(device), min_res=8, dilation=1) for m in edit_masks()]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def inputs(pyrs, device, seed=900):
    """(original [1,4,64,64], [edited input of edit e], timestep [1], context [1,77,96]) NCHW on `device`."""
    x0 = _randn((1, 4, LATENT, LATENT), 4).to(device)
    edits = [x0 + (1.0 + e) * _randn(x0.shape, seed + e).to(device) * p[(LATENT, LATENT)].to(device) for e, p in enumerate(pyrs)]
    return x0, edits, torch.full((1,), 500.0, device=device), _randn((1, 77, 96), 5).to(device)


def _cl(x):
    return x.contiguous(memory_format=CL)


_oracle = {}


def oracle_outputs():
    """Each edit's own sparse forward on the CPU, oracle back end: computed once per process and left unchanged."""
    if not _oracle:
        from oracle import oracle
        from sige_amd import runtime

        model = build_model("cpu")
        pyrs = pyramids("cpu")
        x0, edits, ts, ctx = inputs(pyrs, "cpu")
        torch.set_num_threads(8)
        runtime.register_backend("cpu", oracle)
        try:
            with torch.no_grad():
                model.set_mode("full")
                model(x0, ts, context=ctx)
                model.set_mode("sparse")
                outs = []
                for e, xe in enumerate(edits):
                    model.set_masks(pyrs[e])
                    outs.append(model(xe, ts, context=ctx)[0].clone())
        finally:
            runtime.unregister_backend("cpu")
        assert float((outs[0] - outs[1]).abs().max()) > 1e-2  # (the edits do differ)
        _oracle["outs"] = outs
    return _oracle["outs"]


class spied_attention:
    """hip.attention_tokens with every call written down: (q batch, keys, per-image form?, library launches, served?)."""

    def __init__(self, hip):
        self.hip, self.log = hip, []

    def __enter__(self):
        hip, log = self.hip, self.log
        self.keep = orig = hip.attention_tokens

        def spied(q, k, v, *a, **kw):
            n0 = hip.launch_count()
            out = orig(q, k, v, *a, **kw)
            log.append((q.shape[0], k.shape[1], kw.get("tiles") is not None, hip.launch_count() - n0, out is not None))
            return out

        hip.attention_tokens = spied
        return log

    def __exit__(self, *exc):
        self.hip.attention_tokens = self.keep
        return False


class switches:
    """Module-level switches of sd_transformer for the duration of a `with`."""

    def __init__(self, **kw):
        from sige_amd.workloads import sd_transformer

        self.sdt, self.kw = sd_transformer, kw

    def __enter__(self):
        self.keep = {k: getattr(self.sdt, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.sdt, k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            setattr(self.sdt, k, v)
        return False


class repeatable_dense_ops:
    """torch.backends.cudnn.deterministic for the duration of a `with`.  The dense middle block of the SD U-Net runs on the framework's
    operators, and without the flag two consecutive single-edit forwards of this model on the same inputs were seen to differ in about
    half the output elements by up to 1.6e-7 (first at middle_block.0, 4.8e-7 there; measured before any stacking, on one machine and
    not on another) -- a bit-for-bit comparison of two forwards would then say nothing about the caches."""

    def __enter__(self):
        self.keep = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        return self

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.keep
        return False


def _tiled_transformers(model):
    from sige_amd.workloads.sd_transformer import SpatialTransformer

    return [m for m in model.modules() if isinstance(m, SpatialTransformer) and m.tiled]


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,inplace,switch", [(2, True, {}), (4, True, {}), (2, False, {}), (2, True, {"TOKEN_LINEAR": True}),
                                              (2, True, {"ATTENTION_COMPUTE": "f16"})],
                         ids=["E2", "E4", "E2-fresh-scatters", "E2-token-linear", "E2-f16-attention"])
def test_stacked_edits_vs_cpu_oracle_and_single_edits(E, inplace, switch):
    from sige_amd import hip, stacked
    from sige_amd.tolerance import f16_check

    f16 = switch.get("ATTENTION_COMPUTE") == "f16"
    want = oracle_outputs()
    model = build_model("cuda", inplace)
    pyrs = pyramids("cuda")[:E]
    x0, edits, ts, ctx = inputs(pyrs, "cuda")
    others = inputs(pyrs, "cuda", seed=950)[1]  # (the warm-up's inputs: other noise under the same masks)
    x0, edits, others = _cl(x0), [_cl(x) for x in edits], [_cl(x) for x in others]
    run = lambda x: model(x, ts, context=ctx)  # noqa: E731
    with torch.no_grad(), switches(**switch), repeatable_dense_ops():
        model.set_mode("full")
        run(x0)
        model.set_mode("sparse")
        singles = []
        for e in range(E):
            model.set_masks(pyrs[e])
            run(edits[e])  # (the first forward under a mask packs weights and sizes buffers: not the steady state)
            singles.append(run(edits[e]).clone())
        n0 = hip.launch_count()
        with spied_attention(hip) as single_log:
            run(edits[-1])
        single_launches = hip.launch_count() - n0
        assert single_log and all(not tiles and served for _, _, tiles, _, served in single_log)

        xs, warm = _cl(torch.cat(edits, 0)), _cl(torch.cat(others, 0))
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                run(warm)
                n0 = hip.launch_count()
                with spied_attention(hip) as log, util.poisoned() as p:
                    got = run(xs).clone()
                launches = hip.launch_count() - n0
        finally:
            stacked.unstack_caches(model)
        assert hip.get_edit_batch() == 1 and model.edit_batch == 1
        assert p.n > 0
        assert tuple(got.shape) == (E,) + tuple(singles[0].shape[1:])
        util.assert_finite(got, "stacked output")
        print("sd_unet E=%d inplace=%d %s: %d library launches stacked, %d single" % (E, inplace, switch, launches, single_launches))
        # every tiled self-attention (one query batch, keys that are not the 77 text tokens): the per-image form, ONE launch, served
        tiled = [c for c in log if c[0] == 1 and c[1] != 77]
        assert len(tiled) == len(_tiled_transformers(model)) * model.cfg.transformer_depth, log
        assert all(tiles and n == 1 and served for _, _, tiles, n, served in tiled), log
        assert all(keys == E * (LATENT >> s) ** 2 for (_, keys, _, _, _), s in zip(tiled, (0, 1, 2, 2, 2, 1, 1, 0, 0))), log
        assert all(served and not tiles for b, keys, tiles, _, served in log if not (b == 1 and keys != 77)), log
        assert launches <= single_launches, (launches, single_launches)
        for e in range(E):
            own = float((got[e] - singles[e][0]).abs().max())
            if f16:
                chk = f16_check(got[e], singles[e][0])
                print("sd_unet f16 attention E=%d edit %d: vs single %s" % (E, e, chk))
                util.record_margin("sd_unet_stacked f16 attention vs single", "E=%d edit %d" % (E, e), chk["worst_over_allowed"], 1.0)
                assert chk["ok"], (e, chk)
                continue
            err = float((got[e].cpu() - want[e]).abs().max())
            print("sd_unet E=%d inplace=%d %s edit %d: vs oracle %.3e, vs single %.3e" % (E, inplace, switch, e, err, own))
            util.record_margin("sd_unet_stacked vs oracle", "E=%d inplace=%d %s edit %d" % (E, inplace, switch, e), err, util.CONV_ATOL)
            util.record_margin("sd_unet_stacked vs single", "E=%d inplace=%d %s edit %d" % (E, inplace, switch, e), own, util.SELF_ATOL)
            assert err <= util.CONV_ATOL, (e, err)
            assert own <= util.SELF_ATOL, (e, own)
        assert float((got[0] - got[1]).abs().max()) > 1e-2  # (the edits do differ)
        # back to single edits: the caches are the original's again
        model.set_masks(pyrs[1])
        run(edits[1])
        again = run(edits[1])
        print("sd_unet E=%d: single edit after unstack_caches, max |after - before| %.3e" % (E, float((again - singles[1]).abs().max())))
        assert torch.equal(again, singles[1])


# ---- block level ------------------------------------------------------------------------------------------------------------------
def _mha(q, k, v, heads, scale):
    b, n, c = q.shape
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, c // heads).permute(0, 2, 1, 3)  # noqa: E731
    o = torch.softmax(split(q) @ split(k).transpose(2, 3) * scale, dim=3) @ split(v)
    return o.permute(0, 2, 1, 3).reshape(b, n, c)


def block_reference(st, xs, ctx, dtype, all_images=False):
    """A tiled SpatialTransformer in sparse mode on every edit's own image in `dtype`: [E,C,h,w] (meaningful on the active tiles; a
    sparse forward returns the original's cached output elsewhere).  xs [E,C,h,w] equal the original outside the tiles and every map
    in front of the attention is per token, so K / V of the whole image under the cached affine ARE the persistent tensors'.
    `all_images`: the self-attention's softmax runs over the keys of all E images -- the batched entry on the tall K / V."""
    E, C, h, w = xs.shape
    d = lambda t: t.detach().to(dtype)  # noqa: E731
    lin = lambda m, y: F.linear(y, d(m.weight), None if m.bias is None else d(m.bias))  # noqa: E731
    ln = lambda m, y: F.layer_norm(y, (y.shape[-1],), d(m.weight), d(m.bias), m.eps)  # noqa: E731
    x = xs.to(dtype)
    z = F.conv2d(x * d(st.scale) + d(st.shift), d(st.proj_in.weight), d(st.proj_in.bias))
    z = z.permute(0, 2, 3, 1).reshape(E, h * w, -1)
    blk = st.transformer_blocks[0]
    a1, a2, ff = blk.attn1, blk.attn2, blk.ff
    xn = ln(blk.norm1, z)
    q, k, v = lin(a1.to_q, xn), lin(a1.to_k, xn), lin(a1.to_v, xn)
    if all_images:
        k, v = (t.reshape(1, E * h * w, -1).expand(E, -1, -1) for t in (k, v))
    z = lin(a1.to_out[0], _mha(q, k, v, a1.heads, a1.scale)) + z
    c = ctx.to(dtype).expand(E, -1, -1)
    z = lin(a2.to_out[0], _mha(lin(a2.to_q, ln(blk.norm2, z)), lin(a2.to_k, c), lin(a2.to_v, c), a2.heads, a2.scale)) + z
    a, gate = lin(ff.net[0].proj, ln(blk.norm3, z)).chunk(2, dim=-1)
    z = lin(ff.net[2], a * F.gelu(gate)) + z
    z = z.reshape(E, h, w, -1).permute(0, 3, 1, 2)
    return F.conv2d(z, d(st.proj_out.weight), d(st.proj_out.bias)) + x


def block_inputs(model, st, E, device):
    """(the transformer's input under the original [1,C,h,w], [E,C,h,w] edited inputs, pyramids, context): edit e adds (1 + e) x noise
    inside its mask at the block's resolution.  The model is left in sparse mode behind the full pass on the original."""
    pyrs = pyramids(device)[:E]
    x0, _, ts, ctx = inputs(pyrs, device)
    seen = []
    hook = st.register_forward_hook(lambda m, args, out: seen.append(args[0].detach().clone()))
    try:
        with torch.no_grad():
            model.set_mode("full")
            model(_cl(x0) if device != "cpu" else x0, ts, context=ctx)
    finally:
        hook.remove()
    model.set_mode("sparse")
    h0 = seen[0]
    res = tuple(h0.shape[2:])
    xs = torch.cat([h0 + (1.0 + e) * _randn(h0.shape, 800 + e).to(device) * p[res].to(device) for e, p in enumerate(pyrs)])
    return h0, xs, pyrs, ctx


def _tile_cells(indices, E, h, w, device):
    cells = torch.zeros(E * h, w, dtype=torch.bool, device=device)
    for r, c in indices.tolist():
        cells[max(r, 0):r + 4, max(c, 0):c + 4] = True
    return cells.reshape(E, h, w)


@pytest.mark.parametrize("E", [2, 4])
def test_transformer_on_the_tall_tensor_vs_fp64_per_image(E):
    from sige_amd import hip, stacked

    model = build_model("cuda")
    st = model.input_blocks[5][1]
    h0, xs, pyrs, ctx = block_inputs(model, st, E, "cuda")
    _, _, h, w = h0.shape
    xs = _cl(xs)
    with torch.no_grad():
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                st(stacked.tall(_cl(xs.flip(0))), ctx)  # (sizes buffers; other values on the tiles of every persistent buffer)
                with spied_attention(hip) as log, util.poisoned():
                    got = stacked.untall(st(stacked.tall(xs), ctx), E).clone()
            cells = _tile_cells(st.gather.active_indices, E, h, w, "cuda")
            cached = stacked.untall(st.scatter2.original_outputs[st.cache_id], E).clone()
        finally:
            stacked.unstack_caches(model)
        assert [c[2:] for c in log] == [(True, 1, True), (False, 1, True)], log  # (self-attention per image, cross-attention)
        util.assert_finite(got, "stacked transformer")
        assert all(int(cells[e].sum()) > 0 for e in range(E))
        want = block_reference(st, xs, ctx, torch.float64)
        ref32 = block_reference(st, xs, ctx, torch.float32)
        mixed = block_reference(st, xs, ctx, torch.float64, all_images=True)
        on = cells[:, None].expand_as(want)
        bound = attention_bound(want[on], (ref32.double() - want)[on].abs().max())
        err = float((got.double() - want)[on].abs().max())
        bug = float((mixed - want)[on].abs().max())
        print("sd_unet transformer E=%d: err %.3e, bound %.3e, keys of all images %.3e away" % (E, err, bound, bug))
        util.record_margin("sd_unet_stacked transformer vs fp64", "E=%d" % E, err, bound)
        assert bug >= 10.0 * bound, "the inputs cannot see keys read from a neighbouring image: %.3e < 10 x %.3e" % (bug, bound)
        assert err <= bound, "max |diff| %.3e > %.3e" % (err, bound)
        assert torch.equal(got[~on], cached[~on])  # (outside the active tiles: the original's cached output, bit for bit)


# ---- no silent wrong answer -------------------------------------------------------------------------------------------------------
def _stacked_forward(channels_last=True, before=None, E=2):
    from sige_amd import hip, stacked

    model = build_model("cuda")
    pyrs = pyramids("cuda")[:E]
    x0, edits, ts, ctx = inputs(pyrs, "cuda")
    fmt = _cl if channels_last else (lambda t: t.contiguous())
    with torch.no_grad():
        model.set_mode("full")
        model(_cl(x0), ts, context=ctx)
        model.set_mode("sparse")
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            if before is not None:
                before(model)
            with stacked.edit_batch(model, E):
                model(fmt(torch.cat(edits[:E], 0)), ts, context=ctx)
        finally:
            stacked.unstack_caches(model)
            assert hip.get_edit_batch() == 1


@pytest.mark.parametrize("switch", [{"NATIVE_ATTENTION": False}, {"FUSED_TOKENS": False}, {"NATIVE_LINEAR": True}],
                         ids=["torch-chain", "unfused-branch", "native-linear"])
def test_a_switch_without_a_per_image_form_refuses_stacked_edits(switch):
    with switches(**switch), pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward()


def test_profile_mode_refuses_stacked_edits():
    def profile(model):
        for m in _tiled_transformers(model):
            m.set_mode("profile")
            for blk in m.transformer_blocks:
                blk.set_mode("profile")

    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward(before=profile)


def test_reprojected_keys_refuse_stacked_edits():
    def reproject(model):
        for m in _tiled_transformers(model):
            m.sparse_kv = False

    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward(before=reproject)


def test_a_none_from_the_library_refuses_stacked_edits(monkeypatch):
    from sige_amd import hip

    orig = hip.attention_tokens
    monkeypatch.setattr(hip, "attention_tokens", lambda *a, **kw: None if kw.get("tiles") is not None else orig(*a, **kw))
    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward()
    with switches(TOKEN_LINEAR=True), pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward()


def test_nchw_refuses_stacked_edits():
    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward(channels_last=False)


def test_a_guidance_pair_in_the_full_pass_refuses_stacked_edits():
    """B = 2 in the full pass: the caches are two samples'.  stack_caches refuses them (its own words), and a stacked forward on such a
    model refuses the per-sample affines before any launch, naming stacked edits."""
    from sige_amd import hip, stacked

    model = build_model("cuda")
    pyrs = pyramids("cuda")[:2]
    x0, edits, ts, ctx = inputs(pyrs, "cuda")
    with torch.no_grad():
        model.set_mode("full")
        model(_cl(x0.expand(2, -1, -1, -1)), ts.expand(2), context=ctx.expand(2, -1, -1))
        model.set_mode("sparse")
        with pytest.raises(RuntimeError, match="one original"):
            stacked.stack_caches(model, 2)
        stacked.unstack_caches(model)
        before = hip.launch_count()
        with stacked.edit_batch(model, 2):
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(_cl(torch.cat(edits, 0)), ts, context=ctx)
        assert hip.launch_count() == before
    assert hip.get_edit_batch() == 1 and model.edit_batch == 1


def test_an_input_batch_that_is_not_the_edit_batch_and_full_mode_are_refused():
    from sige_amd import hip, stacked

    model = build_model("cuda")
    pyrs = pyramids("cuda")[:2]
    x0, edits, ts, ctx = inputs(pyrs, "cuda")
    x0 = _cl(x0)
    with torch.no_grad():
        model.set_mode("full")
        model(x0, ts, context=ctx)
        with stacked.edit_batch(model, 2):
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(_cl(torch.cat([x0, x0])), ts, context=ctx)  # (full mode stays one original)
            model.set_mode("sparse")
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(x0, ts, context=ctx)
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(_cl(torch.cat([x0, x0])), torch.tensor([500.0, 400.0], device="cuda"), context=ctx)  # (two timesteps)
    assert hip.get_edit_batch() == 1 and model.edit_batch == 1
