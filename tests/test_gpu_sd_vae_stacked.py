"""Stacked edits (sige_amd/stacked.py) through the SD VAE decoder and encoder (sige_amd.workloads.sd_vae): E = 2 and 4 edits of one
original, each with its own mask, in ONE forward on the GPU.

Configuration: vae_inputs.SMALL at latent 16 and the encoder's small fixture configuration at image 64 -- every level's per-image
height (16, 32, 64) is a power of two >= 4, and the middle block is 192 channels wide: its attention takes hip.attention_wide, here
with the keys of a tile's own image (sige_hip_attention_wide_tiles_f32).  Edits: the two ~5 % rectangles of vae_inputs.edit_mask, a
third on the bottom rows, a fourth on the left columns -- in the tall tensor edit 1's last rows lie over edit 2's first ones; edit e
adds (1 + e) x its own noise (another seed per edit) inside its mask.

Block level: mid.attn_1 alone on the tall tensor against the block in fp64 on that edit's own image (the cached affine, 1x1 convs,
softmax over the image's own 256 keys, proj_out, residual), on the cells of the active tiles.  Bound: the rule of the attention
tests (tests/attention_stress.bound: four times the error of the same chain in fp32 on the GPU, never below 2e-5 (1 + max |truth|)).
The test also computes in fp64 what `the keys of all E images` would give and asserts it is >= 10 bounds away from the truth: the
inputs can see the bug.

Model level, decoder forward() and encoder encode() with per-edit noise: every edit's slice of one stacked forward against THAT
edit's own sparse forward of the same weights on the CPU with the oracle as native back end (util.CONV_ATOL; the way of
test_second_mask_without_a_new_full_pass_vs_cpu_oracle), and against the same model's single-edit GPU forward (util.SELF_ATOL).
Margins go through util.record_margin (kept as profiles/sd_vae_stacked_test_margins.jsonl)."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import test_sd_vae as dec  # noqa: E402
from tests import test_sd_vae_encoder as enc  # noqa: E402
from tests import util  # noqa: E402
from tests.attention_stress import bound as attention_bound  # noqa: E402
from tests.golden import vae_encoder_inputs as enc_inputs  # noqa: E402
from tests.golden import vae_inputs  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
CL = torch.channels_last
SMALL, LATENT, IMAGE = vae_inputs.SMALL, 16, 64
CFG = {"decoder": SMALL, "encoder": enc_inputs.SMALL}
SCALE_FACTOR = 0.18215


# ---- the edits ------------------------------------------------------------------------------------------------------------------
def edit_masks():
    """[4 x bool [64,64]]: ~5 % each."""
    a, b = int(round(IMAGE * 0.22)), int(round(0.05 * IMAGE * IMAGE / int(round(IMAGE * 0.22))))
    third = torch.zeros(IMAGE, IMAGE, dtype=torch.bool)
    third[IMAGE - b:, 9:9 + a] = True   # the bottom rows
    fourth = torch.zeros(IMAGE, IMAGE, dtype=torch.bool)
    fourth[22:22 + a, :b] = True        # the left columns
    return [vae_inputs.edit_mask(IMAGE), vae_inputs.edit_mask(IMAGE, True), third, fourth]


def pyramids(kind, device):
    from sige_amd.utils import dilate_mask, downsample_mask

    return [vae_inputs.pyramid(m.to(device), CFG[kind], dilate_mask, downsample_mask) for m in edit_masks()]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def edit_inputs(kind, pyrs, device):
    """(original [1,c,s,s], [edited input of edit e], [posterior noise of edit e] (encoder) or None), NCHW on `device`."""
    if kind == "decoder":
        z0 = vae_inputs.latents(SMALL, LATENT, 0)[0].to(device)
        edits = [z0 + (1.0 + e) * _randn(z0.shape, 500 + e).to(device) * p[(LATENT, LATENT)].to(device) for e, p in enumerate(pyrs)]
        return z0, edits, None
    x0 = enc_inputs.images(enc_inputs.SMALL, IMAGE, 0)[0].to(device)
    edits = [x0 + (1.0 + e) * _randn(x0.shape, 600 + e).to(device) * m.to(device) for e, m in enumerate(edit_masks())]
    noise = [_randn((1, SMALL["z_channels"], LATENT, LATENT), 700 + e).to(device) for e in range(len(pyrs))]
    return x0, edits, noise


def build(kind, device, channels_last=True, inplace=True, cfg=None):
    """(model, run): run(x, noise) -> the output compared ([B,3,64,64] / the posterior sample z [B,4,16,16] next to the moments)."""
    if kind == "decoder":
        model = dec.build_model(cfg or SMALL, device, channels_last, inplace)
        return model, lambda x, noise=None: model(x)
    model, quant = enc.build_model(cfg or enc_inputs.SMALL, device, channels_last, inplace)
    return model, lambda x, noise=None: torch.cat(model.encode(x, quant, noise=noise, scale_factor=SCALE_FACTOR), dim=1)


def _fmt(x, channels_last):
    return x.contiguous(memory_format=CL) if channels_last else x.contiguous()


_oracle = {}


def oracle_outputs(kind):
    """Each edit's own sparse forward on the CPU, oracle back end: computed once per process and left unchanged."""
    if kind not in _oracle:
        from oracle import oracle
        from sige_amd import runtime

        model, run = build(kind, "cpu", False, False)
        pyrs = pyramids(kind, "cpu")
        x0, edits, noise = edit_inputs(kind, pyrs, "cpu")
        torch.set_num_threads(8)
        runtime.register_backend("cpu", oracle)
        try:
            with torch.no_grad():
                model.set_mode("full")
                run(x0, None if noise is None else noise[0])
                model.set_mode("sparse")
                outs = []
                for e, xe in enumerate(edits):
                    model.set_masks(pyrs[e])
                    outs.append(run(xe, None if noise is None else noise[e])[0].clone())
        finally:
            runtime.unregister_backend("cpu")
        assert float((outs[0] - outs[1]).abs().max()) > 1e-2  # (the edits do differ)
        _oracle[kind] = outs
    return _oracle[kind]


class counted_attention:
    """hip.attention_wide with every call written down: (per-image form?, library launches, served?)."""

    def __init__(self, hip):
        self.hip, self.log = hip, []

    def __enter__(self):
        hip, log = self.hip, self.log
        self.keep = orig = hip.attention_wide

        def counted(*a, **kw):
            n0 = hip.launch_count()
            out = orig(*a, **kw)
            log.append((kw.get("tiles") is not None, hip.launch_count() - n0, out is not None))
            return out

        hip.attention_wide = counted
        return log

    def __exit__(self, *exc):
        self.hip.attention_wide = self.keep
        return False


def _first_conv_launches(kind, model, x):
    """Library launches of the first conv alone in the model's present state (the decoder's 4-channel conv_in is the GEMM library's
    in both forms: 0)."""
    from sige_amd import hip

    if kind == "decoder":
        return 0
    n0 = hip.launch_count()
    model._conv_in(x)
    return hip.launch_count() - n0


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E,inplace", [("decoder", 2, False), ("decoder", 4, True), ("encoder", 2, True), ("encoder", 4, True),
                                            ("encoder", 2, False)])
def test_stacked_edits_vs_cpu_oracle_and_single_edits(kind, E, inplace):
    from sige_amd import hip, stacked

    want = oracle_outputs(kind)
    model, run = build(kind, "cuda", True, inplace)
    pyrs = pyramids(kind, "cuda")[:E]
    x0, edits, noise = edit_inputs(kind, pyrs, "cuda")
    x0, edits = _fmt(x0, True), [_fmt(x, True) for x in edits[:E]]
    nz = (lambda e: None) if noise is None else (lambda e: noise[e])
    with torch.no_grad():
        model.set_mode("full")
        run(x0, nz(0))
        model.set_mode("sparse")
        singles = []
        for e in range(E):
            model.set_masks(pyrs[e])
            run(edits[e], nz(e))  # (the first forward under a mask packs weights and sizes buffers: not the steady state)
            singles.append(run(edits[e], nz(e)).clone())
        first_single = _first_conv_launches(kind, model, edits[-1])
        n0 = hip.launch_count()
        with counted_attention(hip) as single_log:
            run(edits[-1], nz(E - 1))
        single_launches = hip.launch_count() - n0
        assert single_log == [(False, 1, True)]

        xs = _fmt(torch.cat(edits, 0), True)
        ns = None if noise is None else torch.cat(noise[:E], 0)
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                run(xs, ns)
                for name, buf, rewritten in model.persistent_buffers():
                    if rewritten:
                        buf.fill_(float("nan"))  # (the attention's output rows: every destination holds NaN before the launch)
                first_stacked = _first_conv_launches(kind, model, xs)
                n0 = hip.launch_count()
                with counted_attention(hip) as log:
                    got = run(xs, ns).clone()
                launches = hip.launch_count() - n0
        finally:
            stacked.unstack_caches(model)
        assert hip.get_edit_batch() == 1 and model.edit_batch == 1
        assert got.shape[0] == E and tuple(got.shape[1:]) == tuple(singles[0].shape[1:])
        util.assert_finite(got, "stacked output")
        print("sd_vae %s E=%d inplace=%d: %d library launches stacked, %d single (first conv %d / %d)"
              % (kind, E, inplace, launches, single_launches, first_stacked, first_single))
        assert log == [(True, 1, True)], log  # exactly ONE attention launch, the per-image form
        assert launches <= single_launches + (first_stacked - first_single), (launches, single_launches, first_stacked, first_single)
        for e in range(E):
            err = float((got[e].cpu() - want[e]).abs().max())
            own = float((got[e] - singles[e][0]).abs().max())
            print("sd_vae %s E=%d edit %d: vs oracle %.3e, vs single %.3e" % (kind, E, e, err, own))
            util.record_margin("sd_vae_stacked %s vs oracle" % kind, "E=%d inplace=%d edit %d" % (E, inplace, e), err, util.CONV_ATOL)
            util.record_margin("sd_vae_stacked %s vs single" % kind, "E=%d inplace=%d edit %d" % (E, inplace, e), own, util.SELF_ATOL)
            assert err <= util.CONV_ATOL, (e, err)
            assert own <= util.SELF_ATOL, (e, own)
        assert float((got[0] - got[1]).abs().max()) > 1e-2  # (the edits do differ)
        # back to single edits: the caches are the original's again
        model.set_masks(pyrs[1])
        run(edits[1], nz(1))
        assert torch.equal(run(edits[1], nz(1)), singles[1])


# ---- block level ------------------------------------------------------------------------------------------------------------------
def _block_reference(attn, xs, cells, dtype, all_images=False):
    """mid.attn_1 in sparse mode on every edit's own image in `dtype`: [E,C,h,w] (meaningful on `cells` [E,h,w], the active tiles;
    a sparse forward returns the original's cached output elsewhere).  xs [E,C,h,w] equal the original outside `cells`, so K | V
    of the whole image under the cached affine ARE the persistent tensor's.  `all_images`: the softmax runs over the keys of all E
    images -- what the batched attention entry computes on the tall K | V."""
    s, t = (v.to(dtype) for v in attn.affine[attn.cache_id])
    E, C, h, w = xs.shape
    x = xs.to(dtype)
    hn = x * s + t
    conv = lambda m, y: torch.nn.functional.conv2d(y, m.weight.to(dtype), m.bias.to(dtype))  # noqa: E731
    q, k, v = (conv(m, hn).reshape(E, C, h * w).permute(0, 2, 1) for m in (attn.q, attn.k, attn.v))  # [E,hw,C]
    if all_images:
        k = k.reshape(1, E * h * w, C).expand(E, -1, -1)
        v = v.reshape(1, E * h * w, C).expand(E, -1, -1)
    o = torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (C ** -0.5), dim=2), v)
    return x + conv(attn.proj_out, o.permute(0, 2, 1).reshape(E, C, h, w))


def block_inputs(model, E, device):
    """(the middle attention's input under the original [1,C,16,16], [E,C,16,16] edited inputs, pyramids): edit e adds (1 + e) x
    noise inside its mask at the latent's resolution.  The model is left in sparse mode behind the full pass on the original."""
    pyrs = pyramids("decoder", device)[:E]
    z0 = _fmt(vae_inputs.latents(SMALL, LATENT, 0)[0].to(device), device != "cpu")
    seen = []
    hook = model.mid.attn_1.register_forward_hook(lambda m, args, out: seen.append(args[0].detach().clone()))
    try:
        with torch.no_grad():
            model.set_mode("full")
            model(z0)
    finally:
        hook.remove()
    model.set_mode("sparse")
    x0 = seen[0]
    xs = torch.cat([x0 + (1.0 + e) * _randn(x0.shape, 800 + e).to(device) * p[(LATENT, LATENT)].to(device) for e, p in enumerate(pyrs)])
    return x0, xs, pyrs


def _tile_cells(indices, E, h, w, device):
    cells = torch.zeros(E * h, w, dtype=torch.bool, device=device)
    for r, c in indices.tolist():
        cells[max(r, 0):r + 4, max(c, 0):c + 4] = True
    return cells.reshape(E, h, w)


@pytest.mark.parametrize("E", [2, 4])
def test_attention_block_on_the_tall_tensor_vs_fp64_per_image(E):
    from sige_amd import hip, stacked

    model = dec.build_model(SMALL, "cuda", True, True)
    attn = model.mid.attn_1
    x0, xs, pyrs = block_inputs(model, E, "cuda")
    xs = _fmt(xs, True)
    with torch.no_grad():
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                attn(stacked.tall(xs))  # (sizes buffers, packs the derived K | V weights)
                attn._attn_out.fill_(float("nan"))
                with counted_attention(hip) as log:
                    got = stacked.untall(attn(stacked.tall(xs)), E).clone()
            cells = _tile_cells(attn.gather.active_indices, E, LATENT, LATENT, "cuda")
            cached = stacked.untall(attn.out_scatter.original_outputs[attn.cache_id], E).clone()
        finally:
            stacked.unstack_caches(model)
        assert log == [(True, 1, True)], log
        util.assert_finite(got, "stacked attention block")
        assert all(int(cells[e].sum()) > 0 for e in range(E)) and len({int(cells[e].sum()) for e in range(E)}) > 1  # (uneven lists)
        want = _block_reference(attn, xs, cells, torch.float64)
        ref32 = _block_reference(attn, xs, cells, torch.float32)
        mixed = _block_reference(attn, xs, cells, torch.float64, all_images=True)
        on = cells[:, None].expand_as(want)
        bound = attention_bound(want[on], (ref32.double() - want)[on].abs().max())
        err = float((got.double() - want)[on].abs().max())
        bug = float((mixed - want)[on].abs().max())
        print("sd_vae attention block E=%d: err %.3e, bound %.3e, keys of all images %.3e away" % (E, err, bound, bug))
        util.record_margin("sd_vae_stacked attention block vs fp64", "E=%d" % E, err, bound)
        assert bug >= 10.0 * bound, "the inputs cannot see keys read from a neighbouring image: %.3e < 10 x %.3e" % (bug, bound)
        assert err <= bound, "max |diff| %.3e > %.3e" % (err, bound)
        assert torch.equal(got[~on], cached[~on])  # (outside the active tiles: the original's cached output, bit for bit)


# ---- no silent wrong answer -------------------------------------------------------------------------------------------------------
def _stacked_forward(kind, cfg=None, channels_last=True):
    from sige_amd import hip, stacked

    E = 2
    model, run = build(kind, "cuda", channels_last, channels_last, cfg)
    pyrs = pyramids(kind, "cuda")[:E]
    x0, edits, noise = edit_inputs(kind, pyrs, "cuda")
    ns = None if noise is None else torch.cat(noise[:E], 0)
    with torch.no_grad():
        model.set_mode("full")
        run(_fmt(x0, channels_last), None if noise is None else noise[0])
        model.set_mode("sparse")
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, pyrs)
            with stacked.edit_batch(model, E):
                run(_fmt(torch.cat(edits[:E], 0), channels_last), ns)
        finally:
            stacked.unstack_caches(model)
            assert hip.get_edit_batch() == 1


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_a_middle_block_of_128_channels_refuses_stacked_edits(kind):
    """ch 32 with ch_mult ending in 4: the attention is hip.attention_tokens', which has no per-image form."""
    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward(kind, dict(CFG[kind], ch_mult=(1, 2, 4)))


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_the_torch_chain_refuses_stacked_edits(kind):
    from sige_amd.workloads import sd_vae

    keep = sd_vae.NATIVE_ATTENTION
    sd_vae.NATIVE_ATTENTION = False
    try:
        with pytest.raises(RuntimeError, match="stacked edits"):
            _stacked_forward(kind)
    finally:
        sd_vae.NATIVE_ATTENTION = keep


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_nchw_refuses_stacked_edits(kind):
    with pytest.raises(RuntimeError, match="stacked edits"):
        _stacked_forward(kind, channels_last=False)


def test_an_input_batch_that_is_not_the_edit_batch_and_full_mode_are_refused():
    from sige_amd import stacked

    model = dec.build_model(SMALL, "cuda", True, True)
    z0 = _fmt(vae_inputs.latents(SMALL, LATENT, 0)[0].cuda(), True)
    with torch.no_grad():
        model.set_mode("full")
        model(z0)
        with stacked.edit_batch(model, 2):
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(_fmt(torch.cat([z0, z0]), True))  # (full mode stays one original)
            model.set_mode("sparse")
            with pytest.raises(RuntimeError, match="stacked edits"):
                model(z0)
