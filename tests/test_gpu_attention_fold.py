"""proj_out of the dense attention blocks folded into the value projection (sige_amd/workloads/ddpm_unet.py: fold_proj_into_qkv,
FOLD_ATTN_PROJ), its bias / residual / twins in the epilogue of the attention's second kernel
(include/sige_hip.h: sige_hip_attention_residual_nhwc_f32).

Shapes of the single-launch tests.  The channels-last attention takes C % 64 == 0 only (its score kernel gives each of four waves C/4
channels in 16-channel steps), so at (2, 48, 16) and (1, 32, 272) BOTH entry points answer "unsupported" -- that the new one answers
exactly as the old one is what those two shapes can check.  The kernel paths they name are reached at the nearest supported shapes:
(2, 64, 16) one key step (HW = 16) and the batch stride, (1, 64, 272) the HW > 256 softmax and a second value block,
(1, 128, 16) a second 64-channel workgroup column."""
import pytest
import torch

from tests import util

DEV = "cuda"
SHAPES = [(2, 48, 16), (1, 64, 64), (1, 32, 272), (2, 64, 16), (1, 64, 272), (1, 128, 16)]
_HW = {16: (4, 4), 64: (8, 8), 272: (16, 17)}


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(B, C, HW, n_twins, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + C + HW)
    H, W = _HW[HW]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    qkv, res = _cl(r(B, 3 * C, H, W).to(DEV)), _cl(r(B, C, H, W).to(DEV))
    bias = r(C).to(DEV)
    twins = {("t", k): (r(C).to(DEV), r(C).to(DEV)) for k in range(n_twins)}
    return qkv, bias, res, twins


# ---- 1. no extras: the kernel as it was ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_C%d_HW%d" % s)
def test_all_null_epilogue_equals_attention_cl(hip, shape):
    B, C, HW = shape
    qkv, _, _, _ = _inputs(B, C, HW, 0)
    want = hip.attention_cl(qkv, C ** -0.5)
    got = hip.attention_residual_cl(qkv, C ** -0.5)
    if want is None:  # (unsupported by the shared score kernel: both entry points say so)
        assert C % 64 != 0 and got is None
        return
    out, made = got
    assert made == {} and hip.is_cl(out)
    assert torch.equal(out, want)


# ---- 2. the full epilogue ----------------------------------------------------------------------------------------------------
def _check_epilogue(hip, shape, n_twins):
    B, C, HW = shape
    qkv, bias, res, twins = _inputs(B, C, HW, n_twins, seed=1)
    base = hip.attention_cl(qkv, C ** -0.5)
    got = hip.attention_residual_cl(qkv, C ** -0.5, bias, residual=res, twins=twins)
    if base is None:
        assert C % 64 != 0 and got is None
        return
    out, made = got
    # the same three rounded fp32 ops, the library is built without contraction: a mismatch is an fma or a reordered add
    want = (base + bias.view(1, -1, 1, 1)) + res
    util.assert_finite(out, "out")
    assert torch.equal(out, want)
    assert list(made) == list(twins)
    for key, (sc, sh) in twins.items():
        util.assert_finite(made[key], "twin")
        t_want = torch.nn.functional.silu((sh.view(1, -1, 1, 1) + sc.view(1, -1, 1, 1) * out).double()).float()
        torch.testing.assert_close(made[key], t_want, rtol=util.SWISH_RTOL, atol=util.SWISH_ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n_twins", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_C%d_HW%d" % s)
def test_epilogue_bias_residual_twins(hip, shape, n_twins):
    _check_epilogue(hip, shape, n_twins)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_C%d_HW%d" % s)
def test_epilogue_under_poisoned_allocations(hip, shape):
    """Outputs, twins and the score workspace are NaN before the launch: a lane that stores nothing shows."""
    with util.poisoned() as p:
        _check_epilogue(hip, shape, 2)
    assert p.n > 0


@pytest.mark.gpu
def test_partial_epilogues_and_argument_checks(hip):
    """Each optional operand alone (a null one is neither read into the result nor added as a zero); a twin without its affine and
    a misaligned optional pointer are invalid arguments."""
    B, C, HW = 1, 64, 64
    qkv, bias, res, _ = _inputs(B, C, HW, 0, seed=2)
    base = hip.attention_cl(qkv, C ** -0.5)
    assert torch.equal(hip.attention_residual_cl(qkv, C ** -0.5, bias)[0], base + bias.view(1, -1, 1, 1))
    assert torch.equal(hip.attention_residual_cl(qkv, C ** -0.5, None, residual=res)[0], base + res)
    L, ws, out = hip.lib(), torch.empty(B * HW * HW, device=DEV), torch.empty_like(base)
    twin = torch.empty_like(base)
    args = lambda *e: (qkv.data_ptr(), B, C, HW, C ** -0.5, ws.data_ptr(), *e, out.data_ptr(), None)  # noqa: E731
    einval = -1
    assert L.sige_hip_error_string(einval)  # (SIGE_HIP_EINVAL)
    assert L.sige_hip_attention_residual_nhwc_f32(*args(None, None, twin.data_ptr(), bias.data_ptr(), None, None, None, None)) == einval
    assert L.sige_hip_attention_residual_nhwc_f32(*args(bias.data_ptr() + 4, None, None, None, None, None, None, None)) == einval
    assert L.sige_hip_attention_residual_nhwc_f32(*args(None, None, None, None, None, None, None, None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, base)


# ---- 3. the algebra (CPU) ------------------------------------------------------------------------------------------------------
def _block(ch=64, dtype=torch.float64):
    from sige_amd.workloads.ddpm_unet import AttnBlock, DDPMConfig

    torch.manual_seed(3)
    blk = AttnBlock(DDPMConfig(), ch, sparse=False).to(dtype)
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, dtype=dtype) * (0.5 if p.dim() == 1 else p[0].numel() ** -0.5))
    return blk


def _attn_fp64(w, b, x, ch):
    """proj-less attention of tokens x [HW, C] under a [3C, C] qkv matrix: P v."""
    q, k, v = (x @ w.reshape(3 * ch, ch).T + b).split(ch, dim=1)
    return torch.softmax(q @ k.T * ch ** -0.5, dim=1) @ v


def _fold_error(blk, x):
    ch = blk.ch
    want = _attn_fp64(blk.qkv.weight.detach(), blk.qkv.bias.detach(), x, ch) @ blk.proj_out.weight.detach().reshape(ch, ch).T \
        + blk.proj_out.bias.detach()
    conv, bp = blk.folded_proj()
    got = _attn_fp64(conv.weight.detach(), conv.bias.detach(), x, ch) + bp
    return ((got - want).abs().max() / want.abs().max()).item()


def test_fold_algebra_fp64_and_rebuild():
    """W_vp, b' reproduce proj(P v) + b_p in fp64 to 1e-12 relative on random weights, and are rebuilt when the parameters change:
    an in-place edit torch's version counter sees, load_state_dict, .to(); an edit through `.data` moves no version counter (the
    packed-weight caches of sige_amd/nn do not see it either): it is picked up with the caches, at clear_cache()."""
    blk = _block()
    x = torch.randn(48, blk.ch, dtype=torch.float64)
    assert _fold_error(blk, x) < 1e-12
    conv0 = blk.folded_proj()[0]
    assert blk.folded_proj()[0] is conv0  # (kept while nothing changes)
    assert set(blk.state_dict()) == {"norm.weight", "norm.bias", "qkv.weight", "qkv.bias", "proj_out.weight", "proj_out.bias"}
    assert [n for n, _ in blk.named_modules() if n] == ["norm", "qkv", "proj_out"]

    blk.proj_out.weight.data.mul_(2)
    blk.clear_cache()
    assert blk.folded_proj()[0] is not conv0 and _fold_error(blk, x) < 1e-12
    conv1 = blk.folded_proj()[0]
    with torch.no_grad():
        blk.proj_out.weight.mul_(2)
    assert blk.folded_proj()[0] is not conv1 and _fold_error(blk, x) < 1e-12
    conv2 = blk.folded_proj()[0]
    blk.load_state_dict(_block().state_dict())
    assert blk.folded_proj()[0] is not conv2 and _fold_error(blk, x) < 1e-12
    conv3 = blk.folded_proj()[0]
    blk.to(torch.float32)
    conv4, bp = blk.folded_proj()
    assert conv4 is not conv3 and conv4.weight.dtype == bp.dtype == torch.float32
    blk.to(torch.float64)
    assert _fold_error(blk, x) < 1e-12


def test_fold_rounds_fp64_products_once():
    """fp32 parameters: the folded value rows are the fp64 product rounded once (not an fp32 matmul)."""
    blk = _block(dtype=torch.float32)
    ch = blk.ch
    conv, bp = blk.folded_proj()
    wp, wv = blk.proj_out.weight.detach().reshape(ch, ch).double(), blk.qkv.weight.detach().reshape(3 * ch, ch)[2 * ch:].double()
    assert torch.equal(conv.weight.reshape(3 * ch, ch)[2 * ch:], (wp @ wv).float())
    assert torch.equal(conv.weight.reshape(3 * ch, ch)[:2 * ch], blk.qkv.weight.detach().reshape(3 * ch, ch)[:2 * ch])
    assert torch.equal(conv.bias[:2 * ch], blk.qkv.bias.detach()[:2 * ch]) and not conv.bias[2 * ch:].any()
    assert torch.equal(bp, (wp @ blk.qkv.bias.detach()[2 * ch:].double() + blk.proj_out.bias.detach().double()).float())


# ---- 4. block and model --------------------------------------------------------------------------------------------------------
def _small_cfg():
    from sige_amd.workloads.ddpm_unet import DDPMConfig

    # 64 -> 32 (tiled) -> 16 (dense, five attention blocks at C = 64) -> 8 (dense; the middle block's attention at C = 128)
    return DDPMConfig(ch=32, ch_mult=(1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16,), resolution=64, sparse_threshold=32)


def _small_mask():
    m = torch.zeros(64, 64, dtype=torch.bool)
    m[20:31, 12:29] = True
    return m


@pytest.fixture(scope="module")
def small():
    """The small network, its inputs and the CPU oracle's sparse forwards (computed once, shared, left unchanged): two originals
    under cache ids 0 / 1 and the same edit against each -- the recipe of tests/util.ddpm_cpu_oracle."""
    from oracle import oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    torch.manual_seed(0)
    cpu = DDPMSparseUNet(_small_cfg()).eval()
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(1, 3, 64, 64, generator=g)
    x0 = [x0, x0.flip(3) * 0.9]
    noise, mask, t = torch.randn(1, 3, 64, 64, generator=g), _small_mask(), torch.zeros(1)
    backend, _ = util.cpu_backend()
    oracle.set_num_threads(8)
    runtime.register_backend("cpu", backend)
    want = {}
    try:
        with torch.no_grad():
            for cid in (0, 1):
                cpu.set_cache_id(cid)
                cpu.set_mode("full")
                cpu(x0[cid], t)
            cpu.set_masks(downsample_mask(dilate_mask(mask, 5), 8))
            cpu.set_mode("sparse")
            for cid in (0, 1):
                cpu.set_cache_id(cid)
                want[cid] = cpu(x0[cid] + noise * mask, t).clone()
    finally:
        runtime.unregister_backend("cpu")
    return dict(state=cpu.state_dict(), x0=x0, noise=noise, mask=mask, want=want)


def _gpu_model(small):
    from sige_amd.utils import dilate_mask, downsample_mask
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    model = DDPMSparseUNet(_small_cfg()).eval()
    model.load_state_dict(small["state"])
    model = model.to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    td = torch.zeros(1, device=DEV)
    with torch.no_grad(), util.native_full_pass():
        for cid in (0, 1):
            model.set_cache_id(cid)
            model.set_mode("full")
            model(_cl(small["x0"][cid].to(DEV)), td)
    model.set_masks(downsample_mask(dilate_mask(small["mask"].to(DEV), 5), 8))
    model.set_mode("sparse")
    model.set_cache_id(0)
    return model, td


def _edited(small, cid):
    return _cl((small["x0"][cid] + small["noise"] * small["mask"]).to(DEV))


@pytest.mark.gpu
def test_small_ddpm_fold_on_and_off_vs_cpu_oracle(hip, small):
    from sige_amd.workloads import ddpm_unet
    from sige_amd.workloads.ddpm_unet import AttnBlock

    keep = ddpm_unet.FOLD_ATTN_PROJ
    outs, launches = {}, {}
    try:
        for fold in (True, False):
            ddpm_unet.FOLD_ATTN_PROJ = fold
            model, td = _gpu_model(small)
            blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
            assert len(blocks) == 6 and not any(b.sparse for b in blocks)
            x1 = _edited(small, 0)
            with torch.no_grad():
                model(x1, td)  # (consumers register their twins on the first forward)
                model(x1, td)
                n0 = hip.launch_count()
                outs[fold] = model(x1, td).clone()
                launches[fold] = hip.launch_count() - n0
                # (the twin epilogue is exercised: consumers registered with the attention blocks)
                assert sum(len(b._my_twins()) for b in blocks) > 0

                # replay of a captured graph equals the eager forward bit for bit
                g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    model(x1, td)
                    torch.cuda.synchronize()
                    with torch.cuda.graph(g, stream=s):
                        captured = model(x1, td)
                torch.cuda.current_stream().wait_stream(s)
                captured.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(captured, outs[fold]), fold
                del g

                # a second cache's twins carry that cache's affine
                for cid in (1, 0, 1):
                    model.set_cache_id(cid)
                    x1c = _edited(small, cid)
                    model(x1c, td)
                    got = model(x1c, td)
                    err = (got.cpu() - small["want"][cid]).abs().max().item()
                    print("fold=%s cache_id=%d max|gpu - cpu oracle| = %.3e" % (fold, cid, err))
                    util.record_margin("test_small_ddpm_fold_on_and_off_vs_cpu_oracle", "fold=%s cid=%d vs oracle" % (fold, cid), err,
                                       util.CONV_ATOL)
                    assert err <= util.CONV_ATOL, (fold, cid, err)
            err = (outs[fold].cpu() - small["want"][0]).abs().max().item()
            print("fold=%s max|gpu - cpu oracle| = %.3e, %d launches" % (fold, err, launches[fold]))
            assert err <= util.CONV_ATOL, (fold, err)
    finally:
        ddpm_unet.FOLD_ATTN_PROJ = keep
    diff = util.record_margin("test_small_ddpm_fold_on_and_off_vs_cpu_oracle", "fold on vs off", (outs[True] - outs[False]).abs().max().item(),
                              util.SELF_ATOL)
    print("max|fold on - fold off| = %.3e" % diff)
    assert diff <= util.SELF_ATOL
    assert launches[False] - launches[True] == 6, launches  # (one launch per attention block)
