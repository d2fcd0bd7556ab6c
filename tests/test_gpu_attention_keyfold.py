"""The key projection of the dense attention blocks folded into the query projection (sige_amd/workloads/ddpm_unet.py:
fold_keys_into_query, AttnBlock.folded_qv, FOLD_ATTN_QK): the block's conv is C -> 2C with outputs (q'' | v'), the keys are the block
input itself (include/sige_hip.h: sige_hip_attention_residual_qv_nhwc_f32).

Shapes as in tests/test_gpu_attention_fold.py: the channels-last attention takes C % 64 == 0 only, so (2, 48, 16) and (1, 32, 272) can
check one thing -- that all three entries answer "unsupported" alike; the kernel paths are reached at (2, 64, 16) one key step and the
batch stride, (1, 64, 272) the HW > 256 softmax and a second value block, (1, 128, 16) a second 64-channel workgroup column.

Bound of the block-level comparison: 2e-5 * (1 + max|ref|) against the fp64 chain qkv -> softmax -> proj_out -> + x, the project's
fp32-level criterion (an fp32 emulation of the fold sits 8x inside it at C = 512, HW = 256, weights x4)."""
import pytest
import torch

from tests import util
from tests.test_gpu_attention_fold import _edited, _gpu_model, _small_cfg, _small_mask, small  # noqa: F401  (`small`: the fixture)

DEV = "cuda"
SUPPORTED = [(2, 64, 16), (1, 64, 272), (1, 128, 16)]
REFUSED = [(2, 48, 16), (1, 32, 272)]
_HW = {16: (4, 4), 272: (16, 17)}
_ids = lambda s: "B%d_C%d_HW%d" % s  # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---- 1. the block against the fp64 chain -----------------------------------------------------------------------------------------
def _block(C, wmul, seed, dtype=torch.float32):
    """An AttnBlock at nn.Conv2d's default initialisation, qkv weights times `wmul` (x4: a sharp softmax)."""
    from sige_amd.workloads.ddpm_unet import AttnBlock, DDPMConfig

    torch.manual_seed(seed)
    blk = AttnBlock(DDPMConfig(), C, sparse=False).to(dtype).eval()
    with torch.no_grad():
        blk.qkv.weight.mul_(wmul)
        blk.norm.weight.copy_(1 + 0.2 * torch.randn(C, dtype=dtype))
        blk.norm.bias.copy_(0.2 * torch.randn(C, dtype=dtype))
    return blk


def _case(B, C, HW, means, wmul, quirk=False, per_sample=False):
    """Block, input (per-channel means of `means` standard deviations), its GroupNorm affine (fp64 statistics of image 0; `per_sample`:
    image b's affine is (1 + b/4) times that, as a cache made from a batch holds one per image) and the fp64 chain's output.
    `quirk`: the block applies channel 0's scale and shift to every channel (reference_attn_quirk), and so does the chain."""
    H, W = _HW[HW]
    blk = _block(C, wmul, seed=C + HW + means)
    blk.quirk = quirk
    g = torch.Generator().manual_seed(17 * C + HW + means + int(wmul))
    x = torch.randn(B, C, H, W, generator=g) + means * torch.randn(1, C, 1, 1, generator=g)
    xd = x.double()
    G = blk.norm.num_groups
    grp = xd[:1].reshape(G, -1)
    mu, var = grp.mean(1), grp.var(1, unbiased=False)
    inv = torch.rsqrt(var + blk.norm.eps).repeat_interleave(C // G)
    s = inv * blk.norm.weight.detach().double()
    t = blk.norm.bias.detach().double() - mu.repeat_interleave(C // G) * s
    s32, t32 = s.float().reshape(1, C, 1, 1), t.float().reshape(1, C, 1, 1)
    if per_sample:
        f = 1 + torch.arange(B, dtype=torch.float32).reshape(B, 1, 1, 1) / 4
        s32, t32 = (s32 * f).contiguous(), (t32 * f).contiguous()
    # the reference chain in fp64, from the fp32 values every form starts from
    sa, ta = (s32[:, :1], t32[:, :1]) if quirk else (s32, t32)
    xn = xd * sa.double() + ta.double()
    tok = xn.reshape(B, C, HW).transpose(1, 2)  # [B, HW, C]
    wq, bq = blk.qkv.weight.detach().double().reshape(3 * C, C), blk.qkv.bias.detach().double()
    q, k, v = (tok @ wq.T + bq).split(C, dim=2)
    att = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=2) @ v
    out = att @ blk.proj_out.weight.detach().double().reshape(C, C).T + blk.proj_out.bias.detach().double()
    want = out.transpose(1, 2).reshape(B, C, H, W) + xd
    return blk, x, s32, t32, want


def _run_block(blk, x, s, t):
    blk = blk.to(DEV)
    blk.set_mode("sparse")
    blk.affine[blk.cache_id] = (s.to(DEV).contiguous(), t.to(DEV).contiguous())
    with torch.no_grad():
        return blk(_cl(x.to(DEV)))


class _Calls:
    """Counts the calls of one sige_amd.hip function while active."""

    def __init__(self, hip, name):
        self.hip, self.name, self.n = hip, name, 0

    def __enter__(self):
        self.keep = getattr(self.hip, self.name)

        def counted(*a, **k):
            self.n += 1
            return self.keep(*a, **k)

        setattr(self.hip, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.hip, self.name, self.keep)
        return False


@pytest.mark.gpu
@pytest.mark.parametrize("wmul", [1.0, 4.0], ids=["w1", "w4"])
@pytest.mark.parametrize("means", [0, 4], ids=["mean0", "mean4"])
@pytest.mark.parametrize("shape", SUPPORTED, ids=_ids)
def test_key_folded_block_vs_fp64_chain(hip, shape, means, wmul):
    from sige_amd.workloads import ddpm_unet

    assert ddpm_unet.FOLD_ATTN_QK and ddpm_unet.FOLD_ATTN_PROJ
    B, C, HW = shape
    blk, x, s, t, want = _case(B, C, HW, means, wmul)
    with _Calls(hip, "attention_residual_qv_cl") as calls:
        got = _run_block(blk, x, s, t)
    assert calls.n == 1  # (the new entry ran: not the C -> 3C chain)
    util.assert_finite(got, "out")
    err = (got.double().cpu() - want).abs().max().item()
    tol = 2e-5 * (1 + want.abs().max().item())
    print("B%d C%d HW%d means=%d w x%g: max|key fold - fp64 chain| = %.3e (bound %.3e)" % (B, C, HW, means, wmul, err, tol))
    util.record_margin("test_key_folded_block_vs_fp64_chain", "B%d C%d HW%d means=%d wx%g" % (B, C, HW, means, wmul), err, tol)
    assert err <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["quirk", "per_sample_affine"])
def test_key_folded_block_quirk_and_per_sample_affine(hip, variant):
    """reference_attn_quirk: the s of q'' is the quirk's s (channel 0's, for every channel).  A cache made from a batch holds one
    affine per image: the score kernel reads image b's row of it."""
    B, C, HW = 2, 64, 16
    blk, x, s, t, want = _case(B, C, HW, 4, 4.0, quirk=variant == "quirk", per_sample=variant == "per_sample_affine")
    with _Calls(hip, "attention_residual_qv_cl") as calls:
        got = _run_block(blk, x, s, t)
    assert calls.n == 1
    util.assert_finite(got, "out")
    err = (got.double().cpu() - want).abs().max().item()
    tol = 2e-5 * (1 + want.abs().max().item())
    print("%s: max|key fold - fp64 chain| = %.3e (bound %.3e)" % (variant, err, tol))
    util.record_margin("test_key_folded_block_quirk_and_per_sample_affine", variant, err, tol)
    assert err <= tol


# ---- 2. the entry points ---------------------------------------------------------------------------------------------------------
def _entry_inputs(B, C, HW, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + C + HW)
    H, W = (HW // 4, 4) if HW not in _HW else _HW[HW]
    r = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    qkv, res, bias = r(B, 3 * C, H, W), r(B, C, H, W), r(C)
    twins = {("t", k): (r(C), r(C)) for k in range(2)}
    return qkv, res, bias, twins


@pytest.mark.gpu
@pytest.mark.parametrize("shape", REFUSED, ids=_ids)
def test_refused_shapes_get_the_same_answer_from_all_entries(hip, shape):
    B, C, HW = shape
    qkv, res, bias, _ = _entry_inputs(B, C, HW)
    qkv, res = _cl(qkv.to(DEV)), _cl(res.to(DEV))
    q, k, v = qkv.split(C, dim=1)
    qv = _cl(torch.cat([q, v], 1))
    assert hip.attention_cl(qkv, C ** -0.5) is None
    assert hip.attention_residual_cl(qkv, C ** -0.5, bias.to(DEV), residual=res) is None
    assert hip.attention_residual_qv_cl(qv, _cl(k), C ** -0.5, bias.to(DEV), residual=res) is None
    # ... as a status: the library's "unsupported", not an invalid argument
    L = hip.lib()
    ws, out = torch.empty(B * HW * HW, device=DEV), torch.empty_like(res)
    tail = (B, C, HW, C ** -0.5, ws.data_ptr()) + (None,) * 8 + (out.data_ptr(), None)
    assert L.sige_hip_attention_residual_qv_nhwc_f32(qv.data_ptr(), _cl(k).data_ptr(), None, 0, *tail) == hip.UNSUPPORTED
    assert L.sige_hip_attention_residual_nhwc_f32(qkv.data_ptr(), *tail) == hip.UNSUPPORTED
    assert L.sige_hip_attention_nhwc_f32(qkv.data_ptr(), B, C, HW, C ** -0.5, ws.data_ptr(), out.data_ptr(), None) == hip.UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SUPPORTED, ids=_ids)
def test_old_entries_keep_their_bits_and_strides_do_not_matter(hip, shape):
    """The kernels now take query, key and value rows by pointer and stride.  (a) The two qkv entries give the bits they gave before
    that change: their outputs recorded from the library of the commit before it, on an MI355X, for inputs drawn on the CPU
    (tests/golden/attention_qkv_entries_parent.npz; a mismatch says by how much).  (b) The qv entry, given the same q, k and v as separate tensors -- the
    unfolded values, other strides -- runs the same arithmetic: bit-identical to the qkv entry, twins included."""
    B, C, HW = shape
    qkv, res, bias, twins = _entry_inputs(B, C, HW, seed=3)
    qkv, res, bias = _cl(qkv.to(DEV)), _cl(res.to(DEV)), bias.to(DEV)
    twins = {k: (a.to(DEV), b.to(DEV)) for k, (a, b) in twins.items()}
    plain = hip.attention_cl(qkv, C ** -0.5)
    old, old_tw = hip.attention_residual_cl(qkv, C ** -0.5, bias, residual=res, twins=twins)
    q, k, v = qkv.split(C, dim=1)
    with util.poisoned() as p:
        new, new_tw = hip.attention_residual_qv_cl(_cl(torch.cat([q, v], 1)), _cl(k), C ** -0.5, bias, residual=res, twins=twins)
    assert p.n > 0
    util.assert_finite(new, "out")
    assert torch.equal(new, old)
    for key in twins:
        assert torch.equal(new_tw[key], old_tw[key]), key
    bare, made = hip.attention_residual_qv_cl(_cl(torch.cat([q, v], 1)), _cl(k), C ** -0.5)
    assert made == {} and torch.equal(bare, plain)
    rec = util.golden("attention_qkv_entries_parent")
    for name, t in (("attention_cl", plain), ("attention_residual_cl", old), ("twin0", old_tw[("t", 0)]), ("twin1", old_tw[("t", 1)])):
        want = torch.from_numpy(rec["%s/%s" % (_ids(shape), name)])
        diff = (t.cpu() - want).abs().max().item()
        assert torch.equal(t.cpu(), want), (name, "max |now - recorded| = %.3e" % diff)


@pytest.mark.gpu
def test_qv_entry_argument_checks(hip):
    B, C, HW = 1, 64, 16
    qkv, res, bias, _ = _entry_inputs(B, C, HW, seed=4)
    qkv, bias = _cl(qkv.to(DEV)), bias.to(DEV)
    q, k, v = qkv.split(C, dim=1)
    qv, k = _cl(torch.cat([q, v], 1)), _cl(k)
    L, ws, out = hip.lib(), torch.empty(B * HW * HW, device=DEV), torch.empty(B, C, 4, 4, device=DEV)
    args = lambda qp, kp, *e, qs=(None, 0): (qp, kp, *qs, B, C, HW, C ** -0.5, ws.data_ptr(), *e, out.data_ptr(), None)  # noqa: E731
    one = torch.ones(1, C, device=DEV)
    none8 = (None,) * 8
    einval = -1
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), None, *none8)) == einval
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(None, k.data_ptr(), *none8)) == einval
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), k.data_ptr(), bias.data_ptr() + 4, *(None,) * 7)) == einval
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), k.data_ptr() + 4, *none8)) == hip.UNSUPPORTED
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), k.data_ptr(), *none8, qs=(one.data_ptr(), 3))) == einval
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), k.data_ptr(), *none8, qs=(one.data_ptr() + 4, 1))) == einval
    assert L.sige_hip_attention_residual_qv_nhwc_f32(*args(qv.data_ptr(), k.data_ptr(), *none8)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, 4, 4, C).permute(0, 3, 1, 2), hip.attention_cl(qkv, C ** -0.5))


# ---- 3. the algebra (CPU) --------------------------------------------------------------------------------------------------------
def _probs_fp64(blk, x, s, t):
    """softmax rows of the block's own chain and of the key-folded form, tokens x [HW, C], affine s / t [C], in fp64."""
    C = blk.ch
    w, b = blk.qkv.weight.detach().double().reshape(3 * C, C), blk.qkv.bias.detach().double()
    xn = x * s + t
    q, k = xn @ w[:C].T + b[:C], xn @ w[C:2 * C].T + b[C:2 * C]
    want = torch.softmax(q @ k.T * C ** -0.5, dim=1)
    conv, _ = blk.folded_qv()
    M, m = conv.weight.detach().double().reshape(2 * C, C)[:C], conv.bias.detach().double()[:C]
    q2 = s * (xn @ M.T + m)
    return want, torch.softmax(q2 @ x.T * C ** -0.5, dim=1), conv


def test_key_fold_algebra_fp64_and_rebuild():
    """softmax_j(q_i . k_j) == softmax_j(q''_i . x_j) in fp64 to 1e-12 with channel means that t would have removed; the value rows
    and b' are folded_proj()'s; neither conv is a parameter; an edit of qkv.weight through `.data` is picked up at clear_cache()."""
    blk = _block(64, 1.0, seed=5, dtype=torch.float64)
    C = blk.ch
    g = torch.Generator().manual_seed(9)
    x = torch.randn(48, C, generator=g, dtype=torch.float64) + 4 * torch.randn(C, generator=g, dtype=torch.float64)
    s, t = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    want, got, conv0 = _probs_fp64(blk, x, s, t)
    assert (got - want).abs().max().item() < 1e-12
    conv3, bp3 = blk.folded_proj()
    conv, bp = blk.folded_qv()
    assert conv is conv0 and bp is bp3  # (kept while nothing changes)
    assert torch.equal(conv.weight[C:], conv3.weight[2 * C:]) and not conv.bias[C:].any()
    assert set(blk.state_dict()) == {"norm.weight", "norm.bias", "qkv.weight", "qkv.bias", "proj_out.weight", "proj_out.bias"}
    assert [n for n, _ in blk.named_modules() if n] == ["norm", "qkv", "proj_out"]

    blk.qkv.weight.data[:2 * C].mul_(1.5)
    blk.clear_cache()
    want, got, conv1 = _probs_fp64(blk, x, s, t)
    assert conv1 is not conv0 and (got - want).abs().max().item() < 1e-12
    assert not torch.equal(conv1.weight[:C], conv0.weight[:C])  # (M was rebuilt)
    with torch.no_grad():
        blk.qkv.bias.mul_(2)  # (an edit the version counter sees: no clear_cache needed)
    want, got, conv2 = _probs_fp64(blk, x, s, t)
    assert conv2 is not conv1 and (got - want).abs().max().item() < 1e-12


def test_key_fold_rounds_fp64_products_once():
    from sige_amd.workloads.ddpm_unet import fold_keys_into_query

    blk = _block(64, 1.0, seed=6)
    C = blk.ch
    w, b = blk.qkv.weight.detach().reshape(3 * C, C), blk.qkv.bias.detach()
    M, m = fold_keys_into_query(blk.qkv.weight, blk.qkv.bias)
    assert M.dtype == m.dtype == torch.float32
    assert torch.equal(M, (w[C:2 * C].double().T @ w[:C].double()).float())
    assert torch.equal(m, (w[C:2 * C].double().T @ b[:C].double()).float())
    M0, m0 = fold_keys_into_query(blk.qkv.weight, None)
    assert torch.equal(M0, M) and not m0.any()
    conv, _ = blk.folded_qv()
    assert torch.equal(conv.weight.reshape(2 * C, C)[:C], M) and torch.equal(conv.bias[:C], m)


# ---- 4. the small network --------------------------------------------------------------------------------------------------------
def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


@pytest.mark.gpu
def test_small_ddpm_key_fold_on_and_off_vs_cpu_oracle(hip, small):  # noqa: F811
    """Key-folded and not: each within 1e-3 of the CPU oracle, mutually within SELF_ATOL, three launches per attention block either
    way; under NaN-poisoned allocations the key-folded forward keeps its bits."""
    from sige_amd.workloads import ddpm_unet
    from sige_amd.workloads.ddpm_unet import AttnBlock

    keep = ddpm_unet.FOLD_ATTN_QK
    outs, launches, qv_calls = {}, {}, {}
    try:
        for fold in (True, False):
            ddpm_unet.FOLD_ATTN_QK = fold
            model, td = _gpu_model(small)
            blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
            assert len(blocks) == 6
            x1 = _edited(small, 0)
            with torch.no_grad():
                model(x1, td)  # (consumers register their twins on the first forward)
                model(x1, td)
                n0 = hip.launch_count()
                with _Calls(hip, "attention_residual_qv_cl") as calls:
                    outs[fold] = model(x1, td).clone()
                launches[fold], qv_calls[fold] = hip.launch_count() - n0, calls.n
                assert sum(len(b._my_twins()) for b in blocks) > 0  # (the twin epilogue is exercised)
                for cid in (1, 0):  # (a second cache: its own s in q'', its own twins)
                    model.set_cache_id(cid)
                    x1c = _edited(small, cid)
                    model(x1c, td)
                    got = model(x1c, td)
                    err = (got.cpu() - small["want"][cid]).abs().max().item()
                    print("key fold=%s cache_id=%d max|gpu - cpu oracle| = %.3e" % (fold, cid, err))
                    util.record_margin("test_small_ddpm_key_fold_on_and_off_vs_cpu_oracle", "key fold=%s cid=%d vs oracle" % (fold, cid),
                                       err, util.CONV_ATOL)
                    assert err <= util.CONV_ATOL, (fold, cid, err)
                assert torch.equal(got, outs[fold])  # (back on cache 0: the first result again)
                if fold:
                    with util.poisoned() as p:
                        again = model(x1, td).clone()
                    assert p.n > 0
                    util.assert_finite(again, "out under poison")
                    assert torch.equal(again, outs[fold])
    finally:
        ddpm_unet.FOLD_ATTN_QK = keep
    assert qv_calls == {True: 6, False: 0}
    diff = util.record_margin("test_small_ddpm_key_fold_on_and_off_vs_cpu_oracle", "key fold on vs off",
                              (outs[True] - outs[False]).abs().max().item(), util.SELF_ATOL)
    print("max|key fold on - off| = %.3e, launches %s" % (diff, launches))
    assert diff <= util.SELF_ATOL
    assert launches[True] == launches[False], launches  # (the same three launches per block; the conv is a third smaller)


@pytest.mark.gpu
def test_small_ddpm_key_fold_stacked_edits(hip, small):  # noqa: F811
    """E = 2 edits of one original stacked along H: queries, values and KEYS are taken per image.  Edit 0 is the oracle's edit; each
    edit's slice against its own single-edit forward of the same model, and edit 0 against the CPU oracle."""
    from sige_amd import stacked
    from sige_amd.workloads import ddpm_unet

    assert ddpm_unet.FOLD_ATTN_QK
    model, td = _gpu_model(small)
    m2 = torch.zeros(64, 64, dtype=torch.bool)
    m2[40:52, 30:50] = True
    masks = [small["mask"].to(DEV), m2.to(DEV)]
    x0, noise = small["x0"][0].to(DEV), small["noise"].to(DEV)
    edits = [_cl(x0 + noise * m) for m in masks]
    E = len(masks)
    with torch.no_grad():
        singles = []
        for m, xe in zip(masks, edits):
            model.set_masks(_build_masks(m))
            model.set_mode("sparse")
            model(xe, td)
            singles.append(model(xe, td).clone())
        stacked.stack_caches(model, E)
        try:
            stacked.set_masks(model, [_build_masks(m) for m in masks])
            model.set_mode("sparse")
            xs = _cl(torch.cat(edits, 0))
            with stacked.edit_batch(model, E), _Calls(hip, "attention_residual_qv_cl") as calls:
                model(xs, td)
                out = model(xs, td).clone()
        finally:
            stacked.unstack_caches(model)
    assert calls.n == 12
    assert tuple(out.shape) == (E, 3, 64, 64)
    for e in range(E):
        err = util.record_margin("test_small_ddpm_key_fold_stacked_edits", "edit %d stacked vs single" % e,
                                 (out[e] - singles[e][0]).abs().max().item(), util.SELF_ATOL)
        assert err <= util.SELF_ATOL, (e, err)
    err = util.record_margin("test_small_ddpm_key_fold_stacked_edits", "edit 0 vs oracle",
                             (out[0].cpu() - small["want"][0][0]).abs().max().item(), util.CONV_ATOL)
    print("stacked key fold: edit 0 max|gpu - cpu oracle| = %.3e" % err)
    assert err <= util.CONV_ATOL
    assert (singles[1] - singles[0]).abs().max().item() > 1e-2  # (two different edits)


@pytest.mark.gpu
def test_launch_plan_replays_the_key_folded_forward_bit_for_bit(hip):
    """A launch plan (sige_amd/plan.py) recorded on the key-folded forward issues it from C bit-identical to the module forward, also
    under another mask: the new entry point is recorded (SIGE_PLAN_HOOK) and nothing of the fold runs outside the library.  On the
    DDPM-256 network (about a second): the small network cannot be planned with or without the fold, at 32 or at 64 base channels --
    one of its concatenations goes through torch, which no plan replays (LaunchPlan.record says so)."""
    import bench
    from sige_amd.plan import LaunchPlan
    from sige_amd.workloads import ddpm_unet
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    assert ddpm_unet.FOLD_ATTN_QK
    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    x0, noise = bench.make_inputs()
    x0, noise, td = _cl(x0.to(DEV)), _cl(noise.to(DEV)), torch.zeros(1, device=DEV)
    masks = [bench.square_mask(0.012, top=100, left=90).to(DEV), bench.square_mask(0.03, top=20, left=150).to(DEV)]
    with torch.no_grad(), util.native_full_pass():
        model.set_mode("full")
        model(x0, td)
    with torch.no_grad():
        xs = (x0 + noise * masks[0]).clone()
        plan = LaunchPlan(model)
        with _Calls(hip, "attention_residual_qv_cl") as calls:
            plan.record(masks[0], _build_masks, lambda: model(xs, td))
        assert calls.n >= 6 and not plan.shape_bound
        for m in (masks[1], masks[0]):
            xs.copy_(x0 + noise * m)
            plan.bind_mask(m)
            ran = plan.run().clone()
            rep = plan.replay().clone()
            want = model(xs, td)  # (the module-level forward under the index lists the plan bound)
            assert torch.equal(ran, want) and torch.equal(rep, want)
        del plan


@pytest.mark.gpu
def test_key_fold_follows_a_cache_rewritten_in_place(hip, small):  # noqa: F811
    """The multi-GPU path rewrites the cached affines in place: parallel.pack_caches re-points them at views of one flat buffer,
    another original's cache is copied into that buffer, parallel.refresh_derived refreshes what is derived from it -- addresses
    stay, so captured graphs go on replaying.  q'' carries the cached scale s: the kept out-affine vector (s | 1) must follow the
    cache (AttnBlock.rebuild_derived_caches), at its address.  Order: full(A) -> sparse -> pack -> sparse, graph captured -> flat <- cache of B -> refresh_derived -> sparse, eagerly
    and by replaying the graph captured under A: both against the CPU oracle's sparse forward on B."""
    from sige_amd import parallel
    from sige_amd.workloads import ddpm_unet
    from sige_amd.workloads.ddpm_unet import DDPMSparseUNet

    assert ddpm_unet.FOLD_ATTN_QK

    def net_on(x0):
        net = DDPMSparseUNet(_small_cfg()).eval()
        net.load_state_dict(small["state"])
        net = net.to(DEV).to(memory_format=torch.channels_last)
        net.set_scatter_inplace(True)
        with torch.no_grad(), util.native_full_pass():
            net.set_mode("full")
            net(_cl(x0.to(DEV)), td)
        return net

    td = torch.zeros(1, device=DEV)
    with torch.no_grad():
        flat_b = parallel.pack_caches(net_on(small["x0"][1])).clone()  # (what another rank would send: the cache of image B)
        net = net_on(small["x0"][0])
        net.set_masks(_build_masks(small["mask"].to(DEV)))
        net.set_mode("sparse")
        xs = _edited(small, 0).clone()
        net(xs, td)
        flat = parallel.pack_caches(net)
        with _Calls(hip, "attention_residual_qv_cl") as calls:
            net(xs, td)
            got_a = net(xs, td).clone()
        assert calls.n == 12
        err = util.record_margin("test_key_fold_follows_a_cache_rewritten_in_place", "A after pack vs oracle",
                                 (got_a.cpu() - small["want"][0]).abs().max().item(), util.CONV_ATOL)
        assert err <= util.CONV_ATOL, err
        g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            net(xs, td)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                captured = net(xs, td)
        torch.cuda.current_stream().wait_stream(st)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, got_a)

        flat.copy_(flat_b)  # (the broadcast)
        parallel.refresh_derived(net)
        xs.copy_(_edited(small, 1))
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        err_g = util.record_margin("test_key_fold_follows_a_cache_rewritten_in_place", "B by the graph captured under A vs oracle",
                                   (captured.cpu() - small["want"][1]).abs().max().item(), util.CONV_ATOL)
        net(xs, td)
        got_b = net(xs, td)
        err_e = util.record_margin("test_key_fold_follows_a_cache_rewritten_in_place", "B eager vs oracle",
                                   (got_b.cpu() - small["want"][1]).abs().max().item(), util.CONV_ATOL)
        print("cache of B in place: max|gpu - cpu oracle| graph %.3e, eager %.3e; |A - B| %.3e"
              % (err_g, err_e, (small["want"][0] - small["want"][1]).abs().max().item()))
        assert err_g <= util.CONV_ATOL and err_e <= util.CONV_ATOL, (err_g, err_e)
        assert (small["want"][0] - small["want"][1]).abs().max().item() > 1e-2  # (two different originals)
        del g
