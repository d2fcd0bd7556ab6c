"""Kernels under poisoned allocations (tests/util.poisoned): every floating-point tensor torch.empty & co. hand out is filled with
NaN (or 1e30) first, so an output element a kernel never stores, a workspace it reads before writing, a capacity row past the
count or a padding lane multiplied by zero instead of selected away shows up as a non-finite or wildly wrong value.  Without it
the caching allocator hands back the freed block of the previous launch of the same size -- which in a parity test often already
holds the expected answer.

Two parts:
* poisoned twins of the existing single-launch and model-level GPU tests: the same body, the same references and tolerances
  (fp64 / torch / the CPU oracle / the golden vectors), run inside `util.poisoned(v)`; weights, packed weights, workspaces and
  outputs are all allocated inside, so padding in the packed layouts is poisoned too.  Single launches run under NaN and under
  1e30 (a large finite value catches what NaN slips through: row maxima, ReLU, `x > tol` masks); whole forwards under NaN.
* whole forwards written for poison: the benchmarked DDPM-256 configuration from a poisoned full pass with no warm-up forward,
  the conv_in window buffer filled with NaN, graph capture, a launch plan over growing and shrinking masks, fp16 forms."""
import functools

import pytest
import torch

from tests import test_gpu_channels_last as t_cl
from tests import test_gpu_group_norm_offsets as t_gno
from tests import test_gpu_parity as t_par
from tests import test_gpu_round2 as t_r2
from tests import test_gpu_round3 as t_r3
from tests import test_gpu_round4 as t_r4
from tests import test_gpu_round5 as t_r5
from tests import test_gpu_round6 as t_r6
from tests import test_models_golden as t_gold
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
POISON = {"nan": NAN, "big": 1e30}


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


# ---- the poison reaches the device ------------------------------------------------------------------------------------------
def test_poison_reaches_the_device():
    """fp32, fp16, bf16 and channels-last device allocations come out all-NaN; so does one allocated inside a CUDA graph capture,
    read after replay (the fill is captured with it), and integers stay unpoisoned."""
    with util.poisoned() as p:
        a = torch.empty(1000, 37, device=DEV)
        h = torch.empty(4097, device=DEV, dtype=torch.float16)
        b = torch.empty(333, device=DEV, dtype=torch.bfloat16)
        c = torch.empty(2, 40, 17, 23, device=DEV, memory_format=torch.channels_last)
        like = torch.empty_like(c)
        i = torch.empty(64, device=DEV, dtype=torch.int32)
        x = torch.ones(8, device=DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            x + 1  # (warm-up outside the capture)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                inside = torch.empty(3, 64, 5, 7, device=DEV, memory_format=torch.channels_last)
                kept = x * 2
        torch.cuda.current_stream().wait_stream(s)
        inside.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert c.is_contiguous(memory_format=torch.channels_last) and like.is_contiguous(memory_format=torch.channels_last)
    for name, t in (("fp32", a), ("fp16", h), ("bf16", b), ("channels_last", c), ("empty_like", like), ("captured", inside)):
        assert bool(torch.isnan(t.float()).all()), name
    assert torch.equal(kept, torch.full((8,), 2.0, device=DEV))
    assert not bool(torch.isnan(i.float()).any())
    assert p.n == 6
    with util.poisoned(1e30):
        big, big_h = torch.empty(100, device=DEV), torch.empty(100, device=DEV, dtype=torch.float16)
    assert bool((big == 1e30).all()) and bool((big_h == torch.finfo(torch.float16).max).all())


# ---- poisoned twins of the existing tests ------------------------------------------------------------------------------------
def _twin(fn, value, expect_poison=True):
    """`fn` (a test function, its parametrize marks and fixtures) run inside util.poisoned(value).  The twin's source, for
    conftest.tier's scan, is fn's own (inspect follows __wrapped__): a twin of an oracle-parity test is one too."""

    @functools.wraps(fn)
    def twin(*args, **kwargs):
        with util.poisoned(value) as p:
            fn(*args, **kwargs)
        if expect_poison:
            assert p.n > 0, "nothing was allocated under poison"

    twin.pytestmark = list(getattr(fn, "pytestmark", []))
    return twin


# single launches (and short chains of them): NaN and 1e30
SINGLE = [
    # tile conv (conv_mfma.hpp): every output block, NCHW / channels-last, gather / scatter_gather forms, pairs, K split, f16 / f16x3
    (t_par, "test_golden_cases"), (t_par, "test_against_oracle_mid_size"), (t_par, "test_block_conv_vs_torch_and_oracle"),
    (t_par, "test_fused_gather_conv_equals_two_kernels"), (t_par, "test_conv_every_output_block_shape"),
    (t_par, "test_block_conv_direct_groups"), (t_par, "test_full_size_properties"), (t_par, "test_hipgraph_capture_replay"),
    (t_cl, "test_conv_cl_vs_nchw"), (t_cl, "test_lazy_cat_feeds_fused_gather"), (t_cl, "test_epilogue_affine_activation"),
    (t_cl, "test_gather_conv_cl_fused_upsample"),
    (t_r2, "test_dilated_tile_conv"), (t_r2, "test_f16_compute_block_conv_exact_products"),
    (t_r2, "test_f16_compute_fused_gather_and_scatter_gather"), (t_r2, "test_conv_pair_equals_separate_launches"),
    (t_r2, "test_conv_pair_f16_compute"), (t_r2, "test_conv_pair_leftovers_are_launched"),
    (t_r2, "test_ksplit_finished_inside_the_launch"),
    (t_r3, "test_f16x3_tile_conv_is_fp32_level"), (t_r3, "test_f16x3_fused_gather_scatter_gather_and_pair"),
    (t_r4, "test_f16_cache_fused_conv_bit_exact"),
    # tile conv v3 (conv_tile3.hpp)
    (t_r5, "test_tile_conv3_gather_forms_vs_fp64"), (t_r5, "test_tile_conv3_scatter_gather_to_full_vs_old_kernel_and_fp64"),
    (t_r6, "test_tile_conv3_f16_gather_forms"), (t_r6, "test_tile_conv3_f16_scatter_gather_to_full"),
    (t_r6, "test_tile_conv3_f16_router_decides_from_the_tile_count"), (t_r6, "test_tile_conv3_scatter_gather_with_cached_affine"),
    # dense-layer conv (conv_wide.hpp): WIDE_CASES x precisions, forced K splits, stats, the GroupNorm affine from them, pairs
    (t_par, "test_dense_fused_conv_vs_torch"), (t_cl, "test_dense_fused_conv_cl"),
    (t_r2, "test_twin_epilogue_of_a_dense_conv"), (t_r3, "test_wide_conv_vs_fp64"),
    (t_r3, "test_wide_conv_split_k_is_deterministic_and_equals_unsplit"), (t_r3, "test_wide_conv_small_operands_keep_their_precision"),
    (t_r3, "test_wide_conv_twins_and_dense_module_routing"), (t_r3, "test_wide_conv_stats_give_the_group_norm_affine"),
    (t_r3, "test_channel_stats_of_a_tensor_and_the_norm_of_a_cat"), (t_r4, "test_wide_conv_pairs_with_the_shortcut"),
    # (both planes of the statistics: a part that a ragged or partly empty pixel block leaves unwritten shows as NaN)
    (t_gno, "test_channel_stats_route_on_offset_inputs"), (t_gno, "test_wide_conv_stats_route_on_offset_inputs"),
    # data movement: gather / scatter / scatter_gather / block-residual scatter, NCHW and channels-last, in place, fp16 caches
    (t_cl, "test_gather_and_scatter_gather_cl"), (t_cl, "test_scatter_cl_full_and_in_place"),
    (t_r2, "test_grouped_nchw_gather_bit_exact"), (t_r3, "test_scatter_gather_row_form_bit_exact"),
    (t_r4, "test_f16_cache_data_movement_bit_exact"), (t_r5, "test_act_split_and_scatter_gather_split"),
    (t_r5, "test_resize_nearest_is_torch_nearest"),
    # the rest: GroupNorm affine, attention, tokens, SPADE, the small-channel convs, conv_in on the active windows
    (t_par, "test_group_norm_affine_vs_torch"), (t_cl, "test_group_norm_affine_cl"), (t_r3, "test_group_norm_affine_with_channel_bias"),
    (t_r3, "test_affine_act_cl_equals_torch"),
    (t_par, "test_attention_vs_torch"), (t_cl, "test_attention_cl"), (t_r4, "test_attention_one_launch"),
    (t_r4, "test_attention_one_launch_under_a_graph"), (t_r4, "test_attention_tokens_vs_fp64"), (t_r5, "test_token_helpers_vs_torch"),
    (t_r5, "test_spade_modulate_dense_and_conv_img_tail"), (t_gold, "test_spade_modulate_kernel_equals_the_module_chain"),
    (t_cl, "test_conv3x3_small_cout_cl"), (t_cl, "test_conv3x3_small_cin_cl"), (t_cl, "test_input_conv2d_matches_the_plain_conv"),
    (t_r6, "test_conv_in_on_the_active_windows_only"),
]
# the mask pipeline: its outputs are integer / bool (compared bit-exactly, never poisoned); what is poisoned is float scratch
MASKS = [(t_r2, "test_device_mask_helpers_bit_exact"), (t_r2, "test_device_difference_mask")]
# whole forwards and module chains: NaN
MODELS = [
    (t_par, "test_deferred_fusion_in_modules"), (t_par, "test_ddpm_unet_gpu_vs_oracle_backend"),
    (t_par, "test_example_golden_output_on_gpu"), (t_par, "test_resblock_gpu_vs_oracle_backend"),
    (t_cl, "test_ddpm_unet_channels_last_equals_nchw"), (t_cl, "test_conv_scatter_fusion_in_modules"),
    (t_cl, "test_empty_mask_sparse_forward_is_the_cached_result"),
    (t_r2, "test_benchmarked_forward_vs_oracle_at_full_size"), (t_r2, "test_inplace_scatter_buffer_follows_the_cache"),
    (t_r2, "test_sparse_update_with_inplace_buffers"), (t_r2, "test_f16_compute_ddpm_forward_vs_fp32_oracle"),
    (t_r3, "test_sd_unet_at_its_own_size_vs_cpu_oracle"), (t_r4, "test_sd_transformer_native_attention_and_linears"),
    (t_r5, "test_stacked_edits_vs_cpu_oracle"), (t_r5, "test_gaugan_sparse_forward_on_the_library_follows_a_launch_plan"),
    (t_r5, "test_standalone_gathers_and_spade_in_stacked_mode"), (t_r5, "test_sd_transformer_fused_tokens_equal_the_module_chain"),
    (t_gold, "test_gaugan_generator_on_the_gpu_matches_the_reference_fixture"),
    (t_gold, "test_sd_spatial_transformer_on_the_gpu_matches_the_reference_fixture"),
    (t_gold, "test_sd_unet_on_the_gpu_matches_the_reference_fixture"),
]


def _short(mod):
    return mod.__name__.rsplit(".", 1)[-1].replace("test_gpu_", "").replace("test_", "")


for _mod, _name in SINGLE:
    for _tag, _v in POISON.items():
        globals()["test_poison_%s__%s__%s" % (_tag, _short(_mod), _name[5:])] = _twin(getattr(_mod, _name), _v)
for _mod, _name in MASKS:
    globals()["test_poison_nan__%s__%s" % (_short(_mod), _name[5:])] = _twin(getattr(_mod, _name), NAN, expect_poison=False)
for _mod, _name in MODELS:
    globals()["test_poison_nan__%s__%s" % (_short(_mod), _name[5:])] = _twin(getattr(_mod, _name), NAN)
del _mod, _name, _tag, _v


# ---- whole forwards written for poison ---------------------------------------------------------------------------------------
def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _build_masks(mask):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(mask, 5), 8)


def _ddpm(cache_dtype="f32"):
    """bench.py's network (seed-0 weights, ch 128, channels-last, in-place scatter) built and put through its cache-producing
    full pass by the library's exact-fp32 kernels -- inside the caller's poisoned() context, so every cache, packed weight and
    persistent buffer starts out poisoned."""
    import bench
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    torch.manual_seed(0)
    model = DDPMSparseUNet(DDPMConfig()).eval().to(DEV).to(memory_format=torch.channels_last)
    model.set_scatter_inplace(True)
    model.set_cache_dtype(cache_dtype)
    x0, noise = bench.make_inputs()
    t = torch.zeros(1, device=DEV)
    with util.native_full_pass(), torch.no_grad():
        model.set_mode("full")
        full = model(_cl(x0), t)
    return model, _cl(x0), _cl(noise), t, full


@pytest.mark.parametrize("ratio", [0.012, 0.15])
def test_poisoned_benchmarked_forward_vs_oracle(hip, ratio):
    """The benchmarked configuration from a poisoned start: ONE sparse forward, no warm-up forward (the first one takes the
    path without activated twins, the second the one with them), both against the CPU oracle network; then the conv_in window
    buffer (`_h0_buf`: stale and, by design, unread outside the active windows) filled with NaN -- the next forward must not
    move by a bit; then a hipGraph captured under poison (its own allocations re-poisoned by every replay) must equal the eager
    forward bit for bit."""
    import bench

    mask = bench.edit_mask(ratio)
    full_c, (want,) = util.ddpm_cpu_oracle([mask])
    with util.poisoned() as p, torch.no_grad():
        model, x0, noise, t, full = _ddpm()
        x1 = _cl(x0 + noise * mask.to(DEV))
        model.set_masks(_build_masks(mask.to(DEV)))
        model.set_mode("sparse")
        first = model(x1, t).clone()
        second = model(x1, t).clone()
        assert model._h0_buf is not None
        model._h0_buf.fill_(NAN)
        third = model(x1, t).clone()
        g, out = bench.capture(model, x1, t)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
    assert p.n > 100
    for what, got in (("full", full), ("first", first), ("second", second), ("after NaN _h0_buf", third), ("replay", replayed)):
        util.assert_finite(got, what)
    torch.testing.assert_close(full.cpu(), full_c, rtol=0, atol=util.CONV_ATOL)
    torch.testing.assert_close(first.cpu(), want, rtol=0, atol=util.CONV_ATOL)
    torch.testing.assert_close(second.cpu(), want, rtol=0, atol=util.CONV_ATOL)
    assert torch.equal(third, second)
    assert torch.equal(replayed, second)


@pytest.mark.parametrize("form", ["f16_cache", "f16_compute"])
def test_poisoned_f16_forwards_vs_oracle(hip, form):
    """The fp16-cache forward and the `--dtype f16` forward (fp16 operands) from a poisoned start, one sparse forward and one
    more, each judged against the fp32 CPU oracle by the f16 criterion (sige_amd.tolerance)."""
    import bench
    from sige_amd import tolerance

    mask = bench.edit_mask(0.05)
    _, (want,) = util.ddpm_cpu_oracle([mask])
    with util.poisoned(), torch.no_grad():
        model, x0, noise, t, _ = _ddpm("f16" if form == "f16_cache" else "f32")
        if form == "f16_compute":
            model.set_compute_dtype("f16")
        x1 = _cl(x0 + noise * mask.to(DEV))
        model.set_masks(_build_masks(mask.to(DEV)))
        model.set_mode("sparse")
        outs = [model(x1, t).clone() for _ in range(2)]
    for k, got in enumerate(outs):
        util.assert_finite(got, "forward %d" % k)
        r = tolerance.f16_check(got, want)
        assert r["ok"], (k, r)


@pytest.mark.selfcheck
def test_poisoned_launch_plan_follows_mask_changes(hip):
    """A launch plan recorded under poison (its capacity-sized tile buffers: rows past the current count are never written),
    then the mask sequence of test_launch_plan_follows_mask_changes, with masks of fewer (0.002) and more (0.15) tiles than the
    recording: the plan's run and replay must be finite and equal, bit for bit, the module path of a second model with the
    same caches."""
    from sige_amd import parallel
    from sige_amd.plan import LaunchPlan

    import bench

    def m(ratio, top, left):
        return bench.square_mask(ratio, top=top, left=left).to(DEV)

    masks = [m(0.012, 100, 90), m(0.05, 60, 40), m(0.002, 8, 200), m(0.15, 30, 30), m(0.02, 150, 120), m(0.002, 200, 8)]
    with util.poisoned() as p, torch.no_grad():
        model, x0, noise, t, _ = _ddpm()
        ref, *_ = _ddpm()
        for sa, sb in zip(parallel.cache_slots(model), parallel.cache_slots(ref)):
            parallel._get(sb).copy_(parallel._get(sa))
        parallel.refresh_derived(ref)
        xs = (x0 + noise * masks[0]).clone()
        plan = LaunchPlan(model)
        plan.record(masks[0], _build_masks, lambda: model(xs, t))
        counts = set()
        for k, mk in enumerate(masks):
            x1 = x0 + noise * mk
            xs.copy_(x1)
            plan.bind_mask(mk)
            got = plan.run().clone()
            rep = plan.replay().clone()
            ref.set_masks(_build_masks(mk))
            ref.set_mode("sparse")
            if k == 0:
                ref(x1, t)
            want = ref(x1, t)
            util.assert_finite(got, "plan run %d" % k)
            assert torch.equal(got, want), (k, float((got - want).abs().max()))
            assert torch.equal(rep, got), k
            counts.add(tuple(plan.counts))
        del plan
    assert p.n > 100 and len(counts) >= 4


# ---- tile conv (conv_mfma.hpp) at the tile counts where a workgroup runs short ----------------------------------------------
def _tile_counts(tpb, n_all):
    return sorted({1, 2, max(1, tpb - 1), tpb + 1, 2 * tpb + 1, min(301, n_all)})


@pytest.mark.parametrize("value", list(POISON.values()), ids=list(POISON))
@pytest.mark.parametrize("compute", ["f32", "f16"])
@pytest.mark.parametrize("mt", [16, 32])
@pytest.mark.parametrize("k,stride,blk,off,cin,cout", [(3, 1, 6, 1, 72, 40), (1, 1, 4, 0, 44, 24), (3, 2, 5, 0, 44, 200)])
def test_poisoned_tile_conv_short_workgroups(hip, k, stride, blk, off, cin, cout, mt, compute, value, tuning):
    """The channels-last tile conv and its fused gather form at T = 1, 2, one below and one above the tiles per M block
    (MT / output pixels per tile: conv_mfma.hpp TPB) and ~300 tiles, B = 2, channel counts off the chunk size (multiples of 4: channels-last), tile lists that
    hold the (0, 0) and the (H-1, W-1) corner; automatic and forced (4-way) cross-workgroup K split of the gather form.  Against
    an fp64 conv of the (for f16: fp16-rounded) operands, the tolerances of test_conv_every_output_block_shape (fp32) and
    test_f16_compute_block_conv_exact_products (f16)."""
    from sige_amd.utils import reduce_mask

    torch.manual_seed(k * 1000 + cin + cout + mt)
    B, res = 2, 76
    ro = (blk - k) // stride + 1
    with util.poisoned(value) as p:
        x = _cl(torch.randn(B, cin, res, res, device=DEV))
        w = torch.randn(cout, cin, k, k, device=DEV) / (k * cin ** 0.5)
        bias = torch.randn(cout, device=DEV)
        scale, shift = torch.randn(1, cin, 1, 1, device=DEV), torch.randn(1, cin, 1, 1, device=DEV)
        packed = hip.conv_pack_weights(w, blk, blk, (stride, stride), compute)
        q = (lambda t: t.half().double()) if packed.compute == "f16" else (lambda t: t.double())  # noqa: E731
        atol = 2e-5 if packed.compute == "f16" else 1e-4
        # (f16: no SiLU -- the staged swish_fast may round a value next to an fp16 boundary the other way; the affine is exact)
        act = "identity" if packed.compute == "f16" else "swish"
        idx_all = reduce_mask(torch.ones(res, res, dtype=torch.bool, device=DEV), blk, 4, off)
        n_all = idx_all.shape[0]
        hip.conv_force_tile(mt, 1)
        try:
            for T in _tile_counts(mt // (ro * ro), n_all):
                rows = torch.linspace(0, n_all - 1, T).round().long().unique() if T > 1 else torch.tensor([n_all - 1])
                idx = idx_all[rows.to(DEV)].contiguous()
                tiles = hip.gather(x.contiguous(), blk, blk, idx, scale, shift, act, False)
                want = torch.nn.functional.conv2d(q(tiles), q(w), bias.double(), stride).float()
                got = hip.block_conv_cl(_cl(tiles), packed, bias, cout, (k, k), (stride, stride))
                util.assert_finite(got, "block_conv_cl T=%d" % idx.shape[0])
                torch.testing.assert_close(got, want, rtol=0, atol=atol)
                if stride == 1:
                    for ks in (0, 4):
                        hip.conv_force_ksplit(ks)
                        try:
                            one = hip.gather_conv_cl(x, None, (blk, blk), idx, scale, shift, act, packed, bias, cout, (k, k),
                                                     (stride, stride))
                        finally:
                            hip.conv_force_ksplit(0)
                        util.assert_finite(one, "gather_conv_cl T=%d ksplit=%d" % (idx.shape[0], ks))
                        torch.testing.assert_close(one, want, rtol=0, atol=atol)
        finally:
            hip.conv_force_tile(0, 0)
    assert p.n > 0 and ro * ro * (mt // (ro * ro)) == mt
