// Tile conv v3 (conv_tile3.hpp): C ABI.  One entry point for both staging sources, both destinations and both operand forms;
// weights in the layouts of the dense-layer kernel (sige_hip_wide_conv_pack).
#include "conv_call.hpp"
#include "conv_tile3.hpp"

namespace sige {
template <> void launch_conv_tile3_gather<2>(const Tile3Args &, bool, bool, bool, hipStream_t);
template <> void launch_conv_tile3_sg<2>(const Tile3Args &, bool, bool, hipStream_t);
template <> void launch_conv_tile3_gather<2, WIDE_F16>(const Tile3Args &, bool, bool, bool, hipStream_t);
template <> void launch_conv_tile3_sg<2, WIDE_F16>(const Tile3Args &, bool, bool, hipStream_t);
template <> void launch_conv_tile3_gather<4, WIDE_F16>(const Tile3Args &, bool, bool, bool, hipStream_t);
template <> void launch_conv_tile3_sg<4, WIDE_F16>(const Tile3Args &, bool, bool, hipStream_t);
// fp16 operands: 4 tiles per workgroup from this many 2-tile workgroups on (SIGE_HIP_TUNE_TILE3_F16_TPW4_MIN = -1: this value)
constexpr int kTile3F16Tpw4Min = 0;  // (measured, profiles/r6i_tile3_f16_tpw4_bench.json: wins at 834 workgroups only, -0.2 % on the forward: never)
bool conv_hold_pending();  // (block_conv.hip: a shortcut held for a pair launch, an armed sige_hip_conv_side_begin or queued side convs)
int flush_held_conv();  // (block_conv.hip: a shortcut conv held by sige_hip_conv_pair_begin is launched on its own first)
}  // namespace sige

using namespace sige;

static_assert(CALL_GATHER == T3_GATHER && CALL_SCATTER_GATHER == T3_SCATTER_GATHER, "TileConvCall::source is the v3 ABI's `source`");

extern "C" int sige_hip_tile_conv3_supported(int C1, int C2, int Cout) {
    return (C1 > 0 && C2 >= 0 && C1 % 64 == 0 && C2 % 64 == 0 && Cout > 0 && Cout % 64 == 0) ? 1 : 0;
}

extern "C" int sige_hip_tile_conv3_block_supported(int C1, int C2, int Cout, int bH, int bW) {
    return (bH == bW && (bH == 6 || bH == 10)) ? sige_hip_tile_conv3_supported(C1, C2, Cout) : 0;
}

// (no plan hook: the extern "C" wrappers below and the routing entry points of block_conv.hip record themselves)
int sige::tile_conv3_launch(const TileConvCall &c, int prec, int block) {
    if (c.source != T3_GATHER && c.source != T3_SCATTER_GATHER) return SIGE_HIP_EINVAL;
    if (prec != WIDE_F32 && prec != WIDE_F16) return SIGE_HIP_EUNSUPPORTED;
    if (block != 6 && block != 10) return SIGE_HIP_EUNSUPPORTED;
    const bool b10 = block == 10;
    // 10x10 windows: exact fp32 over fp32-stored tensors (the next line but one refuses x2_f16 / res_f16)
    if (b10 && prec != WIDE_F32) return SIGE_HIP_EUNSUPPORTED;
    if (c.x2_f16 && c.source != T3_SCATTER_GATHER) return SIGE_HIP_EINVAL;
    if ((c.x2_f16 || c.res_f16) && prec != WIDE_F16) return SIGE_HIP_EUNSUPPORTED;  // (fp16-stored caches: the f16 form only)
    if (c.B < 0 || c.N < 0 || c.C1 <= 0 || c.C2 < 0 || c.Cout <= 0 || c.H <= 0 || c.W <= 0) return SIGE_HIP_EINVAL;
    if (c.tiles() == 0) return SIGE_HIP_OK;
    const bool sg = c.source == T3_SCATTER_GATHER;
    const float *packed = c.packed_tile3, *scale = c.aff.scale, *shift = c.aff.shift;
    if (!c.x || !packed || !c.out || !c.idx || ((c.C2 || sg) && !c.x2) || (sg && (!c.map || c.Rx <= 0 || c.Sx <= 0))) return SIGE_HIP_EINVAL;
    if (sg && (c.C2 || c.up)) return SIGE_HIP_EUNSUPPORTED;  // (one channel range; round 6: the cached affine + SiLU in the staging path too -- SD's conv2)
    if (!sige_hip_tile_conv3_supported(c.C1, c.C2, c.Cout)) return SIGE_HIP_EUNSUPPORTED;
    if (b10 && sg && (scale || shift)) return SIGE_HIP_EUNSUPPORTED;  // (10x10 windows: the scatter_gather source is raw)
    const int Cin = c.Cin();
    if (int rc = staging_affine_status(c.aff, c.B, Cin, SIGE_HIP_EINVAL, SIGE_HIP_EINVAL)) return rc;
    if (!act_known(c.aff.act)) return SIGE_HIP_EUNSUPPORTED;
    if (int rc = out_affine_status(c.oscale, c.oshift)) return rc;
    if (c.oscale && !act_known(c.oact)) return SIGE_HIP_EUNSUPPORTED;
    if (c.up && ((c.H | c.W) & 1)) return SIGE_HIP_EINVAL;
    if (c.to_full && (c.Ho <= 0 || c.Wo <= 0)) return SIGE_HIP_EINVAL;
    if (!c.to_full && (c.residual || c.x1 || c.twin[0].out || c.twin[1].out)) return SIGE_HIP_EINVAL;
    if (c.x1 && (!c.residual || !c.table1 || c.N1 < 0 || c.R1 <= 0 || c.S1 <= 0 || c.gW1 <= 0)) return SIGE_HIP_EINVAL;
    if (int rc = twins_status(c.twin)) return rc;
    const long src_px = sg ? (long)c.B * c.H * c.W : (long)c.B * (c.H >> (c.up ? 1 : 0)) * (c.W >> (c.up ? 1 : 0));
    if (!offsets_fit(src_px * Cin) || !offsets_fit(c.tiles() * (b10 ? 100 : 36) * Cin)) return SIGE_HIP_EUNSUPPORTED;
    if (!aligned16({c.x, c.x2, packed, c.out, c.bias, scale, shift, c.residual, c.x1, c.oscale, c.oshift}) || !twins_aligned(c.twin))
        return SIGE_HIP_EUNSUPPORTED;
    Tile3Args a{};
    a.x = c.x; a.x2 = c.x2 ? static_cast<const float *>(c.x2) : c.x; a.idx = c.idx; a.map = c.map; a.packed = packed; a.bias = c.bias;
    a.scale = scale; a.shift = shift; a.residual = static_cast<const float *>(c.residual); a.oscale = c.oscale; a.oshift = c.oshift; a.out = c.out;
    a.twin0 = c.twin[0].out; a.tscale0 = c.twin[0].scale; a.tshift0 = c.twin[0].shift;
    a.twin1 = c.twin[1].out; a.tscale1 = c.twin[1].scale; a.tshift1 = c.twin[1].shift;
    a.x1 = c.x1; a.table1 = c.table1; a.gW1 = c.gW1; a.N1 = c.N1; a.R1 = c.R1; a.S1 = c.S1;
    a.B = c.B; a.N = c.N; a.T = c.B * c.N; a.H = c.H; a.W = c.W; a.C1 = c.C1; a.C2 = c.C2; a.Cout = c.Cout; a.up = c.up ? 1 : 0;
    a.act = c.aff.act; a.oact = c.oact; a.aff_sb = (scale && c.aff.scaleB > 1) ? Cin : 0;
    if (!b10 && a.aff_sb && c.N % Tile3Geo<2>::TPW) return SIGE_HIP_EUNSUPPORTED;  // (a workgroup's tiles must share one image's affine)
    a.Rx = c.Rx; a.Sx = c.Sx; a.Ho = c.Ho; a.Wo = c.Wo; a.offH = c.offH; a.offW = c.offW;
    a.ntn = c.Cout / 64; a.nchunks = Cin / 64; a.nchunks1 = c.C1 / 64;
    if (edit_shift_status(c.H, c.B, &a.hp_shift) != SIGE_HIP_OK) return SIGE_HIP_EUNSUPPORTED;
    a.res_f16 = c.res_f16 ? 1 : 0;
    const bool aff = scale != nullptr, cat = c.C2 > 0, full = c.to_full != 0, y16 = c.x2_f16 != 0;
    hipStream_t st = as_stream(c.stream);
    if (b10) {
        // no stacked edits (the kernel's row limits are the image's), and nothing held or queued on the stacked-block kernels:
        // those forms exist for 6x6 / 4x4 blocks only, and a caller that mixes geometries gets its fallback, never a reordering
        if (a.hp_shift || conv_hold_pending()) return SIGE_HIP_EUNSUPPORTED;
        if (sg) launch_conv_tile3_b10_sg(a, full, st);
        else launch_conv_tile3_b10_gather(a, aff, cat, full, st);
        return launch_status(1);
    }
    const int rc = flush_held_conv();
    if (rc != SIGE_HIP_OK) return rc;
    if (prec == WIDE_F16) {
        int t4min = tuning(SIGE_HIP_TUNE_TILE3_F16_TPW4_MIN);
        if (t4min < 0) t4min = kTile3F16Tpw4Min;
        const bool four = t4min > 0 && (long)((a.T + 1) / 2) * a.ntn >= t4min && !(a.aff_sb && c.N % 4);
        if (four) {
            if (sg) launch_conv_tile3_sg<4, WIDE_F16>(a, full, y16, st);
            else launch_conv_tile3_gather<4, WIDE_F16>(a, aff, cat, full, st);
        } else if (sg) launch_conv_tile3_sg<2, WIDE_F16>(a, full, y16, st);
        else launch_conv_tile3_gather<2, WIDE_F16>(a, aff, cat, full, st);
    } else {
        if (sg) launch_conv_tile3_sg<2>(a, full, false, st);
        else launch_conv_tile3_gather<2>(a, aff, cat, full, st);
    }
    return launch_status(1);
}

// the record of both v3 entry points: `packed` is the v3 layout; the affine has one entry per input channel, affineB images
#define SIGE_TILE3_CALL(c)                                                                                                       \
    TileConvCall c{};                                                                                                            \
    c.source = source; c.x = x; c.x2 = x2; c.x2_f16 = y_f16; c.B = B; c.C1 = C1; c.C2 = C2; c.H = H; c.W = W; c.up = upsample2x;   \
    c.idx = active_indices; c.N = N; c.map = scatter_map; c.Rx = Rx; c.Sx = Sx;                                                  \
    c.aff = {scale, shift, affineB, C1 + C2, affineB, C1 + C2, activation};                                                      \
    c.packed_tile3 = packed; c.bias = bias; c.Cout = Cout;                                                                       \
    c.to_full = to_full; c.offH = offsetH; c.offW = offsetW; c.Ho = Ho; c.Wo = Wo; c.residual = residual; c.res_f16 = residual_f16; \
    c.x1 = x1; c.table1 = table1; c.gH1 = gH1; c.gW1 = gW1; c.N1 = N1; c.R1 = R1; c.S1 = S1;                                       \
    c.oscale = out_scale; c.oshift = out_shift; c.oact = out_activation;                                                         \
    c.twin[0] = {twin0, twin_scale0, twin_shift0}; c.twin[1] = {twin1, twin_scale1, twin_shift1};                                \
    c.out = out; c.stream = stream

// compute 0: exact fp32, `packed` = sige_hip_wide_conv_pack(prec = 2), fp32-stored tensors only.  compute 1: fp16 operands
// (BASELINE.json configs[4]), `packed` = sige_hip_wide_conv_pack(prec = 0) of the same weight; activations are fp32 in HBM and
// rounded to fp16 (RNE) in the staging path, products exact, accumulation fp32.  y_f16: source 2's cached tensor x2 holds halves;
// residual_f16: `residual` holds halves (the fp16-stored caches of SIGEModel.set_cache_dtype("f16")).  compute 2: no such kernel.
extern "C" int sige_hip_tile_conv3_nhwc(
        int compute, int source, const float *x, const void *x2, int y_f16, int B, int C1, int C2, int H, int W, int upsample2x,
        const int32_t *active_indices, int N, const int32_t *scatter_map, int Rx, int Sx,
        const float *scale, const float *shift, int affineB, int activation,
        const float *packed, const float *bias, int Cout,
        int to_full, int offsetH, int offsetW, int Ho, int Wo, const void *residual, int residual_f16,
        const float *x1, const int32_t *table1, int gH1, int gW1, int N1, int R1, int S1,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin_scale0, const float *twin_shift0,
        float *twin1, const float *twin_scale1, const float *twin_shift1,
        float *out, void *stream) {
    SIGE_PLAN_HOOK_N(sige_hip_tile_conv3_nhwc, (sige::CountOf<11, 12>, sige::CountOf<31, 34>), compute, source, x, x2, y_f16, B, C1, C2, H, W, upsample2x, active_indices, N, scatter_map, Rx, Sx, scale, shift, affineB, activation, packed, bias, Cout, to_full, offsetH, offsetW, Ho, Wo, residual, residual_f16, x1, table1, gH1, gW1, N1, R1, S1, out_scale, out_shift, out_activation, twin0, twin_scale0, twin_shift0, twin1, twin_scale1, twin_shift1, out, stream);
    if (compute < 0 || compute > 2) return SIGE_HIP_EINVAL;
    if (compute == 2) return SIGE_HIP_EUNSUPPORTED;
    SIGE_TILE3_CALL(c);
    return tile_conv3_launch(c, compute == 1 ? WIDE_F16 : WIDE_F32, 6);
}

// ... with the window edge as an argument: bH = bW = 6 is sige_hip_tile_conv3_nhwc; bH = bW = 10 runs the same kernel over ONE
// 10x10 window (8x8 output pixels) per workgroup -- compute 0 over fp32-stored tensors only, a raw scatter_gather source, no
// stacked edits, nothing held (sige_hip_conv_pair_begin) or queued (sige_hip_conv_side_begin).  This entry point has no plan hook:
// a recording launch plan would not see the call, so while one records it is refused here (the host side refuses such models
// before it records anything: LaunchPlan.record, hip._refuse_in_plan).
extern "C" int sige_hip_tile_conv3_block_nhwc(
        int compute, int source, const float *x, const void *x2, int y_f16, int B, int C1, int C2, int H, int W, int bH, int bW, int upsample2x,
        const int32_t *active_indices, int N, const int32_t *scatter_map, int Rx, int Sx,
        const float *scale, const float *shift, int affineB, int activation,
        const float *packed, const float *bias, int Cout,
        int to_full, int offsetH, int offsetW, int Ho, int Wo, const void *residual, int residual_f16,
        const float *x1, const int32_t *table1, int gH1, int gW1, int N1, int R1, int S1,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin_scale0, const float *twin_shift0,
        float *twin1, const float *twin_scale1, const float *twin_shift1,
        float *out, void *stream) {
    if (compute < 0 || compute > 2) return SIGE_HIP_EINVAL;
    if (bH != bW || (bH != 6 && bH != 10)) return SIGE_HIP_EUNSUPPORTED;
    if (bH == 6)
        return sige_hip_tile_conv3_nhwc(compute, source, x, x2, y_f16, B, C1, C2, H, W, upsample2x, active_indices, N, scatter_map, Rx, Sx, scale, shift,
                                        affineB, activation, packed, bias, Cout, to_full, offsetH, offsetW, Ho, Wo, residual, residual_f16,
                                        x1, table1, gH1, gW1, N1, R1, S1, out_scale, out_shift, out_activation, twin0, twin_scale0, twin_shift0,
                                        twin1, twin_scale1, twin_shift1, out, stream);
    if (sige::g_plan_rec) return SIGE_HIP_EUNSUPPORTED;
    if (compute != 0 || y_f16 || residual_f16) return SIGE_HIP_EUNSUPPORTED;
    if (source == T3_SCATTER_GATHER && (Rx != 8 || Sx != 8)) return SIGE_HIP_EUNSUPPORTED;
    SIGE_TILE3_CALL(c);
    return tile_conv3_launch(c, WIDE_F32, 10);
}
