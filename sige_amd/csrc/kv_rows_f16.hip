// The producer of attention_tokens_f16kv.hip's operands in a sparse pass: the K and V rows of the active tokens -- fp32 [B T 16, C], as
// the q | k | v token linear (parts = 3) or Attention.qkv leaves them, row 16t + 4i + j = cell (i, j) of tile t -- rounded to nearest
// even to fp16 and written over rows (y0 + i) W + x0 + j of the persistent fp16 K and V [B, H W, C]: ONE launch for both tensors, in
// place of the two channels-last Scatter launches of a block (and of the rounding the f16c attention repeats at every load).
// Index list, batch-major tile order (tile t of B T: image t / T, list entry t % T) and the cells off the image (skipped) are the
// in-place channels-last Scatter's (nhwc_ops.hip, scatter_tiles_nhwc_kernel) with offset 0 and stride 1: the token grid's tiles.
// A lane converts 8 channels of one cell of BOTH tensors: two 16-byte loads and one 16-byte store each.  Every index is split with
// 32-bit divisions (for_units: DESIGN.md 5.7).
// Second entry, sige_hip_kv_tiles_store_f16 (below): the producer of attention_wide_f16kv.hip's operands, where K | V is no row matrix
// but ONE channels-last image -- the same tiles, read from the fp32 image and rounded into the same cells of an fp16 image.
#include "common.hpp"

namespace sige {

typedef float kvf32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 kvf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 kvf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ kvf16x8 round8(const float *p) {  // (fptrunc: round to nearest even)
    const kvf16x4 lo = __builtin_convertvector(*reinterpret_cast<const kvf32x4 *>(p), kvf16x4);
    const kvf16x4 hi = __builtin_convertvector(*reinterpret_cast<const kvf32x4 *>(p + 4), kvf16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256) void kv_rows_store_f16_kernel(const float *__restrict__ k_rows, const float *__restrict__ v_rows,
                                                                _Float16 *__restrict__ k16, _Float16 *__restrict__ v16,
                                                                const int32_t *__restrict__ idx, int T, int H, int W, int C, long units) {
    const int C8 = C / 8;
    for_units<256>(units, [&](auto u) {
        const int c = (int)(u % C8) * 8;
        const decltype(u) cell = u / C8;  // 16t + 4i + j
        const int p = (int)(cell & 15);
        const int t = (int)(cell >> 4);
        const int b = t / T, n = t - b * T;
        const int h = idx[2 * n] + (p >> 2), w = idx[2 * n + 1] + (p & 3);
        if (h < 0 || h >= H || w < 0 || w >= W) return;
        const size_t src = (size_t)cell * C + c, dst = (((size_t)b * H + h) * W + w) * C + c;
        *reinterpret_cast<kvf16x8 *>(k16 + dst) = round8(k_rows + src);
        *reinterpret_cast<kvf16x8 *>(v16 + dst) = round8(v_rows + src);
    });
}

// The producer of attention_wide_f16kv.hip's operands in the SD VAE attention block, which has no row matrices: the fused K | V conv
// writes the new tiles straight into the persistent channels-last fp32 image [1,C,H,W] (C = both tensors' channels).  The 4x4 tiles
// of the index list are read from that image and rounded into the SAME cells of an fp16 image of the same shape; every other cell
// of the fp16 image is left as it is.  A lane converts 8 channels of one cell: two 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void kv_tiles_store_f16_kernel(const float *__restrict__ src, _Float16 *__restrict__ dst,
                                                                 const int32_t *__restrict__ idx, int H, int W, int C, long units) {
    const int C8 = C / 8;
    for_units<256>(units, [&](auto u) {
        const int c = (int)(u % C8) * 8;
        const decltype(u) cell = u / C8;  // 16t + 4i + j
        const int p = (int)(cell & 15);
        const int t = (int)(cell >> 4);
        const int h = idx[2 * t] + (p >> 2), w = idx[2 * t + 1] + (p & 3);
        if (h < 0 || h >= H || w < 0 || w >= W) return;
        const size_t at = ((size_t)h * W + w) * C + c;
        *reinterpret_cast<kvf16x8 *>(dst + at) = round8(src + at);
    });
}

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_kv_tiles_store_f16(const float *src, void *dst16, const int32_t *active_indices, int T, int H, int W, int C,
                                           void *stream) {
    SIGE_PLAN_HOOK_N(sige_hip_kv_tiles_store_f16, (sige::CountOf<2, 3>), src, dst16, active_indices, T, H, W, C, stream);
    if (T < 0 || H <= 0 || W <= 0 || C <= 0) return SIGE_HIP_EINVAL;
    if (T == 0) return SIGE_HIP_OK;  // (no tile: nothing is launched)
    if (!src || !dst16 || !active_indices) return SIGE_HIP_EINVAL;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (C % 8 || !al(src) || !al(dst16) || T > 0x7ffffff) return SIGE_HIP_EUNSUPPORTED;
    const long units = (long)T * 16 * (C / 8);
    const long grid = (units + 255) / 256;
    kv_tiles_store_f16_kernel<<<(int)(grid > 16384 ? 16384 : grid), 256, 0, as_stream(stream)>>>(
        src, static_cast<_Float16 *>(dst16), active_indices, H, W, C, units);
    return launch_status();
}

extern "C" int sige_hip_kv_rows_store_f16(const float *k_rows, const float *v_rows, void *k16, void *v16, const int32_t *active_indices,
                                          int tiles_per_image, int B, int H, int W, int C, void *stream) {
    SIGE_PLAN_HOOK_N(sige_hip_kv_rows_store_f16, (sige::CountOf<4, 5>), k_rows, v_rows, k16, v16, active_indices, tiles_per_image, B, H, W, C, stream);
    if (tiles_per_image < 0 || B < 0 || H <= 0 || W <= 0 || C <= 0) return SIGE_HIP_EINVAL;
    const long units = (long)B * tiles_per_image * 16 * (C / 8);
    if ((long)B * tiles_per_image == 0) return SIGE_HIP_OK;  // (no tile: nothing is launched)
    if (!k_rows || !v_rows || !k16 || !v16 || !active_indices) return SIGE_HIP_EINVAL;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (C % 8 || !al(k_rows) || !al(v_rows) || !al(k16) || !al(v16) || (long)B * tiles_per_image > 0x7ffffffL) return SIGE_HIP_EUNSUPPORTED;
    const long grid = (units + 255) / 256;
    kv_rows_store_f16_kernel<<<(int)(grid > 16384 ? 16384 : grid), 256, 0, as_stream(stream)>>>(
        k_rows, v_rows, static_cast<_Float16 *>(k16), static_cast<_Float16 *>(v16), active_indices, tiles_per_image, H, W, C, units);
    return launch_status();
}
