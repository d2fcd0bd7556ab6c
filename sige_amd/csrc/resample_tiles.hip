// Resampling residual blocks (Progressive Distillation U-Net: a ResBlock that pools or upsamples INSIDE the block) on the
// active tiles only, channels-last fp32, ONE launch:
//
//   DOWN  conv1's input tiles   tiles[b*N+n, r, s, c] = mean over the 2x2 source pixels of SiLU(scale[c] * x + shift[c]) at the
//                               pooled position (idx[n] + (r, s)), exactly 0 outside the pooled image (the gather's zero padding:
//                               never transformed).  Average pooling does not commute with SiLU, so the fused gather -> conv path
//                               (one source pixel per tile element) cannot express it.
//         shortcut cells        res[b, oh, ow, c] = mean 2x2 of RAW x, on the cells conv2's Scatter writes for the active tiles
//   UP    shortcut cells        res[b, oh, ow, c] = x[b, oh/2, ow/2, c] (nearest x2); conv1's tiles need no kernel of their own:
//                               SiLU commutes with nearest x2 and the fused gather reads the half-resolution tensor (upsample2x)
//
// The cells are those of the fused scatter epilogue: rows (offH + idx[n][0]) / strH + [0, rH), columns likewise, clipped to the
// output.  Cells outside the active tiles are NOT written (stale; the fused conv2 + residual launch never reads them).  With no
// index list every cell of `res` is written (the dense levels).
//
// Work split: blockIdx.z = (image, tile), .y = one row of the tile (conv1's rows first, then the shortcut's), .x = 256 items (16
// bytes each) of that row -- no loop, no division of a flat index by run-time tile geometry; what is left is the 32-bit i / (C / 4)
// per item and z / N per workgroup.  A lane beyond its row reads the row's last item and an out-of-image position its clamped
// neighbour, both dropped by a select: no load sits behind an exec-masked branch.  The scatter's stride is 1 (the
// block's convs are 3x3 / stride 1): (offset + origin) / stride is a plain sum.
//
// Stacked edits (sige_hip_set_edit_batch: the tensors are E images stacked along H, the list holds the tiles of all of them): a
// tile belongs to the image its window's third row lies in (common.hpp: seam_lo, at the RESAMPLED resolution).  The rows of that
// image, [hlo, hhi), take the place of [0, Ho) in the test above: a window row beyond them is zero padding, a shortcut cell
// beyond them is not written.  Both are derived from the scalar origin: two more wave-uniform integers, the loads stay clamped
// to the tensor and selected.  The forms without a list pool or repeat whole images (an even per-image height: no 2x2 window
// and no x2 repeat straddles a seam) and run as they are.
#include <algorithm>

#include "common.hpp"

namespace sige {

constexpr int kRT = 256;

struct ResampleArgs {
    const float *x;
    int B, C, H, W;          // source tensor [B,H,W,C]
    int Ho, Wo;              // resampled resolution: H/2 x W/2 (DOWN), 2H x 2W (UP)
    const int32_t *idx;      // [N,2] tile origins at the resampled resolution; nullptr: every cell of res
    int N, bH, bW;
    const float *scale, *shift;
    float *tiles;            // [B*N,bH,bW,C] (DOWN) or nullptr
    int tile_rows;           // bH when tiles are written, else 0
    int offH, offW, strH, strW, rH, rW;
    float *res;              // [B,Ho,Wo,C] or nullptr
    int hp_shift;            // stacked edits, tiled forms: log2 of one image's height at the resampled resolution (0 = off)
};

__device__ __forceinline__ float4 rt_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ float4 rt_mean4(float4 a, float4 b, float4 c, float4 d) {
    return make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                       ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

// scale, then shift (two separately rounded ops, as everywhere in the library), then SiLU
__device__ __forceinline__ float4 rt_act4(float4 z, float4 s, float4 t) {
    return make_float4(swish(s.x * z.x + t.x), swish(s.y * z.y + t.y), swish(s.z * z.z + t.z), swish(s.w * z.w + t.w));
}

template <bool UP, bool AFFINE>
__global__ __launch_bounds__(kRT) void resample_tiles_kernel(ResampleArgs a) {
    kernarg_touch<128>();
    const unsigned C4 = (unsigned)a.C >> 2;
    // blockIdx.z = b * N + n (b alone without a list); .y = row; .x = 256 items of the row
    int b = blockIdx.z, n = 0, i0 = 0, i1 = 0;
    if (a.idx) {
        b = __builtin_amdgcn_readfirstlane((int)(blockIdx.z / (unsigned)a.N));  // (wave-uniform: the origin is a scalar load)
        n = __builtin_amdgcn_readfirstlane((int)blockIdx.z - b * a.N);
        // (the list is read-only for the launch and the tile is wave-uniform: a scalar load through the constant address space)
        typedef const __attribute__((address_space(4))) int32_t *cidx_t;
        const cidx_t ip = (cidx_t)(a.idx + 2 * n);
        i0 = ip[0];
        i1 = ip[1];
    }
    const bool tile_phase = !UP && (int)blockIdx.y < a.tile_rows;
    // the row of this workgroup: pooled row `oh`, first column `ow0`, `cols` columns
    int oh, ow0, cols;
    if (tile_phase) { oh = i0 + (int)blockIdx.y; ow0 = i1; cols = a.bW; }
    else if (a.idx) { oh = a.offH + i0 + (int)blockIdx.y - a.tile_rows; ow0 = a.offW + i1; cols = a.rW; }
    else { oh = (int)blockIdx.y; ow0 = 0; cols = a.Wo; }
    const unsigned items = (unsigned)cols * C4;
    if (blockIdx.x * kRT >= items) return;  // (the grid is sized for the longer of the two kinds of row)
    const unsigned i = blockIdx.x * kRT + threadIdx.x;
    const unsigned ic = min(i, items - 1);  // a lane beyond the row reads the row's last item and stores nothing
    const unsigned s = ic / C4;
    const int c = (int)(ic - s * C4) * 4;
    const int ow = ow0 + (int)s;
    // (stacked edits: the rows of the tile's own image, from the scalar origin; [0, Ho) otherwise)
    const int hlo = max(seam_lo(i0, a.hp_shift), 0), hhi = a.hp_shift ? min(hlo + (1 << a.hp_shift), a.Ho) : a.Ho;
    const bool ok = oh >= hlo && oh < hhi && ow >= 0 && ow < a.Wo;
    const int ohc = min(max(oh, 0), a.Ho - 1), owc = min(max(ow, 0), a.Wo - 1);  // clamped address, load, select
    const size_t rowC = (size_t)a.W * a.C;  // one source row
    const float *p = a.x + ((size_t)b * a.H + (UP ? (ohc >> 1) : 2 * ohc)) * rowC + (size_t)(UP ? (owc >> 1) : 2 * owc) * a.C + c;
    float4 v;
    if (UP) {
        v = rt_ld4(p);
    } else {
        float4 v00 = rt_ld4(p), v01 = rt_ld4(p + a.C), v10 = rt_ld4(p + rowC), v11 = rt_ld4(p + rowC + a.C);
        if (AFFINE && tile_phase) {
            const float4 sc = rt_ld4(a.scale + c), sh = rt_ld4(a.shift + c);
            v00 = rt_act4(v00, sc, sh); v01 = rt_act4(v01, sc, sh); v10 = rt_act4(v10, sc, sh); v11 = rt_act4(v11, sc, sh);
        }
        v = rt_mean4(v00, v01, v10, v11);
    }
    if (tile_phase) {
        // conv1's input tile: zero padding outside the pooled image
        if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
        float *o = a.tiles + (((size_t)blockIdx.z * a.bH + blockIdx.y) * a.bW) * a.C + (size_t)i * 4;
        if (i < items) store_out4(o, v);
    } else if (ok && i < items) {
        // a shortcut cell: raw x, pooled (DOWN) or repeated (UP); nothing outside the output
        store_out4(a.res + (((size_t)b * a.Ho + ohc) * a.Wo + owc) * a.C + c, v);
    }
}

}  // namespace sige

using namespace sige;

static bool rt_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int sige_hip_resample_tiles_nhwc_f32(const float *x, int B, int C, int H, int W, int mode,
                                                const int32_t *active_indices, int N, int bH, int bW,
                                                const float *scale, const float *shift, float *tiles,
                                                int offsetH, int offsetW, int strideH, int strideW, int rH, int rW,
                                                float *res, void *stream) {
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || N < 0) return SIGE_HIP_EINVAL;
    if (mode != SIGE_HIP_RESAMPLE_DOWN && mode != SIGE_HIP_RESAMPLE_UP) return SIGE_HIP_EUNSUPPORTED;
    const bool up = mode == SIGE_HIP_RESAMPLE_UP;
    if (tiles && (bH <= 0 || bW <= 0)) return SIGE_HIP_EINVAL;
    if (res && active_indices && (rH <= 0 || rW <= 0 || strideH <= 0 || strideW <= 0)) return SIGE_HIP_EINVAL;
    if (C % 4 || (!up && ((H | W) & 1))) return SIGE_HIP_EUNSUPPORTED;
    if (res && active_indices && (strideH != 1 || strideW != 1)) return SIGE_HIP_EUNSUPPORTED;  // (3x3 / stride-1 blocks only)
    if (tiles && (up || !active_indices)) return SIGE_HIP_EUNSUPPORTED;  // (UP tiles: the fused gather's upsample2x read)
    if ((scale == nullptr) != (shift == nullptr)) return SIGE_HIP_EUNSUPPORTED;
    if (!active_indices && N != 0) return SIGE_HIP_EINVAL;                   // (a tile count without a list)
    if (B == 0 || (active_indices && N == 0)) return SIGE_HIP_OK;
    if (!tiles && !res) return SIGE_HIP_OK;
    if (!x) return SIGE_HIP_EINVAL;
    if (!rt_al16(x) || !rt_al16(tiles) || !rt_al16(res) || !rt_al16(scale) || !rt_al16(shift)) return SIGE_HIP_EUNSUPPORTED;
    // stacked edits: one image's height at the resampled resolution is a power of two >= 4 (the seam test is a shift)
    const int src_shift = stacked_shift(H);
    if (src_shift < 0) return SIGE_HIP_EUNSUPPORTED;
    if (src_shift && !up && active_indices && src_shift < 3) return SIGE_HIP_EUNSUPPORTED;  // (a pooled image of < 4 rows)

    ResampleArgs a;
    a.x = x; a.B = B; a.C = C; a.H = H; a.W = W;
    a.Ho = up ? 2 * H : H / 2; a.Wo = up ? 2 * W : W / 2;
    a.idx = active_indices; a.N = N; a.bH = bH; a.bW = bW;
    a.scale = scale; a.shift = shift; a.tiles = tiles; a.tile_rows = tiles ? bH : 0;
    a.offH = offsetH; a.offW = offsetW; a.strH = strideH; a.strW = strideW; a.rH = rH; a.rW = rW;
    a.res = res;
    a.hp_shift = (src_shift && active_indices) ? (up ? src_shift + 1 : src_shift - 1) : 0;
    const int res_rows = !res ? 0 : (active_indices ? rH : a.Ho);
    const long rows = (long)a.tile_rows + res_rows, zs = active_indices ? (long)B * N : (long)B;
    if (rows > 65535 || zs > 65535) return SIGE_HIP_EUNSUPPORTED;             // (grid y / z)
    const long row_items = (long)(C / 4) * std::max(tiles ? bW : 0, !res ? 0 : (active_indices ? rW : a.Wo));
    const dim3 grid((unsigned)((row_items + kRT - 1) / kRT), (unsigned)rows, (unsigned)zs);
    hipStream_t st = as_stream(stream);
    if (up)
        resample_tiles_kernel<true, false><<<grid, kRT, 0, st>>>(a);
    else if (scale)
        resample_tiles_kernel<false, true><<<grid, kRT, 0, st>>>(a);
    else
        resample_tiles_kernel<false, false><<<grid, kRT, 0, st>>>(a);
    return launch_status();
}
