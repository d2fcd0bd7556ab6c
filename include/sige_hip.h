/*
 * sige_hip.h -- C ABI of libsige_hip.so: the MI355X (gfx950) native backend of
 * SIGE's tiling-based sparse convolution path.
 *
 * This is the drop-in boundary for the path: every entry point replaces one
 * function of the reference's native backend surface (the five functions each of
 * sige/cpu/pybind_cpu.cpp:5-12, sige/cuda/pybind_cuda.cpp:5-12 export), plus the
 * index reduction of sige/utils.py:8-37 and the stacked-block convolution the
 * reference delegates to F.conv2d (sige/nn/base.py:85-92).
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types.  All tensors are dense,
 *     contiguous, fp32 (the reference is fp32-only: sige/nn/base.py:15), NCHW like the
 *     reference's -- except in the entry points named *_nhwc*, which take the same
 *     tensors channels-last ([B,H,W,C], tiles [T,R,S,C]; same arithmetic);
 *     index tensors are int32 [N,2] = (h, w) tile origins in the INPUT
 *     coordinates of the paired conv (sige/utils.py:30-37).
 *   - the CALLER allocates outputs (the reference's wrappers call torch::empty /
 *     y.clone() themselves: gather.cpp:75, scatter.cpp:83); nothing here
 *     allocates, frees or synchronises, so every call is hipGraph-capturable.
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and the
 *     call returns immediately (the reference launches on the legacy default
 *     stream with no error check: sige/cuda/gather_kernel.cu:113).
 *   - broadcastable operands (scale / shift / residual) are passed as a pointer
 *     (NULL = absent) plus their four dims, each either 1 or the full extent
 *     (binary_op_array, sige/cpu/common_cpu.cpp:13-27).
 *   - return value: SIGE_HIP_OK or a negative SIGE_HIP_E* code; the reference's
 *     asserts / __builtin_unreachable (sige/common.cpp:17-23) become
 *     SIGE_HIP_EINVAL / SIGE_HIP_EUNSUPPORTED.
 */
#ifndef SIGE_HIP_H
#define SIGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIGE_HIP_VERSION 310 /* 0.3.10: one entry point per channels-last tile conv, `compute` / cache storage / v3 weights as arguments */

enum {
    SIGE_HIP_OK = 0,
    SIGE_HIP_EINVAL = -1,       /* bad pointer / negative or inconsistent size */
    SIGE_HIP_EUNSUPPORTED = -2, /* unknown activation, unsupported shape */
    SIGE_HIP_ELAUNCH = -3,      /* hipGetLastError() after the launch was not hipSuccess */
    SIGE_HIP_ENODEVICE = -4     /* no gfx950 device visible to the process */
};

/* activation ids: the two names the reference's native code knows
 * (sige/common.cpp:4,11-23). */
enum { SIGE_HIP_ACT_IDENTITY = 0, SIGE_HIP_ACT_SWISH = 1,
       /* library extensions, accepted only by the entry points that say so (the GauGAN helpers below): */
       SIGE_HIP_ACT_RELU = 2, SIGE_HIP_ACT_LEAKY = 3 /* leaky ReLU with the call's `slope` */, SIGE_HIP_ACT_TANH = 4 };

/* ---- thread-safety ("re-entrant, no global state") ---------------------------------------------------------
 * Every compute entry point (gather / scatter / scatter_gather / scatter_map / reduce_mask / mask pipeline / block_conv /
 * wide_conv / group_norm / attention / spade / conv_in / conv_out ...) is RE-ENTRANT: it reads its arguments, enqueues on
 * the stream it is handed and returns; the kernels a call runs depend on its arguments alone.  The product library keeps
 * no process-global mutable dispatch state.  What state there is:
 *   per HOST THREAD  : sige_hip_set_edit_batch (the stacked-edit factor E of the tensors this thread hands over; a launch
 *                      plan records the call, so a replayed plan restores it), sige_hip_conv_pair_begin / _end (the held
 *                      shortcut conv of a pair), sige_hip_plan_begin / _end (the plan this thread is recording into);
 *   per DEVICE, mutex: the K-split ticket buffer (sige_hip_split_tickets_reset) and sige_hip_preload's loaded-device set;
 *   atomic counters  : sige_hip_launch_count, sige_hip_last_launch_device, sige_hip_conv_pairs_fused (measurement aids);
 *   a plan OBJECT    : one thread at a time per plan (create / record / bind / run / destroy are not internally locked).
 *
 * ---- measurement builds only: dispatch knobs ----------------------------------------------------------------------------
 * Round 4 shipped ten process-global `sige_hip_*_force_*` setters.  They are gone from the product library; a library built
 * with -DSIGE_HIP_TUNING (lib/libsige_hip_tuning.so; tools/, bench sections that compare kernel forms, tests that force a form)
 * exports ONE setter / getter over the keys below (atomic; process-wide; 0 / -1 defaults = the product's behaviour). */
enum {
    SIGE_HIP_TUNE_CONV_TILE_MT = 0,          /* pin the tile conv's output block: 16 | 32 pixels (0 = per launch) */
    SIGE_HIP_TUNE_CONV_TILE_NB = 1,          /* ... x nb * mt output channels, nb 1 | 2 (with CONV_TILE_MT) */
    SIGE_HIP_TUNE_CONV_WAVES = 2,            /* waves per workgroup of the channels-last stride-1 kernels: 4 | 8 (0 = per launch) */
    SIGE_HIP_TUNE_CONV_LARGE_GRID_NB1 = 3,   /* unsplit full grids take 32 x 32 blocks from this many 32 x 64 blocks on (-1 = library: exact fp32 always; 0 never) */
    SIGE_HIP_TUNE_CONV_KSPLIT = 4,           /* cross-workgroup K split: 1..8 = at most this many (0 = per launch) */
    SIGE_HIP_TUNE_CONV_KSPLIT_SECOND_PASS = 5, /* 1 = finish a K split by a second launch instead of inside the launch */
    SIGE_HIP_TUNE_GATHER_ONE_TILE_ROWS = 6,  /* 1 = the NCHW gather always in its one-tile-per-workgroup row form */
    SIGE_HIP_TUNE_SCATTER_GATHER_FORM = 7,   /* bit 0: always the element form; bit 1: never the grouped row form */
    SIGE_HIP_TUNE_SMALL_COUT_SCALAR = 8,     /* 1 = conv3x3_small_cout always on its scalar-weight kernel */
    SIGE_HIP_TUNE_WIDE_KSPLIT = 9,           /* dense-layer conv: pin the K split (0 = automatic) */
    SIGE_HIP_TUNE_ATTENTION_FORM = 10,       /* attention_tokens: 1 = 16 queries per workgroup | 2 = 32 (0 = automatic) */
    SIGE_HIP_TUNE_TILE3_F16_TPW4_MIN = 11,  /* tile conv v3, fp16 operands: 4 tiles per workgroup from this many 2-tile workgroups on (-1 = library; 0 never) */
    SIGE_HIP_TUNE_TILE3_F16_PAIR_MIN = 12,  /* tile conv v3, fp16 operands: a conv1 whose 1x1 shortcut is held for the pair kernel goes to v3 anyway (the shortcut launched on its own) from this many workgroups on (-1 = library; 0 never) */
    SIGE_HIP_TUNE_TILE3_F16_SPARSE_MIN = 13, /* tile conv v3, fp16 operands: launches over a SPARSE tile list (fewer tiles than 4x4 cells) go to v3 from this many workgroups on, below the general threshold (-1 = library; 0 = no separate rule) */
    SIGE_HIP_TUNE_TOKEN_LINEAR_FORM = 14,    /* token_linear: 1 = 16 tokens per workgroup | 2 = 64 (0 = automatic, by grid fill) */
    SIGE_HIP_TUNE_COUNT = 15
};
#ifdef SIGE_HIP_TUNING
int sige_hip_tuning_set(int key, int value); /* SIGE_HIP_EINVAL for an unknown key or a value outside the key's range */
int sige_hip_tuning_get(int key);            /* the current value (the default if never set); INT_MIN for an unknown key */
#endif

/* Load the code objects of every translation unit of this library on the CURRENT device now (HIP loads a code object on the
 * first launch of one of its kernels: 44 of them, 0.3 - 40 ms each, which otherwise lands on the first forward that happens to
 * select a not-yet-used kernel variant -- e.g. a new mask whose tile count picks another block shape).  Idempotent per
 * device; not capturable (call it before capturing).  Returns the number of code objects touched, or a negative status. */
int sige_hip_preload(void);

int sige_hip_version(void);
const char *sige_hip_error_string(int status);
/* name of device 0's gcnArchName ("gfx950...") or NULL if no device. */
const char *sige_hip_device_arch(void);
/* number of GPU kernels this library has launched in the process so far (all entry
 * points, all streams): measurement aid -- launches per forward in bench.py. */
int64_t sige_hip_launch_count(void);
/* HIP's current device at the most recent kernel launch of this library (-1: none yet).  Every entry point launches on the
 * CURRENT device with the stream it is handed (like the reference's sige/cuda wrappers, which have no CUDAGuard either); the
 * host side guards (sige_amd/hip.py: _Guarded).  Debug aid for testing that guard. */
int sige_hip_last_launch_device(void);

/* ---- gather : replaces gather_cpu / gather_cuda -------------------------
 * (sige/cpu/gather.cpp:60-114, sige/cuda/gather_kernel.cu:69-124, gather.h:5-12)
 * x [B,C,H,W] -> out [B*N,C,bH,bW];  out-of-image elements are exactly 0.   */
int sige_hip_gather_f32(const float *x, int B, int C, int H, int W, int bH, int bW,
                        const int32_t *active_indices, int N,
                        const float *scale, int scaleB, int scaleC, int scaleH, int scaleW,
                        const float *shift, int shiftB, int shiftC, int shiftH, int shiftW,
                        int activation, int activation_first, float *out, void *stream);

/* ---- scatter : replaces scatter_cpu / scatter_cuda ----------------------
 * (sige/cpu/scatter.cpp:70-109, sige/cuda/scatter_kernel.cu:76-117, scatter.h:5-11)
 * out [B,C,H,W] = y, with the tiles x [B*N,C,R,S] written at (off+idx)/stride
 * (clipped bottom/right) + residual.  `out` must not alias `y`.
 * Works for ARBITRARY index lists (copy pass + tile pass).                   */
int sige_hip_scatter_f32(const float *x, const float *y, int B, int C, int H, int W, int R, int S,
                         int offsetH, int offsetW, int strideH, int strideW,
                         const int32_t *active_indices, int N,
                         const float *residual, int resB, int resC, int resH, int resW,
                         float *out, void *stream);

/* ---- scatter_with_block_residual : replaces scatter_with_block_residual_*
 * (sige/cpu/scatter.cpp:111-135, sige/cuda/scatter_kernel.cu:119-146, scatter.h:13-19)
 * out = scatter(x0, y0, residual = y1); out += x1 - y1 on the shortcut tiles
 * idx1 (coordinates used directly).                                          */
int sige_hip_scatter_with_block_residual_f32(
        const float *x0, const float *y0, const float *x1, const float *y1,
        int B, int C, int H, int W, int R0, int S0, int R1, int S1,
        int offsetH, int offsetW, int strideH, int strideW,
        const int32_t *active_indices0, int N0, const int32_t *active_indices1, int N1,
        float *out, void *stream);

/* ---- tile table + fused single-pass scatter (MI355X-first fast path) ------
 * For index lists produced by reduce_mask, output tiles lie on a regular grid
 * of pitch (R,S) (block_stride = out_tile * conv_stride, sige/nn/gather.py:37),
 * so "which tile covers pixel (h,w)" is a [gH,gW] int32 lookup, gH=ceil(H/R).
 * sige_hip_tile_table_i32 builds it (cells with no tile = -1); the *_fused
 * variants then produce `out` in ONE streaming pass (no clone + overwrite).
 * Results are bit-identical to the two-pass entry points above.             */
int sige_hip_tile_table_i32(const int32_t *active_indices, int N, int offsetH, int offsetW,
                            int strideH, int strideW, int R, int S, int gH, int gW,
                            int32_t *table, void *stream);
int sige_hip_scatter_fused_f32(const float *x, const float *y, int B, int C, int H, int W, int R, int S,
                               const int32_t *table, int gH, int gW, int N,
                               const float *residual, int resB, int resC, int resH, int resW,
                               float *out, void *stream);
int sige_hip_scatter_with_block_residual_fused_f32(
        const float *x0, const float *y0, const float *x1, const float *y1,
        int B, int C, int H, int W, int R0, int S0, int R1, int S1,
        const int32_t *table0, int gH0, int gW0, int N0,
        const int32_t *table1, int gH1, int gW1, int N1,
        float *out, void *stream);

/* ---- get_scatter_map : replaces get_scatter_map_cpu / _cuda ---------------
 * (sige/cpu/scatter_gather.cpp:150-170, scatter_gather_kernel.cu:160-188,
 *  scatter_gather.h:16-22).  map int32 [H,W,3] = (tile, r, s) or -1 triples.  */
int sige_hip_scatter_map_i32(int H, int W, int bH, int bW, int kH, int kW,
                             int offsetH, int offsetW, int strideH, int strideW,
                             const int32_t *active_indices, int N, int32_t *map, void *stream);

/* ---- scatter_gather : replaces scatter_gather_cpu / _cuda -----------------
 * (sige/cpu/scatter_gather.cpp:86-148, scatter_gather_kernel.cu:100-158,
 *  scatter_gather.h:5-14).  x [B*N,C,Rx,Sx] conv-1 output tiles, y [B,C,H,W]
 * cached full tensor -> out [B*N,C,bH,bW] (input tiles of the next conv).    */
int sige_hip_scatter_gather_f32(const float *x, const float *y, int B, int C, int H, int W,
                                int Rx, int Sx, int bH, int bW,
                                const int32_t *active_indices, int N, const int32_t *scatter_map,
                                const float *scale, int scaleB, int scaleC, int scaleH, int scaleW,
                                const float *shift, int shiftB, int shiftC, int shiftH, int shiftW,
                                int activation, int activation_first, float *out, void *stream);

/* ---- mask pipeline : replaces sige.utils.compute_difference_mask / dilate_mask /
 * downsample_mask (sige/utils.py:74-85, 40-71, 88-118) for masks that live on the GPU,
 * without the reference's device -> host synchronisation per pyramid level
 * (`min(threshold, level.max() - eps)`, utils.py:107).  All masks are bytes (0 / 1),
 * row-major [H,W].
 *   difference_mask  out[h,w] = any_c |a[c,h,w] - b[c,h,w]| > eps; a / b addressed through
 *                    element strides (NCHW or channels-last; strideH must equal W*strideW)
 *   dilate_mask      OR of the ORIGINAL mask shifted by 1..dilationH rows and 1..dilationW
 *                    columns (a plus-shaped element, utils.py:57-61); out != mask
 *   mask_pyramid     every level of downsample_mask in ONE launch: level 0 = mask, level k+1 =
 *                    bilinear (align_corners=False) halving of the FLOAT level k; each level
 *                    is thresholded at min(threshold, max(level) - eps) and dilated; levels
 *                    are written back to back into `out` (sizes: sige_hip_mask_pyramid_levels,
 *                    which mirrors the loop `h//=2; w//=2; stop when h<min_h and w<min_w`).
 *                    scratch_floats >= (H/2)*(W/2) + (H/4)*(W/4) + (H*W+3)/4 + 8.          */
int sige_hip_difference_mask_u8(const float *a, const float *b, int C, int H, int W,
                                int64_t strideC, int64_t strideH, int64_t strideW, float eps,
                                uint8_t *out, void *stream);
int sige_hip_dilate_mask_u8(const uint8_t *mask, int H, int W, int dilationH, int dilationW,
                            uint8_t *out, void *stream);
int sige_hip_mask_pyramid_levels(int H, int W, int min_h, int min_w, int *hs, int *ws, int capacity);
int sige_hip_mask_pyramid_u8(const uint8_t *mask, int H, int W, int min_h, int min_w,
                             int dilationH, int dilationW, float threshold, float eps,
                             float *scratch, size_t scratch_floats, uint8_t *out, void *stream);

/* ---- reduce_mask : replaces sige.utils.reduce_mask ------------------------
 * (sige/utils.py:8-37: F.pad -> F.max_pool2d -> nonzero -> stride*i - pad).
 * mask: H*W bytes (non-zero = edited).  Writes up to `capacity` (h,w) pairs in
 * row-major order of the candidate grid to `indices` and the TOTAL number of
 * active tiles to *count (device int32).  The candidate grid is
 * ((H+padH)/strH+1) x ((W+padW)/strW+1); sige_hip_reduce_mask_capacity returns
 * its size.                                                                  */
int sige_hip_reduce_mask_capacity(int H, int W, int strideH, int strideW, int padH, int padW);
int sige_hip_reduce_mask_i32(const uint8_t *mask, int H, int W, int bH, int bW,
                             int strideH, int strideW, int padH, int padW,
                             int32_t *indices, int capacity, int32_t *count, void *stream);

/* ---- demand regions of a dense stage in front of a tiled consumer (not in the reference) ----
 * A dense [Hp,Wp] stage whose output is read ONLY through the (bH x bW) windows of a Gather needs it on N0 = the pixels under
 * those windows; `indices` / `*count` (device int32, at most `capacity` rows used) are the consumer's reduce_mask list over
 * its [inH,inW] input, which is the stage's output itself (upsample2x = 0) or its nearest x2 upsampling (1: inH = 2 Hp).  The
 * 3x3 conv k layers before the output is needed on N0 dilated k times by one pixel (3x3 box, clamped to the image).  For
 * k = 0 .. depth-1 the launch writes the (tileH x tileW) output cells that intersect that set, row-major, as index lists in
 * reduce_mask form: lists[k] = cell origin - (padH, padW) (the 3x3 geometry), lists[depth + k] = cell origin (the 1x1
 * geometry), each int32 [cells,2] with cells = sige_hip_demand_tiles_capacity(...), and counts[k] (device int32) = how many.
 * One workgroup, no host synchronisation; Hp*Wp <= 16384 and cells <= 4096, SIGE_HIP_EUNSUPPORTED beyond (and with stacked
 * edits). */
int sige_hip_demand_tiles_capacity(int Hp, int Wp, int tileH, int tileW);
int sige_hip_demand_tiles_i32(const int32_t *indices, const int32_t *count, int capacity, int bH, int bW,
                              int inH, int inW, int upsample2x, int Hp, int Wp, int tileH, int tileW,
                              int padH, int padW, int depth, int32_t *lists, int32_t *counts, void *stream);

/* ---- change regions of a dense stage behind a tiled producer (not in the reference) ----
 * A dense [Hp,Wp] stage on cached GroupNorm affines is a chain of local operators, and its input -- the persistent output of
 * a tiled layer -- equals the original's outside S0 = the (outH x outW) output tiles that layer's Scatter writes: `indices` /
 * `*count` (device int32, at most `capacity` rows used) are its reduce_mask list for (bH x bW) blocks, tile origin =
 * (index + offset) / stride.  The output of the stage's k-th 3x3 conv can differ from the original's only on S_k = S0 dilated
 * k times by one pixel (3x3 box, clamped to the image).  For k = 1 .. depth the launch writes the (tileH x tileW) output
 * cells that intersect S_k, row-major, as index lists in reduce_mask form: lists[k-1] = cell origin - (padH, padW) (the 3x3
 * geometry), lists[depth + k-1] = cell origin (the 1x1 geometry), each int32 [cells,2] with cells =
 * sige_hip_demand_tiles_capacity(Hp, Wp, tileH, tileW), and counts[k-1] (device int32) = how many.  One workgroup, no host
 * synchronisation; limits as for sige_hip_demand_tiles_i32. */
int sige_hip_change_tiles_i32(const int32_t *indices, const int32_t *count, int capacity, int bH, int bW,
                              int strideH, int strideW, int offsetH, int offsetW, int outH, int outW,
                              int Hp, int Wp, int tileH, int tileW, int padH, int padW, int depth,
                              int32_t *lists, int32_t *counts, void *stream);

/* ---- stacked-block convolution : replaces the F.conv2d call of
 * SIGEConv2d.forward in sparse mode (sige/nn/base.py:88-89) ----------------
 * x [T,Cin,R,S] (*) w [Cout,Cin/groups,kH,kW] + bias -> out [T,Cout,Ro,So],
 * padding 0, dilation 1, Ro=(R-kH)/strH+1.
 * The MFMA path (fp32-in/fp32-acc v_mfma_f32_32x32x2_f32 / 16x16x4_f32, exact
 * fp32 products; the library picks the tile by grid size) needs the weights
 * re-laid once per weight tensor (both tile layouts, back to back):
 *   n = sige_hip_block_conv_packed_size(...)   floats to allocate (0 = this shape
 *                                              has no MFMA path; use _direct)
 *   sige_hip_block_conv_pack_f32(w, ..., packed)
 *   sige_hip_block_conv_f32(x, ..., packed, bias, ..., out)
 * sige_hip_block_conv_direct_f32 is the any-shape (groups, odd tiles, dilation:
 * Ro=(R-(kH-1)*dilationH-1)/strH+1) vector FMA kernel reading the original
 * weight layout.                                                              */
size_t sige_hip_block_conv_packed_size(int Cout, int Cin, int kH, int kW, int R, int S,
                                       int strideH, int strideW, int groups);
int sige_hip_block_conv_pack_f32(const float *w, int Cout, int Cin, int kH, int kW,
                                 float *packed, void *stream);
int sige_hip_block_conv_f32(const float *x, int T, int Cin, int R, int S,
                            const float *packed, const float *bias, int Cout, int kH, int kW,
                            int strideH, int strideW, float *out, void *stream);
int sige_hip_block_conv_direct_f32(const float *x, int T, int Cin, int R, int S,
                                   const float *w, const float *bias, int Cout, int kH, int kW,
                                   int strideH, int strideW, int dilationH, int dilationW, int groups,
                                   float *out, void *stream);
/* ---- SPADE modulation of tiles (GauGAN; gaugan/models/sige_normalization.py:62-88) --------
 * out[B*N,bH,bW,C] = leaky(normalized * (1 + gamma) + beta), channels-last, one pass:
 *   normalized = scale*X + shift with X = x_full [B,H,W,C] at the tile's pixels (x_tiles == NULL:
 *                Gather) or, through map_x, the conv tiles x_tiles [B*Nx,Rx,Sx,C] where one covers
 *                the pixel and the cache x_full elsewhere (ScatterGather);
 *   gamma|beta = gb_tiles [B*Ng,Rg,Sg,2C] / gb_full [B,H,W,2C] through map_g the same way.
 * Pixels outside the image give 0 (as Gather / ScatterGather zero-fill both operands).  leaky != 0
 * applies x > 0 ? x : slope*x.  Same fp32 operations, in the same order, as the module chain
 * Gather | ScatterGather, ScatterGather, split, 1 + gamma, *, + beta, leaky_relu.            */
int sige_hip_spade_modulate_nhwc_f32(
        const float *x_full, const float *x_tiles, const int32_t *map_x, int Nx, int Rx, int Sx,
        const float *scale, int scaleB, int scaleC, const float *shift, int shiftB, int shiftC,
        const float *gb_tiles, const float *gb_full, const int32_t *map_g, int Ng, int Rg, int Sg,
        int B, int C, int H, int W, int bH, int bW, const int32_t *active_indices, int N,
        int leaky, float slope, float *out, void *stream);

/* ---- f16 compute (compute = 1): the same stacked-block convs on the fp16 matrix cores ---------
 * (v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x32_f16, 16x the rate of the f32-input forms).
 * Tensors stay fp32 in HBM (x, y, residual, out, bias, scale / shift): the staging path
 * finishes a value in fp32 (cached GroupNorm affine + SiLU), rounds it to fp16 (RNE) into LDS;
 * weights are packed as fp16 by sige_hip_block_conv_pack_f16c (same fp32 weight tensor in);
 * products are exact and accumulate in fp32.  Not in the reference, which is fp32-only
 * (sige/nn/base.py:15,55-63): BASELINE.json configs[4]; parity vs the fp32 oracle is quoted at
 * 2e-2 abs.  Channels-last entry points only; geometries: 3x3/s1 on 6x6 and
 * 1x1 on 4x4 (packed_size_f16c returns 0 for the stride-2 geometry: pack that conv for fp32).
 * `packed` sizes are in 4-byte units as for the fp32 forms; the convs themselves are the
 * channels-last entry points further down, called with compute = 1.                      */
size_t sige_hip_block_conv_packed_size_f16c(int Cout, int Cin, int kH, int kW, int R, int S,
                                            int strideH, int strideW, int groups);
int sige_hip_block_conv_pack_f16c(const float *w, int Cout, int Cin, int kH, int kW,
                                  float *packed, void *stream);

/* Horizontal fusion of the two independent convs at the head of a residual block.  After pair_begin() the next
 * channels-last fp32 1x1 gather -> conv launch with raw staging (the block's shortcut) is HELD: the call returns
 * SIGE_HIP_OK without launching.  The next channels-last fp32 3x3/s1 gather -> conv launch with affine + SiLU staging on
 * the same stream and with the same destination kind (the block's conv1) then runs both in ONE kernel (workgroups of
 * both convs side by side; the 1x1's own ~5 us launch disappears).  Any other conv launch, and pair_end(), launch the held
 * conv on its own first, so results never depend on whether a pair was formed.  Per host thread; the pointers of the
 * held call must stay valid until it has been launched.  pairs_fused(): how many pairs this process has formed (atomic). */
int sige_hip_conv_pair_begin(void);
int sige_hip_conv_pair_end(void);
int64_t sige_hip_conv_pairs_fused(void);
/* Deferred "side" convs: independent work computed on the CUs that later, small launches leave idle.  After
 * side_begin(budget > 0) the NEXT sige_hip_gather_conv_nhwc call of this thread, if it is eligible -- compute 0, 3x3 / stride 1,
 * raw staging, a full-tensor destination, no twins, and a grid that a launch of its own would not K-split -- is planned
 * (16-pixel output blocks) and QUEUED: the call returns SIGE_HIP_OK without launching.  A call that is not eligible launches
 * as ever; either way side_begin is spent on that one call (it never waits for a later, unrelated conv).  Every later eligible HOST launch on the
 * same stream -- a single exact-fp32 3x3 / stride 1 gather -> conv launch into a full tensor with 16 x 16 output blocks, 4
 * waves, no K split and no held shortcut -- runs min(remaining, budget, 256 - its own grid) blocks of the queue's head in the
 * same kernel.  A block computes exactly what it would in a launch of its own: results do not depend on the slicing.
 * side_flush() launches whatever is left, first queued first, one launch per conv, and disarms a side_begin whose call has
 * not come.  Other launches leave the queue alone, except that a conv launch on another stream, or one whose operands overlap
 * a queued conv's (it reads the queued output, or writes a queued input), flushes the queue first; everything else is the
 * caller's to order: the operands of a queued conv must stay valid and unchanged until it is hosted or flushed, and nothing
 * may read its output before side_flush().  Per host thread.  side_workgroups(0 | 1): side workgroups hosted | flushed so far
 * in this process (atomic; a measurement aid). */
int sige_hip_conv_side_begin(int max_side_workgroups_per_host);
int sige_hip_conv_side_flush(void);
int64_t sige_hip_conv_side_workgroups(int flushed);
/* A K-split launch is finished inside the launch: the last workgroup to finish an output block adds the partial copies of
 * that block up in split order and runs the epilogue (tickets in a library-owned, per-device buffer); when no tickets are to
 * be had, by a second launch over the whole output.  Both add in the same order: identical results. */
/* Tickets of launches made while a stream is being CAPTURED into a hipGraph are bump-allocated (a replayed graph owns its
 * tickets for its lifetime) out of 3 M per device; when they run out, captured K-split launches fall back to the second-pass
 * finish (still correct, one more launch).  A long-running host that re-captures per mask calls this once every hipGraph
 * captured so far on the CURRENT device has been destroyed: the region is handed out again from the start. */
int sige_hip_release_graph_tickets(void);

/* ---- fused gather -> conv and scatter_gather -> conv ------------------------
 * The same MFMA conv with the producer of its input tiles fused into the
 * prologue: the [B*N,Cin,bH,bW] tile tensor of gather (sige/cpu/gather.cpp:4-58)
 * resp. scatter_gather (sige/cpu/scatter_gather.cpp:5-56) is staged straight
 * into LDS and never written to HBM.  Equivalent to
 *     sige_hip_gather_f32(...)          ; sige_hip_block_conv_f32(...)
 *     sige_hip_scatter_gather_f32(...)  ; sige_hip_block_conv_f32(...)
 * for activation_first = 0 and a per-(batch,channel) affine (scale/shift dims
 * [1|B, 1|C, 1, 1], which is what every caller in the reference passes:
 * sige_fused_unet.py:111,118-120); anything else -> SIGE_HIP_EUNSUPPORTED and
 * the caller uses the two-call form.  out [B*N,Cout,Ro,So].                   */
int sige_hip_gather_conv_f32(const float *x, int B, int Cin, int H, int W, int bH, int bW,
                             const int32_t *active_indices, int N,
                             const float *scale, int scaleB, int scaleC, int scaleH, int scaleW,
                             const float *shift, int shiftB, int shiftC, int shiftH, int shiftW,
                             int activation,
                             const float *packed, const float *bias, int Cout, int kH, int kW,
                             int strideH, int strideW, float *out, void *stream);
int sige_hip_scatter_gather_conv_f32(const float *x, const float *y, int B, int Cin, int H, int W,
                                     int Rx, int Sx, int bH, int bW,
                                     const int32_t *active_indices, int N, const int32_t *scatter_map,
                                     const float *scale, int scaleB, int scaleC, int scaleH, int scaleW,
                                     const float *shift, int shiftB, int shiftC, int shiftH, int shiftW,
                                     int activation,
                                     const float *packed, const float *bias, int Cout, int kH, int kW,
                                     int strideH, int strideW, float *out, void *stream);

/* ---- dense layers through the same kernel ("all tiles active") ---------------
 * the U-Net's low-resolution dense blocks in sparse mode
 * (sige_fused_unet.py:112-114,121-123: h*scale+shift -> swish -> nn.Conv2d ->
 * + skip) as ONE launch: gather-conv whose input channels may come from two
 * tensors (x [B,C1,H,W] and x2 [B,C2,H,W]: a fused torch.cat), whose output
 * tiles are written straight into out [B,Cout,Ho,Wo] at (offset+idx)/stride
 * (clipped) plus an optional residual [B,Cout,Ho,Wo].  With the index list of
 * ALL tiles this is a dense conv with padding = offset.  scale/shift: [1|B, 1|Cin]. */
int sige_hip_gather_conv_nchw_f32(const float *x, const float *x2, int B, int C1, int C2, int H, int W,
                                  int bH, int bW, const int32_t *active_indices, int N,
                                  const float *scale, int scaleB, int scaleC,
                                  const float *shift, int shiftB, int shiftC,
                                  int activation,
                                  const float *packed, const float *bias, int Cout, int kH, int kW,
                                  int strideH, int strideW, int offsetH, int offsetW,
                                  const float *residual, int Ho, int Wo, float *out, void *stream);

/* ---- channels-last (NHWC) forms of the fused convolutions ----------------------
 * Same arithmetic, tensors laid out [B,H,W,C] (torch.channels_last) and tiles
 * [T,R,S,C].  In the reference's NCHW layout a gathered 6x6 window is 6 separate
 * 24-byte segments per channel; with the channels contiguous every staging load is a
 * coalesced 16 bytes per lane.  Requirements: channel counts
 * multiples of 4, 16-byte aligned pointers; scale/shift [1|B, 1|C] as above.
 * One entry point per operation; arithmetic, cache storage and routing are arguments:
 *   `compute`   0 exact fp32 | 1 fp16 operands | 2 split fp16 operands -- the arithmetic, and with it which of
 *               sige_hip_block_conv_pack_f32 / _f16c / _f16x3 made `packed`; anything else: SIGE_HIP_EINVAL
 *   `y_f16`, `residual_f16`   the cached tensor `y` / the cached shortcut tensor `residual` (const void *) holds halves --
 *               the fp16-STORED caches described further down -- instead of floats; independent of `compute`
 *   `packed_tile3`, `min_blocks`   the same weights in the tile conv v3 layout and the routing threshold (below)
 *   sige_hip_block_conv_nhwc            x [T,R,S,Cin]              -> out [T,Ro,So,Cout]
 *   sige_hip_gather_conv_nhwc           x [B,H,W,C1] (+ x2 [1,H,W,C2]: a fused cat)
 *        to_full = 0 -> out [B*N,Ro,So,Cout];  to_full = 1 -> out [B,Ho,Wo,Cout] written at
 *        (offset+idx)/stride, clipped, + residual [B,Ho,Wo,Cout] (dense layers)
 *   sige_hip_scatter_gather_conv_nhwc   x [B*N,Rx,Sx,Cin] tiles, y [B,H,W,Cin] -> out [B*N,Ro,So,Cout]; y_f16: 3x3 / stride 1 only */
int sige_hip_block_conv_nhwc(int compute, const float *x, int T, int Cin, int R, int S,
                             const float *packed, const float *bias, int Cout, int kH, int kW,
                             int strideH, int strideW, float *out, void *stream);
/* ... over the tiles of an index list, T = B * N: `count_key` is that list's pointer (not read); a launch plan looks N up under
 * it, so a conv over a tile SLAB follows a new mask like the gather-type entry points do (a plan that records the plain entry
 * point above only replays under the tile counts it was recorded with). */
int sige_hip_block_conv_nhwc_keyed(int compute, const float *x, const int32_t *count_key, int B, int N, int Cin, int R, int S,
                                   const float *packed, const float *bias, int Cout, int kH, int kW,
                                   int strideH, int strideW, float *out, void *stream);
/* Routing: `packed_tile3` (may be NULL) = the weights in the tile conv v3 layout -- sige_hip_wide_conv_pack(prec = 2) for compute 0,
 * (prec = 0) for compute 1.  A launch whose v3 grid (tile pairs x 64-channel output blocks) has >= min_blocks workgroups -- and
 * that is not about to share its launch with a held 1x1 shortcut (sige_hip_conv_pair_begin) -- runs on the v3 kernel (below);
 * every other launch on the stacked-block kernels.  The decision is taken HERE, from N, so that a launch plan (which replays the
 * recorded entry point with the new mask's count) routes like the module-level forward under that mask: the two stay
 * bit-identical.  min_blocks <= 0 or packed_tile3 == NULL: never; compute 2 ignores both, and so does compute 0 over an
 * fp16-stored `y` / `residual` (the exact-fp32 v3 kernel reads fp32 caches only). */
int sige_hip_gather_conv_nhwc(int compute, const float *x, const float *x2, int B, int C1, int C2, int H, int W,
                              int bH, int bW, const int32_t *active_indices, int N,
                              const float *scale, int scaleB, int scaleC,
                              const float *shift, int shiftB, int shiftC,
                              int activation,
                              const float *packed, const float *bias, int Cout, int kH, int kW,
                              int strideH, int strideW,
                              int to_full, int offsetH, int offsetW, const float *residual, int Ho, int Wo,
                              float *workspace, size_t workspace_floats,
                              const float *out_scale, const float *out_shift, int out_activation,
                              int upsample2x,
                              float *twin0, const float *twin0_scale, const float *twin0_shift,
                              float *twin1, const float *twin1_scale, const float *twin1_shift,
                              const float *packed_tile3, int min_blocks,
                              float *out, void *stream);
/* `out_scale` / `out_shift` ([Cout], optional): epilogue out = act(out_scale * (conv + bias + residual) + out_shift)
 * -- the CONSUMER's cached GroupNorm affine + SiLU applied by the producer, once per element; the consumer then
 * gathers with no affine (e.g. conv1 -> conv2 of a ResBlock, sige_fused_unet.py:112-125).
 * `upsample2x` = 1: x / x2 are [B,H/2,W/2,C] and the gather reads pixel (h/2, w/2): the x2 nearest-neighbour
 * upsampling in front of the U-Net's Upsample conv (sige_fused_unet.py: F.interpolate) fused into the gather.
 * `upsample2x` = 2: the same conv (3x3, stride 1, 6x6 tiles, to_full) as four 2x2 "phase" convs on the half-resolution
 * tensor: the 3x3 window of upsampled pixel (2y + a, 2x + b) covers 2x2 source pixels, rows {y - 1 + a, y + a}, columns
 * likewise with b, so 4 multiply-adds per output and channel pair instead of 9.  `packed` is then the phase pack directly
 * followed by the 9-tap pack of the same weights:
 *   n = sige_hip_upsample_phase_packed_size(Cout, Cin)         floats of the phase pack
 *   sige_hip_upsample_phase_pack_f32(w_phases, ..., packed)     w_phases [4,Cout,Cin,2,2], phase 2a + b: the tap sums
 *   sige_hip_block_conv_pack_f32(w, ..., packed + n)            the 9-tap pack (launches the library routes away from the
 *                                                              phase form by their tile count run on it, or on packed_tile3)
 * Exact fp32 (compute 0), one input tensor, no gather affine; bias, residual, out_scale / out_shift and twins as in the
 * 9-tap form.  Anything else (and stacked edits, and a call that sige_hip_conv_side_begin waits for) is
 * SIGE_HIP_EUNSUPPORTED: repeat the call with upsample2x = 1 and the 9-tap pack. */
size_t sige_hip_upsample_phase_packed_size(int Cout, int Cin);
int sige_hip_upsample_phase_pack_f32(const float *w_phases, int Cout, int Cin, float *packed, void *stream);
/* `workspace` (optional, NULL = none): room for up to 8 copies of the output.  When the conv has
 * too few tiles to cover the chip with ANY block shape (the 8x8 layers: 64 pixels, K up to 9216),
 * the channel chunks are split across workgroups that write partial sums there, and a second
 * launch adds them in a fixed order with bias / residual (deterministic; no atomics).
 * sige_hip_conv_ksplit_hint: how many copies such a call would use (1 = no split). */
int sige_hip_conv_ksplit_hint(int T, int Cin, int Cout, int kH, int kW, int strideH, int strideW);
int sige_hip_scatter_gather_conv_nhwc(int compute, const float *x, const void *y, int y_f16, int B, int Cin, int H, int W,
                                      int Rx, int Sx, int bH, int bW,
                                      const int32_t *active_indices, int N, const int32_t *scatter_map,
                                      const float *scale, int scaleB, int scaleC,
                                      const float *shift, int shiftB, int shiftC,
                                      int activation,
                                      const float *packed, const float *bias, int Cout, int kH, int kW,
                                      int strideH, int strideW, float *out, void *stream);

/* conv2 -> Scatter / ScatterWithBlockResidual fused (in-place scatter mode): the scatter_gather-fed 3x3 conv writes
 * out[b, (offset+idx)/1 + r, ..., :] = conv + bias + residual  straight into `out` [B,H,W,Cout], a buffer that already
 * equals the cached tensor outside this mask's tiles.  x1 != NULL: block residual -- `residual` is the cached shortcut
 * tensor y1 and out += x1 - y1 wherever a shortcut tile (table1 over R1 x S1 cells, tiles x1 [B*N1,R1,S1,Cout]) covers
 * the pixel (scatter.cpp:41-68).  The shortcut tiles must lie inside the main tiles (true for index lists that
 * reduce_mask derives from one mask: a 4x4 block hit by the mask is inside an active 6x6 window). */
int sige_hip_scatter_gather_conv_scatter_nhwc(
        int compute, const float *x, const void *y, int y_f16, int B, int Cin, int H, int W, int Rx, int Sx, int bH, int bW,
        const int32_t *active_indices, int N, const int32_t *scatter_map,
        const float *scale, int scaleB, int scaleC, const float *shift, int shiftB, int shiftC, int activation,
        const float *packed, const float *bias, int Cout, int kH, int kW,
        int offsetH, int offsetW, const void *residual, int residual_f16,
        const float *x1, const int32_t *table1, int gH1, int gW1, int N1, int R1, int S1,
        float *twin0, const float *twin0_scale, const float *twin0_shift,
        float *twin1, const float *twin1_scale, const float *twin1_shift,
        const float *packed_tile3, int min_blocks,
        float *out, void *stream);

/* ---- channels-last forms of gather / scatter_gather / scatter ------------------
 * (materialising forms: the tiles are written to HBM; the fused convs above do not
 * need them).  scale / shift: [1|B, C].  Results are bit-identical to the NCHW
 * entry points on the same values.
 *   sige_hip_scatter_nhwc_f32 / sige_hip_scatter_with_block_residual_nhwc_f32:
 *     in_place = 0  reference semantics: `out` [B,H,W,C] is a fresh tensor, written in
 *                   ONE pass (cached tensor outside the tiles, tiles + residual inside);
 *     in_place = 1  `out` is a buffer that already holds the cached tensor y outside
 *                   the tiles of this mask (kept by the caller across calls): only the
 *                   covered pixels are written -- traffic ~ active tiles, not B*H*W*C.
 *   `table` / gH / gW: the tile table of sige_hip_tile_table_i32.                 */
int sige_hip_gather_nhwc_f32(const float *x, int B, int C, int H, int W, int bH, int bW,
                             const int32_t *active_indices, int N,
                             const float *scale, int scaleB, int scaleC,
                             const float *shift, int shiftB, int shiftC,
                             int activation, float *out, void *stream);
int sige_hip_scatter_gather_nhwc_f32(const float *x, const float *y, int B, int C, int H, int W,
                                     int Rx, int Sx, int bH, int bW,
                                     const int32_t *active_indices, int N, const int32_t *scatter_map,
                                     const float *scale, int scaleB, int scaleC,
                                     const float *shift, int shiftB, int shiftC,
                                     int activation, float *out, void *stream);
int sige_hip_scatter_nhwc_f32(const float *x, const float *y, int B, int C, int H, int W, int R, int S,
                              int offsetH, int offsetW, int strideH, int strideW,
                              const int32_t *active_indices, const int32_t *table, int gH, int gW, int N,
                              const float *residual, int in_place, float *out, void *stream);
int sige_hip_scatter_with_block_residual_nhwc_f32(
        const float *x0, const float *y0, const float *x1, const float *y1,
        int B, int C, int H, int W, int R0, int S0, int R1, int S1,
        int offsetH, int offsetW, int strideH, int strideW,
        const int32_t *active_indices0, const int32_t *table0, int gH0, int gW0, int N0,
        const int32_t *active_indices1, const int32_t *table1, int gH1, int gW1, int N1,
        int in_place, float *out, void *stream);

/* ---- committing an edit: the tiles of MANY cached tensors copied in one launch (csrc/commit_tiles.hip) ------------------------
 * The reference accepts an edit by running the sparse forward with `sparse_update` set: every Scatter / ScatterGather then writes
 * its result back into its cache (sige/nn/scatter.py:59-60,114-129, scatter_gather.py:65-77), a whole-tensor copy each.  Here the
 * bytes that differ are the active tiles, and one launch executes a LIST of records, each of which says
 *   over the tile list idx [N,2] (int32, row origin first, as sige_hip_reduce_mask_i32 gives it), write the pixels
 *   (offset + idx) / stride + [0,r) x [0,s) of the channels-last destination dst [1,H,W,C] -- C division, clipped at the bottom
 *   and right border (and never above or left of the image), exactly the pixels sige/cpu/scatter.cpp writes -- from
 *     a FULL source (tile_source = 0): src is fp32 [1,H,W,C]; pixel (h,w) comes from pixel (h,w)  (a persistent Scatter output);
 *     a TILE source (tile_source = 1): src is fp32 [N,r,s,C], the layout the tile convs write; pixel (i,j) of tile n goes to
 *                                      (origin_n + (i,j))  (the reference's scatter without a residual).
 *   scale / shift [C] (both or neither): the value written is SiLU(scale[c] * v + shift[c]) -- two separately rounded operations
 *   and the SiLU of sige_hip_affine_act_nhwc_f32, bit for bit (the activated copy of a ScatterGather cache).
 *   dst_f16 != 0: dst holds halves; the value is rounded to nearest even as sige_hip_convert_f32_f16 rounds it.
 * The records are copied BY VALUE into the kernel arguments: no host-to-device copy, no memory of the caller is read after the call
 * returns, and the launches can be captured.  SIGE_HIP_COMMIT_CAPACITY records fit one launch (the argument block is
 * 8 + 76 * capacity = 3656 of the 4096 bytes a kernel may take); records with N == 0 are dropped first (idx may then be NULL), the
 * rest run in ceil(n_nonempty / capacity) launches, in list order.  *launches (may be NULL) receives that number.
 * Ordering: two tiles of ONE record that cover the same pixel are written in no defined order.  A full source writes the same
 * value twice; for a tile source the reference lets the later tile win, but the lists sige_hip_reduce_mask_i32 builds do not
 * overlap in output space, so the kernel has no ordering machinery.  Records of one call that write the same pixel of the same
 * destination must write the same value (a ScatterWithBlockResidual's output over its main and its shortcut list).
 * src and dst of a record must not overlap.
 * Status, decided for the WHOLE list before anything is launched: SIGE_HIP_EINVAL: n < 0, a null list with n > 0, negative N,
 * non-positive B / C / H / W / r / s / stride, a null src / dst / idx with N > 0, one of scale / shift without the other.
 * SIGE_HIP_EUNSUPPORTED (no kernel for this shape; nothing is written): B != 1, C % 4, C > 16384, r or s > 16, a stride that
 * is no power of two <= 128, |offset| > 127, H * W >= 2^31, more than 2^22 (tile, 64-channel chunk) units in one launch, src /
 * scale / shift / an fp32 dst not 16-byte aligned, an fp16 dst not 8-byte aligned, stacked edits (sige_hip_set_edit_batch > 1:
 * E edits of one original cannot all become the original). */
#define SIGE_HIP_COMMIT_CAPACITY 48
typedef struct sige_hip_commit_record {
    const float *src;
    void *dst;
    const int32_t *idx;
    const float *scale, *shift;
    int N, B, C, H, W;
    int r, s, offsetH, offsetW, strideH, strideW;
    int tile_source, dst_f16;
} sige_hip_commit_record;
int sige_hip_commit_tiles(const sige_hip_commit_record *records, int n, int *launches, void *stream);

/* ---- residual blocks that resample INSIDE the block (Progressive Distillation U-Net), on the active tiles, in ONE launch ----
 * x [B,H,W,C] channels-last; the resampled resolution Ho x Wo is H/2 x W/2 (mode DOWN: 2x2 mean) or 2H x 2W (mode UP:
 * nearest x2); active_indices [N,2]: tile origins AT THE RESAMPLED RESOLUTION, as sige_hip_reduce_mask_i32 gives them.
 *   tiles (DOWN only, or NULL)  [B*N,bH,bW,C] in the layout of sige_hip_gather_nhwc_f32: the mean over the 2x2 source pixels of
 *                               SiLU(scale[c] * x + shift[c]) (scale, shift [C], both or neither; neither = raw pooling) at the
 *                               pooled position origin + (r, s); exactly 0 outside the pooled image -- zero padding is never
 *                               transformed.  What conv1 of the block consumes as plain, pre-activated tiles.
 *   res (or NULL)               [B,Ho,Wo,C], persistent: the resampled RAW x (the block's shortcut), written on the cells
 *                               (offset + origin) / stride + [0,rH) x [0,rW), clipped -- the cells the fused conv -> scatter
 *                               epilogue writes for these tiles.  Every other cell is left as it was.
 *   active_indices == NULL (N = 0, tiles NULL): every cell of res -- the dense levels.
 * SIGE_HIP_EINVAL: null x with work to do, non-positive dims, a tile count without a list.  SIGE_HIP_EUNSUPPORTED: C % 4,
 * odd H or W in DOWN, tiles in UP (the fused gather reads the half-resolution tensor: upsample2x), one of scale / shift
 * alone, a scatter stride other than 1, pointers not 16-byte aligned, B * N or the rows of a launch > 65535.  B * N == 0:
 * SIGE_HIP_OK, nothing launched (answered before the checks below).
 * Stacked edits (sige_hip_set_edit_batch(E)): x is the tall image [B,E*hp,W,C], the list holds the tiles of all E edits at the
 * resampled resolution.  A tile belongs to the image its window's third row lies in (the rule of sige_hip_reduce_mask_i32 and
 * of the conv staging): a window row of `tiles` beyond that image is exactly 0, never the neighbour's pooled pixels, and the
 * rows of its `res` cells are clipped to that image.  The forms without a list need no seam (an even hp).
 * SIGE_HIP_EUNSUPPORTED: E does not divide H, hp is not a power of two or < 4; a list in DOWN with hp < 8. */
enum { SIGE_HIP_RESAMPLE_DOWN = 0, SIGE_HIP_RESAMPLE_UP = 1 };
int sige_hip_resample_tiles_nhwc_f32(const float *x, int B, int C, int H, int W, int mode,
                                     const int32_t *active_indices, int N, int bH, int bW,
                                     const float *scale, const float *shift, float *tiles,
                                     int offsetH, int offsetW, int strideH, int strideW, int rH, int rW,
                                     float *res, void *stream);

/* ---- tile conv v3(csrc/conv_tile3.hpp): the 3x3 / stride-1 stacked-block conv over 6x6 tiles with the dense-layer kernel's
 * K loop -- wave-private stages (no workgroup barrier per channel chunk), 64 output channels per workgroup -- for grids that
 * fill the chip (large edits, stacked edits).  What sige_hip_gather_conv_nhwc (source 1) and
 * sige_hip_scatter_gather_conv_scatter_nhwc (source 2) route to on those grids, and the kernel's own entry point:
 *   source 1: tiles of x [B,H>>up,W>>up,C1] (+ x2 [.., C2]: a fused torch.cat) at active_indices, zero padded, optional cached
 *             affine [affineB in {1,B}, C1+C2] + SiLU;   source 2: x = conv tiles [B*N,Rx,Sx,C1], x2 = the cached tensor
 *             [B,H,W,C1] through scatter_map (raw);
 *   to_full 0: out = tiles [B*N,4,4,Cout];  1: straight into out [B,Ho,Wo,Cout] at offset + origin, clipped, + residual, with x1 /
 *             table1: + (x1 - residual) where a shortcut tile covers the pixel (ScatterWithBlockResidual), twins, out-affine.
 * compute 0: exact fp32 (v_mfma_f32_32x32x2_f32), `packed` = sige_hip_wide_conv_pack(prec = 2) of the [Cout, C1+C2, 3, 3] weight,
 *   fp32-stored tensors only (y_f16 / residual_f16 != 0: SIGE_HIP_EUNSUPPORTED);
 * compute 1 (round 6; BASELINE.json configs[4]): fp16 operands, `packed` = sige_hip_wide_conv_pack(prec = 0); activations fp32 in
 *   HBM, rounded to fp16 (RNE) in the staging path, products exact, accumulation fp32 (v_mfma_f32_32x32x16_f16).  y_f16: the cached
 *   tensor of source 2 (x2) holds halves; residual_f16: `residual` holds halves -- the fp16-stored caches;
 * compute 2: SIGE_HIP_EUNSUPPORTED (no split-fp16 form).  C1, C2, Cout multiples of 64. */
int sige_hip_tile_conv3_supported(int C1, int C2, int Cout);
int sige_hip_tile_conv3_nhwc(
        int compute, int source, const float *x, const void *x2, int y_f16, int B, int C1, int C2, int H, int W, int upsample2x,
        const int32_t *active_indices, int N, const int32_t *scatter_map, int Rx, int Sx,
        const float *scale, const float *shift, int affineB, int activation,
        const float *packed, const float *bias, int Cout,
        int to_full, int offsetH, int offsetW, int Ho, int Wo, const void *residual, int residual_f16,
        const float *x1, const int32_t *table1, int gH1, int gW1, int N1, int R1, int S1,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin_scale0, const float *twin_shift0,
        float *twin1, const float *twin_scale1, const float *twin_shift1,
        float *out, void *stream);
/* ... with the window edge as an argument (block size = bH = bW).  6: exactly sige_hip_tile_conv3_nhwc.  10: the same kernel
 * over ONE 10x10 window per workgroup -- 8x8 = 64 output pixels x 64 output channels, 100 staged pixels per 64 outputs where
 * four 6x6 windows stage 144, one index entry and one run of scatter-map look-ups where they take four.  Tiles are [B*N,8,8,C]
 * (source 2: Rx = Sx = 8), the full destination is written at offset + origin, clipped at the bottom and right, with bias,
 * residual, block residual (x1 / table1 over R1 x S1 cells), twins and the out-affine as above.  Block 10 takes compute 0 over
 * fp32-stored tensors only, a RAW source 2 (no affine), one edit (sige_hip_set_edit_batch(1)), and nothing held by
 * sige_hip_conv_pair_begin or armed / queued by sige_hip_conv_side_begin; this entry point has no launch-plan hook and is
 * refused while a plan records.  Everything else, other edges included: SIGE_HIP_EUNSUPPORTED -- never a wrong answer.
 * sige_hip_gather_conv_nhwc and sige_hip_scatter_gather_conv_scatter_nhwc called with bH = bW = 10, a 3x3 / stride-1 kernel and
 * a non-NULL `packed_tile3` run this form whatever `min_blocks` says (the geometry has no other matrix form; `packed` is not read).
 * sige_hip_tile_conv3_block_supported: 1 if the channel counts and the edge have a kernel. */
int sige_hip_tile_conv3_block_supported(int C1, int C2, int Cout, int bH, int bW);
int sige_hip_tile_conv3_block_nhwc(
        int compute, int source, const float *x, const void *x2, int y_f16, int B, int C1, int C2, int H, int W, int bH, int bW, int upsample2x,
        const int32_t *active_indices, int N, const int32_t *scatter_map, int Rx, int Sx,
        const float *scale, const float *shift, int affineB, int activation,
        const float *packed, const float *bias, int Cout,
        int to_full, int offsetH, int offsetW, int Ho, int Wo, const void *residual, int residual_f16,
        const float *x1, const int32_t *table1, int gH1, int gW1, int N1, int R1, int S1,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin_scale0, const float *twin_shift0,
        float *twin1, const float *twin_scale1, const float *twin_shift1,
        float *out, void *stream);

/* ---- the nearest-x2 Upsample conv as four 2x2 phase convs ON THE TILE CONV V3 (csrc/conv_tile3.hpp: Tile3GeoP):
 * what sige_hip_gather_conv_nhwc(upsample2x = 2) computes, on grids that fill the chip, in exact fp32 and on fp16 operands, under
 * stacked edits too.  A workgroup is 8 tiles x one phase x 64 output channels; the grid is ceil(B N / 8) * (Cout / 64) x 4.
 *   n = sige_hip_upsample_phase_tile3_packed_size(Cout, Cin, prec)   floats; prec 2: exact fp32, 0: fp16 (sige_hip_wide_conv_pack's)
 *   sige_hip_upsample_phase_tile3_pack(w_phases, ..., prec, packed)  w_phases [4,Cout,Cin,2,2] fp32, phase 2a + b: the tap sums;
 *       four sub-packs in the v3 stream order [ntile][wave][chunk][step], 4 steps per chunk, each with padding of its own;
 *       prec 0 rounds the sums once more, to fp16 (RNE, saturated)
 * sige_hip_upsample_phase_tile3_nhwc: x [B,H/2,W/2,C], (H, W) the upsampled size the 6x6 tile origins index, raw (no affine, one
 * tensor), straight into out [B,Ho,Wo,Cout] at offset + origin (clipped) with bias, fp32 `residual`, out-affine and both twins as
 * sige_hip_tile_conv3_nhwc; cells outside the list are untouched.  compute 0: exact fp32; 1: activations rounded to fp16 (RNE,
 * saturated) in the staging path, fp32 accumulation, tensors fp32 in memory.  Stacked edits: a tile reads the rows of its own image.
 * The call runs when its grid has at least `min_blocks` > 0 workgroups.  SIGE_HIP_EUNSUPPORTED -- nothing touched, never a wrong
 * answer -- for a smaller grid, min_blocks <= 0, C or Cout not a multiple of 64, odd H or W, compute 2, a call
 * sige_hip_conv_side_begin waits for, and while a launch plan records (no plan hook).  A shortcut held by sige_hip_conv_pair_begin
 * is launched first; queued side convs are flushed on a hazard.  N = 0 or B = 0: SIGE_HIP_OK, no launch.
 * PRECONDITION the library cannot check (the index list lives on the device): every tile origin is ODD in both coordinates, beside
 * odd offsets (an even offset IS checked: SIGE_HIP_EUNSUPPORTED) -- the lists of a padding-1 3x3 conv, origins (4i - 1, 4j - 1) with offset (1, 1) -- so that a tile's 4x4 output
 * block starts on an even hi-res pixel and splits into whole 2x2 phase blocks.  On any other list the phase decomposition is not the
 * 9-tap conv; such callers keep upsample2x = 1.  (The same holds for sige_hip_gather_conv_nhwc with upsample2x = 2.) */
int sige_hip_upsample_phase_tile3_supported(int C, int Cout);
size_t sige_hip_upsample_phase_tile3_packed_size(int Cout, int Cin, int prec);
int sige_hip_upsample_phase_tile3_pack(const float *w_phases, int Cout, int Cin, int prec, float *packed, void *stream);
int sige_hip_upsample_phase_tile3_nhwc(
        int compute, const float *x, int B, int C, int H, int W, const int32_t *active_indices, int N,
        const float *packed_phase3, const float *bias, int Cout, int offsetH, int offsetW, const float *residual, int Ho, int Wo,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin0_scale, const float *twin0_shift,
        float *twin1, const float *twin1_scale, const float *twin1_shift,
        int min_blocks, float *out, void *stream);

/* ---- token-matrix helpers of Stable Diffusion's spatial transformer (csrc/token_ops.hip; sige_attention.py:86-185): tokens [T,C]
 * row-major fp32.  add_layer_norm: y = x (+ delta + bias[c] when delta != NULL; bias may be NULL); sum_out = y when not NULL;
 * out = LayerNorm(y) * gamma + beta (eps as nn.LayerNorm's).  geglu: out[t,d] = x[t,d] * gelu(x[t,D+d]), x [T,2D] (F.gelu's erf
 * form).  add_bias: out = x + delta + bias[c] (bias may be NULL). */
int sige_hip_add_layer_norm_tokens_f32(const float *x, const float *delta, const float *bias, const float *gamma,
                                       const float *beta, int64_t T, int C, float eps, float *sum_out, float *out, void *stream);
int sige_hip_geglu_tokens_f32(const float *x, int64_t T, int D, float *out, void *stream);
int sige_hip_add_bias_tokens_f32(const float *x, const float *delta, const float *bias, int64_t T, int C, float *out, void *stream);

/* ---- token linear of the same transformer blocks (csrc/token_linear.hip): out[M,N] = epilogue(prologue(x)[M,K] . W^T) for tokens x
 * [M,K] row-major fp32 and W = nn.Linear.weight [N,K], exact fp32 products on the f32 MFMA, fixed summation order (no atomics).
 *   packed_size  floats of the packed weights, 0 = unsupported (N % 16, K % 16; geglu: N = 2 D with D % 32 == 0).  Host only.
 *   supported    1 if token_linear_f32 takes the shape: layer_norm needs K <= 2048; parts in 1..3, (N / parts) % 64 == 0 and no geglu
 *                when parts > 1; tensors below 2 GiB.  Host only.
 *   pack         W [N,K] -> packed (one launch; re-pack after every weight update).  geglu: the rows of W are [value D | gate D].
 *   token_linear prologue: ln_gamma != NULL -> a = (x - mean_r) * rstd_r * gamma[k] + beta[k] (statistics over K, two-pass, eps as
 *                nn.LayerNorm's); epilogue: acc + bias[n] (bias may be NULL), then
 *                  geglu     out0[m,d] = (acc[m,d] + bias[d]) * gelu(acc[m,D+d] + bias[D+d]), out0 [M,D] (F.gelu's erf form)
 *                  residual  out0 = residual + (...), residual shaped like out0 (parts == 1 only)
 *                  parts     column group p of N / parts columns goes to its own contiguous [M, N/parts] tensor out<p>
 *                            (q | k | v over stacked weights); unused out pointers may be NULL.
 *                M == 0 returns OK without a launch.  All pointers 16-byte aligned. */
size_t sige_hip_token_linear_packed_size(int N, int K, int geglu);
int sige_hip_token_linear_supported(int64_t M, int N, int K, int layer_norm, int geglu, int parts);
int sige_hip_token_linear_pack(const float *w, int N, int K, int geglu, float *packed, void *stream);
int sige_hip_token_linear_f32(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                              const float *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                              float *out0, float *out1, float *out2, void *stream);

/* ---- 3x3 / padding-1 conv with <= 4 output channels over a full channels-last tensor
 * (the U-Net's conv_out after norm_out + SiLU, sige_fused_unet.py:430-434, which the
 * reference runs densely in sparse mode too): out [B,H,W,Cout] = conv(act(scale*x + shift)),
 * x [B,H,W,C], weight [Cout,C,3,3] (the nn.Conv2d layout), scale / shift [1|B, C] or NULL. */
int sige_hip_conv3x3_small_cout_nhwc_f32(const float *x, int B, int C, int H, int W,
                                         const float *scale, int scaleB, int scaleC,
                                         const float *shift, int shiftB, int shiftC, int activation,
                                         const float *weight, const float *bias, int Cout,
                                         float *out, void *stream);

/* ... with an activation in front (SIGE_HIP_ACT_IDENTITY | _SWISH | _LEAKY with `slope`) and one behind (_IDENTITY | _TANH): GauGAN's
 * tanh(conv_img(leaky_relu(x, 0.2))) (gaugan/models/spade_generators/sige_fused_spade_generator.py:259-260) in one launch. */
int sige_hip_conv3x3_small_cout_act_nhwc_f32(const float *x, int B, int C, int H, int W, int activation, float slope,
                                             const float *weight, const float *bias, int Cout, int out_activation,
                                             float *out, void *stream);

/* ---- latent head of the SD VAE encoder (csrc/conv_latent_head.hip): norm_out -> SiLU -> conv_out with the autoencoder's 1x1
 * quant_conv folded into the weights (sige_model.py:272-275, ldm/models/autoencoder.py encode()), which the reference runs densely in
 * every mode.  out [B,H,W,Cout] = conv3x3_pad1(act(scale*x + shift)) + bias with the conventions of
 * sige_hip_conv3x3_small_cout_nhwc_f32 (zero padding of the ACTIVATED tensor; act in SIGE_HIP_ACT_IDENTITY | _SWISH), for
 * 5 <= Cout <= 16, C % 64 == 0, C <= 512, all pointers 16-byte aligned; anything else is SIGE_HIP_EUNSUPPORTED without a launch.
 * Exact fp32 operands on the matrix cores, ONE launch; a channel split over workgroups is added up in split order inside the
 * launch, so the result is bit-identical from run to run.
 * z != NULL (Cout even): the posterior of DiagonalGaussianDistribution as a second output, z [B,H,W,Cout/2] =
 * latent_scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), mean = out[..., :Cout/2], logvar = out[..., Cout/2:],
 * noise [B,H,W,Cout/2] (NULL: the mode, latent_scale * mean).  The moments `out` are always written. */
int sige_hip_conv3x3_latent_head_nhwc_f32(const float *x, int B, int C, int H, int W,
                                          const float *scale, int scaleB, int scaleC,
                                          const float *shift, int shiftB, int shiftC, int activation,
                                          const float *weight, const float *bias, int Cout, float *out,
                                          const float *noise, float latent_scale, float *z, void *stream);

/* ---- gamma | beta of a GAN-Compression ("sub-mobile") SPADE layer (csrc/spade_separable.hip): the two SIGESeparableConv2d of
 * gaugan/models/sige_normalization.py:124-127 -- depthwise 3x3 / padding 1 with bias, the InstanceNorm as the per-channel affine the
 * full pass cached (mobile_modules.py:104-114), pointwise 1x1 with bias -- for both branches b in {gamma, beta} in ONE launch:
 *   out[p][b*oc + o] = pw_bias[b][o] + sum_c pw_weight[b][o][c] * (in_shift[b][c] + in_scale[b][c] * (dw_bias[b][c] + sum_tap
 *                      dw_weight[b][c][tap] * actv[p + tap][c]))
 * tiled != 0: actv = T tile slabs [T,6,6,Ch] that carry their halo, out = [T,4,4,2*oc] (H = W = 6; T = 0 is OK without a launch);
 * tiled == 0: actv = one full tensor [H,W,Ch] (T = 1), zero padding at the image border, out = [H,W,2*oc]; refused while edits are
 *   stacked (sige_hip_set_edit_batch).
 * dw_weight [2,Ch,3,3], dw_bias / in_scale / in_shift [2,Ch], pw_weight [2,oc,Ch], pw_bias [2,oc]: the nn.Conv2d layouts, stacked per
 * branch.  Ch % 4 == 0, 8 <= Ch <= 128, oc % 4 == 0, 4 <= oc <= 1024, all pointers 16-byte aligned; anything else is
 * SIGE_HIP_EUNSUPPORTED without a launch.  The depthwise part is fp32 VALU arithmetic in tap order, the pointwise part exact fp32
 * operands on the matrix cores; no atomics: bit-identical from run to run, and the two forms agree bit for bit on the same pixels. */
int sige_hip_spade_separable_nhwc_f32(const float *actv, int tiled, int T, int H, int W, int Ch,
                                      const float *dw_weight, const float *dw_bias, const float *in_scale, const float *in_shift,
                                      const float *pw_weight, const float *pw_bias, int oc, float *out, void *stream);

/* ... the InstanceNorm of a DENSE layer, recomputed per image (mobile_modules.py:116: the blocks below num_sparse_layers run the
 * whole module on the edited label features): actv [H,W,Ch] is E images of h = H / E rows under sige_hip_set_edit_batch(E) (E = 1:
 * one image, any H and W); out_scale / out_shift [E,2,Ch].  For image e, branch b, channel c over the image's h * W pixels, with
 * d = dw_bias[b][c] + sum_tap dw_weight[b][c][tap] * actv[p + tap][c] and zero padding at THAT image's border (seam rows included):
 *   out_scale = 1 / sqrt(var(d) + eps) (biased variance), out_shift = -mean(d) * out_scale.
 * ONE launch, two passes inside it (the mean, then sum (d - mean)^2 with d recomputed in the tap order of the launch above), fixed
 * summation order, no atomics and no workspace: the statistics of image e are bit-identical to a single-image call on that image and
 * from run to run.  Ch as above, all pointers 16-byte aligned, h a power of two >= 4 when E > 1; anything else is
 * SIGE_HIP_EUNSUPPORTED without a launch. */
int sige_hip_spade_separable_stats_nhwc_f32(const float *actv, int H, int W, int Ch, const float *dw_weight, const float *dw_bias,
                                            float eps, float *out_scale, float *out_shift, void *stream);

/* ... and the dense form (tiled == 0) over those E images with ONE AFFINE PER IMAGE, in_scale / in_shift [E,2,Ch]: a pixel of row y
 * belongs to image e = y / h, its taps are zero outside rows [e*h, (e+1)*h) and its affine is image e's; out [H,W,2*oc].  The same
 * kernel and the same arithmetic in the same order: at E = 1 equal to sige_hip_spade_separable_nhwc_f32(tiled = 0) bit for bit. */
int sige_hip_spade_separable_images_nhwc_f32(const float *actv, int H, int W, int Ch, const float *dw_weight, const float *dw_bias,
                                             const float *in_scale, const float *in_shift, const float *pw_weight,
                                             const float *pw_bias, int oc, float *out, void *stream);

/* ---- channels-last helpers of the GauGAN SPADE generator's sparse forward (csrc/spade_ops.hip): what was left to torch kernels
 * in round 4, so that the whole forward goes through this library and a launch plan can record it.
 * resize_nearest: F.interpolate(mode="nearest") by an INTEGER factor up or down, x [B,H,W,C] -> out [B,Ho,Wo,C]
 *   (sige_fused_spade_generator.py:143-146 the label map per block, :243-257 the x2 up-sampling between blocks).
 * act_split: out[part] = act(x[..., part*C/parts : (part+1)*C/parts]) as `parts` dense [pixels, C/parts] tensors one after
 *   the other, `part_stride` floats apart (>= pixels * C/parts: a launch plan sizes it for every candidate tile, so the parts'
 *   addresses do not move with the mask) -- ReLU + torch.split of a block's label features; act in IDENTITY | RELU | LEAKY.
 * scatter_gather_split: scatter_gather (sige/cpu/scatter_gather.cpp:5-56; no affine) + the same act + split in one pass;
 *   out = `parts` dense [B*N,bH,bW,C/parts] tile slabs.
 * spade_modulate_dense: out = leaky?((scale*x + shift) * (1 + gamma) + beta) on a FULL tensor, gb [B,H,W,2C] = gamma | beta,
 *   scale / shift [affineB in {1, B}, C] (sige_normalization.py:74-88 for the blocks below num_sparse_layers). */
int sige_hip_resize_nearest_nhwc_f32(const float *x, int B, int C, int H, int W, int Ho, int Wo, float *out, void *stream);
int sige_hip_act_split_nhwc_f32(const float *x, int64_t pixels, int C, int parts, int64_t part_stride, int activation, float slope,
                                float *out, void *stream);
int sige_hip_scatter_gather_split_nhwc_f32(const float *x, const float *y, int B, int C, int H, int W, int Rx, int Sx, int bH,
                                           int bW, const int32_t *active_indices, int N, const int32_t *scatter_map,
                                           int activation, float slope, int parts, int64_t part_stride, float *out,
                                           void *stream);
int sige_hip_spade_modulate_dense_nhwc_f32(const float *x, const float *scale, const float *shift, int affineB, const float *gb,
                                           int B, int C, int H, int W, int leaky, float slope, float *out, void *stream);

/* ---- 3x3 / padding-1 conv with <= 3 input channels and Cout = 32 / 64 / 128 over a full image
 * (the U-Net's conv_in, sige_fused_unet.py:395: a plain nn.Conv2d in every mode):
 * out [B,H,W,Cout] (channels-last) = conv(x) + bias; x is addressed through its element strides
 * (NCHW or channels-last), weight [Cout,Cin,3,3]. */
int sige_hip_conv3x3_small_cin_nhwc_f32(const float *x, int64_t strideB, int64_t strideC, int64_t strideH, int64_t strideW,
                                        int B, int Cin, int H, int W,
                                        const float *weight, const float *bias, int Cout,
                                        float *out, void *stream);
/* ... evaluated only on the bH x bW windows at active_indices (clipped), written in place into `out` [B,H,W,Cout]; other pixels of
 * `out` keep their contents (round 6: in sparse mode the first conv's output is only read through Gather windows). */
int sige_hip_conv3x3_small_cin_tiles_nhwc_f32(const float *x, int64_t strideB, int64_t strideC, int64_t strideH, int64_t strideW,
                                              int B, int Cin, int H, int W,
                                              const float *weight, const float *bias, int Cout,
                                              const int32_t *active_indices, int N, int bH, int bW,
                                              float *out, void *stream);

/* per-group mean / rstd of a [B,C,H,W] tensor -> per-channel (scale, shift) with
 * GroupNorm(x) == x*scale + shift  (scale = gamma*rstd, shift = beta - mean*scale):
 * the producer of the cached affine (diffusion/models/common.py:37-57) as two
 * streaming launches.  `workspace`: sige_hip_group_norm_affine_workspace floats
 * (always ask: per (batch, group) it holds the splits' partial sums as fp32 pairs in two
 * planes and one pivot pair; contents are scratch).
 * The statistics: the variance is E[v^2] - E[v]^2 of v = x - K, K the group's first
 * element (a one-pass variance of x itself from fp32 sums loses eps32 * (mean / std)^2 of its
 * accuracy); lanes sum v in fp32, everything across lanes and splits is fp64; scale and shift
 * are formed in fp64 and rounded once.  |scale - exact| <= 4e-6 |exact| for |mean| / std up to
 * 3000 and for constant groups (tests/test_gpu_group_norm_offsets.py). */
size_t sige_hip_group_norm_affine_workspace(int B, int C, int H, int W, int groups);
int sige_hip_group_norm_affine_f32(const float *x, int B, int C, int H, int W, int groups, float eps,
                                   const float *gamma, const float *beta, float *workspace,
                                   float *scale, float *shift, void *stream);

/* channels-last form: x [B,H,W,C] */
size_t sige_hip_group_norm_affine_nhwc_workspace(int B, int C, int H, int W, int groups);
int sige_hip_group_norm_affine_nhwc_f32(const float *x, int B, int C, int H, int W, int groups, float eps,
                                        const float *gamma, const float *beta, float *workspace,
                                        float *scale, float *shift, void *stream);

/* the same with a per-channel bias [C] added BEFORE the statistics (a residual block's GroupNorm of h + temb,
 * diffusion/models/ddpm_arch/sige_fused_unet.py:116-117); the affine is returned for x itself:
 * GroupNorm(x + channel_bias) == x * scale + shift.  One batch-independent bias vector.
 * The pivot includes the bias: v = (x - K_x) + (channel_bias - K_b), K_b the bias of the group's first channel, so a bias that
 * IS the group's offset (|bias| >> spread of x) costs no accuracy; shift = beta - (mean - channel_bias) * scale in fp64. */
int sige_hip_group_norm_affine_nhwc_bias_f32(const float *x, int B, int C, int H, int W, int groups, float eps,
                                             const float *gamma, const float *beta, const float *channel_bias,
                                             float *workspace, float *scale, float *shift, void *stream);

/* the same affine from per-channel statistics instead of the tensor: statsK [2][B * tilesK, CK, 2] = per pixel block and channel
 * (sum, sum of squares) as sige_hip_wide_conv_nhwc leaves them (tilesK blocks per batch element, countK = pixels per batch
 * element the sums run over).  Both sums are accumulated in fp64 inside the producing launch (the square of an fp32 value is
 * exact there) and stored as unevaluated fp32 PAIRS hi + lo: plane [0] holds the leading parts -- on their own the fp32 sums -- and plane [1], B * tilesK * CK * 2 floats behind it,
 * the low parts; the finisher adds hi + lo in fp64.  A statsK buffer is therefore 2 * B * tilesK * CK * 2 floats, and one
 * that holds only the first plane is NOT valid input.  Two parts = the GroupNorm of torch.cat([a, b], 1) over C1 + C2 channels without the cat
 * (stats2 NULL / C2 0: one tensor; a group may straddle the parts).  channel_bias [C1 + C2] or NULL as above.  One launch. */
int sige_hip_group_norm_affine_from_stats_f32(const float *stats1, int tiles1, int C1, int count1,
                                              const float *stats2, int tiles2, int C2, int count2,
                                              int B, int groups, float eps, const float *gamma, const float *beta,
                                              const float *channel_bias, float *scale, float *shift, void *stream);

/* per-channel statistics of a channels-last tensor x [B,H,W,C] in that layout, for a tensor whose producer left none:
 * stats [2][B * sige_hip_channel_stats_tiles(H, W), C, 2] (leading parts, then low parts: above), count = H * W.  One pass over x. */
int sige_hip_channel_stats_tiles(int H, int W);
int sige_hip_channel_stats_nhwc_f32(const float *x, int B, int C, int H, int W, float *stats, void *stream);

/* ---- single-head spatial self-attention of the U-Net's dense AttnBlock ------
 * (diffusion/models/ddpm_arch/unet.py AttnBlock.forward, reached from
 * sige_fused_unet.py:186-199): qkv [B,3C,HW] = q, k, v stacked on the channel axis,
 * out[b,c,i] = sum_j v[b,c,j] * softmax_j(scale * sum_c' q[b,c',i] k[b,c',j]).
 * Two launches (score tiles, then softmax + value product); `workspace` holds the
 * [B,HW,HW] scores (sige_hip_attention_workspace floats).  HW and C multiples of 16. */
size_t sige_hip_attention_workspace(int B, int C, int HW);
int sige_hip_attention_f32(const float *qkv, int B, int C, int HW, float scale, float *workspace,
                           float *out, void *stream);
/* channels-last form: qkv [B,HW,3C] -> out [B,HW,C]; C % 64 == 0 */
int sige_hip_attention_nhwc_f32(const float *qkv, int B, int C, int HW, float scale, float *workspace,
                                float *out, void *stream);
/* ... with the epilogue of the 1x1 proj_out conv that follows the attention in the U-Net, for a caller that has folded that
 * conv's matrix into the value projection (softmax rows sum to 1: W_p (P v) + b_p = P (W_p W_v x + W_p b_v) + b_p):
 *   out = (attention + bias[c]) + residual;   twin_k = SiLU(twin_k_shift[c] + twin_k_scale[c] * out)
 * -- separately rounded fp32 ops in that order, the twins as in the full-tensor conv entry points.  bias / twin scale / shift
 * [C]; residual / twins [B,HW,C]; each optional (NULL), all NULL = sige_hip_attention_nhwc_f32 bit for bit.  The same two
 * launches, workspace and supported shapes (SIGE_HIP_EUNSUPPORTED otherwise); SIGE_HIP_EINVAL for a twin without its scale and
 * shift, or an optional pointer that is not 16-byte aligned. */
int sige_hip_attention_residual_nhwc_f32(const float *qkv, int B, int C, int HW, float scale, float *workspace,
                                         const float *bias, const float *residual,
                                         float *twin0, const float *twin0_scale, const float *twin0_shift,
                                         float *twin1, const float *twin1_scale, const float *twin1_shift,
                                         float *out, void *stream);
/* ... with the key projection folded away as well.  With x_n = s*x + t the block's normalised input, q = W_q x_n + b_q and
 * k = W_k x_n + b_k, every term of q_i . k_j that does not depend on the key j cancels in the softmax over j, so
 *   softmax_j(scale q_i . k_j) = softmax_j(scale q''_i . x_j),   q'' = s * ((W_k^T W_q) x_n + W_k^T b_q)
 * and the keys are the block input itself.  qv [B,HW,2C] = (q | v') on the channel axis, keys [B,HW,C] (16-byte aligned).
 * qscale [qscaleB, C] (qscaleB 1 or B; 16-byte aligned) or NULL: the factor s, applied to the query channels as the score kernel
 * loads them (q'' = qscale * q) -- read from the caller's own tensor at every launch, so a caller whose cached scale is rewritten
 * in place keeps no copy of it; NULL: qv holds q'' already.  SIGE_HIP_EINVAL for another qscaleB or a misaligned qscale;
 * everything else -- epilogue, launches, workspace, supported shapes, error codes -- as sige_hip_attention_residual_nhwc_f32. */
int sige_hip_attention_residual_qv_nhwc_f32(const float *qv, const float *keys, const float *qscale, int qscaleB,
                                            int B, int C, int HW, float scale, float *workspace, const float *bias, const float *residual,
                                            float *twin0, const float *twin0_scale, const float *twin0_shift,
                                            float *twin1, const float *twin1_scale, const float *twin1_shift,
                                            float *out, void *stream);
/* the same in ONE launch (round 4): workgroup = 16 queries x 64 keys, exact fp32 MFMA scores, the 64-key slices of a query
 * block combined by the last one to finish (flash-decoding split; the tickets of the conv kernels' K-split finish) -- no score
 * tensor in HBM, 6 launches fewer per DDPM forward.  C in {64, 128, 256, 512}, HW % 16 == 0, HW <= 1024; `workspace` holds the
 * per-slice partial outputs (sige_hip_attention_fused_workspace floats; 0 = shape unsupported).  SIGE_HIP_EUNSUPPORTED: use
 * sige_hip_attention_nhwc_f32. */
size_t sige_hip_attention_fused_workspace(int B, int C, int HW);
int sige_hip_attention_fused_nhwc_f32(const float *qkv, int B, int C, int HW, float scale, float *workspace,
                                      float *out, void *stream);

/* ---- split fp16 operands (compute = 2): fp32-level results from the fp16 matrix cores -------------------
 * The channels-last entry points with compute = 2: every fp32 operand (staged activation after the cached affine + SiLU, weight) is
 * carried as an fp16 pair hi = fp16(v), lo = fp16(v - hi); hi*hi + lo*hi + hi*lo accumulate in fp32 (22-bit operands;
 * the dropped lo*lo term is 2^-22 relative).  Results are inside the fp32 path's 1e-3 (measured ~1e-6 relative against an
 * fp64 conv) at a third of the fp16 matrix rate = 5.3x the f32-input rate.  sige_hip_block_conv_pack_f16x3 scales the
 * weights by a power of two chosen on the device (max |w| * 2^S in [2^13, 2^14): lo parts stay normal fp16 numbers) and
 * stores 2^-S behind the packed data; no host synchronisation.  Geometries as for compute = 1.  */
size_t sige_hip_block_conv_packed_size_f16x3(int Cout, int Cin, int kH, int kW, int R, int S,
                                            int strideH, int strideW, int groups);
int sige_hip_block_conv_pack_f16x3(const float *w, int Cout, int Cin, int kH, int kW,
                                  float *packed, void *stream);

/* ---- dense layers on the fp16 matrix cores ("wide" conv: 8x8 pixels x 64 output channels per workgroup) -------
 * The layers a SIGE network runs DENSELY -- below `sparse_resolution_threshold` in the sparse pass
 * (diffusion/models/ddpm_arch/sige_fused_unet.py:112-123) and every conv of the cache-producing full pass
 * (sige/nn/base.py:85-86; diffusion/samplers/ddim_ddpm_sampler.py:60-66) -- as ONE launch each:
 *
 *   out = out_act(out_scale * (conv(act(scale * cat(x, x2) + shift)) + bias + residual) + out_shift)
 *
 * 3x3 / padding 1 or 1x1, stride 1, channels-last fp32 tensors (x [B,H,W,C1], x2 [B,H,W,C2] or NULL, residual / out /
 * twins [B,H,W,Cout]); zero padding is applied AFTER affine + activation.  `upsample2x`: x (and x2) are the
 * half-resolution tensors [B,H/2,W/2,C] read as their nearest x2 upsampling (F.interpolate fused, sige_fused_unet.py:222-227).
 * scale / shift: [affineB, C1+C2] (affineB 1 or B) or NULL / NULL (then activation must be identity).
 * Arithmetic (`prec`), fp32 accumulation in every form:
 *   0: v_mfma_f32_32x32x16_f16, operands rounded to fp16 (BASELINE.json configs[4]; tolerance 2e-2 + 1e-2 |ref|);
 *   1: the same instruction, every operand split into fp16 hi + lo, products hi*hi + lo*hi + hi*lo (22-bit operands):
 *      fp32-level results, inside the fp32 path's 1e-3.  `wshift`: the weights were packed as w * 2^wshift (a power of two
 *      chosen by the caller so that max |w| * 2^wshift is in [2^13, 2^14): keeps the lo parts normal fp16 numbers);
 *   2: v_mfma_f32_32x32x2_f32, exact fp32 products (wshift must be 0).
 * Shapes: C1, C2 multiples of 64 (3x3) / 128 (1x1), Cout a multiple of 64 (sige_hip_wide_conv_supported).
 * twinK (optional): twinK = SiLU(twin_scaleK * v + twin_shiftK), v = the value `out` receives before its out-affine.
 * workspace (optional, sige_hip_wide_conv_workspace floats): small layers split K across workgroups and finish inside
 * the launch (deterministic summation order); without it they run unsplit.
 * stats (optional, [2][B * ceil(H/8) * ceil(W/8), Cout, 2] floats -- leading parts, then low parts of fp32 pairs, see
 * sige_hip_group_norm_affine_from_stats_f32): per 8x8 pixel block and output channel the (sum, sum of
 * squares) of what `out` receives (before its out-affine) -- the input of sige_hip_group_norm_affine_from_stats_f32, so that
 * the GroupNorm of the output needs no pass over it.                                                              */
int sige_hip_wide_conv_supported(int C1, int C2, int Cout, int kH, int kW);
/* packed size in 4-byte units (0: unsupported shape) */
size_t sige_hip_wide_conv_packed_size(int Cout, int Cin, int kH, int kW, int prec);
int sige_hip_wide_conv_pack(const float *w, int Cout, int Cin, int kH, int kW, int prec, int wshift,
                            float *packed, void *stream);
size_t sige_hip_wide_conv_workspace(int B, int H, int W, int C1, int C2, int Cout, int kH, int kW);
int sige_hip_wide_conv_nhwc(const float *x, const float *x2, int B, int C1, int C2, int H, int W, int upsample2x,
                            const float *scale, const float *shift, int affineB, int activation,
                            const float *packed, int prec, int wshift, const float *bias, int Cout, int kH, int kW,
                            const float *residual, const float *out_scale, const float *out_shift, int out_activation,
                            float *twin0, const float *twin_scale0, const float *twin_shift0,
                            float *twin1, const float *twin_scale1, const float *twin_shift1,
                            float *workspace, size_t workspace_floats, float *out, float *stats, void *stream);

/* out = act(scale[b,c] * x + shift[b,c]) over a channels-last tensor [B,H,W,C] (scale / shift [affineB, C], affineB 1 or B):
 * the activated copy of a ScatterGather cache that the full pass keeps next to the cache (one pass instead of the
 * multiply / add / SiLU / copy kernels of the torch expression; sige_amd.nn.ScatterGather.cache_activated).          */
int sige_hip_affine_act_nhwc_f32(const float *x, int B, int C, int H, int W, const float *scale, const float *shift,
                                 int affineB, int activation, float *out, void *stream);

/* ---- multi-head attention over token matrices (Stable Diffusion's spatial transformer) ---------------------------------
 * out[b, i, h*d .. (h+1)*d) = softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]  for q [B,Nq,C], k / v [B,Nk,C], C = heads * d,
 * row-major fp32 -- a channels-last [B,C,H,W] tensor IS its token matrix [B,HW,C] and channels-last tiles [T,C,4,4] ARE
 * [T*16, C], so the sparse-query attention of stable-diffusion/ldm/modules/sige_attention.py:151-176 (queries = the tokens of
 * the active tiles, keys / values = every token of the scattered feature map, or the text context) needs no rearrange copy
 * and no score tensor in HBM: one launch, exact fp32 products, online softmax (attention.py's CrossAttention.forward does
 * rearrange x 3, einsum, softmax, einsum, rearrange).  Nq % 16 == 0, d % 4 == 0, d <= 160; Nk arbitrary.                */
int sige_hip_attention_tokens_supported(int Nq, int Nk, int C, int heads);
int sige_hip_attention_tokens_f32(const float *q, const float *k, const float *v, int B, int Nq, int Nk, int C,
                                  int heads, float scale, float *out, void *stream);

/* ---- the same attention with fp16 OPERANDS (the f16 compute mode: SIGEModel.set_compute_dtype("f16")) -----------------
 * Arguments, layouts, shape predicate (sige_hip_attention_tokens_supported) and status rules of sige_hip_attention_tokens_f32:
 * q, k, v and out are fp32 token matrices in memory.  Arithmetic contract:
 *   - q, k, v are rounded to nearest even to fp16 in registers (never truncated);
 *   - scores are accumulated in fp32 and scaled in fp32, in units of log2 (exp(x) = exp2(x * log2 e)) like the fp32 form;
 *   - the softmax state (running maximum m, sum l, rescale factor alpha) is fp32; l sums the unrounded probabilities;
 *   - the probabilities are rounded to nearest even to fp16 for the product with v (carried scaled by 2^15 inside the
 *     kernel, so none of them down to 2^-29 is an fp16 subnormal; the factor cancels in O / l);
 *   - O, the merge of the partial results and the division by l are fp32.
 * Finite inputs beyond fp16's range (|x| > 65504) are OUTSIDE the contract: they round to infinity, and an infinity that meets
 * the zero padding of a head makes NaN.
 * B * Nq == 0: SIGE_HIP_OK without a launch.  Null pointers: SIGE_HIP_EINVAL.  A shape the predicate refuses, a pointer that is
 * not 16-byte aligned, one batch's K or V >= 2 GiB: SIGE_HIP_EUNSUPPORTED.                                                  */
int sige_hip_attention_tokens_f16c(const float *q, const float *k, const float *v, int B, int Nq, int Nk, int C,
                                   int heads, float scale, float *out, void *stream);

/* ---- ... both with the keys of a query tile's OWN image (stacked edits, sige_hip_set_edit_batch) --------------------------------
 * The queries are the tokens of T active 4x4 tiles of the tall image [1,C,H,W] = E images of H / E rows (E = the calling
 * thread's edit batch): q, out [16 T, C], tile t = rows 16 t .. 16 t + 15; k, v [H W, C], the rows of the tall image;
 * active_indices = the Gather's device int32 [T,2] list, row origin first.  B = 1.
 * Tile t belongs to image e = origin_row >> log2(H / E), clamped into [0, E - 1] (a bad list cannot move an address outside
 * k / v), and attends to rows [e (H / E) W, (e + 1) (H / E) W) only: the kernels of the two entries above -- a workgroup is one
 * 16-query tile of one head -- with the K and V base pointers and both buffer descriptors moved to the image's first row and
 * spanning ONE image's bytes, so tail masking, the key clamps, the zeros of an out-of-range load and the 2 GiB limit are per
 * image (Nk = (H / E) W).  One launch for the tiles of all E edits; no per-edit count ever reaches the host.  The index list is
 * the per-edit lists one after the other, so consecutive tiles of a head share an image's K / V.  E = 1: the results of
 * sige_hip_attention_tokens_f32 / _f16c bit for bit (the same kernel, the list unread).  _f16c keeps the arithmetic contract
 * stated at sige_hip_attention_tokens_f16c.
 * Status, in this order: SIGE_HIP_EINVAL: T < 0, non-positive H / W / C / heads.  T == 0: SIGE_HIP_OK, nothing launched.
 * SIGE_HIP_EINVAL: null pointers (the index list among them) with work to do.  SIGE_HIP_EUNSUPPORTED: H / E not a power of two
 * >= 4 (or E does not divide H), and everything sige_hip_attention_tokens_f32 refuses with Nq = 16 T, Nk = (H / E) W: the shape
 * predicate, pointers not 16-byte aligned, one image's K or V >= 2 GiB, heads * T past 2^31.                                    */
int sige_hip_attention_tokens_tiles_f32(const float *q, const float *k, const float *v, const int32_t *active_indices,
                                        int T, int H, int W, int C, int heads, float scale, float *out, void *stream);
int sige_hip_attention_tokens_tiles_f16c(const float *q, const float *k, const float *v, const int32_t *active_indices,
                                         int T, int H, int W, int C, int heads, float scale, float *out, void *stream);

/* ---- the same attention for WIDE heads: 160 < d <= 512, d % 16 == 0 (the SD VAE decoder's single 512-channel head) -----
 * q [B,Nq,ldq], k [B,Nk,ldk], v [B,Nk,ldv], out [B,Nq,ldo]: every operand comes with its ROW STRIDE in elements (>= C, a
 * multiple of 4; batch stride = rows * row stride), so k and v may be the two halves of one [B,Nk,2C] tensor and q / out
 * column slices of wider matrices.  Nq % 16 == 0, Nk arbitrary (tail keys masked, fewer key blocks than waves allowed).
 * One launch: exact fp32 products, online softmax; Q staged in LDS, K / V streamed in 64-channel groups; with few query
 * tiles the key blocks are split over workgroups and added up inside the launch (tickets + a library-owned workspace, as the
 * conv K split; first use inside a stream capture or an exhausted region: no split).  The workspace of captured launches is
 * handed out again by sige_hip_release_graph_tickets().
 * SIGE_HIP_EINVAL: non-positive dims, a row stride below C, null pointers with work to do.  SIGE_HIP_EUNSUPPORTED: d <= 160
 * (sige_hip_attention_tokens_f32 serves those), d > 512, d % 16, Nq % 16, pointers not 16-byte aligned, row strides not a
 * multiple of 4, one batch's K or V >= 2 GiB, B * heads or Nq / 16 > 65535.  B * Nq == 0: SIGE_HIP_OK, nothing launched.  */
int sige_hip_attention_wide_supported(int Nq, int Nk, int C, int heads);
int sige_hip_attention_wide_f32(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                int B, int Nq, int Nk, int C, int heads, float scale, float *out, int ldo, void *stream);

/* ---- ... with the keys of a query tile's OWN image (stacked edits, sige_hip_set_edit_batch) ---------------------------------
 * The queries are the tokens of T active 4x4 tiles of the tall image [1,C,H,W] = E images of H / E rows (E = the calling
 * thread's edit batch): q, out [16 T, ld*], tile t = rows 16 t .. 16 t + 15; k, v [H W, ld*], the rows of the tall image (the two
 * halves of one [H W, 2C] tensor, as above); active_indices = the Gather's device int32 [T,2] list, row origin first.  B = 1.
 * Tile t belongs to image e = origin_row >> log2(H / E), clamped into [0, E - 1] (a bad list cannot move an address outside
 * k / v), and attends to rows [e (H / E) W, (e + 1) (H / E) W) only: the kernel of the entry above with both buffer descriptors
 * moved to the image's first row and spanning ONE image's keys, so tail masking, key split and the 2 GiB limit are per image
 * (Nk = (H / E) W).  One launch for the tiles of all E edits; no per-edit count ever reaches the host, so the call can be
 * captured in a graph and replayed under new index lists of the same T.  E = 1: the results of the entry above, bit for bit.
 * SIGE_HIP_EINVAL: T < 0, non-positive H / W / C / heads, a row stride below C, null pointers (the index list among them)
 * with work to do.  SIGE_HIP_EUNSUPPORTED: H / E not a power of two >= 4 (or E does not divide H), and everything the entry
 * above refuses with Nq = 16 T, Nk = (H / E) W.  T == 0: SIGE_HIP_OK, nothing launched.                                     */
int sige_hip_attention_wide_tiles_f32(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                      const int32_t *active_indices, int T, int H, int W, int C, int heads, float scale,
                                      float *out, int ldo, void *stream);

/* ---- ... both with fp16 OPERANDS (the f16 compute mode) ---------------------------------------------------------------------
 * Arguments, layouts, shape predicate (sige_hip_attention_wide_supported), key split and status rules -- the same checks in the
 * same order, nothing launched when refused or empty -- of sige_hip_attention_wide_f32 and sige_hip_attention_wide_tiles_f32;
 * the arithmetic contract stated at sige_hip_attention_tokens_f16c (the split merge is one more fp32 merge of partial results).
 * The key split is in 32-key steps.  E = 1 through the tiles entry: the results of the batched entry, bit for bit.               */
/* how many workgroups share the keys of one query tile when tickets and workspace are available (1: no split; 0: a shape the
 * predicate refuses) -- the launch's own formula, for tests and tools */
int sige_hip_attention_wide_f16c_splits(int B, int Nq, int Nk, int C, int heads);
int sige_hip_attention_wide_f16c(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                 int B, int Nq, int Nk, int C, int heads, float scale, float *out, int ldo, void *stream);
int sige_hip_attention_wide_tiles_f16c(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                       const int32_t *active_indices, int T, int H, int W, int C, int heads, float scale,
                                       float *out, int ldo, void *stream);

/* ---- fp16-STORED caches: the "_f16" forms of SURVEY.md 8b's export list (8f row 4: fp16 cache) ---------------------
 * The reference is fp32-only (sige/nn/base.py:15,55-63).  Here the CACHED tensors of a SIGE model -- Scatter /
 * ScatterGather `original_outputs`, ScatterWithBlockResidual `original_outputs` / `original_residuals`, and the activated
 * copy of a ScatterGather cache -- may be stored as fp16 (SIGEModel.set_cache_dtype("f16"): half the resident bytes,
 * half the bytes of the cache broadcast, no conversion pass on either side of the wire).  Activations, tiles, affines and
 * outputs stay fp32; a cached value is widened exactly when it is read.  Channels-last only.  Arguments as in the
 * "_f32" entry points of the same name, with the cached tensor(s) `const void *` = halves:
 *   gather_nhwc_f16                       x is the fp16 tensor (tiles of a cache)
 *   scatter_gather_nhwc_f16               y
 *   scatter_nhwc_f16                      y          (residual fp32)
 *   scatter_with_block_residual_nhwc_f16  y0 and y1
 *   affine_act_nhwc_f16                   x; out fp16 (out_f16 != 0: the activated copy) or fp32 (a persistent twin)
 *   convert_f16_f32 / convert_f32_f16     n elements, n % 4 == 0 (persistent-output refresh / storing a full-pass output)
 *   scatter_gather_conv_nhwc, scatter_gather_conv_scatter_nhwc
 *                                         (declared above) the fused scatter_gather -> conv (-> scatter) launches read `y`
 *                                         as fp16 when y_f16 != 0 and, in the second, `residual` when residual_f16 != 0 (a
 *                                         fused ScatterWithBlockResidual's cached shortcut), under every `compute`.
 *                                         3x3 / stride 1 only.                                                          */
int sige_hip_gather_nhwc_f16(const void *x, int B, int C, int H, int W, int bH, int bW,
                             const int32_t *active_indices, int N,
                             const float *scale, int scaleB, int scaleC,
                             const float *shift, int shiftB, int shiftC,
                             int activation, float *out, void *stream);
int sige_hip_scatter_gather_nhwc_f16(const float *x, const void *y, int B, int C, int H, int W,
                                     int Rx, int Sx, int bH, int bW,
                                     const int32_t *active_indices, int N, const int32_t *scatter_map,
                                     const float *scale, int scaleB, int scaleC,
                                     const float *shift, int shiftB, int shiftC,
                                     int activation, float *out, void *stream);
int sige_hip_scatter_nhwc_f16(const float *x, const void *y, int B, int C, int H, int W, int R, int S,
                              int offsetH, int offsetW, int strideH, int strideW,
                              const int32_t *active_indices, const int32_t *table, int gH, int gW, int N,
                              const float *residual, int in_place, float *out, void *stream);
int sige_hip_scatter_with_block_residual_nhwc_f16(
        const float *x0, const void *y0, const float *x1, const void *y1,
        int B, int C, int H, int W, int R0, int S0, int R1, int S1,
        int offsetH, int offsetW, int strideH, int strideW,
        const int32_t *active_indices0, const int32_t *table0, int gH0, int gW0, int N0,
        const int32_t *active_indices1, const int32_t *table1, int gH1, int gW1, int N1,
        int in_place, float *out, void *stream);
int sige_hip_affine_act_nhwc_f16(const void *x, int B, int C, int H, int W, const float *scale, const float *shift,
                                 int affineB, int activation, void *out, int out_f16, void *stream);
int sige_hip_convert_f16_f32(const void *src, float *dst, size_t n, void *stream);
int sige_hip_convert_f32_f16(const float *src, void *dst, size_t n, void *stream);

/* ---- stacked edits ("throughput mode"; not in the reference, whose batch shares ONE mask: sige/cpu/gather.cpp:17-21) ----
 * E edited versions of one original image, each with ITS OWN mask, processed by one set of launches: every activation
 * [E,C,H,W] (channels-last) is handed to this library as the tall image [1,C,E*H,W] -- the same bytes --, and masks, index
 * lists, scatter maps, tile tables and the cached tensors are those of the tall image (the cache of the original repeated E
 * times).  A launch then sees the active tiles of all E edits at once -- at a 1 % edit the sum of eight edits' tiles is what a
 * 10 % edit has, and a launch leaves the launch-bound regime.  sige_hip_set_edit_batch(E) tells the library where the seams are:
 * a halo row beyond a tile's own image is zero padding (not the neighbour image's pixels) in the channels-last fused gather /
 * scatter_gather -> conv kernels, the dense-layer conv, the standalone channels-last gather / scatter_gather, the SPADE
 * modulation and sige_hip_scatter_gather_split_nhwc_f32, and a query tile of sige_hip_attention_wide_tiles_f32,
 * sige_hip_attention_tokens_tiles_f32 or sige_hip_attention_tokens_tiles_f16c attends to its own image's keys; entry points whose kernels have no seam test (the NCHW forms) return
 * SIGE_HIP_EUNSUPPORTED while E > 1; per-pixel helpers (nearest resize by an integer factor, act_split, the dense SPADE
 * modulation) need none.  One image's height must be a power of two at every resolution.  Per host thread; 1 = off (default).  Whole-image ops (conv_in / conv_out, attention, GroupNorm) are simply
 * called with B = E on the same memory (sige_amd/stacked.py).  The mask pipeline follows: sige_hip_reduce_mask_i32 lets a
 * candidate tile see only its own image's mask rows, sige_hip_dilate_mask_u8 does not dilate across a seam, and
 * sige_hip_mask_pyramid_u8 builds the pyramid of every image with that image's own maxima and thresholds (one workgroup per
 * image; min_h applies to one image) -- so the index lists of a stacked mask are exactly the per-edit lists.            */
int sige_hip_set_edit_batch(int E);
int sige_hip_get_edit_batch(void);

/* ---- launch plans: a sparse forward that survives a mask change -------------------------------------------------
 * The reference sizes every launch from `activeIndices.size(0)` at call time (sige/cuda/gather_kernel.cu:78-84,111 via
 * sige/utils.py:30 and sige/nn/gather.py:101-107), and two of its three applications run ONE sparse forward per mask
 * (gaugan/runner.py:150-195, diffusion_demo/runner.py:134-164).  A plan records the calls of this library made between
 * sige_hip_plan_begin and _end on the calling thread (each call is executed as usual AND stored with its arguments) into
 * one of two sections -- 0: the mask -> index pipeline (dilation / pyramid / compaction / tile tables / scatter maps / the
 * refresh of the persistent outputs), 1: the sparse forward -- and sige_hip_plan_run replays a section on a stream without
 * any host work per launch.  Arguments that are active-tile counts are not replayed as recorded: the host binds the
 * pointer of every index list / tile table to a SLOT (sige_hip_plan_bind_ptr); at replay a count argument takes the
 * current value of the slot its index-list argument is bound to.  Slots are set by the host (_set_slot) or, inside
 * section 0, by a recorded read-back of the compaction kernels' device-side counts (_record_readback: one
 * hipMemcpyAsync + stream synchronisation, the same single synchronisation torch.nonzero costs the reference).  Output
 * block, grid, K split and tickets are chosen inside each entry point, i.e. again at every replay.  The host keeps every
 * buffer a recorded call points at alive and sized for the largest count (sige_amd/plan.py).
 * Entry points of the NCHW / two-kernel forms receive tile counts without an index list to look them up under; a plan
 * that recorded one is "shape bound" (sige_hip_plan_shape_bound) and only valid under the counts it was recorded with.
 * Replay stops at the first call that fails and returns its status.  A section can be replayed under hipGraph stream
 * capture (section 1; section 0 synchronises).                                                                       */
void *sige_hip_plan_create(void);
int sige_hip_plan_destroy(void *plan);
int sige_hip_plan_begin(void *plan, int section, int append);
int sige_hip_plan_end(void *plan);
int sige_hip_plan_recording(void);
int sige_hip_plan_shape_bound(void *plan);
int sige_hip_plan_calls(void *plan, int section);
/* n new slots (initial count 0); returns the index of the first, -1 on error */
int sige_hip_plan_new_slots(void *plan, int n);
int sige_hip_plan_bind_ptr(void *plan, const void *ptr, int slot);
int sige_hip_plan_set_slot(void *plan, int slot, int count);
/* `ptr` is an index list whose tile count does not depend on the mask (the all-tiles list of a dense layer): a count
 * recorded next to it keeps its value.  A count recorded next to a pointer that is neither bound nor constant cannot follow
 * a new mask: it is counted (plan_unbound) and marks the plan shape bound. */
int sige_hip_plan_bind_const(void *plan, const void *ptr);
int sige_hip_plan_unbound(void *plan);
/* Drop the calls of `section` recorded after the first `calls` (the host side removes an entry-point call that returned an
 * error status while recording: the hook stores a call before the entry point validates it). */
int sige_hip_plan_truncate(void *plan, int section, int calls);
/* copies min(n, slots) counts to `out`; returns the number of slots */
int sige_hip_plan_get_slots(void *plan, int32_t *out, int n);
int sige_hip_plan_record_readback(void *plan, const int32_t *device_counts, int first_slot, int n);
int sige_hip_plan_run(void *plan, int section, void *stream);

/* ---- plain device copy used by the cache broadcast path (packs the cached
 * activations of Scatter / ScatterGather modules into one buffer) ---------- */
int sige_hip_copy_f32(const float *src, float *dst, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGE_HIP_H */
