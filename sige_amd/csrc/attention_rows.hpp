// Shared by the six transposed-score attention units (attention_tokens.hip, attention_tokens_f16.hip, attention_tokens_f16kv.hip,
// attention_wide.hip, attention_wide_f16.hip, attention_wide_f16kv.hip): the row maximum -- lane (kq, j) holds scores of query j, the
// four lane rows kq of a query meet in two v_permlane*_swap --, the weight of a partial softmax state in a merge, the image of a query
// tile under stacked edits; for the four fp16-operand units the vector types, the rounding pack, the shift P is carried with and the
// buffer offset that loads zeros; for the three token units also the workgroup -> (pair, query tile) mapping; on the host the
// argument checks of the batched and of the `_tiles_` entries (_f32 / _f16c / _f16kv alike) and the geometry of the latter.
// (What only the token trio shares: attention_tokens_image.hpp; only the wide trio: attention_wide_image.hpp.)
#pragma once
#include "common.hpp"

namespace sige {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The fp16-operand kernels carry P as exp2(s - m + P_SHIFT), at most 2^15 (attention_tokens_f16.hip says why); the factor is in
// every wave's and every split's l and O alike and cancels in O / l.
constexpr float P_SHIFT = 15.f;
// A buffer offset past every descriptor of the f16kv kernels (one image's K or V < 2 GiB): the load returns zeros.
constexpr unsigned OUT_OF_RANGE = 0x80000000u;

__device__ __forceinline__ f16x8 pack8(f32x4 a, f32x4 b) {  // (fptrunc: round to nearest even)
    const f16x4 lo = __builtin_convertvector(a, f16x4);
    const f16x4 hi = __builtin_convertvector(b, f16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// (the token kernels hold their fragments as float4: as f32x4 from the load on, every instance compiled to other code)
// (written out, not a call of the form above: through the call the Q pack of two f16kv instances was scheduled differently)
__device__ __forceinline__ f16x8 pack8(float4 a, float4 b) {
    const f16x4 lo = __builtin_convertvector(f32x4{a.x, a.y, a.z, a.w}, f16x4);
    const f16x4 hi = __builtin_convertvector(f32x4{b.x, b.y, b.z, b.w}, f16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// (v_permlane32_swap a, b: a's lanes 32..63 <-> b's lanes 0..31; with a == b == v both end up holding a half of v twice, max(a, b)
//  is max(v[l], v[l ^ 32]) in every lane; v_permlane16_swap likewise for the odd / even rows of 16.  Inline asm: the clang builtin of
//  ROCm 7.2 returns its first result twice when both operands are copies of one value -- tools/probe/permlane_swap_probe.hip.)
__device__ __forceinline__ float max_over_rows(float v) {
#ifdef SIGE_ATTENTION_SHFL
    v = fmaxf(v, __shfl_xor(v, 32));
    return fmaxf(v, __shfl_xor(v, 16));
#else
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    a = fmaxf(a, b); b = a;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
#endif
}

// The weight of a partial softmax state with maximum m in a merge under the maximum M >= m (units of log2); a state that saw no
// key (m = -inf, where M may be -inf too) weighs nothing.
__device__ __forceinline__ float merge_weight(float m, float M) { return m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - M); }

// Stacked edits in the token kernels (sige_hip_attention_tokens_tiles_f32 / _f16c / _f16kv): the image of query tile `qtile` -- its origin row
// tiles[2 qtile] of the tall image >> log2 of one image's height, clamped into [0, images - 1] so that no index list can move the
// K / V descriptors outside k / v (the rule of attention_wide.hip).  The index is the same in every lane and made uniform: ONE
// scalar load per workgroup, a shift and two scalar min / max in front of the pointer arithmetic -- no branch, no division.
// TILES = false is the constant 0: the kernels compile to what they were.
template <bool TILES>
__device__ __forceinline__ int tile_image(const int32_t *__restrict__ tiles, int qtile, int img_shift, int images) {
    if constexpr (TILES) {
        const int row = __builtin_amdgcn_readfirstlane(tiles[2 * __builtin_amdgcn_readfirstlane(qtile)]);
        return min(max(row >> img_shift, 0), images - 1);
    } else {
        return 0;
    }
}

// Token kernels: workgroup -> (batch * head pair, query tile).  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs,
// each with its own 4 MB L2: with `xcd_pairs` > 0 (the host sets it when B * heads is a multiple of 8) the pairs are dealt to the XCDs
// -- pair = xcd * xcd_pairs + ... -- so that one L2 holds the K / V of ITS pairs (SD, 64 x 64 latent: 2 x 1.3 MB) instead of every
// L2 streaming all of them (16 x 1.3 MB: each key block re-read from the Infinity Cache by every XCD)
__device__ __forceinline__ void workgroup_pair_tile(int q_tiles, int xcd_pairs, int &pair, int &qtile) {
    if (xcd_pairs > 0) {
        const int id = blockIdx.x, xcd = id & 7, local = id >> 3;
        pair = xcd * xcd_pairs + local / q_tiles;
        qtile = local - (local / q_tiles) * q_tiles;
    } else {
        pair = blockIdx.x / q_tiles;
        qtile = blockIdx.x - pair * q_tiles;
    }
}

// ---- host ----

// The argument check of the six batched entries (row strides: the smallest of them, C where rows are dense).  true: there is a
// launch to make; false: *status is the entry's answer -- bad arguments, or no query and nothing to do.
inline bool attention_batch_args(int B, int Nq, int Nk, int C, int heads, int ld_min, const void *q, const void *k, const void *v,
                                 const void *out, int *status) {
    *status = SIGE_HIP_EINVAL;
    if (B < 0 || Nq < 0 || Nk <= 0 || C <= 0 || heads <= 0) return false;
    if (ld_min < C) return false;
    if ((long)B * Nq == 0) { *status = SIGE_HIP_OK; return false; }
    return q && k && v && out;
}

// The argument check of the six `_tiles_` entries in front of stacked_keys, in the order include/sige_hip.h states: sizes, row strides
// (as above), the empty list, null pointers -- the index list among them.  true: go on; false: *status is the entry's answer.
inline bool attention_tiles_args(int T, int H, int W, int C, int heads, int ld_min, const void *q, const void *k, const void *v,
                                 const void *out, const int32_t *active_indices, int *status) {
    *status = SIGE_HIP_EINVAL;
    if (T < 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return false;
    if (ld_min < C) return false;
    if (T == 0) { *status = SIGE_HIP_OK; return false; }
    return q && k && v && out && active_indices;
}

// Stacked edits (sige_hip_set_edit_batch) as a `_tiles_` entry sees them: the queries are the tokens of T active 4x4 tiles of the
// tall image [1,C,H,W] = `images` images of H / images rows, and tile t attends to the `Nk` keys of ITS image only -- one launch
// for the tiles of all edits, the per-edit tile counts never on the host.  shift 0 = no edit batch: one image, the launch of the
// batched entry, and `tiles` is nullptr -- the index list is not read.
struct StackedKeys {
    const int32_t *tiles;
    int shift, images, Nk;
};

inline int stacked_keys(const int32_t *active_indices, int T, int H, int W, StackedKeys *g) {
    const int s = stacked_shift(H);
    if (s < 0) return SIGE_HIP_EUNSUPPORTED;  // (one image's height: a power of two >= 4)
    const int E = s > 0 ? H >> s : 1;
    if ((long)T * 16 > 0x7fffffffL || (long)(H / E) * W > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    *g = StackedKeys{s > 0 ? active_indices : nullptr, s, E, (H / E) * W};
    return SIGE_HIP_OK;
}

}  // namespace sige
