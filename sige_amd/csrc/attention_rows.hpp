// Shared by the transposed-score attention kernels (attention_tokens.hip, attention_tokens_f16.hip, attention_wide.hip): the row
// maximum -- lane (kq, j) holds scores of query j, the four lane rows kq of a query meet in two v_permlane*_swap -- and the weight
// of a partial softmax state in a merge.
#pragma once
#include "common.hpp"

namespace sige {

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

// Stacked edits in the token kernels (sige_hip_attention_tokens_tiles_f32 / _f16c): the image of query tile `qtile` -- its origin row
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

}  // namespace sige
