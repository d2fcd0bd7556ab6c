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

}  // namespace sige
