// The in-launch finish of a split reduction, device side: the coherent loads / stores of the partial results and the ticket that
// finds the last workgroup.  Five kernels finish this way (conv_mfma.hpp and conv_wide.hpp: K split; attention_wide.hip: key split;
// attention_fused.hip: key slices; conv_latent_head.hip: channel split); each keeps its own workspace layout, read-back loop and
// epilogue.  conv_mfma.hpp spells split_arrive_last()'s sequence out (its register allocation moved through the call: see there);
// what is said here holds for it word for word.  The host side -- the tickets and the workspace -- is split_pool.hip.
#pragma once
#include "common.hpp"

namespace sige {

// 4 / 16 bytes to / from the device's coherence point: relaxed agent-scope atomics (16 bytes = two 8-byte atomics), visible to every
// XCD without cache maintenance once they have completed.
__device__ __forceinline__ void coherent_store(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void coherent_store(float *p, float4 v) {
    unsigned long long *q = reinterpret_cast<unsigned long long *>(p);
    const unsigned long long lo = (unsigned long long)__builtin_bit_cast(unsigned, v.x) | ((unsigned long long)__builtin_bit_cast(unsigned, v.y) << 32);
    const unsigned long long hi = (unsigned long long)__builtin_bit_cast(unsigned, v.z) | ((unsigned long long)__builtin_bit_cast(unsigned, v.w) << 32);
    __hip_atomic_store(q, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float coherent_load(const float *p) { return __hip_atomic_load(const_cast<float *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float4 coherent_load4(const float *p) {
    unsigned long long *q = reinterpret_cast<unsigned long long *>(const_cast<float *>(p));
    const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float4(__builtin_bit_cast(float, (unsigned)lo), __builtin_bit_cast(float, (unsigned)(lo >> 32)),
                       __builtin_bit_cast(float, (unsigned)hi), __builtin_bit_cast(float, (unsigned)(hi >> 32)));
}

// The whole workgroup calls this after its coherent_store()s of one of the `ksplit` partial results of a unit (an output block, a
// query tile): true, for every thread alike, in the workgroup that arrives last -- the one that reads all `ksplit` slices back and
// runs the epilogue.  `cnt` is the unit's ticket (split_tickets), `lds_slot` any int of LDS the caller can spare here.
//
// Why this holds.  A relaxed agent-scope atomic store bypasses the write-back L2 of the workgroup's own XCD: when it has completed
// -- vmcnt has reached 0 -- the value is at the device's coherence point, and a relaxed agent-scope load of ANY XCD reads it from
// there.  So: every wave waits for its own stores (s_waitcnt vmcnt(0)), the barrier makes that true of the whole workgroup, and only
// then does thread 0 draw the ticket, itself an atomic at the coherence point.  The workgroup that draws ksplit - 1 therefore drew
// it after every other split's stores had completed, and its coherent_load*()s, issued after the second barrier, see them.  The
// HIP memory model asks for a release fence before the ticket and an acquire fence behind it; on this device they write back and
// invalidate the whole XCD's L2 in every workgroup -- measured: +11 us per launch -- for data that never was in that L2.  That makes
// this the one place of the library that sits outside the letter of the memory model, and
// tests/test_gpu_round4.py::test_ksplit_finish_stress_two_streams (split launches racing on two streams, bit for bit against the
// unsplit sums) is the test that stands behind it.
//
// The last workgroup puts the ticket back to 0: a ticket is zero between launches (split_pool.hip hands them out zeroed), and no
// launch has to clear one.
//
// The caller guarantees: every store of the partial result is a coherent_store() issued BEFORE the call (plain stores may still
// sit in the L2), and every read-back goes through coherent_load() / coherent_load4() (a plain load may hit a stale line).
// No wait, barrier or atomic below may be dropped or weakened.
__device__ __forceinline__ bool split_arrive_last(int32_t *cnt, int ksplit, int *lds_slot) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *lds_slot = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const bool last = __builtin_amdgcn_readfirstlane(*lds_slot) == ksplit - 1;  // (one value for the workgroup: a scalar branch)
    if (last && threadIdx.x == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    return last;
}

}  // namespace sige
