// What the two wide-head attention units (attention_wide.hip: fp32 operands, 16 keys per step; attention_wide_f16.hip: fp16 operands,
// 32 keys per step) share behind and around the operand path: the kernel's arguments, the accumulator image, the merge of the four
// waves through ONE LDS image, a split's image to its workspace slice (split_finish.hpp), and on the host the key split and the
// launch plan.  (The output stores, the read-back of the slices by the last split and the K / V descriptor pair stay in each kernel:
// as functions of this header they moved the scalar code or the register allocation of every instance --
// profiles/attention_one_home_isa.txt is taken with them where they are.)
//
// The contract between an operand path and this header is the accumulator layout of a lane (kq, j) = (lane >> 4, lane & 15):
//   o[g][e][r'] = O[query j][channel 64g + 16kq + 4r' + e]   (g < G 64-channel groups, e, r' < 4),
//   m_run = the maximum of query j over every key the wave has seen (units of log2), l_run = the sum over THIS lane's keys.
// (The f16 form carries 2^15 O and 2^15 l: the factor is in every wave's and every split's state alike and cancels in O / l.)
// An accumulator IMAGE is SLOTS = 4G + 1 float4 per lane: slot 4g + r' = o[g][0..3][r'] -- 4 consecutive channels --, then (m, l, 0, 0);
// slot s of lane l lies at float4 index 64 s + l, in LDS and in a workspace slice alike.
#pragma once
#include <algorithm>

#include "attention_rows.hpp"
#include "split_finish.hpp"

namespace sige {

// (k, v, ldk, ldv: fp32 pointers and strides in floats for the two units named above.  attention_wide_f16kv.hip passes fp16
// tensors through these same fields -- the pointers cast, the strides in HALVES -- and its kernel casts them back; nothing in this
// header dereferences k or v, and wide_plan's 2 GiB test then counts a half as four bytes: stricter than needed, never laxer.)
struct WideAttnArgs {
    const float *q, *k, *v;
    float *out;
    float *ws;          // [units * ksplit][(4G + 1) * 64] float4: the splits' merged accumulator images (ksplit > 1)
    int32_t *tickets;   // one per (pair, query tile), zero between launches
    int ldq, ldk, ldv, ldo;
    int Nq, Nk, C, heads, d;
    int q_tiles, ksplit, split_len;  // split s takes the key steps [s * split_len, (s + 1) * split_len): steps of the including
                                     // kernel, 16 keys (fp32) or 32 (f16)
    float scale_log2e;
    // per-image keys (the `_tiles_` entries; stacked edits): query tile t is the 4x4 tile with origin row tiles[2t] of the tall
    // image, its keys are the Nk rows of image tiles[2t] >> img_shift.  nullptr: every tile reads the keys of image 0.
    const int32_t *tiles;
    int img_shift, images;
};

constexpr int wide_slots(int G) { return 4 * G + 1; }  // float4 per lane of an accumulator image

// ---- the four waves' (m, l, O) merged in registers through one LDS image: 3 -> 2, 1 -> 0, 2 -> 0 (33 KB at d = 512 instead of the
// 132 KB of four images side by side).  Every wave has left the LDS the image takes; wave 0 ends with the merged state, its l_run
// the sum of query j over the four lane rows. ----
template <int G>
__device__ __forceinline__ void wide_merge_waves(float *smem, int wave, int lane, f32x4 (&o)[G][4], float &m_run, float &l_run) {
    constexpr int SLOTS = wide_slots(G);
    float4 *img = reinterpret_cast<float4 *>(smem);
    auto put = [&]() {
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) img[(4 * g + r) * 64 + lane] = make_float4(o[g][0][r], o[g][1][r], o[g][2][r], o[g][3][r]);
        }
        img[(SLOTS - 1) * 64 + lane] = make_float4(m_run, l_run, 0.f, 0.f);
    };
    auto take = [&]() {
        const float4 ml = img[(SLOTS - 1) * 64 + lane];
        const float M = fmaxf(m_run, ml.x);
        const float f1 = merge_weight(m_run, M), f2 = merge_weight(ml.x, M);  // (a wave without a key step: weight 0)
        m_run = M;
        l_run = f1 * l_run + f2 * ml.y;
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 t = img[(4 * g + r) * 64 + lane];
                o[g][0][r] = f1 * o[g][0][r] + f2 * t.x;
                o[g][1][r] = f1 * o[g][1][r] + f2 * t.y;
                o[g][2][r] = f1 * o[g][2][r] + f2 * t.z;
                o[g][3][r] = f1 * o[g][3][r] + f2 * t.w;
            }
        }
    };
    if (wave == 3) put();
    __syncthreads();
    if (wave == 2) take();
    __syncthreads();
    if (wave == 1) put();
    __syncthreads();
    if (wave == 0) take();
    __syncthreads();
    if (wave == 2) put();
    __syncthreads();
    if (wave == 0) {
        take();
        // the sum of query j over its four lane rows
        l_run += __shfl_xor(l_run, 16);
        l_run += __shfl_xor(l_run, 32);
    }
}

// ---- key split: wave 0's merged image to this workgroup's workspace slice `mine`, as device-coherent stores (split_finish.hpp) ----
template <int G>
__device__ __forceinline__ void wide_publish(float4 *mine, int lane, const f32x4 (&o)[G][4], float m_run, float l_run) {
    constexpr int SLOTS = wide_slots(G);
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            coherent_store(reinterpret_cast<float *>(mine + (4 * g + r) * 64 + lane), make_float4(o[g][0][r], o[g][1][r], o[g][2][r], o[g][3][r]));
    }
    coherent_store(reinterpret_cast<float *>(mine + (SLOTS - 1) * 64 + lane), make_float4(m_run, l_run, 0.f, 0.f));
}

// ---- host ----

// The key split of `units` (pair, query tile) units over `steps` key steps: about one workgroup per CU in all, at least 4 steps (one
// per wave) per split, at most 16 slices to add up -- and no empty split: the count is re-divided by the steps a split takes.
inline int wide_key_split(long units, int steps) {
    const int ksplit = (int)std::max<long>(std::min<long>(std::min<long>(256 / units, steps / 4), 16), 1);
    const int len = (steps + ksplit - 1) / ksplit;
    return (steps + len - 1) / len;
}

// A launch of either form: the kernel's arguments, the 64-channel groups G that select the instance, the grid (split, query tile,
// (batch, head) pair) and the stream.
struct WidePlan {
    WideAttnArgs a;
    int G;
    dim3 grid;
    hipStream_t st;
};

// Both entry points of both forms: q [B,Nq,ldq] against k / v of Nk keys per batch -- or, with `tiles` (B = 1), per image of
// 2^img_shift rows.  `step_keys`: the keys of one step of the form's main loop.  Without tickets or workspace (first use inside a
// capture, regions exhausted): one split.
inline int wide_plan(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv, int B, int Nq, int Nk, int C, int heads,
                     float scale, float *out, int ldo, const int32_t *tiles, int img_shift, int images, void *stream, int step_keys,
                     WidePlan *p) {
    if (!sige_hip_attention_wide_supported(Nq, Nk, C, heads)) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *x) { return (reinterpret_cast<uintptr_t>(x) & 15) == 0; };
    if (!al(q) || !al(k) || !al(v) || !al(out) || ((ldq | ldk | ldv | ldo) & 3)) return SIGE_HIP_EUNSUPPORTED;
    // (32-bit byte offsets into one batch's -- one image's -- K / V)
    if ((size_t)Nk * ldk * sizeof(float) >= 0x7fffffffu || (size_t)Nk * ldv * sizeof(float) >= 0x7fffffffu) return SIGE_HIP_EUNSUPPORTED;
    const int d = C / heads;
    const long units = (long)B * heads * (Nq / 16);
    if ((long)B * heads > 65535 || Nq / 16 > 65535) return SIGE_HIP_EUNSUPPORTED;  // (grid z / y)
    p->G = (d + 63) / 64;
    p->st = as_stream(stream);

    const int steps = (Nk + step_keys - 1) / step_keys;
    int ksplit = wide_key_split(units, steps);
    WideAttnArgs &a = p->a;
    a.ws = nullptr; a.tickets = nullptr;
    if (ksplit > 1) {
        a.tickets = split_tickets(p->st, units);
        if (a.tickets) a.ws = split_workspace(p->st, (size_t)units * ksplit * wide_slots(p->G) * 256);
        if (!a.tickets || !a.ws) ksplit = 1;
    }
    a.split_len = (steps + ksplit - 1) / ksplit;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.Nq = Nq; a.Nk = Nk; a.C = C; a.heads = heads; a.d = d;
    a.q_tiles = Nq / 16; a.ksplit = ksplit;
    a.scale_log2e = scale * 1.44269504088896341f;
    a.tiles = tiles; a.img_shift = img_shift; a.images = images;
    p->grid = dim3((unsigned)ksplit, (unsigned)(Nq / 16), (unsigned)(B * heads));
    return SIGE_HIP_OK;
}

}  // namespace sige
