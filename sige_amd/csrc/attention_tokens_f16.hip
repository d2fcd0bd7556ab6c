// attention_tokens (attention_tokens.hip, the transposed-score kernel) with fp16 OPERANDS on v_mfma_f32_16x16x32_f16: the attention of
// the library's f16 compute mode (fp16 operands, fp32 accumulation, fp32 tensors in memory).  Same launch shape and the same memory
// layouts as the fp32 form -- one workgroup per 16 queries of one (batch, head), four waves over the key steps round-robin, each with
// its own running (m, l, O), merged through LDS; the (batch, head) pairs dealt to the XCDs; K / V as branch-free buffer loads issued
// one step ahead; the row maximum over two v_permlane*_swap (attention_rows.hpp) -- only the operand path differs.
//
// Instruction and step: 16x16x32 (K = 32), 32 keys per wave and step.
//   * scores S^T = K Q^T: slot e of lane (kq, j) in 32-channel unit u is channel 16 (2u + (e >> 2)) + 4kq + (e & 3) of key j (A) and of
//     query j (B): the two halves of a fragment are two of the fp32 kernel's 16-byte loads -- 64 contiguous bytes per key and load, the
//     contraction index permuted identically on both sides --, rounded to fp16 and packed; a half-unit wholly past the head dimension
//     (channels 48 .. 63 at d = 40) is zeros on both sides and is not loaded.  One MFMA per unit and 16-key tile.  The accumulator gives
//     lane (kq, j) the scores of query j against keys 4kq + r of the tile, as in the fp32 kernel.
//   * values O^T = V^T P^T: the probabilities of TWO 16-key tiles fill the 8 B slots of a lane as they lie in the two accumulators --
//     slot e of lane (kq, j) is key key0 + 16 (e >> 2) + 4kq + (e & 3) -- and the A fragment V^T[row j][slot e] is loaded from that same
//     key.  P never goes through LDS.  Which channel row j of tile n IS is free as well: where the tile count is even, lane j takes VC = 2
//     or 4 consecutive channels of a key in one load (d = 160: five 8-byte loads per key slot in place of ten 4-byte ones) and the merge
//     stores them where they belong; an odd tile count (d = 40, 80) keeps one channel per load.  One MFMA per 16-channel tile of O and
//     32 keys.
//   Why not 16x16x16 (16 keys per step, the fp32 kernel's fragments as they are): at d = 40 a 32-key step costs 4 + 3 MFMAs here
//   against 6 + 6 there, and, more to the point once the matrix pipe is no longer the limit, the per-step vector work that does not
//   scale with the keys (two permlane swaps, the ballot, the rescale test, the loop) is paid once per 32 keys instead of once per 16.
//   The price is registers: the next step's operands in flight are 32 keys of K and V in fp32 (48 VGPRs at d = 40 against 24 in the
//   fp32 kernel) while the current step's live on as packed halves (28).  Resource numbers: DESIGN.md 5.21.
//   Measured (tools/attention_tokens_bench.py, profiles/attention_tokens_f16.jsonl; fp32 form -> this one): SD's self-attention at
//   64 x 64 (1 008 queries x 4 096 keys x 8 heads x 40, batch 2) 143.6 -> 117.2 us, 32 x 32 (d = 80) 26.2 -> 18.8, 16 x 16 (d = 160)
//   16.6 -> 14.8, the cross-attentions 8.8 -> 8.2 and 6.2 -> 5.4.  The matrix pipe is no longer the limit (7 MFMAs of ~16 cycles per
//   step and wave at d = 40); the loads are: with K[key j][32u + 8kq .. +7] per lane -- two 16-byte loads 32 bytes apart, the padded
//   channels 48 .. 63 loaded too -- the same kernel took 148.5 us, slower than fp32.
//
// Arithmetic (include/sige_hip.h states the contract): q, k, v rounded to nearest even to fp16 in registers (fptrunc -> v_cvt_pk_f16_f32 /
// v_cvt_f16_f32 under the default rounding mode; never v_cvt_pkrtz), fp32 score accumulation, fp32 scale in units of log2, fp32
// (m, l, alpha); P rounded to nearest even to fp16; O, l and the merge fp32.
// P is carried as exp2(s - m + 15), at most 2^15: a probability below 2^-14 is an fp16 subnormal with fewer bits the smaller it is.
// Subnormal operands DO arrive in this MFMA and survive the conversion (tools/probe/mfma_f16_subnormal_probe.hip, measured), so the
// scaling is not needed for them to count; it is kept because it costs one subtraction per step and everything down to 2^-29 then
// rounds with fp16's full 11 bits (`dust` of tests/attention_f16.py: error 1.3e-4 against the unscaled emulation's 1.3e-3).  l is summed
// from the same scaled, unrounded values: the factor 2^15 cancels in O / l, in the rescale and in the merge (every wave carries it).
#include "attention_rows.hpp"

namespace sige {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float P_SHIFT = 15.f;

__device__ __forceinline__ f16x8 pack8(float4 a, float4 b) {  // (fptrunc: round to nearest even)
    const f16x4 lo = __builtin_convertvector(f32x4{a.x, a.y, a.z, a.w}, f16x4);
    const f16x4 hi = __builtin_convertvector(f32x4{b.x, b.y, b.z, b.w}, f16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// N consecutive floats of a buffer in one load (dword-aligned offsets).  The result goes through ONE __builtin_bit_cast to a float
// vector: indexing the builtin's own return value -- x[1] of a b64 / b128 load -- compiles to a buffer_load_dword and undefined upper
// elements with the clang of ROCm 7.2.
template <int N>
__device__ __forceinline__ void load_row(float (&dst)[N], __amdgpu_buffer_rsrc_t r, int off) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    static_assert(N == 1 || N == 2 || N == 4, "load_row: 1, 2 or 4 floats");
    if constexpr (N == 1) {
        dst[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
    } else if constexpr (N == 2) {
        const f32x2 x = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
        dst[0] = x[0]; dst[1] = x[1];
    } else {
        const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
        dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2]; dst[3] = x[3];
    }
}

// TILES (stacked edits, sige_hip_attention_tokens_tiles_f16c): the keys of the query tile's own image, as in attention_tokens.hip
template <int U32, int DT, bool TILES = false>  // 32-channel units of the scores (d <= 32 * U32), 16-channel tiles of O (d <= 16 * DT)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DT <= 3 ? 4 : 1)))
void attention_tokens_f16_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                 float *__restrict__ out, int Nq, int Nk, int C, int heads, int d, float scale_log2e,
                                 int q_tiles, int xcd_pairs, const int32_t *__restrict__ tiles, int img_shift, int images) {
    constexpr int OS = DT * 16 + 4;  // padded row of the merge buffer (a multiple of 4 floats: 16-byte rows)
    // V: a lane loads VC consecutive channels of a key in ONE load, so row i of O^T's tile n = VC g + c is channel 16 VC g + VC i + c
    // (the rows of an MFMA's A operand may be any channels; the merge puts them back)
    // (three channels per 12-byte load at DT = 3 -- eight loads per step at d = 40 in place of 24 -- need 3-register tuples: tried,
    //  28 bytes of scratch under the 128 VGPRs of 4 waves / SIMD)
    constexpr int VC = DT % 4 == 0 ? 4 : DT % 2 == 0 ? 2 : 1, VG = DT / VC;
    __shared__ float m_lds[4][16], l_lds[4][4][16];
    extern __shared__ __attribute__((aligned(16))) float o_lds[];  // [4 waves][16 queries][OS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, j = lane & 15;
    int pair, qtile;  // (workgroup -> XCD: as in attention_tokens_kernel)
    if (xcd_pairs > 0) {
        const int id = blockIdx.x, xcd = id & 7, local = id >> 3;
        pair = xcd * xcd_pairs + local / q_tiles;
        qtile = local - (local / q_tiles) * q_tiles;
    } else {
        pair = blockIdx.x / q_tiles;
        qtile = blockIdx.x - pair * q_tiles;
    }
    const int head = pair % heads, b = pair / heads;
    const int q0 = qtile * 16;
    const size_t hoff = (size_t)head * d;
    const size_t kv0 = ((size_t)b + tile_image<TILES>(tiles, qtile, img_shift, images)) * Nk * C + hoff;
    const float *kb = k + kv0;
    const float *vb = v + kv0;

    // Q of this lane = the B operand of the scores: query j, slot e of unit u = channel 16 (2u + (e >> 2)) + 4kq + (e & 3) (zeros beyond d)
    f16x8 qh[U32];
    {
        const float *qb = q + ((size_t)b * Nq + q0 + j) * C + hoff;
#pragma unroll
        for (int u = 0; u < U32; ++u) {
            float4 t[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 16 * (2 * u + h) + 4 * kq;
                const float4 x = *reinterpret_cast<const float4 *>(qb + min(c, d - 4));
                t[h] = c < d ? x : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            qh[u] = pack8(t[0], t[1]);
        }
    }
    float m_run = -INFINITY, l_run = 0.f;  // of query j: the maximum over every key so far, the (scaled) sum over THIS lane's keys
    f32x4 o[DT];                           // o[VC g + c][r] = 2^15 O[query j][channel 16 VC g + VC (4kq + r) + c]
#pragma unroll
    for (int n = 0; n < DT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nks = (Nk + 31) / 32;
    // Branch-free buffer loads (see attention_tokens_kernel): a lane whose channels lie past d reads the next head's channels, the next
    // row's, or the zeros a buffer load returns past the end of this batch's [Nk, C] matrix; a lane whose key lies past Nk the last
    // key's.  What it reads is a finite fp16 value (the contract) that meets a ZERO on the other side of the product or lands in a
    // padded column of O that is never stored.
    // TILES: kb / vb and kv_bytes are those of the tile's IMAGE (Nk = one image's keys), so the tail mask, the clamps and the
    // out-of-range zeros are per image; past the last head of the last row of image e < E - 1 lie image e + 1's first channels, which
    // are past THIS descriptor's kv_bytes: zeros, as at the end of the tensor (attention_tokens.hip has the argument in full).
    const unsigned kv_bytes = (unsigned)(((size_t)Nk * C - hoff) * sizeof(float));
    const __amdgpu_buffer_rsrc_t r_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(kb), 0, kv_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(vb), 0, kv_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)C * (unsigned)sizeof(float);
    float4 kn[2][DT];       // the A operand of the scores, tile t, 16-channel unit c: key key0 + 16t + j, channels 16c + 4kq .. +3
    float vn[8][VG][VC];    // the A operand of O^T, slot e: V[key0 + 16 (e >> 2) + 4kq + (e & 3)][channels VC (16g + j) .. + VC - 1]
    auto fetch = [&](int step) {
        const int key0 = step * 32;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned ko = (unsigned)min(key0 + 16 * t + j, Nk - 1) * row_bytes + 16u * kq;
#pragma unroll
            for (int c = 0; c < DT; ++c)
                kn[t][c] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_k, (int)(ko + 64u * c), 0, 0));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned vo = (unsigned)min(key0 + 16 * (e >> 2) + 4 * kq + (e & 3), Nk - 1) * row_bytes + 4u * VC * j;
#pragma unroll
            for (int g = 0; g < VG; ++g) load_row<VC>(vn[e][g], r_v, (int)(vo + 64u * VC * g));
        }
    };
    if (wave < nks) fetch(wave);
    for (int step = wave; step < nks; step += 4) {
        const int key0 = step * 32;
        // this step's operands as packed halves; their fp32 registers then take the next step's loads
        f16x8 kh[2][U32], vh[DT];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int u = 0; u < U32; ++u)
                kh[t][u] = pack8(kn[t][2 * u], 2 * u + 1 < DT ? kn[t][2 * u + 1] : make_float4(0.f, 0.f, 0.f, 0.f));
        }
#pragma unroll
        for (int n = 0; n < DT; ++n) {
            const int g = n / VC, i = n % VC;
            vh[n] = pack8(make_float4(vn[0][g][i], vn[1][g][i], vn[2][g][i], vn[3][g][i]),
                          make_float4(vn[4][g][i], vn[5][g][i], vn[6][g][i], vn[7][g][i]));
        }
        fetch(min(step + 4, nks - 1));  // (past the end: the last step again -- a valid address, never used)
        // ---- S^T = K Q^T: s[t][r] = S[query j][key0 + 16t + 4kq + r] ----
        f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int u = 0; u < U32; ++u) {
#pragma unroll
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[t][u], qh[u], s[t], 0, 0, 0);
        }
        float sv[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sv[t][r] = s[t][r] * scale_log2e;  // (units of log2: exp(x) = exp2(x * log2 e))
        }
        if (key0 + 32 > Nk) {  // (wave-uniform: the tail step only)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sv[t][r] = key0 + 16 * t + 4 * kq + r < Nk ? sv[t][r] : -INFINITY;
            }
        }
        // ---- online softmax of query j ----
        const float mb = max_over_rows(fmaxf(fmaxf(fmaxf(sv[0][0], sv[0][1]), fmaxf(sv[0][2], sv[0][3])),
                                             fmaxf(fmaxf(sv[1][0], sv[1][1]), fmaxf(sv[1][2], sv[1][3]))));  // (finite: a step has a live key)
        if (__builtin_amdgcn_ballot_w64(mb > m_run) != 0) {  // (wave-uniform; once the maxima have settled no step enters)
            const float m_new = fmaxf(m_run, mb);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // (exp2(-inf) = 0 on the first step; 1 for an unchanged row)
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int n = 0; n < DT; ++n) { o[n][0] *= alpha; o[n][1] *= alpha; o[n][2] *= alpha; o[n][3] *= alpha; }
        }
        const float m_off = m_run - P_SHIFT;
        float4 pr[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
            pr[t] = make_float4(__builtin_amdgcn_exp2f(sv[t][0] - m_off), __builtin_amdgcn_exp2f(sv[t][1] - m_off),
                                __builtin_amdgcn_exp2f(sv[t][2] - m_off), __builtin_amdgcn_exp2f(sv[t][3] - m_off));
        l_run += ((pr[0].x + pr[0].y) + (pr[0].z + pr[0].w)) + ((pr[1].x + pr[1].y) + (pr[1].z + pr[1].w));
        // ---- O^T += V^T P^T: slot e of lane row kq contracts key key0 + 16 (e >> 2) + 4kq + (e & 3) on both sides ----
        const f16x8 ph = pack8(pr[0], pr[1]);
#pragma unroll
        for (int n = 0; n < DT; ++n) o[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[n], ph, o[n], 0, 0, 0);
    }

    // ---- merge the four waves' (m, l, O): as the fp32 kernel (the factor 2^15 is in every wave's l and O) ----
    float *ow = o_lds + (size_t)wave * 16 * OS;
    if (kq == 0) m_lds[wave][j] = m_run;
    l_lds[wave][kq][j] = l_run;
#pragma unroll
    for (int n = 0; n < DT; ++n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ow[j * OS + 16 * VC * (n / VC) + VC * (4 * kq + r) + n % VC] = o[n][r];
    }
    __syncthreads();
    // thread -> (query row, 4 consecutive channels)
    const int units_per_row = d / 4;
    for (int e = tid; e < 16 * units_per_row; e += 256) {
        const int row = e / units_per_row, c = (e - row * units_per_row) * 4;
        const float M = fmaxf(fmaxf(m_lds[0][row], m_lds[1][row]), fmaxf(m_lds[2][row], m_lds[3][row]));
        float L = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = m_lds[w][row];
            const float f = merge_weight(mw, M);  // (a wave without a key step: 0)
            L += f * ((l_lds[w][0][row] + l_lds[w][1][row]) + (l_lds[w][2][row] + l_lds[w][3][row]));
            const float4 ov = *reinterpret_cast<const float4 *>(o_lds + ((size_t)w * 16 + row) * OS + c);
            acc.x += f * ov.x; acc.y += f * ov.y; acc.z += f * ov.z; acc.w += f * ov.w;
        }
        const float inv = 1.0f / L;
        *reinterpret_cast<float4 *>(out + ((size_t)b * Nq + q0 + row) * C + hoff + c) =
            make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
}

}  // namespace sige

using namespace sige;

namespace sige {

// Both entry points (as launch_attention_tokens of attention_tokens.hip): Nk keys per batch, or with `tiles` (B = 1) per image.
static int launch_attention_tokens_f16(const float *q, const float *k, const float *v, int B, int Nq, int Nk, int C, int heads,
                                       float scale, float *out, const int32_t *tiles, int img_shift, int images, void *stream) {
    if (!sige_hip_attention_tokens_supported(Nq, Nk, C, heads)) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(q) || !al(k) || !al(v) || !al(out) || (size_t)Nk * C * sizeof(float) >= 0x7fffffffu) return SIGE_HIP_EUNSUPPORTED;
    const int d = C / heads;
    const int units = (d + 15) / 16;
    const float sl = scale * 1.44269504088896341f;
    hipStream_t st = as_stream(stream);
    const int pairs = B * heads, t16 = Nq / 16;
    if ((long)pairs * t16 > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    const int xp = pairs % 8 == 0 ? pairs / 8 : 0;
#define SIGE_ATT16_GO(U)                                                                                                        \
    do {                                                                                                                        \
        const size_t lds = (size_t)4 * 16 * (U * 16 + 4) * sizeof(float);                                                       \
        if (tiles) attention_tokens_f16_kernel<(U + 1) / 2, U, true><<<dim3(t16 * pairs), 256, lds, st>>>(q, k, v, out, Nq, Nk, C, heads, d, sl, t16, xp, tiles, img_shift, images); \
        else attention_tokens_f16_kernel<(U + 1) / 2, U><<<dim3(t16 * pairs), 256, lds, st>>>(q, k, v, out, Nq, Nk, C, heads, d, sl, t16, xp, tiles, img_shift, images); \
    } while (0)
    switch (units) {  // (the head sizes the fp32 entry takes)
        case 1: SIGE_ATT16_GO(1); break;
        case 2: SIGE_ATT16_GO(2); break;
        case 3: SIGE_ATT16_GO(3); break;
        case 4: SIGE_ATT16_GO(4); break;
        case 5: SIGE_ATT16_GO(5); break;
        case 6: SIGE_ATT16_GO(6); break;
        case 8: SIGE_ATT16_GO(8); break;
        case 10: SIGE_ATT16_GO(10); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
#undef SIGE_ATT16_GO
    return launch_status();
}

}  // namespace sige

extern "C" int sige_hip_attention_tokens_f16c(const float *q, const float *k, const float *v, int B, int Nq, int Nk, int C,
                                              int heads, float scale, float *out, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_tokens_f16c, q, k, v, B, Nq, Nk, C, heads, scale, out, stream);
    if (B < 0 || Nq < 0 || Nk <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if ((long)B * Nq == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out) return SIGE_HIP_EINVAL;
    return launch_attention_tokens_f16(q, k, v, B, Nq, Nk, C, heads, scale, out, nullptr, 0, 1, stream);
}

// Stacked edits: sige_hip_attention_tokens_tiles_f32 (attention_tokens.hip) with the arithmetic of the entry above.
extern "C" int sige_hip_attention_tokens_tiles_f16c(const float *q, const float *k, const float *v, const int32_t *active_indices,
                                                    int T, int H, int W, int C, int heads, float scale, float *out, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_tokens_tiles_f16c, q, k, v, active_indices, T, H, W, C, heads, scale, out, stream);
    if (T < 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if (T == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out || !active_indices) return SIGE_HIP_EINVAL;
    const int s = stacked_shift(H);
    if (s < 0) return SIGE_HIP_EUNSUPPORTED;  // (one image's height: a power of two >= 4)
    const int E = s > 0 ? H >> s : 1;
    if ((long)T * 16 > 0x7fffffffL || (long)(H / E) * W > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    return launch_attention_tokens_f16(q, k, v, 1, 16 * T, (H / E) * W, C, heads, scale, out, s > 0 ? active_indices : nullptr, s, E, stream);
}
