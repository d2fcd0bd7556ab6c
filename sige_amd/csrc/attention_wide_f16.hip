// attention_wide (attention_wide.hip: wide heads, 160 < d <= 512, one launch with the key split finished inside it) with fp16 OPERANDS
// on v_mfma_f32_16x16x32_f16: the wide-head attention of the library's f16 compute mode (fp16 operands, fp32 accumulation, fp32
// tensors in memory), built from the fp32 form the way attention_tokens_f16.hip was built from attention_tokens.hip.
//
// Kept from the fp32 form: the shape range and its predicate, a row stride per operand, one workgroup = 16 queries of one
// (batch, head) x one split of the keys, four waves with their own running (m, l, O) merged through ONE LDS slot, the split finish of
// split_finish.hpp (fp32 workspace slices in the SAME accumulator image, a ticket, the last workgroup adds them up in split order),
// K / V as branch-free clamped buffer loads through a register ring that runs across step boundaries, kernarg_touch, and -- under
// the template flag TILES -- the per-image keys of stacked edits.  The accumulator layout o[g][e][r'] is the fp32 kernel's, so the
// wave merge, the workspace image and the output stores are its code word for word.
//
// What differs is the operand path.  Step: 32 keys per wave (two 16-key tiles t = 0, 1), as in attention_tokens_f16.hip.
//   * Q stage: fp16 in LDS (16.6 KB at d = 512 in place of 33 KB; the LDS allocation is still the 33 KB merge image), laid out in
//     fragment order: the 8 halves of lane (kq, j) for 32-channel unit U -- slot e = channel 32U + 16 (e >> 2) + 4kq + (e & 3) of query
//     j -- are 16 contiguous bytes, ONE ds_read_b128 per MFMA B operand; zeros beyond d.
//   * scores S^T = K Q^T: a ring chunk is the fp32 kernel's K chunk of ONE 16-key tile -- K[key j][64c + 16uu + 4kq .. +3], uu = 0..3:
//     four 16-byte loads, 64 contiguous bytes per key and load instruction --; chunks uu = 2u', 2u' + 1 rounded and packed are the A
//     fragment of unit 2c + u' with the contraction index permuted exactly as Q's.  2 MFMAs per chunk (8 in the fp32 kernel ... per 16
//     keys and 64 channels: 16 x 16 x 4).  A 16-channel half-unit past d is ZERO on the K side too (its Q side is): what lies there
//     may be anything -- another operand's channels, padding -- and anything times zero is not zero for everything.
//   * values O^T = V^T P^T: a ring chunk is the fp32 kernel's V chunk -- V[key 16hf + 4kq + r][64g + 4j .. +3], r = 0..3 -- of one HALF
//     hf of the step; the two halves give every lane 8 keys x 4 channels, and component e of those 8 keys, rounded and packed, is the
//     A fragment of the tile whose row j is channel 64g + 4j + e.  The B fragment is the probabilities of the two score accumulators
//     as they lie: slot e of lane (kq, j) = key key0 + 16 (e >> 2) + 4kq + (e & 3) on both sides.  P never goes through LDS.  4 MFMAs
//     per 64 channels and 32 keys (32 in the fp32 kernel).
//   * the ring: wide_ring(G) chunks of 16 registers (the fp32 kernel's 4: fp16 products finish sooner, the loads do not), 4G chunks
//     per step, fp32 as loaded and packed to halves at their use.
//
// Arithmetic: the contract of sige_hip_attention_tokens_f16c (include/sige_hip.h), word for word -- q, k, v rounded to nearest even to fp16
// in registers (fptrunc; never v_cvt_pkrtz), fp32 scores scaled in fp32 in units of log2, fp32 (m, l, alpha), l from the unrounded
// probabilities, P carried as exp2(s - m + 15) and rounded to nearest even to fp16 (attention_tokens_f16.hip says why 15), O, the wave
// merge, the split merge and the division by l in fp32.  The factor 2^15 is in every wave's and every split's l and O alike.
// Resource numbers and times: DESIGN.md 5.28.
#include <algorithm>

#include "attention_rows.hpp"
#include "split_finish.hpp"

namespace sige {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float WIDE_P_SHIFT = 15.f;

struct WideF16Args {
    const float *q, *k, *v;
    float *out;
    float *ws;          // [units * ksplit][(4G + 1) * 64] float4: the splits' merged accumulator images (ksplit > 1)
    int32_t *tickets;   // one per (pair, query tile), zero between launches
    int ldq, ldk, ldv, ldo;
    int Nq, Nk, C, heads, d;
    int q_tiles, ksplit, split_steps;  // split s takes the 32-key steps [s * split_steps, (s + 1) * split_steps)
    float scale_log2e;
    const int32_t *tiles;  // TILES: the Gather's index list (sige_hip_attention_wide_tiles_f16c)
    int img_shift, images;
};

__device__ __forceinline__ f16x8 wide_pack8(f32x4 a, f32x4 b) {  // (fptrunc: round to nearest even)
    const f16x4 lo = __builtin_convertvector(a, f16x4);
    const f16x4 hi = __builtin_convertvector(b, f16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ring depth: the largest divisor of the 4G chunks of a step that is <= 8 (slots stay compile-time across steps)
constexpr int wide_f16_ring(int G) { return (2 * G) % 8 == 0 ? 8 : (2 * G) % 7 == 0 ? 7 : (2 * G) % 6 == 0 ? 6 : 5; }

template <int G, bool TILES>  // 64-channel groups covering the head dimension: 64 (G - 1) < d <= 64 G
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void attention_wide_f16_kernel(WideF16Args a) {
    kernarg_touch<sizeof(WideF16Args)>();
    constexpr int QSH = 64 * G + 8;            // padded row of the Q stage, in halves (16-byte rows)
    constexpr int SLOTS = 4 * G + 1;           // float4 per lane of an accumulator image: o[g][.][r'] at 4g + r', then (m, l)
    constexpr int NB = wide_f16_ring(G), CH = 4 * G;
    static_assert(CH % NB == 0 && NB >= 3 && 16 * QSH / 2 <= SLOTS * 256, "ring / LDS");
    __shared__ __attribute__((aligned(16))) float smem[SLOTS * 256];
    __shared__ int ticket_lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, j = lane & 15;
    const unsigned split = blockIdx.x, qtile = blockIdx.y, pair = blockIdx.z;
    const unsigned unit = pair * (unsigned)a.q_tiles + qtile;
    const unsigned b = pair / (unsigned)a.heads, head = pair - b * (unsigned)a.heads;
    const int q0 = (int)qtile * 16, d = a.d;
    const size_t hoff = (size_t)head * d;
    const int image = tile_image<TILES>(a.tiles, (int)qtile, a.img_shift, a.images);

    // ---- Q stage: 16 rows x 64 G channels as fp16 in fragment order, zeros beyond d (clamped address, load, mask) ----
    _Float16 *const qs = reinterpret_cast<_Float16 *>(smem);
    {
        const float *qb = a.q + ((size_t)b * a.Nq + q0) * a.ldq + hoff;
        for (int e = tid; e < 16 * 16 * G; e += 256) {
            const int row = e / (16 * G), c = (e - row * (16 * G)) * 4;
            const float4 t = *reinterpret_cast<const float4 *>(qb + (size_t)row * a.ldq + min(c, d - 4));
            const unsigned keep = c < d ? 0xffffffffu : 0u;  // (a mask, not a select: see attention_wide.hip)
            auto mk = [&](float x) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & keep); };
            // channel c = 32U + 16h + 4kq' + i  ->  half U * 32 + kq' * 8 + 4h + i of the row
            const int at = (c >> 5) * 32 + ((c & 15) >> 2) * 8 + ((c >> 4) & 1) * 4;
            *reinterpret_cast<f16x4 *>(qs + row * QSH + at) = __builtin_convertvector(f32x4{mk(t.x), mk(t.y), mk(t.z), mk(t.w)}, f16x4);
        }
    }
    __syncthreads();

    // the 32-key steps of this split: [ks0, ks1), dealt round-robin to the waves
    const int nks = (a.Nk + 31) / 32;
    const int ks0 = (int)split * a.split_steps, ks1 = min(nks, ks0 + a.split_steps);  // (host: every split has a step)

    float m_run = -INFINITY, l_run = 0.f;  // of query j: the maximum over every key so far, the (scaled) sum over THIS lane's keys
    f32x4 o[G][4];                         // o[g][e][r'] = 2^15 O[query j][channel 64g + 16kq + 4r' + e]
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[g][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // K / V of batch b (TILES: of the tile's image, B = 1), head `head`: valid bytes from the head's first channel of key 0 to the
    // end of the last key's C channels -- ONE image's keys; a read outside them returns the descriptor's zeros
    const size_t krow0 = ((size_t)b + (size_t)image) * a.Nk;
    const unsigned k_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldk + a.C - hoff) * sizeof(float));
    const unsigned v_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldv + a.C - hoff) * sizeof(float));
    const __amdgpu_buffer_rsrc_t r_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k + krow0 * a.ldk + hoff), 0, k_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v + krow0 * a.ldv + hoff), 0, v_bytes, 0x00020000);
    const int k_row = a.ldk * (int)sizeof(float), v_row = a.ldv * (int)sizeof(float);

    f32x4 ring[NB][4];
    // chunk cc of step `step`: cc < 2G: K[key 16t + j][64c + 16uu + 4kq .. +3], c = cc >> 1, t = cc & 1, uu = 0..3;
    //                          else:    V[key 16hf + 4kq + r][64g + 4j .. +3], g = (cc - 2G) >> 1, hf = cc & 1, r = 0..3.
    // A key past Nk (the tail step) reads the last key's row (its scores are masked, its P is 0); channels past d read the row's
    // next bytes or, beyond the tensor, the zeros of an out-of-range buffer load: K's are zeroed or skipped before the product,
    // V's land in columns of O that are never stored.
    auto fetch = [&](f32x4 (&dst)[4], const int cc, const int step) {
        const int key0 = step * 32;
        if (cc < 2 * G) {
            const int off = min(key0 + 16 * (cc & 1) + j, a.Nk - 1) * k_row + (64 * (cc >> 1) + 4 * kq) * (int)sizeof(float);
#pragma unroll
            for (int uu = 0; uu < 4; ++uu)
                dst[uu] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_k, off + 64 * uu, 0, 0));
        } else {
            const int cbytes = (64 * ((cc - 2 * G) >> 1) + 4 * j) * (int)sizeof(float);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                dst[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    r_v, min(key0 + 16 * (cc & 1) + 4 * kq + r, a.Nk - 1) * v_row + cbytes, 0, 0));
        }
    };

    const int first = ks0 + wave;
    if (first < ks1) {
        const int last = first + ((ks1 - 1 - first) / 4) * 4;  // this wave's last step
#pragma unroll
        for (int c = 0; c < NB - 1; ++c) fetch(ring[c], c, first);
        const _Float16 *qrow = qs + j * QSH + 8 * kq;
        for (int step = first; step < ks1; step += 4) {
            const int key0 = step * 32;
            const int nxt = min(step + 4, last);  // (past the end: the last step again -- valid addresses, never used)
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            // chunk c + NB - 1 goes into the slot chunk c - 1 has left (a V half waits in its slot for the other half: the pair is
            // used at the odd chunk, in front of that chunk's fetch)
            auto fetch_ahead = [&](const int c) {
                const int ahead = c + NB - 1;
                if (ahead < CH) fetch(ring[ahead % NB], ahead, step);
                else fetch(ring[ahead % NB], ahead - CH, nxt);
            };
            // (three loops, not one over the 4G chunks with the softmax inside: past ~16 000 estimated instructions #pragma unroll is
            //  not honoured, and a ring indexed at run time goes to LDS or scratch)
#pragma unroll
            for (int c = 0; c < 2 * G; ++c) {
                f32x4 (&cur)[4] = ring[c % NB];
                // ---- S^T = K Q^T: s[t][r] = S[query j][key0 + 16t + 4kq + r]; units past d skipped, half-units past d zeroed ----
                const int gc = c >> 1, t = c & 1;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int U = 2 * gc + u;
                    if (gc < G - 1 || 32 * U < d) {  // (wave-uniform; compile-time below the last group)
                        f32x4 hi = cur[2 * u + 1];
                        if (gc == G - 1 && 32 * U + 16 >= d) hi = f32x4{0.f, 0.f, 0.f, 0.f};
                        const f16x8 qv = *reinterpret_cast<const f16x8 *>(qrow + 32 * U);
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wide_pack8(cur[2 * u], hi), qv, s[t], 0, 0, 0);
                    }
                }
                fetch_ahead(c);
            }
            // ---- online softmax of query j (units of log2: exp(x) = exp2(x * log2 e)) ----
            float sv[2][4];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sv[tt][r] = s[tt][r] * a.scale_log2e;
            }
            if (key0 + 32 > a.Nk) {  // (wave-uniform: the tail step only)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sv[tt][r] = key0 + 16 * tt + 4 * kq + r < a.Nk ? sv[tt][r] : -INFINITY;
                }
            }
            const float mb = max_over_rows(fmaxf(fmaxf(fmaxf(sv[0][0], sv[0][1]), fmaxf(sv[0][2], sv[0][3])),
                                                 fmaxf(fmaxf(sv[1][0], sv[1][1]), fmaxf(sv[1][2], sv[1][3]))));  // (finite: a step has a live key)
            if (__builtin_amdgcn_ballot_w64(mb > m_run) != 0) {  // (wave-uniform; once the maxima have settled no step enters)
                const float m_new = fmaxf(m_run, mb);
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // (exp2(-inf) = 0 on the first step)
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int g = 0; g < G; ++g) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[g][e][0] *= alpha; o[g][e][1] *= alpha; o[g][e][2] *= alpha; o[g][e][3] *= alpha; }
                }
            }
            const float m_off = m_run - WIDE_P_SHIFT;
            f32x4 pr[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
                pr[tt] = f32x4{__builtin_amdgcn_exp2f(sv[tt][0] - m_off), __builtin_amdgcn_exp2f(sv[tt][1] - m_off),
                               __builtin_amdgcn_exp2f(sv[tt][2] - m_off), __builtin_amdgcn_exp2f(sv[tt][3] - m_off)};
            l_run += ((pr[0][0] + pr[0][1]) + (pr[0][2] + pr[0][3])) + ((pr[1][0] + pr[1][1]) + (pr[1][2] + pr[1][3]));
            const f16x8 ph = wide_pack8(pr[0], pr[1]);
#pragma unroll
            for (int c = 2 * G; c < CH; ++c) {
                f32x4 (&cur)[4] = ring[c % NB];
                if (c & 1) {
                    // ---- O^T += V^T P^T: slot e of lane row kq contracts key key0 + 16 (e >> 2) + 4kq + (e & 3) on both sides ----
                    const int g = (c - 2 * G) >> 1;
                    f32x4 (&lo)[4] = ring[(c - 1) % NB];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        o[g][e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            wide_pack8(f32x4{lo[0][e], lo[1][e], lo[2][e], lo[3][e]}, f32x4{cur[0][e], cur[1][e], cur[2][e], cur[3][e]}),
                            ph, o[g][e], 0, 0, 0);
                }
                fetch_ahead(c);
            }
        }
    }
    __syncthreads();  // (every wave is done with the Q stage)

    // ---- merge the four waves' (m, l, O) in registers through one LDS image: 3 -> 2, 1 -> 0, 2 -> 0 (attention_wide.hip) ----
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

    float *const orow = a.out + ((size_t)b * a.Nq + q0 + j) * a.ldo + hoff + 16 * kq;
    if (a.ksplit <= 1) {
        if (wave == 0) {
            const float inv = 1.0f / l_run;
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 64 * g + 16 * kq + 4 * r;
                    if (c < d) *reinterpret_cast<float4 *>(orow + 64 * g + 4 * r) =
                        make_float4(o[g][0][r] * inv, o[g][1][r] * inv, o[g][2][r] * inv, o[g][3][r] * inv);
                }
            }
        }
        return;
    }

    // ---- key split: this workgroup's image to its workspace slice, a ticket, the last split of the tile adds them up ----
    float4 *const ws = reinterpret_cast<float4 *>(a.ws) + (size_t)unit * a.ksplit * (SLOTS * 64);
    if (wave == 0) {
        float4 *mine = ws + (size_t)split * (SLOTS * 64);
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                coherent_store(reinterpret_cast<float *>(mine + (4 * g + r) * 64 + lane), make_float4(o[g][0][r], o[g][1][r], o[g][2][r], o[g][3][r]));
        }
        coherent_store(reinterpret_cast<float *>(mine + (SLOTS - 1) * 64 + lane), make_float4(m_run, l_run, 0.f, 0.f));
    }
    if (!split_arrive_last(a.tickets + unit, a.ksplit, &ticket_lds)) return;  // (the protocol: split_finish.hpp)
    // thread (wave, lane) -> slots wave, wave + 4, ... of lane `lane`; the slices in split order with a running maximum, four slices'
    // loads in flight at a time (attention_wide.hip)
    float M = -INFINITY, L = 0.f;
    float4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p0 = 0; p0 < a.ksplit; p0 += 4) {
        float4 ml[4], t[4][G];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 *src = ws + (size_t)min(p0 + u, a.ksplit - 1) * (SLOTS * 64);  // (past the end: the last slice again, not used)
            ml[u] = coherent_load4(reinterpret_cast<const float *>(src + (SLOTS - 1) * 64 + lane));
#pragma unroll
            for (int g = 0; g < G; ++g) t[u][g] = coherent_load4(reinterpret_cast<const float *>(src + (4 * g + wave) * 64 + lane));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p0 + u < a.ksplit) {  // (workgroup-uniform)
                const float Mn = fmaxf(M, ml[u].x);
                const float fo = merge_weight(M, Mn), fp = merge_weight(ml[u].x, Mn);
                M = Mn;
                L = fo * L + fp * ml[u].y;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    acc[g].x = fo * acc[g].x + fp * t[u][g].x; acc[g].y = fo * acc[g].y + fp * t[u][g].y;
                    acc[g].z = fo * acc[g].z + fp * t[u][g].z; acc[g].w = fo * acc[g].w + fp * t[u][g].w;
                }
            }
        }
    }
    const float inv = 1.0f / L;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = 64 * g + 16 * kq + 4 * wave;
        if (c < d) *reinterpret_cast<float4 *>(orow + 64 * g + 4 * wave) = make_float4(acc[g].x * inv, acc[g].y * inv, acc[g].z * inv, acc[g].w * inv);
    }
}

// Both entry points (as launch_attention_wide of attention_wide.hip): Nk keys per batch, or with `tiles` (B = 1) per image.
static int launch_attention_wide_f16(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv, int B, int Nq, int Nk, int C,
                                     int heads, float scale, float *out, int ldo, const int32_t *tiles, int img_shift, int images, void *stream) {
    if (!sige_hip_attention_wide_supported(Nq, Nk, C, heads)) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(q) || !al(k) || !al(v) || !al(out) || ((ldq | ldk | ldv | ldo) & 3)) return SIGE_HIP_EUNSUPPORTED;
    // (32-bit byte offsets into one batch's -- one image's -- K / V)
    if ((size_t)Nk * ldk * sizeof(float) >= 0x7fffffffu || (size_t)Nk * ldv * sizeof(float) >= 0x7fffffffu) return SIGE_HIP_EUNSUPPORTED;
    const int d = C / heads, G = (d + 63) / 64;
    const long units = (long)B * heads * (Nq / 16);
    if ((long)B * heads > 65535 || Nq / 16 > 65535) return SIGE_HIP_EUNSUPPORTED;  // (grid z / y)
    hipStream_t st = as_stream(stream);

    // key split: about one workgroup per CU in all, at least 4 steps (one per wave) per split, at most 16 slices to add up
    const int nks = (Nk + 31) / 32;
    int ksplit = (int)std::min<long>(std::min<long>(256 / units, nks / 4), 16);
    WideF16Args a;
    a.ws = nullptr; a.tickets = nullptr;
    if (ksplit > 1) {
        a.tickets = split_tickets(st, units);
        if (a.tickets) a.ws = split_workspace(st, (size_t)units * ksplit * (4 * G + 1) * 256);
        if (!a.tickets || !a.ws) ksplit = 1;
    }
    if (ksplit < 1) ksplit = 1;
    a.split_steps = (nks + ksplit - 1) / ksplit;
    ksplit = (nks + a.split_steps - 1) / a.split_steps;  // (no empty split)
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.Nq = Nq; a.Nk = Nk; a.C = C; a.heads = heads; a.d = d;
    a.q_tiles = Nq / 16; a.ksplit = ksplit;
    a.scale_log2e = scale * 1.44269504088896341f;
    a.tiles = tiles; a.img_shift = img_shift; a.images = images;
    const dim3 grid((unsigned)ksplit, (unsigned)(Nq / 16), (unsigned)(B * heads));
#define SIGE_WIDE16_GO(GG)                                                                     \
    do {                                                                                       \
        if (tiles) attention_wide_f16_kernel<GG, true><<<grid, 256, 0, st>>>(a);               \
        else attention_wide_f16_kernel<GG, false><<<grid, 256, 0, st>>>(a);                    \
    } while (0)
    switch (G) {
        case 3: SIGE_WIDE16_GO(3); break;
        case 4: SIGE_WIDE16_GO(4); break;
        case 5: SIGE_WIDE16_GO(5); break;
        case 6: SIGE_WIDE16_GO(6); break;
        case 7: SIGE_WIDE16_GO(7); break;
        case 8: SIGE_WIDE16_GO(8); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
#undef SIGE_WIDE16_GO
    return launch_status();
}

}  // namespace sige

using namespace sige;

// the key split of a launch whose pools have room (the formula of launch_attention_wide_f16; tests)
extern "C" int sige_hip_attention_wide_f16c_splits(int B, int Nq, int Nk, int C, int heads) {
    if (B <= 0 || !sige_hip_attention_wide_supported(Nq, Nk, C, heads)) return 0;
    const long units = (long)B * heads * (Nq / 16);
    const int nks = (Nk + 31) / 32;
    int ksplit = (int)std::min<long>(std::min<long>(256 / units, nks / 4), 16);
    if (ksplit < 1) ksplit = 1;
    const int steps = (nks + ksplit - 1) / ksplit;
    return (nks + steps - 1) / steps;
}

extern "C" int sige_hip_attention_wide_f16c(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                            int B, int Nq, int Nk, int C, int heads, float scale, float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_f16c, q, ldq, k, ldk, v, ldv, B, Nq, Nk, C, heads, scale, out, ldo, stream);
    if (B < 0 || Nq < 0 || Nk <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return SIGE_HIP_EINVAL;
    if ((long)B * Nq == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out) return SIGE_HIP_EINVAL;
    return launch_attention_wide_f16(q, ldq, k, ldk, v, ldv, B, Nq, Nk, C, heads, scale, out, ldo, nullptr, 0, 1, stream);
}

// Stacked edits: sige_hip_attention_wide_tiles_f32 (attention_wide.hip) with the arithmetic of the entry above.
extern "C" int sige_hip_attention_wide_tiles_f16c(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                                  const int32_t *active_indices, int T, int H, int W, int C, int heads, float scale,
                                                  float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_tiles_f16c, q, ldq, k, ldk, v, ldv, active_indices, T, H, W, C, heads, scale, out, ldo, stream);
    if (T < 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return SIGE_HIP_EINVAL;
    if (T == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out || !active_indices) return SIGE_HIP_EINVAL;
    const int s = stacked_shift(H);
    if (s < 0) return SIGE_HIP_EUNSUPPORTED;  // (one image's height: a power of two >= 4)
    const int E = s > 0 ? H >> s : 1;         // (shift 0 = no edit batch: one image -- the other entry's launch)
    if ((long)T * 16 > 0x7fffffffL || (long)(H / E) * W > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    return launch_attention_wide_f16(q, ldq, k, ldk, v, ldv, 1, 16 * T, (H / E) * W, C, heads, scale, out, ldo,
                                     s > 0 ? active_indices : nullptr, s, E, stream);
}
