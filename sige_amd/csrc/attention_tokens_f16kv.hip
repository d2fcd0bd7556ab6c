// attention_tokens_f16 (attention_tokens_f16.hip: the transposed-score kernel on v_mfma_f32_16x16x32_f16) for K and V that are STORED
// as fp16: k, v are _Float16 [B,Nk,C] token matrices (heads as strides), q and out stay fp32.  The f16c kernel rounds every K / V
// element to fp16 each time it loads it; here the producer (kv_rows_f16.hip, or one .half() of the full pass) rounded it once, so
// this kernel reads half the bytes, converts nothing and takes its operands as they lie in memory.  Launch shape, state and launcher:
// attention_tokens_image.hpp; arithmetic: the contract of sige_hip_attention_tokens_f16c (include/sige_hip.h) with "k, v rounded to
// fp16" already done.  What is its own is the load path:
//
//   * scores S^T = K Q^T.  Slot e of lane (kq, j) in 32-channel unit u is channel 32u + 8kq + e of key j (A) and of query j (B): the
//     A fragment IS one 16-byte buffer load, used as the MFMA operand as it arrives; Q is permuted identically as it is packed.  (The
//     f16c kernel found this order slower in fp32 -- two loads 32 bytes apart --; in fp16 it is one load.)  A lane whose 8 channels lie
//     past the head (d = 40: unit 1, kq >= 1) loads from an offset past the descriptor's range: the hardware returns exact zeros, no
//     branch, and nothing of the neighbouring head -- whose bytes may be Inf or NaN for all this head knows -- reaches the product
//     (Q is zeroed there as well).  d % 8 == 0, so a lane's 8 channels are live or dead together.
//     Loads per 32-key step and lane: 2 U32 (d = 40: 4, d = 80: 6, d = 160: 10; the f16c kernel 6 / 10 / 20 plus as many conversions).
//   * values O^T = V^T P^T.  The probabilities of the two 16-key tiles fill the 8 B slots of a lane as they lie in the accumulators --
//     slot e of lane (kq, j) is key key0 + 16 (e >> 2) + 4kq + (e & 3) --, and the A fragment V^T[row j][slot e] comes from that key.
//     Which channel row j of tile n IS is free: the DT 16-channel tiles of O are cut, greedily, into groups of VC = 4, 2, 1 tiles, and
//     in a group lane j loads VC CONSECUTIVE halves of a key in one 8- / 4- / 2-byte load (rows j of the group's tiles are channels
//     base + VC j + c; the merge puts them back).  The loaded dwords hold one key and VC channels, a fragment dword two keys of one
//     channel: one v_perm_b32 per fragment dword transposes them (VC = 1: one v_lshl_or).  Dead rows (channels past d) load zeros
//     from out of range like the scores' dead lanes.
//     Loads per step and lane: 8 per group (d = 40: DT = 3 = 2 + 1, 16; d = 80: 5 = 4 + 1, 16; d = 160: 10 = 4 + 4 + 2, 24; the f16c
//     kernel 24 / 40 / 40), and 4 DT permutes in place of 4 DT conversions.
//     Rejected: padding d = 40 to one group of four (8 loads, but a fourth MFMA per step and 16 more LDS columns in the merge); 2-byte
//     d16 / d16_hi pairs that land packed (inline asm only: the compiler cannot count such a load in s_waitcnt).
//   * prefetch.  Nothing is converted, so the registers a load fills ARE the operand: K's fragments are reloaded for the wave's next
//     step right after the score MFMAs have issued, V's raw dwords right after the permutes, and stay in flight through the rest of
//     this step and the head of the next -- one register set, no copy: loads run one step ahead.  (Two sets, two steps ahead, were
//     not tried.)  Resources per instance: DESIGN.md 5.33.
//
// Branch-free buffer loads throughout; end of keys and end of batch as in the f16c kernel: a key past Nk is the last key (its scores
// are masked to -inf), the descriptor spans one batch's (TILES: one image's) [Nk, C] halves from this head's first channel on.
#include "attention_tokens_image.hpp"  // (the workgroup's place, the merge image, the launcher; attention_rows.hpp: pack8, P_SHIFT, OUT_OF_RANGE)

namespace sige {

// The greedy cut of DT tiles into groups of 4, 2, 1: group g's tile count, first tile, and the number of groups; the dwords a lane
// holds per key slot over all groups (a 2-byte load fills one)
constexpr int kv16_groups(int DT) { return DT / 4 + (DT % 4) / 2 + DT % 2; }
constexpr int kv16_vc(int DT, int g) { return g < DT / 4 ? 4 : (g == DT / 4 && DT % 4 >= 2) ? 2 : 1; }
constexpr int kv16_first(int DT, int g) { return g <= DT / 4 ? 4 * g : 4 * (DT / 4) + 2; }
constexpr int kv16_dwords(int DT) { return 2 * (DT / 4) + (DT % 4) / 2 + DT % 2; }
constexpr int kv16_dword0(int DT, int g) { return g <= DT / 4 ? 2 * g : 2 * (DT / 4) + 1; }

// One register set of a step's operands: K's fragments as loaded, V's dwords as loaded (key slot e, the groups one after the other)
template <int U32, int DT>
struct Kv16Set {
    u32x4 k[2][U32];
    unsigned v[8][kv16_dwords(DT)];
};

// TILES (stacked edits, sige_hip_attention_tokens_tiles_f16kv): the keys of the query tile's own image, as in attention_tokens.hip
template <int U32, int DT, bool TILES = false>  // 32-channel units of the scores (d <= 32 U32), 16-channel tiles of O (d <= 16 DT)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DT <= 3 ? 4 : 1)))
void attention_tokens_f16kv_kernel(const float *__restrict__ q, const _Float16 *__restrict__ k, const _Float16 *__restrict__ v,
                                   float *__restrict__ out, int Nq, int Nk, int C, int heads, int d, float scale_log2e,
                                   int q_tiles, int xcd_pairs, const int32_t *__restrict__ tiles, int img_shift, int images) {
    constexpr int OS = tokens_image_row(DT);
    constexpr int G = kv16_groups(DT);
    __shared__ float m_lds[4][16], l_lds[4][4][16];
    extern __shared__ __attribute__((aligned(16))) float o_lds[];  // [4 waves][16 queries][OS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, j = lane & 15;
    int pair, qtile;  // (workgroup -> XCD: attention_rows.hpp)
    workgroup_pair_tile(q_tiles, xcd_pairs, pair, qtile);
    const int head = pair % heads, b = pair / heads;
    const int q0 = qtile * 16;
    const size_t hoff = (size_t)head * d;
    const size_t kv0 = ((size_t)b + tile_image<TILES>(tiles, qtile, img_shift, images)) * Nk * C + hoff;

    // Q of this lane = the B operand of the scores: query j, slot e of unit u = channel 32u + 8kq + e (zeros beyond d)
    f16x8 qh[U32];
    {
        const float *qb = q + ((size_t)b * Nq + q0 + j) * C + hoff;
#pragma unroll
        for (int u = 0; u < U32; ++u) {
            const int c = 32 * u + 8 * kq;
            const float *p = qb + min(c, d - 8);
            const float4 x = *reinterpret_cast<const float4 *>(p), y = *reinterpret_cast<const float4 *>(p + 4);
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            qh[u] = pack8(c < d ? x : z, c < d ? y : z);
        }
    }
    float m_run = -INFINITY, l_run = 0.f;  // of query j: the maximum over every key so far, the (scaled) sum over THIS lane's keys
    f32x4 o[DT];                           // o[first_g + c][r] = 2^15 O[query j][channel 16 first_g + VC_g (4kq + r) + c]
#pragma unroll
    for (int n = 0; n < DT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nks = (Nk + 31) / 32;
    // TILES: both descriptors are those of the tile's IMAGE (Nk = one image's keys): the tail mask, the clamps and the out-of-range
    // zeros are per image (attention_tokens.hip has the argument in full)
    const unsigned kv_bytes = (unsigned)(((size_t)Nk * C - hoff) * sizeof(_Float16));
    const __amdgpu_buffer_rsrc_t r_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(k + kv0), 0, kv_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(v + kv0), 0, kv_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)C * (unsigned)sizeof(_Float16);
    // the column part of a lane's offsets: bytes into a key's row, or OUT_OF_RANGE where the lane's channels lie past the head
    // (row part < 2^31, so the sum neither wraps nor comes back into range)
    unsigned kcol[U32], vcol[G];
#pragma unroll
    for (int u = 0; u < U32; ++u) kcol[u] = 32 * u + 8 * kq < d ? 2u * (32 * u + 8 * kq) : OUT_OF_RANGE;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = 16 * kv16_first(DT, g) + kv16_vc(DT, g) * j;
        vcol[g] = c < d ? 2u * c : OUT_OF_RANGE;
    }
    auto fetch_k = [&](Kv16Set<U32, DT> &s, int step) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned ko = (unsigned)min(step * 32 + 16 * t + j, Nk - 1) * row_bytes;
#pragma unroll
            for (int u = 0; u < U32; ++u)
                s.k[t][u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r_k, (int)(ko + kcol[u]), 0, 0));
        }
    };
    auto fetch_v = [&](Kv16Set<U32, DT> &s, int step) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned vo = (unsigned)min(step * 32 + 16 * (e >> 2) + 4 * kq + (e & 3), Nk - 1) * row_bytes;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int w0 = kv16_dword0(DT, g), off = (int)(vo + vcol[g]);
                if (kv16_vc(DT, g) == 4) {
                    // (ONE bit_cast of the builtin's result: attention_tokens_f16.hip, load_row, says why)
                    const u32x2 x = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r_v, off, 0, 0));
                    s.v[e][w0] = x[0]; s.v[e][w0 + 1] = x[1];
                } else if (kv16_vc(DT, g) == 2) {
                    s.v[e][w0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_raw_buffer_load_b32(r_v, off, 0, 0));
                } else {
                    s.v[e][w0] = (unsigned)__builtin_bit_cast(unsigned short, __builtin_amdgcn_raw_buffer_load_b16(r_v, off, 0, 0));
                }
            }
        }
    };
    // One 32-key step on register set `s`, which is refilled for step `next` as its registers come free
    auto do_step = [&](Kv16Set<U32, DT> &s, int step, int next) {
        const int key0 = step * 32;
        // ---- S^T = K Q^T: sc[t][r] = S[query j][key0 + 16t + 4kq + r] ----
        f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int u = 0; u < U32; ++u) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
                sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.k[t][u]), qh[u], sc[t], 0, 0, 0);
        }
        fetch_k(s, next);
        float sv[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sv[t][r] = sc[t][r] * scale_log2e;  // (units of log2: exp(x) = exp2(x * log2 e))
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
        const f16x8 ph = pack8(pr[0], pr[1]);
        // ---- V's fragments: dword p of tile n = (slot 2p, slot 2p + 1) of the tile's channel, from the dwords (one key, VC channels) ----
        u32x4 vh[DT];
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int c = 0; c < kv16_vc(DT, g); ++c) {
                const int w = kv16_dword0(DT, g) + (c >> 1);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned lo = s.v[2 * p][w], hi = s.v[2 * p + 1][w];
                    vh[kv16_first(DT, g) + c][p] = kv16_vc(DT, g) == 1 ? (lo | (hi << 16))  // (a 2-byte load zero-extends)
                                                   : __builtin_amdgcn_perm(hi, lo, (c & 1) ? 0x07060302u : 0x05040100u);
                }
            }
        }
        fetch_v(s, next);
        // ---- O^T += V^T P^T: slot e of lane row kq contracts key key0 + 16 (e >> 2) + 4kq + (e & 3) on both sides ----
#pragma unroll
        for (int n = 0; n < DT; ++n) o[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vh[n]), ph, o[n], 0, 0, 0);
    };

    // (a refill past the wave's last step loads the last step again: a valid address, never used)
    Kv16Set<U32, DT> set;
    fetch_k(set, min(wave, nks - 1));
    fetch_v(set, min(wave, nks - 1));
    for (int step = wave; step < nks; step += 4) do_step(set, step, min(step + 4, nks - 1));

    // ---- merge the four waves' (m, l, O): as the f16c kernel (the factor 2^15 is in every wave's l and O) ----
    float *ow = o_lds + (size_t)wave * 16 * OS;
    if (kq == 0) m_lds[wave][j] = m_run;
    l_lds[wave][kq][j] = l_run;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int c = 0; c < kv16_vc(DT, g); ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ow[j * OS + 16 * kv16_first(DT, g) + kv16_vc(DT, g) * (4 * kq + r) + c] = o[kv16_first(DT, g) + c][r];
        }
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

// Both entry points (as launch_attention_tokens_f16 of attention_tokens_f16.hip): Nk keys per batch, or with `tiles` (B = 1) per image.
static int launch_attention_tokens_f16kv(const float *q, const _Float16 *k, const _Float16 *v, int B, int Nq, int Nk, int C, int heads,
                                         float scale, float *out, const int32_t *tiles, int img_shift, int images, void *stream) {
    // (d % 8 == 0: the tile counts of d = 8 .. 160)
    return launch_tokens(std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(), sizeof(_Float16), sige_hip_attention_tokens_f16kv_supported,
                         q, k, v, out, B, Nq, Nk, C, heads, scale, tiles, stream, [&](auto U, auto TILES, const TokensLaunch &l) -> void {
        constexpr int DT = decltype(U)::value;
        attention_tokens_f16kv_kernel<(DT + 1) / 2, DT, decltype(TILES)::value><<<dim3(l.t16 * l.pairs), 256, tokens_image_bytes(DT), l.st>>>(
            q, k, v, out, Nq, Nk, C, heads, l.d, l.scale_log2e, l.t16, l.xcd_pairs, tiles, img_shift, images);
    });
}

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_attention_tokens_f16kv_supported(int Nq, int Nk, int C, int heads) {
    return sige_hip_attention_tokens_supported(Nq, Nk, C, heads) && (C / heads) % 8 == 0;
}

extern "C" int sige_hip_attention_tokens_f16kv(const float *q, const void *k16, const void *v16, int B, int Nq, int Nk, int C,
                                               int heads, float scale, float *out, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_tokens_f16kv, q, k16, v16, B, Nq, Nk, C, heads, scale, out, stream);
    int status;
    if (!attention_batch_args(B, Nq, Nk, C, heads, C, q, k16, v16, out, &status)) return status;
    return launch_attention_tokens_f16kv(q, static_cast<const _Float16 *>(k16), static_cast<const _Float16 *>(v16), B, Nq, Nk, C, heads,
                                         scale, out, nullptr, 0, 1, stream);
}

// Stacked edits: sige_hip_attention_tokens_tiles_f16c (attention_tokens_f16.hip) on fp16-stored K / V.
extern "C" int sige_hip_attention_tokens_tiles_f16kv(const float *q, const void *k16, const void *v16, const int32_t *active_indices,
                                                     int T, int H, int W, int C, int heads, float scale, float *out, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_tokens_tiles_f16kv, q, k16, v16, active_indices, T, H, W, C, heads, scale, out, stream);
    int status;
    if (!attention_tiles_args(T, H, W, C, heads, C, q, k16, v16, out, active_indices, &status)) return status;
    StackedKeys g;
    if ((status = stacked_keys(active_indices, T, H, W, &g))) return status;
    return launch_attention_tokens_f16kv(q, static_cast<const _Float16 *>(k16), static_cast<const _Float16 *>(v16), 1, 16 * T, g.Nk, C,
                                         heads, scale, out, g.tiles, g.shift, g.images, stream);
}
