// attention_wide_f16 (attention_wide_f16.hip: wide heads, 160 < d <= 512, fp16 operands on v_mfma_f32_16x16x32_f16, one launch with
// the key split finished inside it) for K and V that are STORED as fp16: k, v are _Float16 token matrices with a row stride each
// (heads as strides; the two column halves of one [B,Nk,2C] tensor), q and out stay fp32.  The f16c kernel pulls K and V as fp32 and
// rounds every element each time it arrives; here the producer (kv_rows_f16.hip: sige_hip_kv_tiles_store_f16, or one whole-tensor
// rounded copy) rounded it once, so a workgroup reads half the bytes, converts nothing, and the registers a load fills ARE the MFMA
// operand -- the step attention_tokens_f16kv.hip took from attention_tokens_f16.hip.
//
// Kept from the f16c form (attention_wide_image.hpp): the shape range and its predicate, a row stride per operand, one workgroup =
// 16 queries of one (batch, head) x one split of the keys, four waves round-robin over 32-key steps with their own (m, l, O), the
// accumulator image o[g][e][r'], wide_merge_waves, wide_publish, split_arrive_last and the split finish, wide_plan / wide_key_split
// (the key split is the f16c launch's: sige_hip_attention_wide_f16c_splits), TILES for stacked edits, kernarg_touch.
//
// The operand path:
//   * Q stage: fp16 in LDS in NATURAL channel order, zeros beyond d (a padded row of 64 G + 8 halves): slot e of lane (kq, j) in
//     32-channel unit U is channel 32U + 8kq + e of query j -- 16 contiguous bytes, one ds_read_b128 per MFMA B operand.
//   * scores S^T = K Q^T: the A fragment of unit U is ONE 16-byte buffer load of the 8 consecutive halves 32U + 8kq .. + 7 of key j,
//     used as it arrives (the f16c kernel: two fp32 loads 64 bytes apart and a pack8).  A lane whose 8 channels lie past the
//     head (d % 32 == 16: the last live unit's kq >= 2; d % 64 <= 32: the whole last unit) loads from an offset past the descriptor:
//     the hardware returns exact zeros, no branch, and nothing that lies behind the head -- the next head's channels, the V half of
//     a K | V row, Inf or NaN for all this head knows -- reaches the product.  Only the last group's two units can be dead, so two
//     lane registers hold their column offsets; every other unit's is an immediate.
//   * values O^T = V^T P^T: lane (kq, j) loads the 4 CONSECUTIVE halves 64g + 4j .. + 3 of key key0 + 16hf + 4kq + r (one 8-byte
//     load; a row of 16 lanes is 128 contiguous bytes of the key).  The two dwords hold one key and 4 channels, a fragment dword two
//     keys of one channel: one v_perm_b32 per fragment dword transposes them in registers (the scheme of attention_tokens_f16kv.hip,
//     VC = 4), and channel e of the lane's 8 keys is the A fragment of the tile whose row j is channel 64g + 4j + e -- the f16c
//     kernel's tiles, so the accumulator image is unchanged.  An LDS transposed read would put V through the LDS the Q stage and
//     the merge image share and add a barrier per step; the permutes run on the VALU under the MFMAs.  Lanes past d load zeros
//     from out of range like the scores'.  P stays in registers as the B operand: slot e = key key0 + 16 (e >> 2) + 4kq + (e & 3).
//   * the ring: a chunk is 8 registers -- K: the two units of one 64-channel group and one 16-key tile; V: one half-step's four
//     keys of one group --, half the f16c chunk, 4G chunks per step.  Nothing is converted at use, so a chunk's registers are free
//     the moment its MFMAs (K) or permutes (V) have issued: the depth is the largest divisor of 4G up to 16 (G = 3: 12, 4: 16,
//     5: 10, 6: 12, 7: 14, 8: 16), at most the 128 registers of the f16c ring but TWICE its keys-times-channels in flight.  Slots
//     are compile-time (three unrolled loops per step, as in the f16c kernel).
// Arithmetic: the contract of sige_hip_attention_tokens_f16c with "k, v rounded to fp16" already done in memory -- q and P rounded
// to nearest even (fptrunc), fp32 scores scaled in units of log2, fp32 (m, l, alpha), l from the unrounded probabilities, P carried
// as exp2(s - m + 15), O, both merges and the division in fp32.  Resource numbers and times: DESIGN.md 5.34 (as compiled, the wait at
// the head of the score loop is vmcnt(0): the ring drains once per step; what that costs is not measured).
#include "attention_wide_image.hpp"

namespace sige {

// (f16x8 / u32x4, pack8, P_SHIFT, OUT_OF_RANGE: attention_rows.hpp)

// ring depth: the largest divisor of the 4G chunks of a step that is <= 16 (slots stay compile-time across steps)
constexpr int wide_kv16_ring(int G) { return 4 * G <= 16 ? 4 * G : 2 * G; }

template <int G, bool TILES>  // 64-channel groups covering the head dimension: 64 (G - 1) < d <= 64 G
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void attention_wide_f16kv_kernel(WideAttnArgs a) {
    kernarg_touch<sizeof(WideAttnArgs)>();
    constexpr int QSH = 64 * G + 8;            // padded row of the Q stage, in halves (16-byte rows)
    constexpr int SLOTS = wide_slots(G);       // float4 per lane of an accumulator image (the merge reuses the Q stage's LDS)
    constexpr int NB = wide_kv16_ring(G), CH = 4 * G;
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

    // ---- Q stage: 16 rows x 64 G channels as fp16 in channel order, zeros beyond d (clamped address, load, mask) ----
    _Float16 *const qs = reinterpret_cast<_Float16 *>(smem);
    {
        const float *qb = a.q + ((size_t)b * a.Nq + q0) * a.ldq + hoff;
        for (int e = tid; e < 16 * 16 * G; e += 256) {
            const int row = e / (16 * G), c = (e - row * (16 * G)) * 4;
            const float4 t = *reinterpret_cast<const float4 *>(qb + (size_t)row * a.ldq + min(c, d - 4));
            const unsigned keep = c < d ? 0xffffffffu : 0u;  // (a mask, not a select: see attention_wide.hip)
            auto mk = [&](float x) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & keep); };
            *reinterpret_cast<f16x4 *>(qs + row * QSH + c) = __builtin_convertvector(f32x4{mk(t.x), mk(t.y), mk(t.z), mk(t.w)}, f16x4);
        }
    }
    __syncthreads();

    // the 32-key steps of this split: [ks0, ks1), dealt round-robin to the waves
    const int nks = (a.Nk + 31) / 32;
    const int ks0 = (int)split * a.split_len, ks1 = min(nks, ks0 + a.split_len);  // (host: every split has a step)

    float m_run = -INFINITY, l_run = 0.f;  // of query j: the maximum over every key so far, the (scaled) sum over THIS lane's keys
    f32x4 o[G][4];                         // o[g][e][r'] = 2^15 O[query j][channel 64g + 16kq + 4r' + e] (attention_wide_image.hpp)
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[g][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // K / V of batch b (TILES: of the tile's image, B = 1), head `head`, as halves: valid bytes from the head's first channel of key
    // 0 to the end of the last key's C channels -- ONE image's keys; a read outside them returns the descriptor's zeros
    const _Float16 *const k16 = reinterpret_cast<const _Float16 *>(a.k), *const v16 = reinterpret_cast<const _Float16 *>(a.v);
    const size_t krow0 = ((size_t)b + (size_t)image) * a.Nk;
    const unsigned k_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldk + a.C - hoff) * sizeof(_Float16));
    const unsigned v_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldv + a.C - hoff) * sizeof(_Float16));
    const __amdgpu_buffer_rsrc_t r_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(k16 + krow0 * a.ldk + hoff), 0, k_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(v16 + krow0 * a.ldv + hoff), 0, v_bytes, 0x00020000);
    const unsigned k_row = (unsigned)a.ldk * (unsigned)sizeof(_Float16), v_row = (unsigned)a.ldv * (unsigned)sizeof(_Float16);
    // the column part of a lane's offsets in the LAST group, bytes into a key's row, or OUT_OF_RANGE where the lane's channels
    // lie past the head (row part < 2^31: the sum neither wraps nor comes back into range); below the last group every channel is live
    unsigned k_last[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = 32 * (2 * G - 2 + u) + 8 * kq;
        k_last[u] = c < d ? 2u * c : OUT_OF_RANGE;
    }
    const unsigned v_last = 64 * (G - 1) + 4 * j < d ? 2u * (64 * (G - 1) + 4 * j) : OUT_OF_RANGE;

    unsigned ring[NB][8];
    // chunk cc of step `step`: cc < 2G: K[key 16t + j][32 (2c + u) + 8kq .. +7], c = cc >> 1, t = cc & 1, u = 0, 1 -> dwords 4u .. 4u + 3;
    //                          else:    V[key 16hf + 4kq + r][64g + 4j .. +3], g = (cc - 2G) >> 1, hf = cc & 1, r = 0..3 -> dwords 2r, 2r + 1.
    // A key past Nk (the tail step) reads the last key's row (its scores are masked, its P is 0).
    auto fetch = [&](unsigned (&dst)[8], const int cc, const int step) {
        const int key0 = step * 32;
        if (cc < 2 * G) {
            const int c = cc >> 1;
            const unsigned row = (unsigned)min(key0 + 16 * (cc & 1) + j, a.Nk - 1) * k_row;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const unsigned off = row + (c < G - 1 ? 16u * kq + 64u * (2 * c + u) : k_last[u]);
                const u32x4 x = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r_k, (int)off, 0, 0));
                dst[4 * u] = x[0]; dst[4 * u + 1] = x[1]; dst[4 * u + 2] = x[2]; dst[4 * u + 3] = x[3];
            }
        } else {
            const int g = (cc - 2 * G) >> 1;
            const unsigned col = g < G - 1 ? 128u * g + 8u * j : v_last;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned off = (unsigned)min(key0 + 16 * (cc & 1) + 4 * kq + r, a.Nk - 1) * v_row + col;
                const u32x2 x = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r_v, (int)off, 0, 0));
                dst[2 * r] = x[0]; dst[2 * r + 1] = x[1];
            }
        }
    };

    const int first = ks0 + wave;
    if (first < ks1) {
        const int last = first + ((ks1 - 1 - first) / 4) * 4;  // this wave's last step
#pragma unroll
        for (int c = 0; c < NB - 1; ++c) {
            if (c < CH) fetch(ring[c], c, first);
        }
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
            // (three loops, not one over the 4G chunks with the softmax inside: see attention_wide_f16.hip)
#pragma unroll
            for (int c = 0; c < 2 * G; ++c) {
                unsigned (&cur)[8] = ring[c % NB];
                // ---- S^T = K Q^T: s[t][r] = S[query j][key0 + 16t + 4kq + r]; what lies past d is zero on both sides ----
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f16x8 qv = *reinterpret_cast<const f16x8 *>(qrow + 32 * (2 * (c >> 1) + u));
                    const u32x4 kv = u32x4{cur[4 * u], cur[4 * u + 1], cur[4 * u + 2], cur[4 * u + 3]};
                    s[c & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, kv), qv, s[c & 1], 0, 0, 0);
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
            const float m_off = m_run - P_SHIFT;
            f32x4 pr[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
                pr[tt] = f32x4{__builtin_amdgcn_exp2f(sv[tt][0] - m_off), __builtin_amdgcn_exp2f(sv[tt][1] - m_off),
                               __builtin_amdgcn_exp2f(sv[tt][2] - m_off), __builtin_amdgcn_exp2f(sv[tt][3] - m_off)};
            l_run += ((pr[0][0] + pr[0][1]) + (pr[0][2] + pr[0][3])) + ((pr[1][0] + pr[1][1]) + (pr[1][2] + pr[1][3]));
            const f16x8 ph = pack8(pr[0], pr[1]);
#pragma unroll
            for (int c = 2 * G; c < CH; ++c) {
                if (c & 1) {
                    // ---- O^T += V^T P^T: slot e of lane row kq contracts key key0 + 16 (e >> 2) + 4kq + (e & 3) on both sides.
                    // Fragment dword p of channel e = (key slot 2p, slot 2p + 1): the low or high halves of the two keys' dword e >> 1 ----
                    const int g = (c - 2 * G) >> 1;
                    unsigned (&lo)[8] = ring[(c - 1) % NB];
                    unsigned (&hi)[8] = ring[c % NB];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
                        const int w = e >> 1;
                        const u32x4 vh = u32x4{__builtin_amdgcn_perm(lo[2 + w], lo[w], sel), __builtin_amdgcn_perm(lo[6 + w], lo[4 + w], sel),
                                               __builtin_amdgcn_perm(hi[2 + w], hi[w], sel), __builtin_amdgcn_perm(hi[6 + w], hi[4 + w], sel)};
                        o[g][e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vh), ph, o[g][e], 0, 0, 0);
                    }
                }
                fetch_ahead(c);
            }
        }
    }
    __syncthreads();  // (every wave is done with the Q stage)

    // ---- the four waves merged; then the output rows from wave 0's registers, or -- key split -- this workgroup's image to its
    // workspace slice, a ticket, and the last split of the tile adds the slices up ----
    wide_merge_waves<G>(smem, wave, lane, o, m_run, l_run);
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
    float4 *const ws = reinterpret_cast<float4 *>(a.ws) + (size_t)unit * a.ksplit * (SLOTS * 64);
    if (wave == 0) wide_publish<G>(ws + (size_t)split * (SLOTS * 64), lane, o, m_run, l_run);
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

// Both entry points (wide_plan, on the fp16 operands' own alignment rules) on this unit's instances.  The kernel's arguments carry
// k / v as the `const float *` of WideAttnArgs and the kernel reads them as halves: the plan never dereferences them.
static int launch_attention_wide_f16kv(const float *q, int ldq, const void *k16, int ldk, const void *v16, int ldv, int B, int Nq, int Nk,
                                       int C, int heads, float scale, float *out, int ldo, const int32_t *tiles, int img_shift, int images,
                                       void *stream) {
    if (!sige_hip_attention_wide_f16kv_supported(Nq, Nk, C, heads)) return SIGE_HIP_EUNSUPPORTED;
    if (((ldk | ldv) & 7)) return SIGE_HIP_EUNSUPPORTED;  // (a lane's 16-byte load is 8 halves of one row; pointers: wide_plan)
    WidePlan p;
    // (wide_plan's strides are fp32 counts: its 2 GiB limit on one image's K / V is twice as strict as halves need)
    const int status = wide_plan(q, ldq, static_cast<const float *>(k16), ldk, static_cast<const float *>(v16), ldv, B, Nq, Nk, C, heads, scale,
                                 out, ldo, tiles, img_shift, images, stream, 32, &p);
    if (status != SIGE_HIP_OK) return status;
#define SIGE_WIDE16KV_GO(GG)                                                                   \
    do {                                                                                       \
        if (tiles) attention_wide_f16kv_kernel<GG, true><<<p.grid, 256, 0, p.st>>>(p.a);       \
        else attention_wide_f16kv_kernel<GG, false><<<p.grid, 256, 0, p.st>>>(p.a);            \
    } while (0)
    switch (p.G) {
        case 3: SIGE_WIDE16KV_GO(3); break;
        case 4: SIGE_WIDE16KV_GO(4); break;
        case 5: SIGE_WIDE16KV_GO(5); break;
        case 6: SIGE_WIDE16KV_GO(6); break;
        case 7: SIGE_WIDE16KV_GO(7); break;
        case 8: SIGE_WIDE16KV_GO(8); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
#undef SIGE_WIDE16KV_GO
    return launch_status();
}

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_attention_wide_f16kv_supported(int Nq, int Nk, int C, int heads) {
    return sige_hip_attention_wide_supported(Nq, Nk, C, heads);  // (d % 16 == 0: a lane's 8 halves are live or dead together)
}

extern "C" int sige_hip_attention_wide_f16kv(const float *q, int ldq, const void *k16, int ldk, const void *v16, int ldv,
                                             int B, int Nq, int Nk, int C, int heads, float scale, float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_f16kv, q, ldq, k16, ldk, v16, ldv, B, Nq, Nk, C, heads, scale, out, ldo, stream);
    int status;
    if (!attention_batch_args(B, Nq, Nk, C, heads, std::min({ldq, ldk, ldv, ldo}), q, k16, v16, out, &status)) return status;
    return launch_attention_wide_f16kv(q, ldq, k16, ldk, v16, ldv, B, Nq, Nk, C, heads, scale, out, ldo, nullptr, 0, 1, stream);
}

// Stacked edits: sige_hip_attention_wide_tiles_f16c (attention_wide_f16.hip) on fp16-stored K / V.
extern "C" int sige_hip_attention_wide_tiles_f16kv(const float *q, int ldq, const void *k16, int ldk, const void *v16, int ldv,
                                                   const int32_t *active_indices, int T, int H, int W, int C, int heads, float scale,
                                                   float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_tiles_f16kv, q, ldq, k16, ldk, v16, ldv, active_indices, T, H, W, C, heads, scale, out, ldo, stream);
    int status;
    if (!attention_tiles_args(T, H, W, C, heads, std::min({ldq, ldk, ldv, ldo}), q, k16, v16, out, active_indices, &status)) return status;
    StackedKeys g;
    if ((status = stacked_keys(active_indices, T, H, W, &g))) return status;
    return launch_attention_wide_f16kv(q, ldq, k16, ldk, v16, ldv, 1, 16 * T, g.Nk, C, heads, scale, out, ldo, g.tiles, g.shift, g.images, stream);
}
