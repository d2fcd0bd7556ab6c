// Attention over token matrices for WIDE heads (160 < d <= 512, d % 16 == 0), one launch: out = softmax(scale * q k^T) v per
// (batch, head).  The SD VAE decoder's middle block (stable-diffusion/ldm/modules/diffusionmodules/model.py:180-252, SIGEAttnBlock)
// is single-head attention over 512 channels: the queries are the tokens of the active 4x4 tiles, the keys / values all 64 x 64
// positions of the scattered K / V tensors.  attention_tokens.hip keeps Q, a look-ahead K block and the O accumulators of the whole
// head in registers -- at d = 512 over 384 registers per lane for those alone -- and stops at d = 160.
//
// Form: the transposed-score kernel of attention_tokens.hip with the head dimension cut into 64-channel GROUPS.
//   workgroup = 16 queries of one (batch, head) x one SPLIT of the key blocks; its 4 waves take the split's 16-key blocks round-robin,
//   each with its own running (max, sum, O) -- online softmax in units of log2 --, and meet at the end;
//   Q (16 x d) is staged ONCE in LDS (zeros beyond d) and read as the B operand of S^T = K Q^T, one ds_read_b128 per 4 MFMAs;
//   K and V stream through a ring of NB register chunks (4 x 16 bytes per lane each = one 64-channel group of 16 keys), issued
//   NB - 1 chunks ahead of their use as branch-free buffer loads (clamped key row, range-checked by the descriptor), across block
//   boundaries: per block G chunks of K, then G chunks of V;
//   O^T = V^T P^T: lane (kq, j) loads V[key 4kq + r][64g + 4j .. +3] (16 bytes), the four components are the A operands of four
//   16 x 16 tiles whose row m is channel 64g + 4m + e -- the accumulators o[g][e][r'] of a lane are then 4 CONSECUTIVE channels
//   (64g + 16kq + 4r' + e) of query j: 128 accumulator registers at d = 512, 16-byte stores.
// Registers at d = 512: 128 (O) + 64 (ring) + ~40; LDS 33 KB (the Q stage, reused by the merge).
//
// The four waves merge in registers through ONE LDS slot of the accumulator image (3 -> 2, 1 -> 0, 2 -> 0: 33 KB instead of the
// 132 KB of four images side by side).  A 16-query workgroup at d = 512 against 4 096 keys is 134 MFLOP = 218 us of one CU's fp32
// matrix pipe, and a sparse edit has a handful of query tiles: the host splits the key blocks over `ksplit` workgroups per tile
// (about one workgroup per CU in all); every split leaves its merged (m, l, O) in a workspace slice as device-coherent stores,
// takes a ticket, and the LAST one adds the slices up in split order and writes the output -- the in-launch split
// finish (split_finish.hpp), no second launch.  Without tickets or workspace (first use inside a capture, regions exhausted) ksplit = 1.
//
// q [B,Nq,ldq], k [B,Nk,ldk], v [B,Nk,ldv], out [B,Nq,ldo]: row strides in elements, head h at channels [h*d, (h+1)*d) of a row.
//
// Stacked edits (sige_hip_attention_wide_tiles_f32): a workgroup IS one 4x4 tile x one key split, so it can read its
// keys from the tile's own image -- the tile's origin row from the Gather's index list (one wave-uniform load), e = row >> log2(rows
// of an image), clamped, and both buffer descriptors start at image e's first key row and span ONE image's Nk keys.  Everything
// else -- the split arithmetic, tail masking, clamped key rows, the range check -- is per image without knowing it.  Without an
// index list e = 0: the batched entry's launch, bit for bit.
#include <algorithm>

#include "attention_rows.hpp"  // (max_over_rows, merge_weight: shared with attention_tokens.hip)
#include "split_finish.hpp"

namespace sige {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WideAttnArgs {
    const float *q, *k, *v;
    float *out;
    float *ws;          // [units * ksplit][(4G + 1) * 64] float4: the splits' merged accumulator images (ksplit > 1)
    int32_t *tickets;   // one per (pair, query tile), zero between launches
    int ldq, ldk, ldv, ldo;
    int Nq, Nk, C, heads, d;
    int q_tiles, ksplit, split_blocks;  // split s takes key blocks [s * split_blocks, (s + 1) * split_blocks)
    float scale_log2e;
    // per-image keys (sige_hip_attention_wide_tiles_f32; stacked edits): query tile t is the 4x4 tile with origin row tiles[2t] of
    // the tall image, its keys are the Nk rows of image tiles[2t] >> img_shift.  nullptr: every tile reads the keys of image 0.
    const int32_t *tiles;
    int img_shift, images;
};

// ring depth: the largest divisor of the 2G chunks of a key block that is <= 8 (slots stay compile-time across blocks)
constexpr int wide_ring(int G) { return (2 * G) % 8 == 0 ? 8 : (2 * G) % 7 == 0 ? 7 : (2 * G) % 6 == 0 ? 6 : 5; }

template <int G>  // 64-channel groups covering the head dimension: 64 (G - 1) < d <= 64 G
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void attention_wide_kernel(WideAttnArgs a) {
    kernarg_touch<sizeof(WideAttnArgs)>();
    constexpr int QS = 64 * G + 4;             // padded row of the Q stage
    constexpr int SLOTS = 4 * G + 1;           // float4 per lane of an accumulator image: o[g][.][r'] at 4g + r', then (m, l)
    constexpr int NB = wide_ring(G), CH = 2 * G;
    constexpr int LDS_FLOATS = 16 * QS > SLOTS * 256 ? 16 * QS : SLOTS * 256;
    __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];
    __shared__ int ticket_lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, j = lane & 15;
    // workgroup -> (split, query tile, (batch, head) pair) = blockIdx.(x, y, z): one 32-bit division by a run-time value
    const unsigned split = blockIdx.x, qtile = blockIdx.y, pair = blockIdx.z;
    const unsigned unit = pair * (unsigned)a.q_tiles + qtile;
    const unsigned b = pair / (unsigned)a.heads, head = pair - b * (unsigned)a.heads;
    const int q0 = (int)qtile * 16, d = a.d;
    const size_t hoff = (size_t)head * d;
    // the tile's origin row: ONE wave-uniform load per workgroup (the address is the same in every lane; the branch is the same for
    // the whole launch), issued in front of the Q stage and first used behind it
    int tile_row = 0;
    if (a.tiles) tile_row = a.tiles[2 * qtile];

    // ---- Q stage: 16 rows x 64 G channels, zeros beyond d (clamped address, load, select) ----
    {
        const float *qb = a.q + ((size_t)b * a.Nq + q0) * a.ldq + hoff;
        for (int e = tid; e < 16 * 16 * G; e += 256) {
            const int row = e / (16 * G), c = (e - row * (16 * G)) * 4;
            const float4 t = *reinterpret_cast<const float4 *>(qb + (size_t)row * a.ldq + min(c, d - 4));
            const unsigned keep = c < d ? 0xffffffffu : 0u;  // (a mask, not a select: the compiler turns `c < d ? load : 0` into a branch around the load)
            auto mk = [&](float x) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & keep); };
            *reinterpret_cast<float4 *>(smem + row * QS + c) = make_float4(mk(t.x), mk(t.y), mk(t.z), mk(t.w));
        }
    }
    __syncthreads();

    // the key blocks of this split: [kb0, kb1), dealt round-robin to the waves
    const int nkb = (a.Nk + 15) / 16;
    const int kb0 = (int)split * a.split_blocks, kb1 = min(nkb, kb0 + a.split_blocks);  // (host: every split has a block)

    float m_run = -INFINITY, l_run = 0.f;  // of query j: the maximum over every key so far, the sum over THIS lane's keys
    f32x4 o[G][4];                         // o[g][e][r'] = O[query j][channel 64g + 16kq + 4r' + e]
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[g][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // K / V of batch b (of image `image`: B = 1 there), head `head`: valid bytes from the head's first channel of key 0 to the end of
    // the last key's C channels -- ONE image's keys, a read outside them returns the descriptor's zeros
    // (clamped: no index list can move the descriptors outside k / v; without `tiles`: shift 0, one image -- 0)
    const int image = min(max(__builtin_amdgcn_readfirstlane(tile_row) >> a.img_shift, 0), a.images - 1);
    const size_t krow0 = ((size_t)b + (size_t)image) * a.Nk;
    const unsigned k_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldk + a.C - hoff) * sizeof(float));
    const unsigned v_bytes = (unsigned)((((size_t)a.Nk - 1) * a.ldv + a.C - hoff) * sizeof(float));
    const __amdgpu_buffer_rsrc_t r_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k + krow0 * a.ldk + hoff), 0, k_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v + krow0 * a.ldv + hoff), 0, v_bytes, 0x00020000);
    const int k_row = a.ldk * (int)sizeof(float), v_row = a.ldv * (int)sizeof(float);

    float4 ring[NB][4];
    // chunk cc of key block kblk: cc < G: K[key j][64cc + 16uu + 4kq .. +3], uu = 0..3 (the A operand of the scores);
    //                             else:   V[key 4kq + r][64(cc - G) + 4j .. +3], r = 0..3 (the A operands of O^T, k-step r).
    // A key past Nk (the tail block) reads the last key's row (its scores are masked, its P is 0); channels past d read the
    // row's next bytes or, beyond the tensor, the zeros of an out-of-range buffer load: K's are never multiplied (the unit is
    // skipped), V's land in columns of O that are never stored.
    auto fetch = [&](float4 (&dst)[4], const int cc, const int kblk) {
        const int key0 = kblk * 16;
        if (cc < G) {
            const int off = min(key0 + j, a.Nk - 1) * k_row + (64 * cc + 4 * kq) * (int)sizeof(float);
#pragma unroll
            for (int uu = 0; uu < 4; ++uu)
                dst[uu] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_k, off + 64 * uu, 0, 0));
        } else {
            const int cbytes = (64 * (cc - G) + 4 * j) * (int)sizeof(float);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                dst[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                    r_v, min(key0 + 4 * kq + r, a.Nk - 1) * v_row + cbytes, 0, 0));
        }
    };

    const int first = kb0 + wave;
    if (first < kb1) {
        const int last = first + ((kb1 - 1 - first) / 4) * 4;  // this wave's last block
#pragma unroll
        for (int c = 0; c < NB - 1; ++c) fetch(ring[c], c, first);
        const float *qrow = smem + j * QS + 4 * kq;
        for (int kblk = first; kblk < kb1; kblk += 4) {
            const int key0 = kblk * 16;
            const int nxt = min(kblk + 4, last);  // (past the end: the last block again -- valid addresses, never used)
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
            float pr[4];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                // chunk c + NB - 1 goes into the slot chunk c - 1 has just left
                const int ahead = c + NB - 1;
                if (ahead < CH) fetch(ring[ahead % NB], ahead, kblk);
                else fetch(ring[ahead % NB], ahead - CH, nxt);
                float4 (&cur)[4] = ring[c % NB];
                if (c < G) {
                    // ---- S^T = K Q^T: s[r] = S[query j][key0 + 4kq + r]; whole 16-channel units, those past d skipped ----
#pragma unroll
                    for (int uu = 0; uu < 4; ++uu) {
                        if (64 * c + 16 * uu < d) {  // (wave-uniform)
                            const float4 qv = *reinterpret_cast<const float4 *>(qrow + 64 * c + 16 * uu);
                            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[uu].x, qv.x, s0, 0, 0, 0);
                            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[uu].y, qv.y, s1, 0, 0, 0);
                            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[uu].z, qv.z, s0, 0, 0, 0);
                            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[uu].w, qv.w, s1, 0, 0, 0);
                        }
                    }
                    if (c == G - 1) {
                        // ---- online softmax of query j (units of log2: exp(x) = exp2(x * log2 e)) ----
                        float sv[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) sv[r] = (s0[r] + s1[r]) * a.scale_log2e;
                        if (key0 + 16 > a.Nk) {  // (wave-uniform: the tail block only)
#pragma unroll
                            for (int r = 0; r < 4; ++r) sv[r] = key0 + 4 * kq + r < a.Nk ? sv[r] : -INFINITY;
                        }
                        const float mb = max_over_rows(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])));  // (finite: a block has a live key)
                        if (__builtin_amdgcn_ballot_w64(mb > m_run) != 0) {  // (wave-uniform; once the maxima have settled no block enters)
                            const float m_new = fmaxf(m_run, mb);
                            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // (exp2(-inf) = 0 on the first block)
                            m_run = m_new;
                            l_run *= alpha;
#pragma unroll
                            for (int g = 0; g < G; ++g) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) { o[g][e][0] *= alpha; o[g][e][1] *= alpha; o[g][e][2] *= alpha; o[g][e][3] *= alpha; }
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) pr[r] = __builtin_amdgcn_exp2f(sv[r] - m_run);
                        l_run += (pr[0] + pr[1]) + (pr[2] + pr[3]);
                    }
                } else {
                    // ---- O^T += V^T P^T: k-step r contracts keys key0 + 4kq + r ----
                    const int g = c - G;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[r].x, pr[r], o[g][0], 0, 0, 0);
                        o[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[r].y, pr[r], o[g][1], 0, 0, 0);
                        o[g][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[r].z, pr[r], o[g][2], 0, 0, 0);
                        o[g][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[r].w, pr[r], o[g][3], 0, 0, 0);
                    }
                }
            }
        }
    }
    __syncthreads();  // (every wave is done with the Q stage)

    // ---- merge the four waves' (m, l, O) in registers through one LDS image: 3 -> 2, 1 -> 0, 2 -> 0 ----
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
        const float f1 = merge_weight(m_run, M), f2 = merge_weight(ml.x, M);  // (a wave without a key block: weight 0)
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
    // thread (wave, lane) -> slots wave, wave + 4, ... of lane `lane`: slot 4g + wave = channels 64g + 16kq + 4 wave .. +3 of query j.
    // The slices in split order with a running maximum, four slices' loads in flight at a time (a dependent round trip to the
    // coherence point per slice was most of a small launch)
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

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_attention_wide_supported(int Nq, int Nk, int C, int heads) {
    if (Nq <= 0 || Nk <= 0 || C <= 0 || heads <= 0 || C % heads) return 0;
    const int d = C / heads;
    return (Nq % 16 == 0 && d % 16 == 0 && d > 160 && d <= 512) ? 1 : 0;
}

namespace sige {

// Both entry points: q [B,Nq,ldq] against k / v of Nk keys per batch -- or, with `tiles` (B = 1), per image of 2^img_shift rows.
static int launch_attention_wide(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv, int B, int Nq, int Nk, int C,
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

    // key split: about one workgroup per CU in all, at least 4 key blocks (one per wave) per split, at most 16 slices to add up
    const int nkb = (Nk + 15) / 16;
    int ksplit = (int)std::min<long>(std::min<long>(256 / units, nkb / 4), 16);
    WideAttnArgs a;
    a.ws = nullptr; a.tickets = nullptr;
    if (ksplit > 1) {
        a.tickets = split_tickets(st, units);
        if (a.tickets) a.ws = split_workspace(st, (size_t)units * ksplit * (4 * G + 1) * 256);
        if (!a.tickets || !a.ws) ksplit = 1;
    }
    if (ksplit < 1) ksplit = 1;
    a.split_blocks = (nkb + ksplit - 1) / ksplit;
    ksplit = (nkb + a.split_blocks - 1) / a.split_blocks;  // (no empty split)
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.Nq = Nq; a.Nk = Nk; a.C = C; a.heads = heads; a.d = d;
    a.q_tiles = Nq / 16; a.ksplit = ksplit;
    a.scale_log2e = scale * 1.44269504088896341f;
    a.tiles = tiles; a.img_shift = img_shift; a.images = images;
    const dim3 grid((unsigned)ksplit, (unsigned)(Nq / 16), (unsigned)(B * heads));
    switch (G) {
        case 3: attention_wide_kernel<3><<<grid, 256, 0, st>>>(a); break;
        case 4: attention_wide_kernel<4><<<grid, 256, 0, st>>>(a); break;
        case 5: attention_wide_kernel<5><<<grid, 256, 0, st>>>(a); break;
        case 6: attention_wide_kernel<6><<<grid, 256, 0, st>>>(a); break;
        case 7: attention_wide_kernel<7><<<grid, 256, 0, st>>>(a); break;
        case 8: attention_wide_kernel<8><<<grid, 256, 0, st>>>(a); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
    return launch_status();
}

}  // namespace sige

extern "C" int sige_hip_attention_wide_f32(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                           int B, int Nq, int Nk, int C, int heads, float scale, float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_f32, q, ldq, k, ldk, v, ldv, B, Nq, Nk, C, heads, scale, out, ldo, stream);
    if (B < 0 || Nq < 0 || Nk <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return SIGE_HIP_EINVAL;
    if ((long)B * Nq == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out) return SIGE_HIP_EINVAL;
    return launch_attention_wide(q, ldq, k, ldk, v, ldv, B, Nq, Nk, C, heads, scale, out, ldo, nullptr, 0, 1, stream);
}

// Stacked edits (sige_hip_set_edit_batch): the queries are the tokens of T active 4x4 tiles of the tall image [1,C,H,W] = E images
// of H / E rows, and tile t attends to the (H / E) W keys of ITS image only -- one launch for the tiles of all E edits, the
// per-edit tile counts never on the host.
extern "C" int sige_hip_attention_wide_tiles_f32(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                                 const int32_t *active_indices, int T, int H, int W, int C, int heads, float scale,
                                                 float *out, int ldo, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_attention_wide_tiles_f32, q, ldq, k, ldk, v, ldv, active_indices, T, H, W, C, heads, scale, out, ldo, stream);
    if (T < 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0) return SIGE_HIP_EINVAL;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return SIGE_HIP_EINVAL;
    if (T == 0) return SIGE_HIP_OK;
    if (!q || !k || !v || !out || !active_indices) return SIGE_HIP_EINVAL;
    const int s = stacked_shift(H);
    if (s < 0) return SIGE_HIP_EUNSUPPORTED;  // (one image's height: a power of two >= 4)
    const int E = s > 0 ? H >> s : 1;         // (shift 0 = no edit batch: one image, base 0 -- the other entry's launch)
    if ((long)T * 16 > 0x7fffffffL || (long)(H / E) * W > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    return launch_attention_wide(q, ldq, k, ldk, v, ldv, 1, 16 * T, (H / E) * W, C, heads, scale, out, ldo, active_indices, s, E, stream);
}
