// What the token linear's two units share (token_linear.hip: exact fp32 products; token_linear_f16.hip: fp16 operands): the argument
// struct, the LayerNorm statistics prologue and everything behind the K loop -- the four waves' K shares meeting in LDS in wave order,
// bias / GEGLU / residual / parts, the stores.  The accumulator layouts of the fp32 and the fp16 MFMAs are the same (32x32: column
// lane & 31, row (q & 3) + 8 (q >> 2) + 4 (lane >> 5); 16x16: column lane & 15, row 4 (lane >> 4) + q), so the epilogue is one piece of code.
#pragma once
#include "conv_mfma.hpp"
#include "split_finish.hpp"

namespace sige {

constexpr int kTokMaxLnK = 2048;      // token_ops.hip's limit (kMaxPerLane * 64)
constexpr int kTokSlots = 512;        // 64-token workgroups the chip holds at once: 256 CUs x 2 (LDS and registers)
constexpr int kTokRP = 68;            // padded row of the reduction buffer, in floats

struct TokArgs {
    const float *x, *gamma, *beta;
    const void *packed;     // fp32 (token_linear.hip) | fp16 (token_linear_f16.hip) in the unit's own lane order
    const float *bias, *residual;
    float *out0, *out1, *out2;
    float eps;
    int M, K, N;            // N: columns of the product (2 D for GEGLU)
    int No;                 // columns (= row stride) of one output: N / parts, D for GEGLU
    int ntn, nchunks, tpp;  // 64-column blocks, channel chunks (64 | 128 channels), column blocks per part
    int x_bytes, w_bytes;   // ranges of the two buffer descriptors
};
// ... of the K-split instances (the unsplit ones keep TokArgs: their kernel argument segment, and with it their code, stays what it was)
struct TokSplitArgs : TokArgs {
    int32_t *tickets;       // one per 16 x 64 output block (split_pool.hip)
    float *ws;              // [block][split][16][64] partial sums
    int ksplit, cps;        // workgroups per output block, chunks per split: split s walks chunks [s cps, min((s + 1) cps, nchunks))
};

__device__ __forceinline__ f32x4 buf4(rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ float gelu_erf(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

inline bool tok_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- LayerNorm statistics of the workgroup's BM rows: 256 / BM lanes per row, two passes over the row; row rl of M tile mt -> mean[mt],
//      rstd[mt] of the calling lane (through smem[0 .. 2 BM); ends behind a barrier) ----
template <int BM, int MT>
__device__ __forceinline__ void tok_row_stats(const TokArgs &a, rsrc_t rx, float *smem, int tid, int row0, int rl, float (&mean)[MT],
                                              float (&rstd)[MT]) {
    constexpr int TPR = 256 / BM;
    const int r = tid / TPR, sub = tid % TPR;
    const unsigned rb = row0 + r < a.M ? (unsigned)((row0 + r) * a.K) * 4u : kOOB;
    const int iters = (a.K / 4 + TPR - 1) / TPR;
    // (U requests in flight per round trip; a row share of up to U float4 -- K <= 64 U at 16 lanes per row -- stays in registers
    //  for the second pass)
    constexpr int U = 8;
    auto load8 = [&](int i0, f32x4 (&v)[U], bool (&in)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = (sub + TPR * (i0 + u)) * 4;
            in[u] = k < a.K;
            v[u] = buf4(rx, in[u] ? rb + (unsigned)k * 4u : kOOB);
        }
    };
    auto sum8 = [&](const f32x4 (&v)[U]) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) t += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);  // (absent pieces read 0)
        return t;
    };
    auto sq8 = [&](const f32x4 (&v)[U], const bool (&in)[U], float mu) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float d0 = v[u][0] - mu, d1 = v[u][1] - mu, d2 = v[u][2] - mu, d3 = v[u][3] - mu;
            t += in[u] ? (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3) : 0.f;
        }
        return t;
    };
    auto row_sum = [&](float t) {
#pragma unroll
        for (int d = TPR / 2; d >= 1; d >>= 1) t += __shfl_xor(t, d);
        return t;
    };
    f32x4 v[U];
    bool in[U];
    float mu, q = 0.f;
    if (iters <= U) {  // (uniform)
        load8(0, v, in);
        mu = row_sum(sum8(v)) / (float)a.K;
        q = sq8(v, in, mu);
    } else {
        float s = 0.f;
        for (int i0 = 0; i0 < iters; i0 += U) {
            load8(i0, v, in);
            s += sum8(v);
        }
        mu = row_sum(s) / (float)a.K;
        for (int i0 = 0; i0 < iters; i0 += U) {
            load8(i0, v, in);
            q += sq8(v, in, mu);
        }
    }
    q = row_sum(q);
    const float rs = 1.0f / sqrtf(q / (float)a.K + a.eps);
    if (sub == 0) {
        smem[2 * r] = mu;
        smem[2 * r + 1] = rs;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        mean[mt] = smem[2 * (mt * 32 + rl)];
        rstd[mt] = smem[2 * (mt * 32 + rl) + 1];
    }
}

// ---- everything behind the K loop.  tok_finish: a workgroup that owns its output block alone (its statements stay as they were
//      written: moving them into the pieces below changed the unsplit kernels' register allocation; it shares tok_sum4 only).
//      tok_finish_split: one of the `ksplit` workgroups that share a block, from pieces -- the four waves' K shares meeting in LDS
//      (tok_meet, tok_sum4), the epilogue's operands (tok_epi_prefetch), one epilogue unit (tok_epi_unit).
//      acc[mt][nt]: the wave's K share of the BM x 64 block in the MFMA's C / D layout (rl = lane & 31 | lane & 15, kg = lane >> 5 |
//      lane >> 4); smem: 4 * BM * kTokRP floats ----

// epilogue units of a lane: one float4 = 4 consecutive output columns of one row per step
template <int BM, bool GEGLU>
struct TokEpi {
    static constexpr int EU = GEGLU ? (BM * 8 + 255) / 256 : BM * 16 / 256;
    static constexpr int CW = GEGLU ? 8 : 16;  // float4 units per row
    float *outp;
    bool ok[EU];
    unsigned addr[EU];
    float4 bv[EU], bg[EU], rv[EU];
};

// where this lane's units go, and their bias and residual requested (clamped addresses: every lane loads, `ok` decides the store)
template <int BM, bool GEGLU>
__device__ __forceinline__ void tok_epi_prefetch(const TokArgs &a, int tid, int ntile, int row0, TokEpi<BM, GEGLU> &e) {
    constexpr int EU = TokEpi<BM, GEGLU>::EU, CW = TokEpi<BM, GEGLU>::CW;
    const int part = GEGLU ? 0 : ntile / a.tpp;
    e.outp = part == 0 ? a.out0 : (part == 1 ? a.out1 : a.out2);
#pragma unroll
    for (int k = 0; k < EU; ++k) {
        const int o = tid + 256 * k;
        const int n4 = o & (CW - 1), m = (o / CW) & (BM - 1);
        const int row = row0 + m;
        // (GEGLU: D % 32 == 0, every column of the block is real)
        const int co = GEGLU ? ntile * 32 + 4 * n4 : ntile * 64 + 4 * n4;
        e.ok[k] = o < BM * CW && row < a.M && (GEGLU || co < a.N);
        e.addr[k] = e.ok[k] ? (unsigned)(row * a.No + (co - part * a.No)) : 0u;
        e.bv[k] = e.bg[k] = e.rv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias) {
            e.bv[k] = *reinterpret_cast<const float4 *>(a.bias + (GEGLU ? co : min(co, a.N - 4)));
            if constexpr (GEGLU) e.bg[k] = *reinterpret_cast<const float4 *>(a.bias + a.No + co);
        }
        if (a.residual) e.rv[k] = *reinterpret_cast<const float4 *>(a.residual + e.addr[k]);
    }
}

// the four waves' K shares meet in LDS (ends behind a barrier)
template <int BM, int MT, int NT, typename acc_t>
__device__ __forceinline__ void tok_meet(float *smem, const acc_t (&acc)[MT][NT], int wave, int rl, int kg) {
    constexpr bool BIG = BM == 64;
    constexpr int RP = kTokRP;
    __syncthreads();  // (every lane has read its rows' statistics)
    {
        float *r = smem + wave * BM * RP;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < (BIG ? 16 : 4); ++q) {
                    // C / D maps: 32x32 -- column lane & 31, row (q & 3) + 8 (q >> 2) + 4 (lane >> 5); 16x16 -- column lane & 15, row 4 (lane >> 4) + q
                    const int m = BIG ? mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg : 4 * kg + q;
                    r[m * RP + nt * (BIG ? 32 : 16) + rl] = acc[mt][nt][q];
                }
    }
    __syncthreads();
}

// columns c .. c + 3 of row m of the block: the four waves' shares, in wave order
template <int BM>
__device__ __forceinline__ float4 tok_sum4(const float *smem, int m, int c) {
    constexpr int RP = kTokRP;
    const float *r0 = smem + m * RP + c;
    float4 s = *reinterpret_cast<const float4 *>(r0);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4 *>(r0 + w * BM * RP);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    return s;
}

__device__ __forceinline__ float4 tok_add4(float4 p, float4 q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); }

// unit k of the lane from its sums over K (s: the columns themselves, GEGLU: the value columns and g their gates): bias, GEGLU,
// residual, the store
template <int BM, bool GEGLU>
__device__ __forceinline__ void tok_epi_unit(const TokArgs &a, const TokEpi<BM, GEGLU> &e, int k, float4 s, float4 g) {
    if (a.bias) s = tok_add4(s, e.bv[k]);
    if constexpr (GEGLU) {
        if (a.bias) g = tok_add4(g, e.bg[k]);
        s = make_float4(s.x * gelu_erf(g.x), s.y * gelu_erf(g.y), s.z * gelu_erf(g.z), s.w * gelu_erf(g.w));
    }
    if (a.residual) s = tok_add4(e.rv[k], s);
    if (e.ok[k]) store_out4(e.outp + e.addr[k], s);
}

// The workgroup owns its block: bias and residual are requested ahead of the reduction's barriers, the epilogue reads LDS.
template <int BM, bool GEGLU, int MT, int NT, typename acc_t>
__device__ __forceinline__ void tok_finish(const TokArgs &a, float *smem, const acc_t (&acc)[MT][NT], int tid, int wave, int ntile, int row0,
                                           int rl, int kg) {
    constexpr bool BIG = BM == 64;
    constexpr int RP = kTokRP;
    // ---- epilogue units of this lane: one float4 = 4 consecutive output columns of one row per step.  Bias and residual are
    //      requested here, ahead of the reduction's barriers (clamped addresses: every lane loads, `ok` decides the store) ----
    constexpr int EU = GEGLU ? (BM * 8 + 255) / 256 : BM * 16 / 256;
    constexpr int CW = GEGLU ? 8 : 16;  // float4 units per row
    const int part = GEGLU ? 0 : ntile / a.tpp;
    float *const outp = part == 0 ? a.out0 : (part == 1 ? a.out1 : a.out2);
    bool ok[EU];
    unsigned addr[EU];
    float4 bv[EU], bg[EU], rv[EU];
#pragma unroll
    for (int k = 0; k < EU; ++k) {
        const int o = tid + 256 * k;
        const int n4 = o & (CW - 1), m = (o / CW) & (BM - 1);
        const int row = row0 + m;
        // (GEGLU: D % 32 == 0, every column of the block is real)
        const int co = GEGLU ? ntile * 32 + 4 * n4 : ntile * 64 + 4 * n4;
        ok[k] = o < BM * CW && row < a.M && (GEGLU || co < a.N);
        addr[k] = ok[k] ? (unsigned)(row * a.No + (co - part * a.No)) : 0u;
        bv[k] = bg[k] = rv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias) {
            bv[k] = *reinterpret_cast<const float4 *>(a.bias + (GEGLU ? co : min(co, a.N - 4)));
            if constexpr (GEGLU) bg[k] = *reinterpret_cast<const float4 *>(a.bias + a.No + co);
        }
        if (a.residual) rv[k] = *reinterpret_cast<const float4 *>(a.residual + addr[k]);
    }

    // ---- the four waves' K shares meet in LDS ----
    __syncthreads();  // (every lane has read its rows' statistics)
    {
        float *r = smem + wave * BM * RP;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < (BIG ? 16 : 4); ++q) {
                    // C / D maps: 32x32 -- column lane & 31, row (q & 3) + 8 (q >> 2) + 4 (lane >> 5); 16x16 -- column lane & 15, row 4 (lane >> 4) + q
                    const int m = BIG ? mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg : 4 * kg + q;
                    r[m * RP + nt * (BIG ? 32 : 16) + rl] = acc[mt][nt][q];
                }
    }
    __syncthreads();

    auto sum4 = [&](int m, int c) -> float4 { return tok_sum4<BM>(smem, m, c); };
    auto add4 = [](float4 p, float4 q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); };
#pragma unroll
    for (int k = 0; k < EU; ++k) {
        const int o = tid + 256 * k;
        const int n4 = o & (CW - 1), m = (o / CW) & (BM - 1);
        float4 s = sum4(m, 4 * n4);
        if (a.bias) s = add4(s, bv[k]);
        if constexpr (GEGLU) {
            float4 g = sum4(m, 32 + 4 * n4);
            if (a.bias) g = add4(g, bg[k]);
            s = make_float4(s.x * gelu_erf(g.x), s.y * gelu_erf(g.y), s.z * gelu_erf(g.z), s.w * gelu_erf(g.w));
        }
        if (a.residual) s = add4(rv[k], s);
        if (ok[k]) store_out4(outp + addr[k], s);
    }
}

// Split `split` of the `ksplit` workgroups that share the 16 x 64 block `unit` (split_finish.hpp has the protocol).  Every lane takes
// the float4 units it would have stored -- GEGLU: the value unit and its gate unit --, adds the four waves' shares and sends the sums
// to the workgroup's slice ws[(unit * ksplit + split) * 1024 + m * 64 + c] as coherent stores; the workgroup that draws the last ticket
// reads every slice back, each lane the units of its own lane position, adds them in split order 0 .. ksplit - 1 and runs the one
// epilogue.  Bias and residual are loaded by that last workgroup only (the other ksplit - 1 have no use for them), requested ahead of
// the read-back so that both round trips fly together.  The rows beyond M and the padded columns travel through the slices like the
// others (zeros or finite LayerNorm values of absent rows); `ok` keeps them out of the output.
template <bool GEGLU, typename acc_t>
__device__ __forceinline__ void tok_finish_split(const TokSplitArgs &a, float *smem, const acc_t (&acc)[1][4], int tid, int wave, int ntile,
                                                 int row0, int rl, int kg, int unit, int split) {
    constexpr int BM = 16;
    typedef TokEpi<BM, GEGLU> Epi;
    static_assert(Epi::EU == 1, "one epilogue unit per lane in the 16-token form");
    tok_meet<BM>(smem, acc, wave, rl, kg);
    const int n4 = tid & (Epi::CW - 1), m = (tid / Epi::CW) & (BM - 1);
    const bool mine = tid < BM * Epi::CW;  // (GEGLU: the lower 128 lanes hold the block's 128 value units, the upper 128 idle)
    float *const ws = a.ws + (size_t)unit * a.ksplit * (BM * 64) + m * 64 + 4 * n4;
    if (mine) {
        float *dst = ws + (size_t)split * (BM * 64);
        coherent_store(dst, tok_sum4<BM>(smem, m, 4 * n4));
        if constexpr (GEGLU) coherent_store(dst + 32, tok_sum4<BM>(smem, m, 32 + 4 * n4));
    }
    if (!split_arrive_last(a.tickets + unit, a.ksplit, reinterpret_cast<int *>(smem))) return;  // (the protocol: split_finish.hpp)
    Epi e;
    tok_epi_prefetch<BM, GEGLU>(a, tid, ntile, row0, e);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), g = s;
    // the slices in split order, four slices' loads in flight at a time
    for (int p0 = 0; p0 < a.ksplit; p0 += 4) {
        float4 ts[4], tg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *src = ws + (size_t)min(p0 + u, a.ksplit - 1) * (BM * 64);  // (past the end: the last slice again, not used)
            ts[u] = tg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (mine) {
                ts[u] = coherent_load4(src);
                if constexpr (GEGLU) tg[u] = coherent_load4(src + 32);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p0 + u < a.ksplit) {  // (workgroup-uniform)
                s = tok_add4(s, ts[u]);
                if constexpr (GEGLU) g = tok_add4(g, tg[u]);
            }
        }
    }
    tok_epi_unit<BM, GEGLU>(a, e, 0, s, g);
}

// ---- host side: the launch arguments but the unit's own (packed, ntn, nchunks, tpp, w_bytes) ----
inline TokArgs tok_args(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps, const float *bias, int N,
                        int geglu, const float *residual, int parts, float *out0, float *out1, float *out2) {
    TokArgs a;
    a.x = x; a.gamma = ln_gamma; a.beta = ln_beta; a.bias = bias; a.residual = residual;
    a.out0 = out0; a.out1 = parts > 1 ? out1 : out0; a.out2 = parts > 2 ? out2 : out0;
    a.eps = ln_eps;
    a.M = (int)M; a.K = K; a.N = N;
    a.No = geglu ? N / 2 : N / parts;
    a.x_bytes = (int)(M * K * 4);
    return a;
}

// grid fill of the 64-token form (as plan_conv chooses its tile): its grid comes in rounds of `slots` workgroups and in whole 64-row
// blocks; the share of the rounds' row slots that real rows fill
inline double tok_fill64(int64_t M, int ntn, int slots) {
    const long b64 = ((M + 63) / 64) * ntn, rounds = (b64 + slots - 1) / slots;
    return (double)M * ntn / (64.0 * (double)(rounds * slots));
}

// ---- host side of the K split (16-token form) ----
// split s of `ksplit` walks chunks [s cps, min((s + 1) cps, nchunks)), cps = ceil(nchunks / ksplit)
inline int tok_cps(int nchunks, int ksplit) { return (nchunks + ksplit - 1) / ksplit; }
// the splits of `ksplit` that are not empty (a forced split is clipped to this)
inline int tok_clip_split(int nchunks, int ksplit) { return (nchunks + tok_cps(nchunks, ksplit) - 1) / tok_cps(nchunks, ksplit); }

// The rule (measured per shape): a split pays where the 16-token grid is below 1.5 workgroups per CU AND K is deep --
// 5120 channels, the second feed-forward layer at 1280 channels, is the one depth of SD's at which it was seen to win; at 2560 and below
// the workgroups are too short for the finish to pay back.  There: the largest of 2 | 4 | 8 whose grid stays within five workgroups per
// CU and whose every split -- the shorter last one too -- keeps `min_chunks` chunks (1280 channels in either unit).
constexpr long kTokSplitBelow = 384;
constexpr long kTokSplitGridMax = 1280;
constexpr int kTokSplitDepth = 4;       // chunks of the whole K, in units of `min_chunks`, from which the rule splits at all
constexpr int kTokMaxSplit = 16;        // slices the last workgroup adds up, at most (a forced split)
inline int tok_split_rule(int64_t M, int ntn, int nchunks, int min_chunks) {
    const long grid = (long)((M + 15) / 16) * ntn;
    if (grid >= kTokSplitBelow || nchunks < kTokSplitDepth * min_chunks) return 1;
    int best = 1;
    for (int k = 2; k <= 8; k *= 2) {
        const int last = nchunks - (k - 1) * tok_cps(nchunks, k);  // (< 1: an empty split)
        if (grid * k <= kTokSplitGridMax && last >= min_chunks) best = k;
    }
    return best;
}

// the f16 unit's half of sige_hip_token_linear_ksplit (token_linear_f16.hip)
int token_linear_ksplit_f16(int64_t M, int N, int K, int layer_norm, int geglu, int parts);

// The split of a launch: `ksplit` as the entry points take it (0 = `rule`, 1 = none, 2 .. = forced) -> the split to run, tickets and
// workspace in `a`; 0 = refused (a forced split beyond the chunks or kTokMaxSplit, or without tickets / workspace -- the rule's own
// split falls back to 1 then).
inline int tok_plan_split(TokSplitArgs &a, int64_t M, int ksplit, int rule, hipStream_t st) {
    const bool forced = ksplit >= 2;
    if (forced && (ksplit > a.nchunks || ksplit > kTokMaxSplit)) return 0;
    int ks = forced ? tok_clip_split(a.nchunks, ksplit) : (ksplit == 0 ? rule : 1);
    a.tickets = nullptr; a.ws = nullptr;
    if (ks > 1) {
        const long units = (long)((M + 15) / 16) * a.ntn;
        a.tickets = split_tickets(st, units);
        if (a.tickets) a.ws = split_workspace(st, (size_t)units * ks * 1024);
        if (!a.tickets || !a.ws) {
            if (forced) return 0;
            ks = 1;
        }
    }
    a.ksplit = ks;
    a.cps = tok_cps(a.nchunks, ks);
    return ks;
}

}  // namespace sige
