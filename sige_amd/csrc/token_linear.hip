// Token linear of Stable Diffusion's transformer blocks (ldm/modules/attention.py: CrossAttention.to_q / to_k / to_v / to_out,
// GEGLU.proj, FeedForward.net[2]) with what sits around it folded in: LayerNorm on the way in, bias / GEGLU / residual on the way out.
//
//   out[M, N] = epilogue( prologue(x)[M, K] . W^T )        x [M, K] row-major fp32 (a channels-last tile slab IS that matrix),
//                                                          W = nn.Linear.weight [N, K]
//   prologue  none | LayerNorm over K: a = (x - mean_r) * rstd_r * gamma_k + beta_k, statistics two-pass (exact mean first) like
//             add_layer_norm_kernel (token_ops.hip), computed by every workgroup for its own rows (they are L2 resident)
//   epilogue  acc + bias[n] | residual[m, n] + (acc + bias[n]) | GEGLU: (acc[m, d] + b[d]) * gelu(acc[m, D + d] + b[D + d]), N = 2 D |
//             parts: the N columns as 1 .. 3 equal groups, each to its own contiguous [M, N / parts] tensor (q | k | v in one launch)
//
// Exact fp32 products on v_mfma_f32_32x32x2_f32 (64 tokens x 64 columns per workgroup, 2 x 2 tiles per wave) or v_mfma_f32_16x16x4_f32
// (16 tokens x 64 columns, 1 x 4 tiles per wave); the four waves of a workgroup split K -- wave w owns channels 16 w .. 16 w + 15 of
// every 64-channel chunk -- and meet in LDS, in wave order: no atomics, the same call gives the same bits.
//
// A Linear has no halo and no tap reuse, and a lane of the MFMA owns one row: the A fragments go from global memory straight to
// registers (8 | 4 consecutive channels of the lane's row per chunk: the k order inside a chunk is free as long as the packed weights
// follow it), a row's mean and rstd are two registers of the lane.  Weights are packed once per (ntile, chunk, wave) as 1024 floats in
// the 32x32x2 form's lane order, zero padded to 64 columns and 64 channels; the 16-token form reads the same tensor through a permuted
// lane address.  GEGLU: a workgroup's 64 packed columns are 32 value columns and THEIR 32 gate columns.
// Row tails and dead channel slices: the buffer descriptor's range check (offset kOOB reads 0); column tails: the zero padding.
#include "token_linear.hpp"

namespace sige {
namespace {

// BM: token rows per workgroup (64 | 16).  SPLIT (16-token form): blockIdx.y of gridDim.y = a.ksplit workgroups that share the output
// block blockIdx.x -- the split is the slow grid dimension, so the workgroups of one block are dispatched a whole grid row apart, to
// different CUs / XCDs --, each on its own run of chunks; they finish inside the launch (token_linear.hpp: tok_finish_split).
template <int BM, bool LN, bool GEGLU, bool SPLIT = false>
__global__ __launch_bounds__(256) void token_linear_kernel(const typename std::conditional<SPLIT, TokSplitArgs, TokArgs>::type a) {
    static_assert(!SPLIT || BM == 16, "the K split is a variant of the 16-token form");
    kernarg_touch<sizeof(a)>();
    constexpr bool BIG = BM == 64;
    constexpr int MT = BIG ? 2 : 1;   // M tiles per wave
    constexpr int NT = BIG ? 2 : 4;   // N tiles per wave
    constexpr int AP = BIG ? 2 : 1;   // 16-byte A pieces per lane, tile and chunk
    constexpr int RP = kTokRP;
    __shared__ __attribute__((aligned(16))) float smem[4 * BM * RP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = blockIdx.x % a.ntn, mtile = blockIdx.x / a.ntn;
    const int row0 = mtile * BM;
    const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, a.x_bytes, 0x00020000);
    const rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.packed), 0, a.w_bytes, 0x00020000);
    // this lane's rows and channel group: 32x32x2 -- row lane & 31 of each M tile, channels 8 kq .. 8 kq + 7 of the wave's 16 (MFMA step
    // s contracts channels s and 8 + s); 16x16x4 -- row lane & 15, channels 4 kg .. 4 kg + 3 (step s: channels s, 4 + s, 8 + s, 12 + s)
    const int rl = BIG ? (lane & 31) : (lane & 15), kg = BIG ? (lane >> 5) : (lane >> 4);
    constexpr int KPL = BIG ? 8 : 4;  // channels per lane and chunk

    // ---- LayerNorm statistics of the workgroup's rows: 256 / BM lanes per row, two passes over the row ----
    float mean[MT], rstd[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mean[mt] = 0.f, rstd[mt] = 1.f;
    if constexpr (LN) {
        tok_row_stats<BM>(a, rx, smem, tid, row0, rl, mean, rstd);
    }

    // ---- K loop: the registers of chunk c + 1 are requested before the MFMAs of chunk c ----
    unsigned abase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = row0 + mt * 32 + rl;
        abase[mt] = row < a.M ? (unsigned)(row * a.K + kg * KPL) * 4u : kOOB;
    }
    // packed weights [ntile][chunk][wave][nt][piece][lane of the 32x32x2 form][4]; the 16x16x4 form's lane (row rl, group kg) of N
    // tile t reads what lane (kg >> 1) * 32 + (t & 1) * 16 + rl, piece kg & 1 of N tile t >> 1 holds
    const unsigned bbase = ((unsigned)(ntile * a.nchunks) * 4u + wave) * 4096u;
    unsigned boff[NT][AP];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int p = 0; p < AP; ++p)
            boff[nt][p] = BIG ? bbase + (nt * 2 + p) * 1024 + lane * 16
                              : bbase + ((nt >> 1) * 2 + (kg & 1)) * 1024 + ((kg >> 1) * 32 + (nt & 1) * 16 + rl) * 16;
    struct Frag {
        f32x4 a[MT][AP], b[NT][AP], g[AP], e[AP];
    };
    auto load = [&](int chunk, Frag &f) {
        const int kb = chunk * 64 + wave * 16;
        const bool live = kb < a.K;  // (wave-uniform; K % 16 == 0: a wave's slice of a chunk is whole or absent)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int p = 0; p < AP; ++p) f.a[mt][p] = buf4(rx, live ? abase[mt] + (unsigned)(kb + 4 * p) * 4u : kOOB);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int p = 0; p < AP; ++p) f.b[nt][p] = buf4(rw, boff[nt][p] + (unsigned)chunk * 16384u);
        if constexpr (LN) {
            const int kk = min(kb + kg * KPL, a.K - KPL);
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                f.g[p] = *reinterpret_cast<const f32x4 *>(a.gamma + kk + 4 * p);
                f.e[p] = *reinterpret_cast<const f32x4 *>(a.beta + kk + 4 * p);
            }
        }
    };
    typedef typename std::conditional<BIG, f32x16, f32x4>::type acc_t;
    acc_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < (BIG ? 16 : 4); ++r) acc[mt][nt][r] = 0.0f;

    // this workgroup's chunks [c0, c1): all of them, or its split's run (never empty: host side)
    int c0 = 0, c1 = a.nchunks;
    if constexpr (SPLIT) {
        c0 = (int)blockIdx.y * a.cps;
        c1 = min(c0 + a.cps, a.nchunks);
    }
    Frag cur, nxt;
    load(c0, cur);
    for (int c = c0; c < c1; ++c) {
        load(min(c + 1, c1 - 1), nxt);
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks the prefetch down to its first use)
        if constexpr (LN) {
            const bool live = c * 64 + wave * 16 < a.K;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int p = 0; p < AP; ++p)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float z = (cur.a[mt][p][j] - mean[mt]) * rstd[mt] * cur.g[p][j] + cur.e[p][j];
                        cur.a[mt][p][j] = live ? z : 0.f;
                    }
        }
#pragma unroll
        for (int p = 0; p < AP; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if constexpr (BIG) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[mt][p][j], cur.b[nt][p][j], acc[mt][nt], 0, 0, 0);
                        else acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[mt][p][j], cur.b[nt][p][j], acc[mt][nt], 0, 0, 0);
                    }
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }

    if constexpr (SPLIT) tok_finish_split<GEGLU>(a, smem, acc, tid, wave, ntile, row0, rl, kg, (int)blockIdx.x, (int)blockIdx.y);
    else tok_finish<BM, GEGLU>(a, smem, acc, tid, wave, ntile, row0, rl, kg);
}

// packed[((ntile * nchunks + chunk) * 4 + wave) * 1024 + ((nt * 2 + piece) * 64 + lane) * 4 + j] =
//   W[col(ntile, nt * 32 + (lane & 31))][chunk * 64 + wave * 16 + (lane >> 5) * 8 + piece * 4 + j], 0 beyond N / K
// (one float4 per lane; the unit count is a multiple of 1024, the grid is exact)
__global__ __launch_bounds__(256) void token_linear_pack_kernel(const float *__restrict__ w, int N, int K, int D, int nchunks,
                                                               float *__restrict__ packed) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(u & 63), sub = (int)(u >> 6) & 3, wave = (int)(u >> 8) & 3;
    const int rest = (int)(u >> 10);
    const int chunk = rest % nchunks, ntile = rest / nchunks;
    const int nl = (sub >> 1) * 32 + (lane & 31);
    // GEGLU (D > 0): block j holds value columns 32 j .. 32 j + 31, then their gate columns D + 32 j ..
    const int n = D > 0 ? (nl < 32 ? ntile * 32 + nl : D + ntile * 32 + nl - 32) : ntile * 64 + nl;
    const int k = chunk * 64 + wave * 16 + (lane >> 5) * 8 + (sub & 1) * 4;
    const bool ok = n < N && k < K;
    const float4 v = *reinterpret_cast<const float4 *>(w + (ok ? (size_t)n * K + k : 0));
    *reinterpret_cast<float4 *>(packed + (size_t)u * 4) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

// 64-column blocks of the packed tensor; 0 = the shape is not supported
inline int tok_ntn(int N, int K, int geglu) {
    if (N <= 0 || K <= 0 || N % 16 || K % 16) return 0;
    if (geglu) return (N % 2 || (N / 2) % 32) ? 0 : N / 64;
    return (N + 63) / 64;
}
inline int tok_nchunks(int K) { return (K + 63) / 64; }

// every split keeps at least this many 64-channel chunks (the rule's other constants: token_linear.hpp)
constexpr int kTokSplitMinChunks = 20;

template <int BM>
void launch_tok(const TokArgs &a, bool ln, bool geglu, unsigned grid, hipStream_t st) {
    if (ln && geglu) token_linear_kernel<BM, true, true><<<grid, 256, 0, st>>>(a);
    else if (ln) token_linear_kernel<BM, true, false><<<grid, 256, 0, st>>>(a);
    else if (geglu) token_linear_kernel<BM, false, true><<<grid, 256, 0, st>>>(a);
    else token_linear_kernel<BM, false, false><<<grid, 256, 0, st>>>(a);
}

// grid (output blocks, splits)
void launch_tok_split(const TokSplitArgs &a, bool ln, bool geglu, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks, (unsigned)a.ksplit);
    if (ln && geglu) token_linear_kernel<16, true, true, true><<<grid, 256, 0, st>>>(a);
    else if (ln) token_linear_kernel<16, true, false, true><<<grid, 256, 0, st>>>(a);
    else if (geglu) token_linear_kernel<16, false, true, true><<<grid, 256, 0, st>>>(a);
    else token_linear_kernel<16, false, false, true><<<grid, 256, 0, st>>>(a);
}

}  // namespace
}  // namespace sige

using namespace sige;

extern "C" size_t sige_hip_token_linear_packed_size(int N, int K, int geglu) {
    const int ntn = tok_ntn(N, K, geglu);
    if (!ntn) return 0;
    const size_t floats = (size_t)ntn * tok_nchunks(K) * 4096;
    return floats * 4 > 0x7fffffffUL ? 0 : floats;  // (32-bit byte offsets into the packed tensor)
}

extern "C" int sige_hip_token_linear_supported(int64_t M, int N, int K, int layer_norm, int geglu, int parts) {
    if (M < 0 || parts < 1 || parts > 3 || !sige_hip_token_linear_packed_size(N, K, geglu)) return 0;
    if (layer_norm && K > kTokMaxLnK) return 0;
    if (parts > 1 && (geglu || N % parts || (N / parts) % 64)) return 0;
    // 32-bit element offsets into x and the outputs, and a one-dimensional grid of 16-row workgroups
    if (M * K * 4 > 0x7fffffffL || M * N * 4 > 0x7fffffffL) return 0;
    if (((M + 15) / 16) * tok_ntn(N, K, geglu) > 0x7fffffffL) return 0;
    return 1;
}

extern "C" int sige_hip_token_linear_pack(const float *w, int N, int K, int geglu, float *packed, void *stream) {
    if (N <= 0 || K <= 0) return SIGE_HIP_EINVAL;
    if (!w || !packed) return SIGE_HIP_EINVAL;
    const size_t floats = sige_hip_token_linear_packed_size(N, K, geglu);
    if (!floats || !tok_al16(w) || !tok_al16(packed)) return SIGE_HIP_EUNSUPPORTED;
    token_linear_pack_kernel<<<(unsigned)(floats / 1024), 256, 0, as_stream(stream)>>>(w, N, K, geglu ? N / 2 : 0, tok_nchunks(K), packed);
    return launch_status();
}

namespace sige {

// The 64-token form by grid fill (as plan_conv chooses its tile): it reads every weight byte for four times the rows, but its grid
// comes in rounds of kTokSlots workgroups and in whole 64-row blocks; it runs where real rows fill at least 0.8 of the rounds' slots
// (measured per shape: DESIGN.md 5.12), the 16-token form's four times finer grid everywhere else
static bool tok_big(int64_t M, int ntn) {
    const int knob = tuning(SIGE_HIP_TUNE_TOKEN_LINEAR_FORM);
    return knob ? knob == 2 : tok_fill64(M, ntn, kTokSlots) >= 0.8;
}

// Both launching entry points.  ksplit: -1 = sige_hip_token_linear_f32 (form by fill, no split) | sige_hip_token_linear_split_f32's
static int token_linear_f32(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps, const float *packed,
                            const float *bias, int N, int geglu, const float *residual, int parts, float *out0, float *out1, float *out2,
                            int ksplit, void *stream) {
    if (M < 0 || K <= 0 || N <= 0 || parts < 1 || parts > 3 || ksplit < -1) return SIGE_HIP_EINVAL;
    if (M == 0) return SIGE_HIP_OK;
    if (!x || !packed || !out0 || (parts > 1 && !out1) || (parts > 2 && !out2) || (ln_gamma && !ln_beta)) return SIGE_HIP_EINVAL;
    if (!sige_hip_token_linear_supported(M, N, K, ln_gamma != nullptr, geglu, parts)) return SIGE_HIP_EUNSUPPORTED;
    if (parts > 1 && residual) return SIGE_HIP_EUNSUPPORTED;
    if (!tok_al16(x) || !tok_al16(packed) || !tok_al16(out0) || !tok_al16(out1) || !tok_al16(out2) || !tok_al16(bias) || !tok_al16(residual) || !tok_al16(ln_gamma) || !tok_al16(ln_beta))
        return SIGE_HIP_EUNSUPPORTED;
    TokSplitArgs a;
    static_cast<TokArgs &>(a) = tok_args(x, M, K, ln_gamma, ln_beta, ln_eps, bias, N, geglu, residual, parts, out0, out1, out2);
    a.packed = packed;
    a.ntn = tok_ntn(N, K, geglu);
    a.nchunks = tok_nchunks(K);
    a.tpp = parts > 1 ? a.No / 64 : a.ntn;
    a.w_bytes = (int)(sige_hip_token_linear_packed_size(N, K, geglu) * 4);
    hipStream_t st = as_stream(stream);
    const bool ln = ln_gamma != nullptr;
    const unsigned blocks16 = (unsigned)(((M + 15) / 16) * a.ntn);
    int ks = 1;
    if (ksplit >= 0) {
        ks = tok_plan_split(a, M, ksplit, sige_hip_token_linear_ksplit(M, N, K, ln, geglu, parts, 0), st);
        if (!ks) return SIGE_HIP_EUNSUPPORTED;
    }
    if (ks > 1) launch_tok_split(a, ln, geglu != 0, blocks16, st);
    else if (ksplit <= 0 && tok_big(M, a.ntn)) launch_tok<64>(a, ln, geglu != 0, (unsigned)(((M + 63) / 64) * a.ntn), st);
    else launch_tok<16>(a, ln, geglu != 0, blocks16, st);
    return launch_status();
}

}  // namespace sige

extern "C" int sige_hip_token_linear_f32(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                         const float *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                                         float *out0, float *out1, float *out2, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_token_linear_f32, x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, stream);
    return token_linear_f32(x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, -1, stream);
}

extern "C" int sige_hip_token_linear_split_f32(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                               const float *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                                               float *out0, float *out1, float *out2, int ksplit, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_token_linear_split_f32, x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, ksplit, stream);
    if (ksplit < 0) return SIGE_HIP_EINVAL;
    return token_linear_f32(x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, ksplit, stream);
}

// The split the rule picks, for either unit: 0 = unsupported, 1 = no split (also wherever the 64-token form runs)
extern "C" int sige_hip_token_linear_ksplit(int64_t M, int N, int K, int layer_norm, int geglu, int parts, int f16) {
    if (f16) return token_linear_ksplit_f16(M, N, K, layer_norm, geglu, parts);
    if (!sige_hip_token_linear_supported(M, N, K, layer_norm, geglu, parts)) return 0;
    const int ntn = tok_ntn(N, K, geglu);
    if (M == 0 || tok_big(M, ntn)) return 1;
    return tok_split_rule(M, ntn, tok_nchunks(K), kTokSplitMinChunks);
}
