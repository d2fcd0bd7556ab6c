// The token linear (token_linear.hip: out[M, N] = epilogue( prologue(x)[M, K] . W^T ), same arguments, prologue and epilogues) with fp16
// OPERANDS on v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x32_f16: the token linear of the f16 compute mode -- fp32 tensors in memory, fp32
// LayerNorm, fp32 accumulation, fp32 bias / GEGLU / residual; prologue(x) and W each rounded to nearest even to fp16.
//
// Two row-block forms: 64 tokens x 64 columns per workgroup (2 x 2 tiles of 32x32 per wave, two MFMA steps of depth 16 per chunk) and 16
// tokens x 64 columns (1 x 4 tiles of 16x16, one step of depth 32).  A chunk is 128 channels; the four waves split K -- wave w owns
// channels 32 w .. 32 w + 31 of every chunk -- and meet in LDS in wave order (token_linear.hpp): no atomics, the same call gives the same
// bits.  K % 32 == 0 (the MFMA's depth): a wave's slice of a chunk is whole or absent.
//
// A: a lane owns a row.  32x32x16 -- row lane & 31 of each M tile, channels 16 kq .. 16 kq + 15 of the wave's 32 (kq = lane >> 5; step s
// contracts the lane's channels 8 s .. 8 s + 7); 16x16x32 -- row lane & 15, channels 8 kg .. 8 kg + 7 (kg = lane >> 4).  Either way the 8
// channels of a step are two adjacent 16-byte buffer loads of fp32 x and a lane's bytes of a chunk are contiguous (64 | 32 bytes; in the
// 16-token form the four lanes of a row cover one 128-byte line); LayerNorm in fp32 in registers, then fptrunc (v_cvt_pk_f16_f32, round
// to nearest even) to the f16x8 operand.
// B: packed once as fp16 in that channel order: a (column block, chunk, wave) unit is 64 columns x 32 channels = 4096 bytes,
// [N tile][step][lane of the 32x32x16 form][8 halves] -- every B fragment is ONE 16-byte load per lane, N tile and step; zero padded to 64
// columns and whole chunks.  The 16-token form's lane (row rl, group kg) of N tile t reads what lane (kg >> 1) * 32 + (t & 1) * 16 + rl
// of step kg & 1 of N tile t >> 1 holds.  GEGLU: a block's 64 packed columns are 32 value columns and THEIR 32 gate columns.
// Row tails and dead channel slices: the buffer descriptor's range check (offset kOOB reads 0); column tails: the zero padding.
// Arithmetic contract: include/sige_hip.h (sige_hip_token_linear_f16c).  Form rule, resources and times: DESIGN.md 5.30.
#include "token_linear.hpp"

namespace sige {
namespace {

__device__ __forceinline__ f16x8 tok_pack8(f32x4 a, f32x4 b) {  // (fptrunc: round to nearest even)
    const f16x4 lo = __builtin_convertvector(a, f16x4);
    const f16x4 hi = __builtin_convertvector(b, f16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// BM: token rows per workgroup (64 | 16).  SPLIT (16-token form): blockIdx.y of gridDim.y = a.ksplit workgroups that share the output
// block blockIdx.x -- the split is the slow grid dimension, so the workgroups of one block are dispatched a whole grid row apart, to
// different CUs / XCDs --, each on its own run of chunks; they finish inside the launch (token_linear.hpp: tok_finish_split).
template <int BM, bool LN, bool GEGLU, bool SPLIT = false>
__global__ __launch_bounds__(256) void token_linear_f16_kernel(const typename std::conditional<SPLIT, TokSplitArgs, TokArgs>::type a) {
    static_assert(!SPLIT || BM == 16, "the K split is a variant of the 16-token form");
    kernarg_touch<sizeof(a)>();
    constexpr bool BIG = BM == 64;
    constexpr int MT = BIG ? 2 : 1;   // M tiles per wave
    constexpr int NT = BIG ? 2 : 4;   // N tiles per wave
    constexpr int ST = BIG ? 2 : 1;   // MFMA steps per wave and chunk (depth 16 | 32: the wave's 32 channels)
    constexpr int KPL = 8 * ST;       // consecutive channels of the lane's row per chunk
    __shared__ __attribute__((aligned(16))) float smem[4 * BM * kTokRP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = blockIdx.x % a.ntn, mtile = blockIdx.x / a.ntn;
    const int row0 = mtile * BM;
    const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, a.x_bytes, 0x00020000);
    const rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.packed), 0, a.w_bytes, 0x00020000);
    const int rl = BIG ? (lane & 31) : (lane & 15), kg = BIG ? (lane >> 5) : (lane >> 4);

    float mean[MT], rstd[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mean[mt] = 0.f, rstd[mt] = 1.f;
    if constexpr (LN) tok_row_stats<BM>(a, rx, smem, tid, row0, rl, mean, rstd);

    // ---- K loop: the registers of chunk c + 1 are requested before the MFMAs of chunk c ----
    unsigned abase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = row0 + mt * 32 + rl;
        abase[mt] = row < a.M ? (unsigned)(row * a.K + kg * KPL) * 4u : kOOB;
    }
    const unsigned bbase = ((unsigned)(ntile * a.nchunks) * 4u + wave) * 4096u;
    unsigned boff[NT][ST];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int s = 0; s < ST; ++s)
            boff[nt][s] = BIG ? bbase + (nt * 2 + s) * 1024 + lane * 16
                              : bbase + ((nt >> 1) * 2 + (kg & 1)) * 1024 + ((kg >> 1) * 32 + (nt & 1) * 16 + rl) * 16;
    struct Frag {
        f32x4 a[MT][2 * ST], b[NT][ST], g[2 * ST], e[2 * ST];  // (b: 8 halves, carried as the 16 bytes they were loaded as)
    };
    auto load = [&](int chunk, Frag &f) {
        const int kb = chunk * 128 + wave * 32;
        const bool live = kb < a.K;  // (wave-uniform; K % 32 == 0: a wave's slice of a chunk is whole or absent)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int p = 0; p < 2 * ST; ++p) f.a[mt][p] = buf4(rx, live ? abase[mt] + (unsigned)(kb + 4 * p) * 4u : kOOB);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int s = 0; s < ST; ++s) f.b[nt][s] = buf4(rw, boff[nt][s] + (unsigned)chunk * 16384u);
        if constexpr (LN) {
            const int kk = min(kb + kg * KPL, a.K - KPL);
#pragma unroll
            for (int p = 0; p < 2 * ST; ++p) {
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
            const bool live = c * 128 + wave * 32 < a.K;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int p = 0; p < 2 * ST; ++p)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float z = (cur.a[mt][p][j] - mean[mt]) * rstd[mt] * cur.g[p][j] + cur.e[p][j];
                        cur.a[mt][p][j] = live ? z : 0.f;
                    }
        }
#pragma unroll
        for (int s = 0; s < ST; ++s) {
            f16x8 ah[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ah[mt] = tok_pack8(cur.a[mt][2 * s], cur.a[mt][2 * s + 1]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f16x8 bh = __builtin_bit_cast(f16x8, cur.b[nt][s]);
                    if constexpr (BIG) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bh, acc[mt][nt], 0, 0, 0);
                    else acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], bh, acc[mt][nt], 0, 0, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }

    if constexpr (SPLIT) tok_finish_split<GEGLU>(a, smem, acc, tid, wave, ntile, row0, rl, kg, (int)blockIdx.x, (int)blockIdx.y);
    else tok_finish<BM, GEGLU>(a, smem, acc, tid, wave, ntile, row0, rl, kg);
}

// packed (halves)[((ntile * nchunks + chunk) * 4 + wave) * 2048 + ((nt * 2 + step) * 64 + lane) * 8 + j] =
//   fp16(W[col(ntile, nt * 32 + (lane & 31))][chunk * 128 + wave * 32 + (lane >> 5) * 16 + step * 8 + j]), 0 beyond N / K
// (8 halves = one 16-byte store per lane; the unit count is a multiple of 1024, the grid is exact)
__global__ __launch_bounds__(256) void token_linear_pack_f16_kernel(const float *__restrict__ w, int N, int K, int D, int nchunks,
                                                                   f16x8 *__restrict__ packed) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(u & 63), sub = (int)(u >> 6) & 3, wave = (int)(u >> 8) & 3;
    const int rest = (int)(u >> 10);
    const int chunk = rest % nchunks, ntile = rest / nchunks;
    const int nl = (sub >> 1) * 32 + (lane & 31);
    // GEGLU (D > 0): block j holds value columns 32 j .. 32 j + 31, then their gate columns D + 32 j ..
    const int n = D > 0 ? (nl < 32 ? ntile * 32 + nl : D + ntile * 32 + nl - 32) : ntile * 64 + nl;
    const int k = chunk * 128 + wave * 32 + (lane >> 5) * 16 + (sub & 1) * 8;
    const bool ok = n < N && k < K;  // (K % 8 == 0: the 8 channels are all there or none)
    const f32x4 *src = reinterpret_cast<const f32x4 *>(w + (ok ? (unsigned)(n * K + k) : 0u));  // (N K <= 2^30: packed_size_f16)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 h = __builtin_bit_cast(u32x4, tok_pack8(src[0], src[1]));  // (every lane loads: the clamped address; `ok` masks the bits)
    packed[u] = __builtin_bit_cast(f16x8, h & (ok ? 0xffffffffu : 0u));
}

// 64-column blocks of the packed tensor; 0 = the shape is not supported
inline int tokh_ntn(int N, int K, int geglu) {
    if (N <= 0 || K <= 0 || N % 16 || K % 32) return 0;
    if (geglu) return (N % 2 || (N / 2) % 32) ? 0 : N / 64;
    return (N + 63) / 64;
}
inline int tokh_nchunks(int K) { return (K + 127) / 128; }

// The 64-token form reads every weight byte for four times the rows, but its grid comes in whole 64-row blocks and -- measured -- in
// rounds of ONE workgroup per CU: it runs where real rows fill at least 0.7 of the row slots of those rounds.  Timed at the 35 shapes of
// DESIGN.md 5.30's tables: every shape at or above 0.70 has the 64-token form level or ahead (0.81 - 0.99 of the 16-token form's time),
// every shape at or below 0.64 has it level or behind (1.00 - 2.4 x).  (The fp32 kernel's rule -- 0.8 of rounds of 512 -- would send three
// shapes where this form wins by 7 - 10 % to the 16-token form.)
constexpr int kTokRoundF16 = 256;
constexpr double kTokFillF16 = 0.7;
// every split of the K split keeps at least this many 128-channel chunks (the rule's other constants: token_linear.hpp)
constexpr int kTokSplitMinChunksF16 = 10;

template <int BM>
void launch_tokh(const TokArgs &a, bool ln, bool geglu, unsigned grid, hipStream_t st) {
    if (ln && geglu) token_linear_f16_kernel<BM, true, true><<<grid, 256, 0, st>>>(a);
    else if (ln) token_linear_f16_kernel<BM, true, false><<<grid, 256, 0, st>>>(a);
    else if (geglu) token_linear_f16_kernel<BM, false, true><<<grid, 256, 0, st>>>(a);
    else token_linear_f16_kernel<BM, false, false><<<grid, 256, 0, st>>>(a);
}

// grid (output blocks, splits)
void launch_tokh_split(const TokSplitArgs &a, bool ln, bool geglu, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks, (unsigned)a.ksplit);
    if (ln && geglu) token_linear_f16_kernel<16, true, true, true><<<grid, 256, 0, st>>>(a);
    else if (ln) token_linear_f16_kernel<16, true, false, true><<<grid, 256, 0, st>>>(a);
    else if (geglu) token_linear_f16_kernel<16, false, true, true><<<grid, 256, 0, st>>>(a);
    else token_linear_f16_kernel<16, false, false, true><<<grid, 256, 0, st>>>(a);
}

}  // namespace
}  // namespace sige

using namespace sige;

extern "C" size_t sige_hip_token_linear_packed_size_f16(int N, int K, int geglu) {
    const int ntn = tokh_ntn(N, K, geglu);
    if (!ntn) return 0;
    const size_t halves = (size_t)ntn * tokh_nchunks(K) * 8192;
    return halves * 2 > 0x7fffffffUL ? 0 : halves;  // (32-bit byte offsets into the packed tensor)
}

extern "C" int sige_hip_token_linear_supported_f16c(int64_t M, int N, int K, int layer_norm, int geglu, int parts) {
    if (M < 0 || parts < 1 || parts > 3 || !sige_hip_token_linear_packed_size_f16(N, K, geglu)) return 0;
    if (layer_norm && K > kTokMaxLnK) return 0;
    if (parts > 1 && (geglu || N % parts || (N / parts) % 64)) return 0;
    // 32-bit element offsets into x and the outputs, and a one-dimensional grid of 16-row workgroups
    if (M * K * 4 > 0x7fffffffL || M * N * 4 > 0x7fffffffL) return 0;
    if (((M + 15) / 16) * tokh_ntn(N, K, geglu) > 0x7fffffffL) return 0;
    return 1;
}

extern "C" int sige_hip_token_linear_pack_f16(const float *w, int N, int K, int geglu, void *packed, void *stream) {
    if (N <= 0 || K <= 0) return SIGE_HIP_EINVAL;
    if (!w || !packed) return SIGE_HIP_EINVAL;
    const size_t halves = sige_hip_token_linear_packed_size_f16(N, K, geglu);
    if (!halves || !tok_al16(w) || !tok_al16(packed)) return SIGE_HIP_EUNSUPPORTED;
    token_linear_pack_f16_kernel<<<(unsigned)(halves / 2048), 256, 0, as_stream(stream)>>>(w, N, K, geglu ? N / 2 : 0, tokh_nchunks(K),
                                                                                          static_cast<f16x8 *>(packed));
    return launch_status();
}

namespace sige {

static bool tokh_big(int64_t M, int ntn) {
    const int knob = tuning(SIGE_HIP_TUNE_TOKEN_LINEAR_FORM);
    return knob ? knob == 2 : tok_fill64(M, ntn, kTokRoundF16) >= kTokFillF16;
}

int token_linear_ksplit_f16(int64_t M, int N, int K, int layer_norm, int geglu, int parts) {
    if (!sige_hip_token_linear_supported_f16c(M, N, K, layer_norm, geglu, parts)) return 0;
    const int ntn = tokh_ntn(N, K, geglu);
    if (M == 0 || tokh_big(M, ntn)) return 1;
    return tok_split_rule(M, ntn, tokh_nchunks(K), kTokSplitMinChunksF16);
}

// Both launching entry points.  ksplit: -1 = sige_hip_token_linear_f16c (form by fill, no split) | sige_hip_token_linear_split_f16c's
static int token_linear_f16c(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps, const void *packed,
                             const float *bias, int N, int geglu, const float *residual, int parts, float *out0, float *out1, float *out2,
                             int ksplit, void *stream) {
    if (M < 0 || K <= 0 || N <= 0 || parts < 1 || parts > 3 || ksplit < -1) return SIGE_HIP_EINVAL;
    if (M == 0) return SIGE_HIP_OK;
    if (!x || !packed || !out0 || (parts > 1 && !out1) || (parts > 2 && !out2) || (ln_gamma && !ln_beta)) return SIGE_HIP_EINVAL;
    if (!sige_hip_token_linear_supported_f16c(M, N, K, ln_gamma != nullptr, geglu, parts)) return SIGE_HIP_EUNSUPPORTED;
    if (parts > 1 && residual) return SIGE_HIP_EUNSUPPORTED;
    if (!tok_al16(x) || !tok_al16(packed) || !tok_al16(out0) || !tok_al16(out1) || !tok_al16(out2) || !tok_al16(bias) || !tok_al16(residual) || !tok_al16(ln_gamma) || !tok_al16(ln_beta))
        return SIGE_HIP_EUNSUPPORTED;
    TokSplitArgs a;
    static_cast<TokArgs &>(a) = tok_args(x, M, K, ln_gamma, ln_beta, ln_eps, bias, N, geglu, residual, parts, out0, out1, out2);
    a.packed = packed;
    a.ntn = tokh_ntn(N, K, geglu);
    a.nchunks = tokh_nchunks(K);
    a.tpp = parts > 1 ? a.No / 64 : a.ntn;
    a.w_bytes = (int)(sige_hip_token_linear_packed_size_f16(N, K, geglu) * 2);
    hipStream_t st = as_stream(stream);
    const bool ln = ln_gamma != nullptr;
    const unsigned blocks16 = (unsigned)(((M + 15) / 16) * a.ntn);
    int ks = 1;
    if (ksplit >= 0) {
        ks = tok_plan_split(a, M, ksplit, token_linear_ksplit_f16(M, N, K, ln, geglu, parts), st);
        if (!ks) return SIGE_HIP_EUNSUPPORTED;
    }
    if (ks > 1) launch_tokh_split(a, ln, geglu != 0, blocks16, st);
    else if (ksplit <= 0 && tokh_big(M, a.ntn)) launch_tokh<64>(a, ln, geglu != 0, (unsigned)(((M + 63) / 64) * a.ntn), st);
    else launch_tokh<16>(a, ln, geglu != 0, blocks16, st);
    return launch_status();
}

}  // namespace sige

extern "C" int sige_hip_token_linear_f16c(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                          const void *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                                          float *out0, float *out1, float *out2, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_token_linear_f16c, x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, stream);
    return token_linear_f16c(x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, -1, stream);
}

extern "C" int sige_hip_token_linear_split_f16c(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                                const void *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                                                float *out0, float *out1, float *out2, int ksplit, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_token_linear_split_f16c, x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, ksplit, stream);
    if (ksplit < 0) return SIGE_HIP_EINVAL;
    return token_linear_f16c(x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, ksplit, stream);
}
