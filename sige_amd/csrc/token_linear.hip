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
#include "conv_mfma.hpp"

namespace sige {
namespace {

constexpr int kTokMaxLnK = 2048;      // token_ops.hip's limit (kMaxPerLane * 64)
constexpr int kTokSlots = 512;        // 64-token workgroups the chip holds at once: 256 CUs x 2 (LDS and registers)

struct TokArgs {
    const float *x, *gamma, *beta, *packed, *bias, *residual;
    float *out0, *out1, *out2;
    float eps;
    int M, K, N;            // N: columns of the product (2 D for GEGLU)
    int No;                 // columns (= row stride) of one output: N / parts, D for GEGLU
    int ntn, nchunks, tpp;  // 64-column blocks, 64-channel chunks, column blocks per part
    int x_bytes, w_bytes;   // ranges of the two buffer descriptors
};

__device__ __forceinline__ f32x4 buf4(rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ float gelu_erf(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

// BM: token rows per workgroup (64 | 16).
template <int BM, bool LN, bool GEGLU>
__global__ __launch_bounds__(256) void token_linear_kernel(const TokArgs a) {
    kernarg_touch<sizeof(TokArgs)>();
    constexpr bool BIG = BM == 64;
    constexpr int MT = BIG ? 2 : 1;   // M tiles per wave
    constexpr int NT = BIG ? 2 : 4;   // N tiles per wave
    constexpr int AP = BIG ? 2 : 1;   // 16-byte A pieces per lane, tile and chunk
    constexpr int RP = 68;
    __shared__ __attribute__((aligned(16))) float smem[4 * BM * RP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = blockIdx.x % a.ntn, mtile = blockIdx.x / a.ntn;
    const int row0 = mtile * BM;
    const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, a.x_bytes, 0x00020000);
    const rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.packed), 0, a.w_bytes, 0x00020000);
    // this lane's rows and channel group: 32x32x2 -- row lane & 31 of each M tile, channels 8 kq .. 8 kq + 7 of the wave's 16 (MFMA step
    // s contracts channels s and 8 + s); 16x16x4 -- row lane & 15, channels 4 kg .. 4 kg + 3 (step s: channels s, 4 + s, 8 + s, 12 + s)
    const int rl = BIG ? (lane & 31) : (lane & 15), kg = BIG ? (lane >> 5) : (lane >> 4);
    constexpr int KPL = BIG ? 8 : 4;  // channels per lane and chunk

    // ---- LayerNorm statistics of the workgroup's rows: 256 / BM lanes per row, two passes over the row ----
    float mean[MT], rstd[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mean[mt] = 0.f, rstd[mt] = 1.f;
    if constexpr (LN) {
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

    Frag cur, nxt;
    load(0, cur);
    for (int c = 0; c < a.nchunks; ++c) {
        load(min(c + 1, a.nchunks - 1), nxt);
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

    auto sum4 = [&](int m, int c) -> float4 {  // the four waves' shares, in wave order
        const float *r0 = smem + m * RP + c;
        float4 s = *reinterpret_cast<const float4 *>(r0);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float4 v = *reinterpret_cast<const float4 *>(r0 + w * BM * RP);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        return s;
    };
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

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 64-column blocks of the packed tensor; 0 = the shape is not supported
inline int tok_ntn(int N, int K, int geglu) {
    if (N <= 0 || K <= 0 || N % 16 || K % 16) return 0;
    if (geglu) return (N % 2 || (N / 2) % 32) ? 0 : N / 64;
    return (N + 63) / 64;
}
inline int tok_nchunks(int K) { return (K + 63) / 64; }

template <int BM>
void launch_tok(const TokArgs &a, bool ln, bool geglu, unsigned grid, hipStream_t st) {
    if (ln && geglu) token_linear_kernel<BM, true, true><<<grid, 256, 0, st>>>(a);
    else if (ln) token_linear_kernel<BM, true, false><<<grid, 256, 0, st>>>(a);
    else if (geglu) token_linear_kernel<BM, false, true><<<grid, 256, 0, st>>>(a);
    else token_linear_kernel<BM, false, false><<<grid, 256, 0, st>>>(a);
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
    if (!floats || !al16(w) || !al16(packed)) return SIGE_HIP_EUNSUPPORTED;
    token_linear_pack_kernel<<<(unsigned)(floats / 1024), 256, 0, as_stream(stream)>>>(w, N, K, geglu ? N / 2 : 0, tok_nchunks(K), packed);
    return launch_status();
}

extern "C" int sige_hip_token_linear_f32(const float *x, int64_t M, int K, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                         const float *packed, const float *bias, int N, int geglu, const float *residual, int parts,
                                         float *out0, float *out1, float *out2, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_token_linear_f32, x, M, K, ln_gamma, ln_beta, ln_eps, packed, bias, N, geglu, residual, parts, out0, out1, out2, stream);
    if (M < 0 || K <= 0 || N <= 0 || parts < 1 || parts > 3) return SIGE_HIP_EINVAL;
    if (M == 0) return SIGE_HIP_OK;
    if (!x || !packed || !out0 || (parts > 1 && !out1) || (parts > 2 && !out2) || (ln_gamma && !ln_beta)) return SIGE_HIP_EINVAL;
    if (!sige_hip_token_linear_supported(M, N, K, ln_gamma != nullptr, geglu, parts)) return SIGE_HIP_EUNSUPPORTED;
    if (parts > 1 && residual) return SIGE_HIP_EUNSUPPORTED;
    if (!al16(x) || !al16(packed) || !al16(out0) || !al16(out1) || !al16(out2) || !al16(bias) || !al16(residual) || !al16(ln_gamma) || !al16(ln_beta))
        return SIGE_HIP_EUNSUPPORTED;
    TokArgs a;
    a.x = x; a.gamma = ln_gamma; a.beta = ln_beta; a.packed = packed; a.bias = bias; a.residual = residual;
    a.out0 = out0; a.out1 = parts > 1 ? out1 : out0; a.out2 = parts > 2 ? out2 : out0;
    a.eps = ln_eps;
    a.M = (int)M; a.K = K; a.N = N;
    a.No = geglu ? N / 2 : N / parts;
    a.ntn = tok_ntn(N, K, geglu);
    a.nchunks = tok_nchunks(K);
    a.tpp = parts > 1 ? a.No / 64 : a.ntn;
    a.x_bytes = (int)(M * K * 4);
    a.w_bytes = (int)(sige_hip_token_linear_packed_size(N, K, geglu) * 4);
    // grid fill (as plan_conv chooses its tile): the 64-token form reads every weight byte for four times the rows, but its grid comes
    // in rounds of kTokSlots workgroups and in whole 64-row blocks; it runs where real rows fill at least 0.8 of the rounds' slots
    // (measured per shape: DESIGN.md 5.12), the 16-token form's four times finer grid everywhere else
    const long b64 = ((M + 63) / 64) * a.ntn, rounds = (b64 + kTokSlots - 1) / kTokSlots;
    const double fill = (double)M * a.ntn / (64.0 * (double)(rounds * kTokSlots));
    const int knob = tuning(SIGE_HIP_TUNE_TOKEN_LINEAR_FORM);
    const bool big = knob ? knob == 2 : fill >= 0.8;
    hipStream_t st = as_stream(stream);
    if (big) launch_tok<64>(a, ln_gamma != nullptr, geglu != 0, (unsigned)(((M + 63) / 64) * a.ntn), st);
    else launch_tok<16>(a, ln_gamma != nullptr, geglu != 0, (unsigned)(((M + 15) / 16) * a.ntn), st);
    return launch_status();
}
