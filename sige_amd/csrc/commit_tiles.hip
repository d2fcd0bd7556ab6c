// sige_hip_commit_tiles: the tiles of many cached tensors copied in ONE launch -- how an accepted edit becomes the new original.
//
// The reference commits an edit by a sparse forward with `sparse_update` set: every Scatter, ScatterWithBlockResidual and
// ScatterGather copies its WHOLE result over its cache (sige/nn/scatter.py:59-60,114-129, scatter_gather.py:65-77); for DDPM-256
// that is 38 tensors, 672.7 MB.  The bytes that differ are the active tiles.  One launch here executes a list of records
// (include/sige_hip.h: sige_hip_commit_record), each "write the pixels under the tiles of `idx` of one channels-last destination from
// a full tensor of the same shape, or from the tiles a conv wrote", optionally through SiLU(scale[c] * v + shift[c]) and into fp16
// storage.  The records travel BY VALUE in the kernel arguments -- no staging copy, nothing of the caller is read later, the launch
// can be captured --, kCap = SIGE_HIP_COMMIT_CAPACITY of them per launch: 8 + 48 * (4 + 72) = 3656 bytes of the 4096 a kernel takes.
//
// Work split: a workgroup is one (record, tile, 64-channel chunk); 256 lanes = 16 pixels x 16 four-channel units, one 16-byte
// load and store each (a 4x4 tile in one pass).  The map from blockIdx is scalar arithmetic on the kernel-argument segment: the
// per-record workgroup prefix counts are 48 dwords read in three wide scalar loads and compared branch-free; the record found is
// read from the segment at a run-time index (the constant address space: scalar loads, never scratch).
// no division by a run-time value (the chunk count and the tile width come with host-computed reciprocals, the
// stride as a shift), no load behind an exec-masked branch (lanes off the tile or off the image load a clamped address and skip the
// store only).
//
// Doubly covered pixels: two tiles of one record covering one pixel are written in no defined order.  A full source writes the same
// value twice.  A tile source is the reference's scatter, where the later tile wins -- but the lists reduce_mask builds do not
// overlap in output space, so there is no ordering machinery here.
#include <climits>
#include <vector>

#include "common.hpp"

namespace sige {

constexpr int kCap = SIGE_HIP_COMMIT_CAPACITY;
constexpr int kChunk = 64;            // channels per workgroup
constexpr int kLanes = 256;
constexpr int kMaxUnits = 1 << 22;    // (tile, chunk) units of one launch: the reciprocal of the chunk count is exact below 2^32 / 256

enum { COMMIT_TILE_SOURCE = 1, COMMIT_DST_F16 = 2, COMMIT_AFFINE = 4 };

struct CommitRec {  // 72 bytes
    const float *src;
    void *dst;
    const int32_t *idx;
    const float *scale, *shift;
    int N, C, H, W;
    uint32_t chunk_magic;   // floor(2^32 / chunks) + 1: unit / chunks == (unit * magic) >> 32 for unit * chunks < 2^32
    uint32_t s_magic;       // floor(2^16 / s) + 1:      p / s == (p * magic) >> 16 for p < 256, s <= 16
    uint8_t r, s, chunks_m1, flags;
    int8_t offH, offW;
    uint8_t shH, shW;       // log2 of the stride
};
static_assert(sizeof(CommitRec) == 72, "record layout");

struct CommitArgs {
    int n, pad;
    int wg_end[kCap];       // workgroups of this launch up to and including record i (INT_MAX past the last record)
    CommitRec rec[kCap];
};
static_assert(sizeof(CommitArgs) == 8 + 76 * kCap && sizeof(CommitArgs) <= 4096 - 256, "kernel-argument space (256 bytes left for hidden arguments)");

typedef _Float16 c_h16x4 __attribute__((ext_vector_type(4)));

// C's division (towards zero) by 2^sh
__device__ __forceinline__ int cdiv_pow2(int x, int sh) { return (x + ((x >> 31) & ((1 << sh) - 1))) >> sh; }

// PASSES: 16-pixel passes a workgroup makes over its tile (1: every tile of the launch has at most 16 pixels, 4: 64, 16: 256),
// unrolled -- no rolled loop whose every trip waits for its own load
template <int PASSES>
__global__ __launch_bounds__(kLanes) void commit_tiles_kernel(CommitArgs) {
    typedef const __attribute__((address_space(4))) CommitArgs *kargs_t;
    kargs_t a = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument: offset 0 of the segment)
    const int bid = blockIdx.x;
    // record = how many prefix counts lie at or below this workgroup; its first workgroup = the largest of them
    int ri = 0, start = 0;
#pragma unroll
    for (int i = 0; i < kCap; ++i) {
        const int e = a->wg_end[i];
        const bool past = bid >= e;
        ri += past ? 1 : 0;
        start = past ? e : start;
    }
    ri = __builtin_amdgcn_readfirstlane(ri);  // (uniform by construction: keeps the record's fields in scalar registers)
    start = __builtin_amdgcn_readfirstlane(start);
    typedef const __attribute__((address_space(4))) CommitRec *krec_t;
    const krec_t Rp = &a->rec[ri];
    const float *src = Rp->src, *scale = Rp->scale, *shift = Rp->shift;
    void *dst = Rp->dst;
    const int32_t *idx = Rp->idx;
    const int C = Rp->C, H = Rp->H, W = Rp->W, r = Rp->r, s = Rp->s, chunks = Rp->chunks_m1 + 1, flags = Rp->flags;
    const uint32_t chunk_magic = Rp->chunk_magic, s_magic = Rp->s_magic;
    const int offH = Rp->offH, offW = Rp->offW, shH = Rp->shH, shW = Rp->shW;

    const unsigned unit = (unsigned)(bid - start);
    const int n = chunks > 1 ? (int)(((uint64_t)unit * chunk_magic) >> 32) : (int)unit;
    const int chunk = (int)unit - n * chunks;
    const int h0 = cdiv_pow2(offH + idx[2 * n], shH), w0 = cdiv_pow2(offW + idx[2 * n + 1], shW);

    const int tid = threadIdx.x, q = tid & 15, p0 = tid >> 4;
    const int c = chunk * kChunk + q * 4;
    const bool cok = c < C;
    const int cc = cok ? c : 0;
    const int RS = r * s;
    const bool tile = flags & COMMIT_TILE_SOURCE, affine = flags & COMMIT_AFFINE, f16 = flags & COMMIT_DST_F16;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (affine) {  // (a uniform branch)
        sc = *reinterpret_cast<const float4 *>(scale + cc);
        sh = *reinterpret_cast<const float4 *>(shift + cc);
    }
    // every pass's load is issued before the first store: lanes past the tile, or off the image, load a clamped address (a pass
    // past the tile reads its last pixel again) and skip the store only
    float4 v[PASSES];
    size_t at[PASSES];
    bool ok[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int p = k * 16 + p0;
        const int pc = min(p, RS - 1);
        const int th = (int)(((unsigned)pc * s_magic) >> 16), tw = pc - th * s;
        const int h = h0 + th, w = w0 + tw;
        ok[k] = cok && p < RS && h >= 0 && h < H && w >= 0 && w < W;
        const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1);
        at[k] = (size_t)(hc * W + wc) * C + cc;
        const int pix = tile ? (n * r + th) * s + tw : hc * W + wc;
        v[k] = *reinterpret_cast<const float4 *>(src + (size_t)pix * C + cc);
    }
    if (affine) {
        // the expression of affine_act_nhwc_kernel (nhwc_ops.hip): scale, then shift, separately rounded; swish()
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            float4 z = v[k];
            z.x = sc.x * z.x; z.y = sc.y * z.y; z.z = sc.z * z.z; z.w = sc.w * z.w;
            z.x = sh.x + z.x; z.y = sh.y + z.y; z.z = sh.z + z.z; z.w = sh.w + z.w;
            z.x = swish(z.x); z.y = swish(z.y); z.z = swish(z.z); z.w = swish(z.w);
            v[k] = z;
        }
    }
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        if (!ok[k]) continue;
        if (f16) {
            const c_h16x4 hv = {(_Float16)v[k].x, (_Float16)v[k].y, (_Float16)v[k].z, (_Float16)v[k].w};
            *reinterpret_cast<c_h16x4 *>(static_cast<_Float16 *>(dst) + at[k]) = hv;
        } else {
            store_out4(static_cast<float *>(dst) + at[k], v[k]);
        }
    }
}

static bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int log2_exact(int v) {
    for (int s = 0; s < 8; ++s)
        if (v == (1 << s)) return s;
    return -1;
}

// the status of one record (include/sige_hip.h); fills the kernel's form of it
static int pack_record(const sige_hip_commit_record &r, CommitRec *o, long *units) {
    if (r.N < 0 || r.B <= 0 || r.C <= 0 || r.H <= 0 || r.W <= 0 || r.r <= 0 || r.s <= 0 || r.strideH <= 0 || r.strideW <= 0) return SIGE_HIP_EINVAL;
    if ((r.scale == nullptr) != (r.shift == nullptr)) return SIGE_HIP_EINVAL;
    if (r.N > 0 && (!r.src || !r.dst || !r.idx)) return SIGE_HIP_EINVAL;
    const int shH = log2_exact(r.strideH), shW = log2_exact(r.strideW);
    if (r.B != 1 || r.C % 4 || r.C > 16384 || r.r > 16 || r.s > 16 || shH < 0 || shW < 0) return SIGE_HIP_EUNSUPPORTED;
    if (r.offsetH < -127 || r.offsetH > 127 || r.offsetW < -127 || r.offsetW > 127) return SIGE_HIP_EUNSUPPORTED;
    if ((long)r.H * r.W >= 0x7fffffffL || stacked_shift(r.H) != 0) return SIGE_HIP_EUNSUPPORTED;
    if (!aligned(r.src, 16) || !aligned(r.scale, 16) || !aligned(r.shift, 16) || !aligned(r.dst, r.dst_f16 ? 8 : 16)) return SIGE_HIP_EUNSUPPORTED;
    const int chunks = (r.C + kChunk - 1) / kChunk;
    *units = (long)r.N * chunks;
    if (*units > kMaxUnits) return SIGE_HIP_EUNSUPPORTED;
    o->src = r.src; o->dst = r.dst; o->idx = r.idx; o->scale = r.scale; o->shift = r.shift;
    o->N = r.N; o->C = r.C; o->H = r.H; o->W = r.W;
    o->chunk_magic = chunks > 1 ? (uint32_t)((1ull << 32) / (unsigned)chunks) + 1u : 0u;  // (one chunk: the kernel takes unit itself)
    o->s_magic = 65536u / (unsigned)r.s + 1u;
    o->r = (uint8_t)r.r; o->s = (uint8_t)r.s; o->chunks_m1 = (uint8_t)(chunks - 1);
    o->flags = (uint8_t)((r.tile_source ? COMMIT_TILE_SOURCE : 0) | (r.dst_f16 ? COMMIT_DST_F16 : 0) | (r.scale ? COMMIT_AFFINE : 0));
    o->offH = (int8_t)r.offsetH; o->offW = (int8_t)r.offsetW; o->shH = (uint8_t)shH; o->shW = (uint8_t)shW;
    return SIGE_HIP_OK;
}

static int commit_impl(const sige_hip_commit_record *records, int n, int *launches, void *stream) {
    if (launches) *launches = 0;
    if (n < 0 || (n > 0 && !records)) return SIGE_HIP_EINVAL;
    // the whole list is judged before the first launch: a refused list leaves every destination as it was
    std::vector<CommitRec> recs;
    std::vector<long> units;
    recs.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        CommitRec c{};
        long u = 0;
        const int status = pack_record(records[i], &c, &u);
        if (status != SIGE_HIP_OK) return status;
        if (u == 0) continue;  // (no tile: the record is dropped, and a list of such records launches nothing)
        recs.push_back(c);
        units.push_back(u);
    }
    for (size_t first = 0; first < recs.size(); first += kCap) {
        long total = 0;
        for (size_t i = first; i < recs.size() && i < first + kCap; ++i) total += units[i];
        if (total > kMaxUnits) return SIGE_HIP_EUNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    int issued = 0;
    for (size_t first = 0; first < recs.size(); first += kCap) {
        CommitArgs a;
        const int m = (int)(recs.size() - first < (size_t)kCap ? recs.size() - first : (size_t)kCap);
        a.n = m; a.pad = 0;
        int end = 0, max_rs = 0;
        for (int i = 0; i < kCap; ++i) {
            if (i < m) {
                end += (int)units[first + i];
                max_rs = max_rs > recs[first + i].r * recs[first + i].s ? max_rs : recs[first + i].r * recs[first + i].s;
                a.wg_end[i] = i == m - 1 ? INT_MAX : end;  // (the last record owns every workgroup from its first on)
                a.rec[i] = recs[first + i];
            } else {
                a.wg_end[i] = INT_MAX;
                a.rec[i] = CommitRec{};
            }
        }
        if (max_rs <= 16) commit_tiles_kernel<1><<<end, kLanes, 0, st>>>(a);
        else if (max_rs <= 64) commit_tiles_kernel<4><<<end, kLanes, 0, st>>>(a);
        else commit_tiles_kernel<16><<<end, kLanes, 0, st>>>(a);
        ++issued;
    }
    if (launches) *launches = issued;
    if (!issued) return SIGE_HIP_OK;  // (nothing launched, no launch counted)
    return launch_status(issued);
}

// a recorded call owns a COPY of its records (the caller's array is not read after the call returns); at replay every record's
// tile count is the current count of the slot its index list is bound to, like a CountOf argument of the other entry points
struct CommitPlanCall : PlanCall {
    std::vector<sige_hip_commit_record> recs;
    int run(Plan &p, hipStream_t st) override {
        std::vector<sige_hip_commit_record> now = recs;
        for (auto &r : now) r.N = p.lookup(static_cast<const void *>(r.idx), r.N);
        return commit_impl(now.data(), (int)now.size(), nullptr, static_cast<void *>(st));
    }
};

static void commit_plan_hook(const sige_hip_commit_record *records, int n) {
    Plan *p = g_plan_rec;
    if (!p || n < 0 || (n > 0 && !records)) return;
    auto *call = new CommitPlanCall;
    call->recs.assign(records, records + n);
    for (const auto &r : call->recs) {
        const void *key = static_cast<const void *>(r.idx);
        if (!key || p->slot_of.count(key) || p->const_ptrs.count(key)) continue;
        ++call->unbound;
        ++p->unbound;
        p->shape_bound = true;
    }
    p->calls[g_plan_section].emplace_back(call);
}

}  // namespace sige

// (the plan hook of this entry is its own: SIGE_PLAN_HOOK stores arguments by value, and `records` points at the caller's memory)
#define SIGE_PLAN_HOOK_COMMIT(records, n) \
    do {                                  \
        if (sige::g_plan_rec) sige::commit_plan_hook(records, n); \
    } while (0)

extern "C" int sige_hip_commit_tiles(const sige_hip_commit_record *records, int n, int *launches, void *stream) {
    SIGE_PLAN_HOOK_COMMIT(records, n);
    return sige::commit_impl(records, n, launches, stream);
}
