// What the three transposed-score token-attention units (attention_tokens.hip: fp32 operands, 16 keys per step;
// attention_tokens_f16.hip: fp16 operands from fp32 K / V, 32 keys per step; attention_tokens_f16kv.hip: K / V stored as fp16) share
// around the operand path: the workgroup's place -- its lane, its (batch, head) pair and query tile, where its K / V begin --, the
// geometry of the LDS image the four waves merge through, and on the host the launcher of both entry points of a unit.
// (attention_tokens_kernel, round 4's form kept for the A/B of the tuning build, has another state layout and keeps its own code.)
//
// The contract between an operand path and this header: one workgroup of 256 threads per 16 queries of one (batch, head); lane
// (kq, j) = (lane >> 4, lane & 15) of each of the four waves ends its key steps with
//   m_run = the maximum of query j over every key the wave has seen (units of log2; -inf: the wave had no step),
//   l_run = the sum over THIS lane's keys,
//   o[n][r], n < DT, r < 4 = O[query j][a channel of the unit's own choice]
// -- which channel row j of the MFMA's A operand IS is free, and each load path picks the order its loads like: 16n + 4kq + r
// (fp32), 16 VC (n / VC) + VC (4kq + r) + n % VC (f16c), the greedy groups of kv16_first / kv16_vc (f16kv) -- and writes them to
// row j of its wave's image at that channel: [4 waves][16 queries][tokens_image_row(DT)] floats of dynamic LDS.  (The fp16-operand
// forms carry 2^15 O and 2^15 l: the factor is in every wave's state alike and cancels in O / l.)
//
// What stays in each kernel, because as a function of this header it changed instructions (profiles/attention_tokens_one_home_isa.txt
// is taken with them where they are): the K / V descriptor pair and `k + kv0` right behind tokens_place (inside it: the prologue's
// scalar code scheduled and allocated differently, ~30 lines per instance); the f16kv kernel's whole prologue (schedule, ~100 lines
// per instance); the merge through LDS with the output store as ONE function taking the unit's channel map (same metadata rows, but
// the store's two packed multiplies commuted in every instance and 33 lines moved in <5, 10>: schedule, 122 lines over the f16c
// unit); the online-softmax step (as a function it moved the register allocation of the main loop); the fragments as float4 (as
// f32x4 from the load on every f16c instance compiled to other code: pack8 has a float4 form, attention_rows.hpp).
#pragma once
#include <utility>

#include "attention_rows.hpp"

namespace sige {

// ---- the workgroup's place ----
struct TokensPlace {
    int tid, wave, kq, j;  // thread, wave (uniform), lane (kq, j)
    int b, q0;             // batch, the tile's first query
    size_t hoff;           // the head's first channel
    size_t kv0;            // in elements: where this head's K / V of the batch (TILES: of the tile's own image) begin
};

// TILES: the keys of the query tile's own image (tile_image, attention_rows.hpp); (workgroup -> XCD: workgroup_pair_tile)
template <bool TILES>
__device__ __forceinline__ TokensPlace tokens_place(int Nk, int C, int heads, int d, int q_tiles, int xcd_pairs,
                                                    const int32_t *__restrict__ tiles, int img_shift, int images) {
    TokensPlace p;
    p.tid = threadIdx.x;
    const int lane = p.tid & 63;
    p.wave = __builtin_amdgcn_readfirstlane(p.tid >> 6);
    p.kq = lane >> 4; p.j = lane & 15;
    int pair, qtile;
    workgroup_pair_tile(q_tiles, xcd_pairs, pair, qtile);
    const int head = pair % heads;
    p.b = pair / heads;
    p.q0 = qtile * 16;
    p.hoff = (size_t)head * d;
    p.kv0 = ((size_t)p.b + tile_image<TILES>(tiles, qtile, img_shift, images)) * Nk * C + p.hoff;
    return p;
}

// The merge image: a padded row (a multiple of 4 floats: 16-byte rows), and the dynamic LDS of a launch
constexpr int tokens_image_row(int DT) { return DT * 16 + 4; }
constexpr size_t tokens_image_bytes(int DT) { return (size_t)4 * 16 * tokens_image_row(DT) * sizeof(float); }

// ---- host ----

// What a unit's launch of one instance takes from the launcher
struct TokensLaunch {
    int d;              // channels of a head
    int t16, pairs;     // 16-query tiles, (batch, head) pairs: the grid is their product
    int xcd_pairs;      // pairs per XCD where they are dealt to the XCDs, else 0 (workgroup_pair_tile)
    float scale_log2e;  // (units of log2: exp(x) = exp2(x * log2 e))
    hipStream_t st;
};

// Both entry points of a unit: q [B,Nq,C] against k / v of Nk keys per batch -- or, with `tiles` (B = 1), per image.  `elem`: bytes
// of a K / V element (32-bit byte offsets into one batch's -- one image's -- K / V); `supported`: the unit's shape predicate;
// Us...: the 16-channel tile counts the unit has an instance for; go(U, TILES, launch) launches instance <U, TILES> (two
// std::integral_constant).  (A left fold: the instances are then instantiated, and emitted, in the order of Us.)
template <int... Us, class Supported, class Go>
inline int launch_tokens(std::integer_sequence<int, Us...>, size_t elem, Supported supported, const void *q, const void *k, const void *v,
                         const void *out, int B, int Nq, int Nk, int C, int heads, float scale, const int32_t *tiles, void *stream, Go go) {
    if (!supported(Nq, Nk, C, heads)) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(q) || !al(k) || !al(v) || !al(out) || (size_t)Nk * C * elem >= 0x7fffffffu) return SIGE_HIP_EUNSUPPORTED;
    TokensLaunch l;
    l.d = C / heads;
    const int units = (l.d + 15) / 16;
    l.scale_log2e = scale * 1.44269504088896341f;
    l.st = as_stream(stream);
    l.pairs = B * heads; l.t16 = Nq / 16;
    if ((long)l.pairs * l.t16 > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    l.xcd_pairs = l.pairs % 8 == 0 ? l.pairs / 8 : 0;
    auto one = [&](auto U) -> bool {
        if (units != decltype(U)::value) return false;
        if (tiles) go(U, std::true_type(), l);
        else go(U, std::false_type(), l);
        return true;
    };
    if (!(... || one(std::integral_constant<int, Us>()))) return SIGE_HIP_EUNSUPPORTED;
    return launch_status();
}

}  // namespace sige
