// Bookkeeping of one buffer that serves the in-launch split finish (split_finish.hpp): a RING for eager launches -- a slice is only
// live while its launch runs, so the oldest slices are handed out again after a wrap -- followed by a bump-allocated GRAPH region for
// launches recorded into a hipGraph, whose slice is baked into the graph and must never be handed out again before every graph is
// gone (release_graph).  Offsets and counts in elements; no HIP here (split_pool.hip holds the buffers), so a host program can
// exercise it: tests/test_split_pool.py.
#pragma once
#include <stddef.h>

namespace sige {

struct SplitPool {
    static constexpr size_t kNone = ~size_t(0);
    size_t ring, graph;  // capacity of each part: the ring is [0, ring), the graph region [ring, ring + graph)
    size_t ring_pos = 0, graph_pos = 0;

    // offset of `n` elements, or kNone: a request larger than the ring (from either part), the graph region exhausted
    size_t take(size_t n, bool capturing) {
        if (n > ring) return kNone;
        if (capturing) {
            if (graph_pos + n > graph) return kNone;
            const size_t at = ring + graph_pos;
            graph_pos += n;
            return at;
        }
        if (ring_pos + n > ring) ring_pos = 0;
        const size_t at = ring_pos;
        ring_pos += n;
        return at;
    }

    // every captured graph is gone: the graph region starts over
    void release_graph() { graph_pos = 0; }
};

}  // namespace sige
