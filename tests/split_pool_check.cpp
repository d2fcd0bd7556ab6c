// Host program of tests/test_split_pool.py: the bookkeeping of sige_amd/csrc/split_pool.hpp (a ring for eager launches, a bump region for
// captured ones) on small capacities.  Built with -fsanitize=address,undefined; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>

#include "split_pool.hpp"

using sige::SplitPool;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

int main() {
    const size_t none = SplitPool::kNone;
    {  // ring takes advance, and wrap to 0 when the next request does not fit
        SplitPool p{10, 6};
        CHECK(p.take(4, false) == 0);
        CHECK(p.take(4, false) == 4);
        CHECK(p.take(2, false) == 8);   // (fits exactly: no wrap)
        CHECK(p.take(1, false) == 0);   // (full: wraps)
        CHECK(p.take(7, false) == 1);
        CHECK(p.take(3, false) == 0);   // (8 + 3 > 10: wraps although 2 are left)
        CHECK(p.take(0, false) == 3 && p.ring_pos == 3);
        CHECK(p.take(10, false) == 0 && p.ring_pos == 10);  // (the whole ring)
        CHECK(p.graph_pos == 0);
    }
    {  // a request larger than the ring is refused, eager or captured, and moves nothing
        SplitPool p{10, 30};
        CHECK(p.take(3, false) == 0);
        CHECK(p.take(11, false) == none);
        CHECK(p.take(11, true) == none);
        CHECK(p.take(none, false) == none && p.take(none - 1, true) == none);
        CHECK(p.ring_pos == 3 && p.graph_pos == 0);
    }
    {  // graph takes advance behind the ring and are refused once the region is exhausted: no wrap, never inside the ring
        SplitPool p{10, 6};
        CHECK(p.take(5, false) == 0);
        CHECK(p.take(4, true) == 10);
        CHECK(p.take(3, true) == none);  // (4 + 3 > 6)
        CHECK(p.take(2, true) == 14);    // (a smaller one still fits)
        CHECK(p.take(1, true) == none && p.take(0, true) == 16);
        CHECK(p.graph_pos == 6 && p.ring_pos == 5);
        // release_graph() restarts the graph region and leaves the ring position alone
        p.release_graph();
        CHECK(p.graph_pos == 0 && p.ring_pos == 5);
        CHECK(p.take(6, true) == 10);
        CHECK(p.take(5, false) == 5 && p.take(1, false) == 0);
    }
    {  // interleaved takes: every slice inside its own part, graph slices pairwise disjoint, ring slices disjoint between two wraps
        SplitPool p{64, 100};
        unsigned long long seed = 12345;
        size_t graph_end = p.ring, ring_end = 0;
        for (int i = 0; i < 2000; ++i) {
            seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
            const size_t n = (size_t)(seed >> 33) % 20;
            const bool capturing = (seed >> 60) & 1;
            if (i % 500 == 499) { p.release_graph(); graph_end = p.ring; }
            const size_t at = p.take(n, capturing);
            if (capturing) {
                if (at == none) { CHECK(graph_end + n > p.ring + p.graph); continue; }
                CHECK(at == graph_end && at >= p.ring && at + n <= p.ring + p.graph);
                graph_end = at + n;
            } else {
                CHECK(at != none && at + n <= p.ring);
                CHECK(at == ring_end || (at == 0 && ring_end + n > p.ring));
                ring_end = at + n;
            }
        }
    }
    puts("split_pool ok");
    return 0;
}
