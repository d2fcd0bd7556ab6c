// Host side of the in-launch split finish (split_finish.hpp): the tickets and the workspace of the splits, one buffer of each per
// device, laid out as a ring for eager launches and a bump region for captured ones (split_pool.hpp).
#include <mutex>

#include "common.hpp"
#include "split_pool.hpp"

namespace sige {

namespace {

template <typename T, size_t RING, size_t GRAPH, bool ZEROED>
struct DevicePools {
    struct Dev { T *buf = nullptr; bool failed = false; SplitPool pool{RING, GRAPH}; };
    Dev dev[32];
    std::mutex mu;

    // `n` elements that stay valid while the launch on `st` runs (captured: for the life of the graph).  nullptr: device outside
    // 0..31, a request larger than the ring, first use during a capture, graph region exhausted, allocation failed once
    T *take(hipStream_t st, size_t n) {
        int d = -1;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 32 || n > RING) return nullptr;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) return nullptr;
        const bool capturing = cs != hipStreamCaptureStatusNone;
        std::lock_guard<std::mutex> lock(mu);
        Dev &t = dev[d];
        if (!t.buf) {
            if (capturing || t.failed) return nullptr;
            const size_t bytes = (RING + GRAPH) * sizeof(T);
            if (hipMalloc(&t.buf, bytes) != hipSuccess ||
                (ZEROED && (hipMemset(t.buf, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess))) {
                t.buf = nullptr; t.failed = true;
                (void)hipGetLastError();
                return nullptr;
            }
        }
        const size_t at = t.pool.take(n, capturing);
        return at == SplitPool::kNone ? nullptr : t.buf + at;
    }

    void release_graph(int d) {
        std::lock_guard<std::mutex> lock(mu);
        dev[d].pool.release_graph();
    }
};

// Tickets: one int per unit of a split launch, zero whenever no such launch is running (zeroed once, put back by the last
// workgroup).  2^20 in the ring = hundreds of launches in flight before a wrap could meet a running one.
DevicePools<int32_t, size_t(1) << 20, size_t(3) << 20, true> g_tickets;
// Workspace of the splits whose slices are not part of the output tensor (attention_wide.hip, conv_latent_head.hip): floats,
// 32 MiB + 96 MiB, written before they are read -- not zeroed.
DevicePools<float, size_t(8) << 20, size_t(24) << 20, false> g_workspace;

}  // namespace

int32_t *split_tickets(hipStream_t st, long blocks) {
    if (tuning(SIGE_HIP_TUNE_CONV_KSPLIT_SECOND_PASS)) return nullptr;
    return g_tickets.take(st, (size_t)blocks);
}

float *split_workspace(hipStream_t st, size_t floats) { return g_workspace.take(st, floats); }

}  // namespace sige

// every captured graph of the device is gone: the graph regions of both pools start over
extern "C" int sige_hip_release_graph_tickets(void) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return SIGE_HIP_EINVAL;
    sige::g_workspace.release_graph(dev);
    sige::g_tickets.release_graph(dev);
    return SIGE_HIP_OK;
}
