// tile_memory_stub.cpp -- TEST INFRASTRUCTURE, beside hip_stub.cpp: the stand-in for launch_tile_order_remembering, the
// sort of a batch's tile costs with its memory (kifs_support_kernels.hip: tile_order_kernel with `seen`).  Restated on
// the CPU from the kernel's documented rule: seen[i] = cost << 8 | age keeps tile i's largest cost of the last `window`
// sorts -- a new cost at least as large, or an entry `window` sorts old, replaces it -- the order is by descending
// (seen >> 8) >> shift in 1024 bins (here: stable inside a bin), and cost[] is left zeroed.  "Device memory" is the main
// stand-in's malloc'ed memory, so a table too short for `tile_count` words is AddressSanitizer's to report.  The hooks
// hand the driver the latest call's tables, so that it can plant costs and check which buffers a sort was given.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"

struct StubMemorySort {
    uint32_t *cost, *seen, *order;
    uint32_t tile_count, tiles_x, shift, window;
    hipStream_t stream;
    long calls;
};
static StubMemorySort g_memory_sort{};
static long g_memory_fail_in = -1;

extern "C" {
void stub_memory_sort(StubMemorySort* out) { *out = g_memory_sort; }
void stub_memory_fail_in(long n) { g_memory_fail_in = n; }  // the n-th memory sort from now on fails to launch, once
}

namespace kifs {

hipError_t launch_tile_order_remembering(uint32_t* cost, uint32_t* seen, uint32_t* order, uint32_t tile_count, uint32_t tiles_x,
                                         uint32_t shift, uint32_t window, hipStream_t st) {
    if (g_memory_fail_in > 0 && --g_memory_fail_in == 0) {
        g_memory_fail_in = -1;
        return hipErrorLaunchFailure;
    }
    if (!cost || !seen || !order || tiles_x == 0 || window < 1 || window > 255 || shift > 31) {
        std::fprintf(stderr, "tile_memory_stub: a sort of %u tiles with cost %p seen %p order %p tiles_x %u shift %u window %u\n", tile_count,
                     (void*)cost, (void*)seen, (void*)order, tiles_x, shift, window);
        std::abort();
    }
    g_memory_sort = StubMemorySort{cost, seen, order, tile_count, tiles_x, shift, window, st, g_memory_sort.calls + 1};
    std::vector<std::pair<uint32_t, uint32_t>> keyed(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) {
        const uint32_t now = std::min(cost[i], (1u << 24) - 1u), old = seen[i], age = (old & 0xffu) + 1u;
        seen[i] = (now >= (old >> 8) || age >= window) ? now << 8 : ((old & ~0xffu) | age);
        keyed[i] = {1023u - std::min((seen[i] >> 8) >> shift, 1023u), i};  // heaviest bin first, stable
    }
    std::sort(keyed.begin(), keyed.end());
    for (uint32_t i = 0; i < tile_count; ++i) {
        const uint32_t t = keyed[i].second;
        order[i] = (t % tiles_x) | ((t / tiles_x) << 16);
        cost[t] = 0;
    }
    return hipSuccess;
}

}  // namespace kifs
