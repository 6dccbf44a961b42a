// MoE routing (fp8mi_moe_route): the index arithmetic the host launcher and the kernels (fp8mi_moe.hip) share - which form a call takes,
// how many workgroups, where a workgroup's assignments lie and how the workspace is laid out.  One set of functions for both sides and
// for the host program that checks them without a GPU (tests/c/moe_route_index.cpp).
//
// The n = T k assignments are cut into chunks of kMoeRouteChunk; workgroup b owns the assignments [b chunk, min(n, (b + 1) chunk)),
// wave w of it the 64 that start at b chunk + 64 w, one per lane: inside a workgroup, and over the workgroups in order, assignments are
// visited in index order - what makes the ranks stable.  n <= kMoeRouteSingleMax is ONE workgroup that does everything (no workspace);
// beyond it three launches share
//     int32 base[G][blocks]   a workgroup's count per expert, turned by the scan (one workgroup per expert, over that expert's contiguous
//                             row) into the count of all EARLIER workgroups
//     int32 total[G]          every expert's count over all workgroups
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FP8MI_ROUTE_FN __host__ __device__ inline
#else
#define FP8MI_ROUTE_FN inline
#endif

constexpr int kMoeRouteThreads = 1024;                     // one workgroup: sixteen waves, one assignment per lane
constexpr int kMoeRouteWaves = kMoeRouteThreads / 64;
constexpr int kMoeRouteChunk = kMoeRouteThreads;           // FP8MI_MOE_ROUTE_CHUNK
constexpr int kMoeRouteSingleMax = kMoeRouteChunk;         // FP8MI_MOE_ROUTE_SINGLE_MAX
constexpr int kMoeRouteMaxExperts = 1024;                  // the grouped GEMM's maximum; one expert per thread in the scan

FP8MI_ROUTE_FN bool fp8mi_moe_route_single(int64_t n) { return n <= kMoeRouteSingleMax; }

FP8MI_ROUTE_FN int64_t fp8mi_moe_route_blocks(int64_t n) { return (n + kMoeRouteChunk - 1) / kMoeRouteChunk; }

// the assignment lane `lane` of wave `wave` of workgroup `block` holds (it may lie at or beyond n)
FP8MI_ROUTE_FN int64_t fp8mi_moe_route_index(int64_t block, int wave, int lane) { return block * kMoeRouteChunk + 64 * wave + lane; }

// workspace layout, in int32 elements
FP8MI_ROUTE_FN int64_t fp8mi_moe_route_ws_base(int64_t n, int64_t block, int g) { return g * fp8mi_moe_route_blocks(n) + block; }
FP8MI_ROUTE_FN int64_t fp8mi_moe_route_ws_total(int64_t n, int G, int g) { return fp8mi_moe_route_blocks(n) * G + g; }

// the scan of one expert's row of `blocks` counts by kMoeRouteThreads threads: thread t owns the entries [first(t), first(t + 1))
FP8MI_ROUTE_FN int64_t fp8mi_moe_route_scan_first(int64_t blocks, int t)
{
    const int64_t per = (blocks + kMoeRouteThreads - 1) / kMoeRouteThreads, b = t * per;
    return b < blocks ? b : blocks;
}

// bytes of the workspace (a multiple of 16): 0 for the one-launch form
FP8MI_ROUTE_FN int64_t fp8mi_moe_route_ws_bytes(int64_t n, int G)
{
    if (fp8mi_moe_route_single(n)) return 0;
    return (fp8mi_moe_route_ws_total(n, G, G) * 4 + 15) / 16 * 16;
}
