// csrc/fp8mi_moe_route.h, the index arithmetic fp8mi_moe_route's host launcher and kernels share, as a host program of its own
// (tests/test_moe_route_host.py compiles and runs it; no GPU, no libfp8mi.so).  For every n of a list that sits on the edges of the forms:
//   - the form: one launch iff n <= kMoeRouteSingleMax, and then one workgroup and no workspace;
//   - the walk: over the workgroups, their waves and a wave's lanes IN THAT ORDER the assignment index runs through
//     0, 1, 2, ... without a gap or a repeat and passes n - 1 (what makes the ranks stable and the tail complete);
//   - the workspace: base[g][b] and total[g] are distinct int32 slots inside fp8mi_moe_route_ws_bytes, an expert's counts are
//     contiguous in b, and the bytes are a multiple of 16, 0 for the one-launch form and non-decreasing in n and in G;
//   - the scan's split of an expert's row among the threads: consecutive, disjoint segments that cover [0, blocks).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fp8mi_moe_route.h"

static int check(int64_t n, int G)
{
    const int64_t blocks = fp8mi_moe_route_blocks(n);
    if (fp8mi_moe_route_single(n) != (n <= kMoeRouteSingleMax)) { printf("n=%lld: wrong form\n", (long long)n); return 1; }
    if (fp8mi_moe_route_single(n) && (blocks > 1 || fp8mi_moe_route_ws_bytes(n, G) != 0)) { printf("n=%lld: the one-launch form has %lld workgroups\n", (long long)n, (long long)blocks); return 1; }
    if (blocks * kMoeRouteChunk < n || (blocks > 0 && (blocks - 1) * kMoeRouteChunk >= n)) { printf("n=%lld: %lld workgroups\n", (long long)n, (long long)blocks); return 1; }
    int64_t next = 0;
    for (int64_t b = 0; b < blocks; ++b)
        for (int w = 0; w < kMoeRouteWaves; ++w)
            for (int l = 0; l < 64; ++l) {
                if (fp8mi_moe_route_index(b, w, l) != next) { printf("n=%lld: (b=%lld w=%d l=%d) is not assignment %lld\n", (long long)n, (long long)b, w, l, (long long)next); return 1; }
                ++next;
            }
    if (next < n) { printf("n=%lld: the walk ends at %lld\n", (long long)n, (long long)next); return 1; }
    if (fp8mi_moe_route_single(n)) return 0;
    const int64_t bytes = fp8mi_moe_route_ws_bytes(n, G);
    if (bytes % 16 != 0) { printf("n=%lld G=%d: %lld workspace bytes\n", (long long)n, G, (long long)bytes); return 1; }
    std::vector<char> seen((size_t)(bytes / 4), 0);
    for (int64_t b = 0; b < blocks; ++b)
        for (int g = 0; g < G; ++g) {
            const int64_t at = fp8mi_moe_route_ws_base(n, b, g);
            if (b > 0 && at != fp8mi_moe_route_ws_base(n, b - 1, g) + 1) { printf("n=%lld G=%d: expert %d is not contiguous at workgroup %lld\n", (long long)n, G, g, (long long)b); return 1; }
            if (at < 0 || at >= bytes / 4 || seen[(size_t)at]++) { printf("n=%lld G=%d: base[%lld][%d] at %lld\n", (long long)n, G, (long long)b, g, (long long)at); return 1; }
        }
    for (int g = 0; g < G; ++g) {
        const int64_t at = fp8mi_moe_route_ws_total(n, G, g);
        if (at < 0 || at >= bytes / 4 || seen[(size_t)at]++) { printf("n=%lld G=%d: total[%d] at %lld\n", (long long)n, G, g, (long long)at); return 1; }
    }
    int64_t at = 0;
    for (int t = 0; t <= kMoeRouteThreads; ++t) {
        const int64_t first = fp8mi_moe_route_scan_first(blocks, t);
        if (first < at || first > blocks || (t == 0 && first != 0)) { printf("n=%lld: the scan's segment %d starts at %lld\n", (long long)n, t, (long long)first); return 1; }
        at = first;
    }
    if (at != blocks) { printf("n=%lld: the scan's segments end at %lld of %lld\n", (long long)n, (long long)at, (long long)blocks); return 1; }
    return 0;
}

int main()
{
    static_assert(kMoeRouteChunk == kMoeRouteWaves * 64 && kMoeRouteThreads == 64 * kMoeRouteWaves, "a chunk is one assignment per lane");
    static_assert(kMoeRouteSingleMax <= kMoeRouteChunk, "the one-launch form is one workgroup");
    static_assert(kMoeRouteMaxExperts <= kMoeRouteThreads, "the scan holds one expert per thread");
    const int64_t ns[] = {0, 1, 10, 63, 64, 65, 512, kMoeRouteSingleMax - 1, kMoeRouteSingleMax, kMoeRouteSingleMax + 1, 2 * kMoeRouteChunk - 1,
                          2 * kMoeRouteChunk, 3 * kMoeRouteChunk + 5, 65536, 100000};
    const int Gs[] = {1, 3, 8, 9, 64, 65, 256, 1024};
    int bad = 0, cases = 0;
    for (int64_t n : ns)
        for (int G : Gs) { bad += check(n, G); ++cases; }
    // non-decreasing in n (a dense sweep over the first chunks, then large steps up to the int32 limit) and in G
    for (int G : Gs) {
        int64_t prev = 0;
        for (int64_t n = 0; n <= 5 * kMoeRouteChunk; ++n) {
            const int64_t b = fp8mi_moe_route_ws_bytes(n, G);
            if (b < prev) { printf("G=%d: workspace bytes fall at n=%lld\n", G, (long long)n); ++bad; }
            prev = b;
        }
        for (int64_t n = 5 * kMoeRouteChunk; n <= 0x7FFFFFFFll; n += 9999991) {
            const int64_t b = fp8mi_moe_route_ws_bytes(n, G);
            if (b < prev) { printf("G=%d: workspace bytes fall at n=%lld\n", G, (long long)n); ++bad; }
            prev = b;
        }
        ++cases;
    }
    for (int64_t n : ns) {
        int64_t prev = 0;
        for (int G = 1; G <= kMoeRouteMaxExperts; ++G) {
            const int64_t b = fp8mi_moe_route_ws_bytes(n, G);
            if (b < prev) { printf("n=%lld: workspace bytes fall at G=%d\n", (long long)n, G); ++bad; }
            prev = b;
        }
        ++cases;
    }
    // the largest call: 2^31 - 1 assignments of 1024 experts still has int64 room
    if (fp8mi_moe_route_ws_bytes(0x7FFFFFFFll, 1024) != ((fp8mi_moe_route_blocks(0x7FFFFFFFll) * 1024 + 1024) * 4 + 15) / 16 * 16) { printf("largest workspace\n"); ++bad; }
    ++cases;
    if (bad) { printf("FAILED %d of %d\n", bad, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
