// fp8mi_group_slot (csrc/fp8mi_group_slot.h), the grouped GEMM's slot -> (group, m-tile) resolution, against a brute-force enumeration
// of the clamped groups: a host program of its own (tests/test_grouped_host.py compiles and runs it; no GPU, no libfp8mi.so).
// For every case and BM in {32, 64, 128}: the slots 0 .. T - 1 (T = M_total / BM + G, what the host launches) resolve to exactly the
// tiles of the clamped groups, once each and in order; every resolved row lies in [0, M_total); the real tiles number at most T; slots
// behind the last real tile resolve to "none"; fp8mi_group_tiles counts exactly the real tiles.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fp8mi_group_slot.h"

struct Case {
    const char *name;
    int64_t M_total;
    std::vector<int32_t> offs;
};

struct Tile { int group, tile; int64_t start; int rows; };

static int check(const Case &c, int BM)
{
    const int G = (int)c.offs.size();
    // the definition, written out on its own: start_0 = 0, start_g = end_{g-1}, end_g = clamp(offs[g], start_g, M_total)
    std::vector<int> owner((size_t)c.M_total, -1);
    std::vector<Tile> want;
    int64_t start = 0;
    for (int g = 0; g < G; ++g) {
        int64_t end = c.offs[g];
        if (end < start) end = start;
        if (end > c.M_total) end = c.M_total;
        for (int64_t r = start; r < end; ++r) {
            if (owner[(size_t)r] != -1) { printf("%s: row %lld has two owners\n", c.name, (long long)r); return 1; }
            owner[(size_t)r] = g;
        }
        for (int64_t r = start, t = 0; r < end; r += BM, ++t) want.push_back(Tile{g, (int)t, start, (int)(end - start)});
        start = end;
    }
    const int64_t T = c.M_total / BM + G;
    if ((int64_t)want.size() > T) { printf("%s BM=%d: %zu real tiles, %lld slots\n", c.name, BM, want.size(), (long long)T); return 1; }
    if (fp8mi_group_tiles(c.offs.data(), G, c.M_total, BM) != (int64_t)want.size()) {
        printf("%s BM=%d: fp8mi_group_tiles gives %lld, the groups have %zu tiles\n", c.name, BM, (long long)fp8mi_group_tiles(c.offs.data(), G, c.M_total, BM), want.size());
        return 1;
    }
    std::vector<int> covered((size_t)c.M_total, 0);
    for (int64_t slot = 0; slot < T + 4; ++slot) {
        const Fp8miGroupSlot s = fp8mi_group_slot(c.offs.data(), G, c.M_total, BM, slot);
        if (slot >= (int64_t)want.size()) {
            if (s.group != -1) { printf("%s BM=%d: surplus slot %lld resolved to group %d\n", c.name, BM, (long long)slot, s.group); return 1; }
            continue;
        }
        const Tile &w = want[(size_t)slot];
        if (s.group != w.group || s.tile != w.tile || s.start != w.start || s.rows != w.rows) {
            printf("%s BM=%d slot %lld: got (g=%d t=%d start=%lld rows=%d), want (g=%d t=%d start=%lld rows=%d)\n", c.name, BM, (long long)slot, s.group, s.tile,
                   (long long)s.start, s.rows, w.group, w.tile, (long long)w.start, w.rows);
            return 1;
        }
        // the rows this tile computes: [start + tile * BM, min(start + rows, that + BM))
        const int64_t r0 = s.start + (int64_t)s.tile * BM, r1 = r0 + BM < s.start + s.rows ? r0 + BM : s.start + s.rows;
        if (r0 < 0 || r1 > c.M_total || r0 >= r1) { printf("%s BM=%d slot %lld: rows [%lld, %lld) leave [0, %lld)\n", c.name, BM, (long long)slot, (long long)r0, (long long)r1, (long long)c.M_total); return 1; }
        for (int64_t r = r0; r < r1; ++r) {
            if (owner[(size_t)r] != s.group || covered[(size_t)r]++) { printf("%s BM=%d: row %lld tiled twice or for the wrong group\n", c.name, BM, (long long)r); return 1; }
        }
    }
    for (int64_t r = 0; r < c.M_total; ++r)
        if ((owner[(size_t)r] != -1) != (covered[(size_t)r] == 1)) { printf("%s BM=%d: row %lld owned but not tiled\n", c.name, BM, (long long)r); return 1; }
    return 0;
}

int main()
{
    std::vector<Case> cases;
    cases.push_back({"sizes 0 1 130 64 33 0 in 240", 240, {0, 1, 131, 195, 228, 228}});
    cases.push_back({"all groups empty", 100, {0, 0, 0, 0}});
    cases.push_back({"one group, all rows", 77, {77}});
    cases.push_back({"one group, some rows", 77, {50}});
    {
        Case c{"1024 groups of one row", 1024, {}};
        for (int g = 0; g < 1024; ++g) c.offs.push_back(g + 1);
        cases.push_back(c);
    }
    cases.push_back({"decreasing offs", 240, {100, 50, 200, 10, 240}});
    cases.push_back({"offs beyond M_total", 240, {100, 300, 500}});
    cases.push_back({"negative offs", 128, {-5, 40, -1, 90}});
    // (the three vectors tests/test_gpu_grouped.py runs on the GPU, G = 6 in 240 rows)
    cases.push_back({"decreasing offs, G = 6", 240, {100, 50, 200, 10, 240, 240}});
    cases.push_back({"offs beyond M_total, G = 6", 240, {100, 300, 500, 500, 500, 500}});
    cases.push_back({"negative offs, G = 6", 240, {-5, 40, -1, 90, 90, INT32_MIN}});
    cases.push_back({"alternating M_total and 0", 256, {256, 0, 256, 0, 256, 0, 256, 0}});
    cases.push_back({"INT32 extremes", 200, {INT32_MIN, INT32_MAX, 3}});
    int bad = 0, n = 0;
    for (const Case &c : cases)
        for (int BM : {32, 64, 128}) { bad += check(c, BM); ++n; }
    if (bad) { printf("FAILED %d of %d\n", bad, n); return 1; }
    printf("ok %d\n", n);
    return 0;
}
