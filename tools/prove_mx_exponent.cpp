// Host-only proof that the integer RCEIL exponent of the fused MX producers (fp8-mps-metal_amd/csrc/fp8mi_mx_exponent.h) equals the
// recipe's   clamp(ceilf((float)log2((double)d)), -127, 127) + 127   for EVERY non-negative float d: all 2^31 bit patterns up to and
// including +inf (the NaN patterns above it never reach the function: a block with a NaN gets the scale byte 0xFF ahead of it).
//
//   g++ -O2 -std=c++17 -pthread tools/prove_mx_exponent.cpp -o /tmp/prove_mx_exponent && /tmp/prove_mx_exponent
//
// Prints, for every exponent E, the largest mantissa field whose recipe value is still E (the per-binade thresholds the header
// states), then the count of patterns compared and of mismatches.  Exit status 0 only when there is none.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../fp8-mps-metal_amd/csrc/fp8mi_mx_exponent.h"

static float from_bits(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

static uint32_t recipe(uint32_t db)   // mx_exponent (fp8mi_mx.h) after its division, on the host
{
    const float d = from_bits(db);
    float l = std::ceil((float)std::log2((double)d));
    l = l < -127.0f ? -127.0f : (l > 127.0f ? 127.0f : l);
    return (uint32_t)((int)l + 127);
}

int main()
{
    // the thresholds as the recipe has them, by bisection inside every normal binade (the recipe is monotone in d)
    std::printf("largest mantissa field that keeps the exponent E (normal binades; '-' where the clamp hides it):\n");
    int last = -1;
    for (int E = -126; E <= 127; ++E) {
        const uint32_t base = (uint32_t)(E + 127) << 23;
        if (recipe(base | 0x7FFFFFu) == recipe(base)) continue;   // clamped: every mantissa gives the same byte
        uint32_t lo = 0, hi = 0x7FFFFFu;                          // recipe(base | lo) == recipe(base) < recipe(base | hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            (recipe(base | mid) == recipe(base) ? lo : hi) = mid;
        }
        if ((int)lo != last || E == -126 || (E & (E - 1)) == 0 || (-E & (-E - 1)) == 0) std::printf("  E = %4d: %u\n", E, lo);
        last = (int)lo;
    }

    const unsigned nt = std::thread::hardware_concurrency() ? std::min(16u, std::thread::hardware_concurrency()) : 4u;
    const uint64_t total = 0x7F800001ull;   // 0 .. +inf inclusive
    std::vector<uint64_t> bad(nt, 0), first(nt, ~0ull);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            const uint64_t b0 = total * t / nt, b1 = total * (t + 1) / nt;
            for (uint64_t b = b0; b < b1; ++b) {
                if (mx_rceil_biased((uint32_t)b) != recipe((uint32_t)b)) {
                    if (!bad[t]) first[t] = b;
                    ++bad[t];
                }
            }
        });
    for (auto &x : th) x.join();
    uint64_t nbad = 0;
    for (unsigned t = 0; t < nt; ++t) {
        nbad += bad[t];
        if (bad[t])
            std::printf("  mismatch at %#010llx: integer %u, recipe %u\n", (unsigned long long)first[t], mx_rceil_biased((uint32_t)first[t]),
                        recipe((uint32_t)first[t]));
    }
    std::printf("compared %llu patterns (0x00000000 .. 0x7f800000): %llu mismatches\n", (unsigned long long)total, (unsigned long long)nbad);
    return nbad ? 1 : 0;
}
