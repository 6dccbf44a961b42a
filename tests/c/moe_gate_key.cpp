// csrc/fp8mi_moe_gate.h, the ordered-key map and the sort word fp8mi_moe_gate's kernel selects with, as a host program of its own
// (tests/test_moe_gate_host.py compiles and runs it; no GPU, no libfp8mi.so):
//   - ordered32 is strictly monotone over a dense sample of floats in increasing order: -inf, every exponent's ends and a few values
//     between them, the denormals, the zeros, +inf - and the comparison agrees with the floats' own;
//   - -0 and +0 collide; every NaN (several payloads, both signs) collides at the top, above +inf;
//   - unordered32 inverts the map up to that canonicalisation;
//   - every real expert's word, -inf and negative keys included, exceeds the pad word, for e up to 1023;
//   - at equal keys the lower index wins, and the key decides before the index does;
//   - a word gives back its index and its key;
//   - the launch geometry: slots per lane and lanes per group.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fp8mi_moe_gate.h"

static uint32_t bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static float float_of(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static int fails = 0;
static long checks = 0;

static void expect(bool ok, const char *what, uint32_t a, uint32_t b)
{
    ++checks;
    if (!ok && fails++ < 20) printf("FAIL %s (%08x, %08x)\n", what, a, b);
}

int main()
{
    // positive magnitudes in increasing order: denormals, then every exponent's first value, a few inside, its last
    std::vector<uint32_t> mags;
    const uint32_t fracs[] = {0x000000u, 0x000001u, 0x000002u, 0x2AAAAAu, 0x400000u, 0x555555u, 0x7FFFFEu, 0x7FFFFFu};
    for (uint32_t ex = 0; ex < 255; ++ex)
        for (uint32_t f : fracs) {
            const uint32_t b = (ex << 23) | f;
            if (b != 0) mags.push_back(b);
        }
    mags.push_back(0x7F800000u);   // +inf
    std::vector<uint32_t> all;     // increasing as floats: -inf .. -denormal, +0, +denormal .. +inf
    for (size_t i = mags.size(); i-- > 0;) all.push_back(mags[i] | 0x80000000u);
    all.push_back(0u);
    for (uint32_t b : mags) all.push_back(b);
    for (size_t i = 0; i + 1 < all.size(); ++i) {
        const uint32_t a = all[i], b = all[i + 1];
        expect(float_of(a) < float_of(b), "the sample is not increasing", a, b);
        expect(fp8mi_gate_ordered32(a) < fp8mi_gate_ordered32(b), "ordered32 is not strictly monotone", a, b);
    }
    for (uint32_t b : all) expect(fp8mi_gate_unordered32(fp8mi_gate_ordered32(b)) == b, "unordered32 does not invert ordered32", b, fp8mi_gate_ordered32(b));

    // the zeros collide (and come back as +0); NaNs collide at the top
    expect(bits_of(-0.0f) == 0x80000000u && bits_of(0.0f) == 0u && bits_of(-INFINITY) == 0xFF800000u, "the bit patterns below are not these floats'", 0u, 0u);
    expect(fp8mi_gate_ordered32(0x80000000u) == fp8mi_gate_ordered32(0u), "-0 and +0 differ", 0x80000000u, 0u);
    expect(fp8mi_gate_unordered32(fp8mi_gate_ordered32(0x80000000u)) == 0u, "-0 does not come back as +0", 0x80000000u, 0u);
    expect(fp8mi_gate_ordered32(0x80000001u) < fp8mi_gate_ordered32(0u) && fp8mi_gate_ordered32(0u) < fp8mi_gate_ordered32(1u), "zero is not between the denormals", 0u, 0u);
    const uint32_t nans[] = {0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 0x7FA5A5A5u, 0xFFC00000u, 0xFF800001u, 0xFFFFFFFFu, 0xFFDEAD00u};
    for (uint32_t n : nans) {
        expect(isnan(float_of(n)), "not a NaN", n, 0u);
        expect(fp8mi_gate_ordered32(n) == 0xFFFFFFFFu, "a NaN is not at the top", n, fp8mi_gate_ordered32(n));
        expect(fp8mi_gate_ordered32(n) > fp8mi_gate_ordered32(0x7F800000u), "a NaN is not above +inf", n, 0u);
        expect(isnan(float_of(fp8mi_gate_unordered32(fp8mi_gate_ordered32(n)))), "a NaN does not come back as one", n, 0u);
    }
    expect(fp8mi_gate_ordered32(0xFF800000u) == 0x007FFFFFu, "-inf is not the smallest value", 0xFF800000u, fp8mi_gate_ordered32(0xFF800000u));

    // words: above the pad word for every key and index; key before index; the lower index first among equal keys
    const uint32_t keys[] = {0xFF800000u, 0xFF7FFFFFu, 0xBF800000u, 0x80000001u, 0x80000000u, 0u, 1u, 0x3F800000u, 0x7F7FFFFFu, 0x7F800000u, 0x7FC00000u, 0xFFC00000u};
    for (uint32_t e = 0; e < (uint32_t)kMoeGateMaxExperts; ++e)
        for (uint32_t kb : keys) {
            const uint64_t w = fp8mi_gate_word(kb, e);
            expect(w > kMoeGatePadWord, "a real expert's word is not above the pad word", kb, e);
            expect(fp8mi_gate_word_index(w) == e, "a word does not give back its index", kb, e);
            expect(fp8mi_gate_ordered32(fp8mi_gate_word_key(w)) == fp8mi_gate_ordered32(kb), "a word does not give back its key", kb, e);
            if (e > 0) expect(fp8mi_gate_word(kb, e - 1) > w, "the lower index does not win at equal keys", kb, e);
        }
    expect(fp8mi_gate_word(0x80000000u, 3) > fp8mi_gate_word(0u, 4) && fp8mi_gate_word(0u, 3) > fp8mi_gate_word(0x80000000u, 4), "-0 against +0 is not decided by the index", 0u, 0u);
    expect(fp8mi_gate_word(0xFFC00000u, 5) > fp8mi_gate_word(0x7FC00001u, 6), "NaNs are not decided by the index", 0u, 0u);
    expect(fp8mi_gate_word(0x3F800001u, 1023) > fp8mi_gate_word(0x3F800000u, 0), "the key does not decide before the index", 0u, 0u);
    expect(fp8mi_gate_word(0xFF800000u, 1023) > kMoeGatePadWord, "-inf at the last index", 0u, 0u);

    // geometry
    for (int G = 1; G <= kMoeGateMaxExperts; ++G) {
        const int E = fp8mi_gate_slots(G);
        expect((E == 1 || E == 2 || E == 4 || E == 8 || E == 16) && 64 * E >= G && (E == 1 || 32 * E < G), "slots per lane", (uint32_t)G, (uint32_t)E);
    }
    for (int n = 1; n <= kMoeGateMaxGroups; ++n) {
        const int L = 1 << fp8mi_gate_team_log2(n);
        expect(n * L <= 64 && 2 * n * L > 64, "lanes per group", (uint32_t)n, (uint32_t)L);
    }
    if (fails) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
