// The RCEIL exponent of an MX block by integer arithmetic on the bits of descale = fl32(amax / max_pos): what the fused MX producers
// (fp8mi_actquant.hip, fp8mi_normquant.hip) use in place of mx_exponent's `double` log2 (fp8mi_mx.h).  Plain C++ with no device
// dependency, so that tools/prove_mx_exponent.cpp can compile this very text on the host and compare it with
//   clamp(ceilf((float)log2((double)d)), -127, 127) + 127
// over all 2^31 non-negative float patterns (DESIGN.md 5.8 quotes its output).
//
// d = 2^E (1 + m): log2 d = E + log2(1 + m).  For m = 0 that is E.  For m > 0 the exact ceiling is E + 1 - but torch takes log2 in
// fp32, correctly rounded, and E + log2(1 + m) ROUNDS TO E while log2(1 + m) is no more than half the distance from E to the next
// float towards E + 1.  That distance depends on |E|'s binade alone (2^(k - 23) for 2^k <= |E| < 2^(k + 1); half of that below a
// negative power of two, where the floats towards zero are twice as dense), so the rule is "E, plus one where the mantissa field
// exceeds a per-binade threshold": 0 for |E| < 4 and 1, 2, 5, 11, 22, 44 mantissa steps for k = 2 .. 7 (ln 2 x 2^(k - 1), floored).
#pragma once

#include <stdint.h>

#ifndef FP8MI_MXEXP_FN
#define FP8MI_MXEXP_FN static inline
#endif

// db: the bits of a float d >= 0 or +inf (not a NaN) -> the biased exponent byte 0 .. 254
FP8MI_MXEXP_FN uint32_t mx_rceil_biased(uint32_t db)
{
    if (db >= 0x7F800000u) return 254u;   // inf -> 127
    if (db == 0u) return 0u;              // log2(0) = -inf -> -127
    int E;
    uint32_t m;
    if (db >= 0x00800000u) {
        E = (int)(db >> 23) - 127;
        m = db & 0x7FFFFFu;
    } else {                              // subnormal: normalise
        const int p = 31 - __builtin_clz(db);
        E = p - 149;
        m = (db << (23 - p)) & 0x7FFFFFu;
    }
    const int a = E < 0 ? -E : E;
    int k = 31 - __builtin_clz((uint32_t)a | 1u);
    if (E < 0 && (a & (a - 1)) == 0) k -= 1;   // below a negative power of two the spacing is that of the binade underneath
    k = k < 0 ? 0 : k;
    const uint32_t lo = 0x02010000u, hi = 0x2C160B05u;   // thresholds 0 0 1 2 | 5 11 22 44, one byte per k
    const uint32_t T = ((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xFFu;
    int l = E + (m > T ? 1 : 0);
    l = l < -127 ? -127 : (l > 127 ? 127 : l);
    return (uint32_t)(l + 127);
}
