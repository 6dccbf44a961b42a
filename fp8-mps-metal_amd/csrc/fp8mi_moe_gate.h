// The MoE gate (fp8mi_moe_gate): the order on keys and the launch geometry the host launcher and the kernel (fp8mi_moe_gate.hip) share.
// One set of functions for both sides and for the host program that checks them without a GPU (tests/c/moe_gate_key.cpp).
//
// The order of include/fp8mi.h - the larger key first, every NaN above +inf and all NaNs equal, -0 == +0, the smaller index first among
// equal keys - is the UNSIGNED order of one 64-bit word per expert:
//     word(key, e) = ordered32(key) << 32 | (0xFFFFFFFF - e)
// ordered32 is the sign-flip map of a float's bits onto unsigned integers, with NaN canonicalised to the maximum and -0 to +0.  The
// smallest value it takes is that of -inf, 0x007FFFFF, so every real expert's word is above kMoeGatePadWord = 0, the word of a pad slot
// (e >= G) and of an expert outside the kept groups: "first in the order" is one unsigned maximum, and a pad never wins while a real
// expert is left.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FP8MI_GATE_FN __host__ __device__ inline
#else
#define FP8MI_GATE_FN inline
#endif

constexpr int kMoeGateMaxExperts = 1024;      // the grouped GEMM's maximum
constexpr int kMoeGateMaxK = 64;              // FP8MI_MOE_GATE_MAX_K: result j lives in lane j
constexpr int kMoeGateMaxGroups = 64;         // a group's score lives in one lane
constexpr int kMoeGateTokensPerBlock = 4;     // one wave per token
constexpr uint64_t kMoeGatePadWord = 0;

// a float's bits -> an unsigned integer with the same order; NaN (either sign, any payload) -> 0xFFFFFFFF; -0 -> +0's value
FP8MI_GATE_FN uint32_t fp8mi_gate_ordered32(uint32_t bits)
{
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// its inverse up to the canonicalisation: the bits of a float that ordered32 maps to `o` (a NaN for 0xFFFFFFFF, +0 for a zero)
FP8MI_GATE_FN uint32_t fp8mi_gate_unordered32(uint32_t o) { return (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o; }

FP8MI_GATE_FN uint64_t fp8mi_gate_word(uint32_t key_bits, uint32_t e) { return ((uint64_t)fp8mi_gate_ordered32(key_bits) << 32) | (0xFFFFFFFFu - e); }
FP8MI_GATE_FN uint32_t fp8mi_gate_word_index(uint64_t w) { return 0xFFFFFFFFu - (uint32_t)w; }
FP8MI_GATE_FN uint32_t fp8mi_gate_word_key(uint64_t w) { return fp8mi_gate_unordered32((uint32_t)(w >> 32)); }

// keys per lane: lane l of a token's wave holds the experts [l E, (l + 1) E); E is the smallest of 1, 2, 4, 8, 16 with 64 E >= G
FP8MI_GATE_FN int fp8mi_gate_slots(int G)
{
    int E = 1;
    while (64 * E < G) E *= 2;
    return E;
}

// log2 of the lanes that share one group's reduction: the largest power of two L with n_group L <= 64; group g owns lanes [g L, (g + 1) L)
FP8MI_GATE_FN int fp8mi_gate_team_log2(int n_group)
{
    int lg = 0;
    while ((2 << lg) * n_group <= 64) ++lg;
    return lg;
}
