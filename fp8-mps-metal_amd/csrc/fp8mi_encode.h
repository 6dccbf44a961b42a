// Device-side encoders shared by the cast kernels (fp8mi_cast.hip) and the per-row quantiser (fp8mi_rowwise.hip): float32 -> e4m3fn byte(s)
// in both encode modes, float32 -> e5m2 byte, and the typed loads of the three input dtypes.  Header-only, force-inlined.
#pragma once

#include "fp8mi_common.h"

// ---------------------------------------------------------------------------
// encode: float32 bits -> fp8 byte, integer-only.
// ---------------------------------------------------------------------------

// reference semantics (fp8_matmul.metal:44-92, exact-arithmetic behaviour of
// its Python twin test_fp8_correctness.py:53-106)
FP8MI_DEVICE uint32_t encode_ref_bits(uint32_t bits)
{
    uint32_t a = bits & 0x7FFFFFFFu;
    uint32_t sign = (a != 0u) ? ((bits >> 24) & 0x80u) : 0u;  // `val < 0`: -0.0 has no sign (:46)
    uint32_t e = a >> 23, man = a & 0x7FFFFFu;
    // normal range: top three mantissa bits, RNE on the low 20, clamp (no carry, :79-81)
    uint32_t qn = (man + 0x7FFFFu + ((man >> 20) & 1u)) >> 20;
    qn = min(qn, 7u);
    uint32_t eb = e - 120u;
    qn = (eb == 15u && qn == 7u) ? 6u : qn;  // never the NaN pattern (:87-89)
    uint32_t normal = (eb << 3) | qn;
    // subnormal range [2^-9, 2^-6): mant = RNE(val * 512), clamp to 7 (:64-70)
    uint32_t s = 141u - e;  // 21..23 in this range
    s = min(max(s, 1u), 31u);
    uint32_t full = man | 0x800000u;
    uint32_t qs = (full + ((1u << (s - 1u)) - 1u) + ((full >> s) & 1u)) >> s;
    qs = min(qs, 7u);
    uint32_t r = (a < 0x3C800000u) ? qs : normal;  // < 2^-6
    r = (a < 0x3B000000u) ? 0u : r;                 // < 2^-9 flushes, sign kept (:58-60)
    r = (a >= 0x43E00000u) ? 0x7Eu : r;             // >= 448 saturates, also inf (:53-55)
    r |= sign;
    return (a > 0x7F800000u) ? 0x7Fu : r;           // NaN in: outside the reference's domain
}

// OCP e4m3fn round-to-nearest-even with overflow to NaN: what torch-CPU
// `.to(torch.float8_e4m3fn)` produces (non-default mode).
FP8MI_DEVICE uint32_t encode_rne_bits(uint32_t bits)
{
    uint32_t a = bits & 0x7FFFFFFFu;
    uint32_t sign = (bits >> 24) & 0x80u;
    uint32_t e = a >> 23, man = a & 0x7FFFFFu;
    uint32_t v = ((e - 120u) << 23) | man;
    uint32_t n = (v + 0x7FFFFu + ((v >> 20) & 1u)) >> 20;  // carry may bump the exponent
    uint32_t s = min(max(141u - e, 1u), 31u);
    uint32_t full = man | 0x800000u;
    uint32_t qs = (full + ((1u << (s - 1u)) - 1u) + ((full >> s) & 1u)) >> s;
    qs = (e < 110u) ? 0u : qs;  // below 2^-17: far under half the smallest subnormal
    uint32_t r = (e < 121u) ? qs : n;
    r = (r > 0x7Eu) ? 0x7Fu : r;
    r = (a > 0x7F800000u) ? 0x7Fu : r;
    return r | sign;
}

template <int MODE>
FP8MI_DEVICE uint32_t encode_bits(float v)
{
    uint32_t b = __float_as_uint(v);
    return MODE == FP8MI_ENC_REFERENCE ? encode_ref_bits(b) : encode_rne_bits(b);
}

// Reference-semantics encode of TWO floats around the hardware convert.
// v_cvt_pk_fp8_f32 does the in-range work (OCP round-to-nearest-even onto the
// e4m3 grid, subnormals included); what the reference does differently
// (fp8_matmul.metal:44-92) is patched with a few integer ops per element:
//   * no carry: if rounding bumped the exponent field (1.9375 -> 2.0, or the
//     top subnormal -> 2^-6) the reference keeps mantissa 7 of the ORIGINAL
//     binade, which is exactly "one code below" the carried result;
//   * |x| < 2^-9 flushes to zero (sign kept), |x| >= 448 and inf saturate to
//     0x7E - both selected explicitly, so the hardware's own underflow /
//     overflow behaviour is never relied upon;
//   * -0.0 -> 0x00; NaN (outside the reference's domain) -> 0x7F.
// 19 VALU ops per element instead of 37 for the all-integer form; verified on
// the same 147k golden vectors.
FP8MI_DEVICE uint32_t encode_ref_pair(float v0, float v1)
{
    const uint32_t b0 = __float_as_uint(v0), b1 = __float_as_uint(v1);
    const uint32_t a0 = b0 & 0x7FFFFFFFu, a1 = b1 & 0x7FFFFFFFu;
    const uint32_t pk = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(a0), __uint_as_float(a1), 0, false);
    uint32_t h0 = pk & 0xFFu, h1 = (pk >> 8) & 0xFFu;
    // exponent field the reference keeps: that of the input's own binade (0 below 2^-6)
    const uint32_t e0 = max(a0 >> 23, 120u) - 120u, e1 = max(a1 >> 23, 120u) - 120u;
    h0 -= ((h0 >> 3) != e0) ? 1u : 0u;
    h1 -= ((h1 >> 3) != e1) ? 1u : 0u;
    h0 = (a0 < 0x3B000000u) ? 0u : h0;
    h1 = (a1 < 0x3B000000u) ? 0u : h1;
    h0 = (a0 >= 0x43E00000u) ? 0x7Eu : h0;
    h1 = (a1 >= 0x43E00000u) ? 0x7Eu : h1;
    h0 |= (a0 != 0u) ? ((b0 >> 24) & 0x80u) : 0u;
    h1 |= (a1 != 0u) ? ((b1 >> 24) & 0x80u) : 0u;
    h0 = (a0 > 0x7F800000u) ? 0x7Fu : h0;
    h1 = (a1 > 0x7F800000u) ? 0x7Fu : h1;
    return h0 | (h1 << 8);
}

// torch / OCP semantics (FP8MI_ENC_RNE) of TWO floats around the same hardware convert: gfx950's v_cvt_pk_fp8_f32 IS
// OCP round-to-nearest-even onto the e4m3fn grid, so inside [2^-9, 448] its byte is torch-CPU's byte; the edges are
// selected explicitly so that the instruction's own underflow / overflow behaviour is never relied upon:
//   |x| <= 2^-10 -> 0 (the tie with the smallest subnormal goes to even), 2^-10 < |x| < 2^-9 -> 0x01,
//   448 < |x| <= 464 -> 0x7E (464 ties to even), |x| > 464, inf and NaN -> 0x7F; the sign bit is the input's (-0.0 -> 0x80).
// ~12 VALU ops per element instead of ~37 for encode_rne_bits (kept for the scalar tails); byte-exact against
// torch-CPU `.to(float8_e4m3fn)` on the 147k golden vectors (tests/test_gpu_parity.py, the check of test_mps_vs_cpu.py:283-357).
FP8MI_DEVICE uint32_t encode_rne_pair(float v0, float v1)
{
    const uint32_t b0 = __float_as_uint(v0), b1 = __float_as_uint(v1);
    const uint32_t a0 = b0 & 0x7FFFFFFFu, a1 = b1 & 0x7FFFFFFFu;
    const uint32_t pk = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(a0), __uint_as_float(a1), 0, false);
    uint32_t h0 = pk & 0xFFu, h1 = (pk >> 8) & 0xFFu;
    h0 = (a0 < 0x3B000000u) ? 1u : h0;
    h1 = (a1 < 0x3B000000u) ? 1u : h1;
    h0 = (a0 <= 0x3A800000u) ? 0u : h0;
    h1 = (a1 <= 0x3A800000u) ? 0u : h1;
    h0 = (a0 > 0x43E00000u) ? 0x7Eu : h0;
    h1 = (a1 > 0x43E00000u) ? 0x7Eu : h1;
    h0 = (a0 > 0x43E80000u) ? 0x7Fu : h0;   // also inf and NaN
    h1 = (a1 > 0x43E80000u) ? 0x7Fu : h1;
    h0 |= (b0 >> 24) & 0x80u;
    h1 |= (b1 >> 24) & 0x80u;
    return h0 | (h1 << 8);
}

// four floats -> four packed bytes
template <int MODE>
FP8MI_DEVICE uint32_t encode4(float v0, float v1, float v2, float v3)
{
    if (MODE == FP8MI_ENC_REFERENCE) return encode_ref_pair(v0, v1) | (encode_ref_pair(v2, v3) << 16);
    return encode_rne_pair(v0, v1) | (encode_rne_pair(v2, v3) << 16);
}

template <int IN>
struct InVec;  // loads 16 elements as float

template <>
struct InVec<FP8MI_F32> {
    static FP8MI_DEVICE void load(const void *in, int64_t i16, float (&f)[16])
    {
        const f32x4 *p = (const f32x4 *)in + i16 * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 v = __builtin_nontemporal_load(p + j);
            f[4 * j] = v[0]; f[4 * j + 1] = v[1]; f[4 * j + 2] = v[2]; f[4 * j + 3] = v[3];
        }
    }
    static FP8MI_DEVICE float load1(const void *in, int64_t i) { return ((const float *)in)[i]; }
    static constexpr int kPer = 4;  // elements per 16-byte load
    static FP8MI_DEVICE void loadv(const void *in, int64_t iv, float (&f)[8])
    {
        f32x4 v = __builtin_nontemporal_load((const f32x4 *)in + iv);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    }
};

template <>
struct InVec<FP8MI_F16> {
    static FP8MI_DEVICE void load(const void *in, int64_t i16, float (&f)[16])
    {
        const u32x4 *p = (const u32x4 *)in + i16 * 2;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x4 v = __builtin_nontemporal_load(p + j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // NB: bit_cast straight from the vector element v[q] miscompiles
                // (every q reads element 0, hipcc 7.2); go through a scalar.
                const uint32_t w = v[q];
                f[8 * j + 2 * q] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
                f[8 * j + 2 * q + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
            }
        }
    }
    static FP8MI_DEVICE float load1(const void *in, int64_t i) { return (float)((const _Float16 *)in)[i]; }
    static constexpr int kPer = 8;
    static FP8MI_DEVICE void loadv(const void *in, int64_t iv, float (&f)[8])
    {
        u32x4 v = __builtin_nontemporal_load((const u32x4 *)in + iv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = v[q];  // (bit_cast straight from v[q] miscompiles, see load())
            f[2 * q] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
            f[2 * q + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
        }
    }
};

template <>
struct InVec<FP8MI_BF16> {
    static FP8MI_DEVICE void load(const void *in, int64_t i16, float (&f)[16])
    {
        const u32x4 *p = (const u32x4 *)in + i16 * 2;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x4 v = __builtin_nontemporal_load(p + j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f[8 * j + 2 * q] = __uint_as_float(v[q] << 16);
                f[8 * j + 2 * q + 1] = __uint_as_float(v[q] & 0xFFFF0000u);
            }
        }
    }
    static FP8MI_DEVICE float load1(const void *in, int64_t i)
    {
        return __uint_as_float((uint32_t)((const uint16_t *)in)[i] << 16);
    }
    static constexpr int kPer = 8;
    static FP8MI_DEVICE void loadv(const void *in, int64_t iv, float (&f)[8])
    {
        u32x4 v = __builtin_nontemporal_load((const u32x4 *)in + iv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f[2 * q] = __uint_as_float(v[q] << 16);
            f[2 * q + 1] = __uint_as_float(v[q] & 0xFFFF0000u);
        }
    }
};

// Encode: round to nearest even onto the e5m2 grid (1-5-2, bias 15: an e5m2 byte is the high byte of an IEEE half), byte for
// byte torch's CPU cast: finite values that round past 57344 become +-inf (0x7C / 0xFC: from 61440 up), NaN becomes 0x7F with the
// input's sign bit, -0.0 is 0x80, subnormals go down to 2^-16 (below 2^-17, and 2^-17 itself, to zero).  On fp32 bits:
//   normal results (|v| >= 2^-14): rebias, add the round-to-nearest-even increment below bit 21, keep bits 21 and up - a mantissa
//   carry runs into the exponent, and past exponent 30 into the inf pattern;
//   subnormal results: |v| + 128.0f rounds |v| to a multiple of 2^-16 (the ulp of [128, 256)) to nearest even in the fp32 adder, and
//   the count of 2^-16 steps is the sum's low mantissa bits.
FP8MI_DEVICE uint32_t encode_e5m2_bits(float v)
{
    uint32_t b = __float_as_uint(v);
    const uint32_t sign = (b >> 24) & 0x80u;
    b &= 0x7FFFFFFFu;
    uint32_t r;
    if (b >= 0x47800000u) {                 // |v| >= 65536, inf, NaN
        r = b > 0x7F800000u ? 0x7Fu : 0x7Cu;
    } else if (b < (113u << 23)) {          // |v| < 2^-14
        const float t = __uint_as_float(b) + 128.0f;
        r = __float_as_uint(t) - (134u << 23);
    } else {
        const uint32_t odd = (b >> 21) & 1u;
        r = (b - (112u << 23) + 0xFFFFFu + odd) >> 21;
    }
    return r | sign;
}

constexpr int kEncE5M2 = 2;   // ENC template argument: FP8MI_ENC_REFERENCE (0), FP8MI_ENC_RNE (1) for e4m3, or this

// The scale of an amax-scaled quantiser and the inverse scale it publishes, with the format's largest value - scale = FMAX / amax evaluated in
// double, as the reference's Python float arithmetic (fp8_mps_native.py:174-176, :189); amax == 0 -> 1.  The one place that holds the
// expressions: the per-tensor casts (fp8mi_cast.hip) and every row quantiser (fp8mi_rowquant.h) take them from here.
template <int ENC>
constexpr double kFormatMax = ENC == kEncE5M2 ? 57344.0 : 448.0;

template <int ENC>
FP8MI_DEVICE float scale_of_amax(float amax) { return amax > 0.0f ? (float)(kFormatMax<ENC> / (double)amax) : 1.0f; }

template <int ENC>
FP8MI_DEVICE float inv_scale_of_amax(float amax) { return amax > 0.0f ? (float)(1.0 / (kFormatMax<ENC> / (double)amax)) : 1.0f; }

// both at once, the division shared (the row quantisers: one lane evaluates it for its row)
template <int ENC>
FP8MI_DEVICE void scale_of_amax(float amax, float &scale, float &inv)
{
    scale = 1.0f;
    inv = 1.0f;
    if (amax > 0.0f) {
        const double s = kFormatMax<ENC> / (double)amax;
        scale = (float)s;
        inv = (float)(1.0 / s);
    }
}

// The blockwise (one fp32 scale s per block) recipe's element steps, stated in fp8mi_cast.hip: the IEEE quotient clamped to +-448, and its
// byte - a NaN quotient is stored as 0x7F
FP8MI_DEVICE float group_quotient(float y, float s)
{
    const float q = y / s;   // the IEEE division of the recipe
    return q < -448.0f ? -448.0f : (q > 448.0f ? 448.0f : q);
}

FP8MI_DEVICE uint32_t group_quant1(float y, float s)
{
    const float q = group_quotient(y, s);
    return q != q ? 0x7Fu : encode_rne_bits(__float_as_uint(q));
}
