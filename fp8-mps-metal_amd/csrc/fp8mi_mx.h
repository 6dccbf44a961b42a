// The element and exponent helpers of the MX recipes (one E8M0 scale per 32 elements of a row), shared by the stand-alone quantisers
// (fp8mi_cast.hip, where the recipes are stated in full) and the fused producers (fp8mi_rowquant.h).  Header-only, force-inlined.
#pragma once

#include "fp8mi_common.h"

namespace {

FP8MI_DEVICE float pow2_f32(int k)   // 2^k for -149 <= k <= 127, exact (subnormals built from bits)
{
    return k >= -126 ? __uint_as_float((uint32_t)(k + 127) << 23) : __uint_as_float(1u << (k + 149));
}

// the RCEIL exponent of a block whose amax is `amax`, for a format whose largest value is max_pos
FP8MI_DEVICE uint32_t mx_exponent(float amax, float max_pos)
{
    const float descale = amax / max_pos;
    if (descale != descale) return 0xFFu;
    float l = ceilf((float)log2((double)descale));
    l = l < -127.0f ? -127.0f : (l > 127.0f ? 127.0f : l);   // log2(0) = -inf -> -127; inf -> 127
    return (uint32_t)((int)l + 127);
}

// y (|y| <= 6, or NaN) -> bfloat16 bits, RNE; NaN -> 0xFFFF
FP8MI_DEVICE uint32_t bf16_rne_bits(float y)
{
    const uint32_t u = __float_as_uint(y);
    return y != y ? 0xFFFFu : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// a bfloat16 value -> e2m1 code: torchao's _f32_to_floatx_unpacked(x, 2, 1) step for step (int32 arithmetic, uint8 results)
FP8MI_DEVICE uint32_t e2m1_from_bf16(uint32_t bf)
{
    const uint32_t xb = bf << 16, sign = xb & 0x80000000u, ab = xb ^ sign;
    const float x = __uint_as_float(ab);
    uint32_t code;
    if (x >= 6.0f) code = 7u;                                                               // saturate
    else if (x < 1.0f) code = (__float_as_uint(x + 4194304.0f) - (149u << 23)) & 0xFFu;      // below the normal range: + 2^22 rounds
    else code = ((ab + 0xC1000000u + 0x1FFFFFu + ((ab >> 22) & 1u)) >> 22) & 0xFFu;         // normal (and NaN): exponent rebias + RNE
    return code | (sign ? 8u : 0u);
}

// the clamp-and-encode steps of the MX recipes (stated in full in fp8mi_cast.hip): the block's factor, the fp32 product clamped to the
// format's largest value, and the e2m1 code of that product
FP8MI_DEVICE float mx_factor(uint32_t e) { return e == 0 ? 1.0f : pow2_f32(127 - (int)e); }

FP8MI_DEVICE float mx_scaled(float y, float f, float lim)   // the fp32 product, clamped; a NaN stays the NaN it is
{
    const float v = y * f;
    return v != v ? v : (v < -lim ? -lim : (v > lim ? lim : v));
}

FP8MI_DEVICE uint32_t mx_e2m1(float y, float f) { return e2m1_from_bf16(bf16_rne_bits(mx_scaled(y, f, 6.0f))); }

}  // namespace
