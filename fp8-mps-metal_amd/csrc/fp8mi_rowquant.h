// Helpers shared by the row-quantising kernels (fp8mi_rowwise.hip, fp8mi_actquant.hip): unpacking a 16-byte piece, the row maximum
// (DPP inside a row of 16 lanes, readlane across), the per-row scale in double precision and the encoders of a piece.
#pragma once

#include "fp8mi_common.h"
#include "fp8mi_encode.h"

namespace {

constexpr int kEncE5M2 = 2;   // ENC template argument: FP8MI_ENC_REFERENCE (0), FP8MI_ENC_RNE (1) for e4m3, or this

// a 16-byte piece as loaded -> its kPer floats (4 for fp32, 8 for the 16-bit types)
template <int IN>
FP8MI_DEVICE void unpack(const u32x4 &v, float (&f)[8])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t w = v[q];
        if (IN == FP8MI_F32) {
            f[q] = __uint_as_float(w);
        } else if (IN == FP8MI_F16) {
            f[2 * q] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
            f[2 * q + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
        } else {
            f[2 * q] = __uint_as_float(w << 16);
            f[2 * q + 1] = __uint_as_float(w & 0xFFFF0000u);
        }
    }
}

template <int IN>
FP8MI_DEVICE float piece_amax(const u32x4 &v, float m)
{
    float f[8];
    unpack<IN>(v, f);
#pragma unroll
    for (int j = 0; j < InVec<IN>::kPer; ++j) m = fmaxf(m, fabsf(f[j]));   // fmaxf drops NaN operands
    return m;
}

// the e5m2 recipe's value ahead of the encode: the fp32 product, rounded, clamped to +-57344 (a NaN stays NaN)
FP8MI_DEVICE float e5m2_scaled(float x, float scale)
{
    float v = x * scale;
    asm("" : "+v"(v));
    return v > 57344.0f ? 57344.0f : (v < -57344.0f ? -57344.0f : v);
}

template <int ENC>
FP8MI_DEVICE uint32_t quant1(float x, float scale)
{
    if (ENC == kEncE5M2) return encode_e5m2_bits(e5m2_scaled(x, scale));
    return encode_bits<ENC>(x * scale);   // float32 multiply, as `inp * scale` (fp8_mps_native.py:179)
}

template <int ENC>
FP8MI_DEVICE uint32_t quant4(float x0, float x1, float x2, float x3, float scale)
{
    if (ENC == kEncE5M2)
        return encode_e5m2_bits(e5m2_scaled(x0, scale)) | (encode_e5m2_bits(e5m2_scaled(x1, scale)) << 8) |
               (encode_e5m2_bits(e5m2_scaled(x2, scale)) << 16) | (encode_e5m2_bits(e5m2_scaled(x3, scale)) << 24);
    return encode4<ENC == kEncE5M2 ? FP8MI_ENC_RNE : ENC>(x0 * scale, x1 * scale, x2 * scale, x3 * scale);
}

// encode the kPer elements of piece `v` of a row and stream them out (4 or 8 bytes per lane)
template <int IN, int ENC>
FP8MI_DEVICE void quant_piece(const u32x4 &raw, float scale, uint8_t *orow, int64_t v)
{
    float f[8];
    unpack<IN>(raw, f);
    const uint32_t w0 = quant4<ENC>(f[0], f[1], f[2], f[3], scale);
    if (InVec<IN>::kPer == 4) {
        __builtin_nontemporal_store(w0, (uint32_t *)orow + v);
    } else {
        const uint32_t w1 = quant4<ENC>(f[4], f[5], f[6], f[7], scale);
        __builtin_nontemporal_store(u32x2{w0, w1}, (u32x2 *)orow + v);
    }
}

// wave64 all-lanes maximum of non-negative, NaN-free values: DPP inside each row of 16 lanes, then the four rows as scalars
// (the structure of wave_sum; a `__shfl_xor` butterfly is six dependent ds_bpermute round trips)
template <int CTRL>
FP8MI_DEVICE float dpp_max(float x)   // an inactive source lane reads as 0, the identity here
{
    const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false);
    return fmaxf(x, __builtin_bit_cast(float, y));
}

FP8MI_DEVICE float wave_max(float v)
{
    v = dpp_max<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v = dpp_max<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v = dpp_max<0x141>(v);   // row_half_mirror
    v = dpp_max<0x140>(v);   // row_mirror
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)),
                r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// scale_from_amax / encode_kernel<..., FROM_AMAX>'s expressions with the format's largest value, evaluated by lane 0 alone and
// broadcast; `publish`: this wave also writes the row's inverse scale (and amax)
template <int ENC>
FP8MI_DEVICE float row_scale(float amax, int lane, bool publish, float *__restrict__ inv_scales, float *__restrict__ amax_out, int64_t r)
{
    constexpr double kMax = ENC == kEncE5M2 ? 57344.0 : 448.0;
    float scale = 1.0f;
    if (lane == 0) {
        float inv = 1.0f;
        if (amax > 0.0f) {
            const double s = kMax / (double)amax;
            scale = (float)s;
            inv = (float)(1.0 / s);
        }
        if (publish) {
            inv_scales[r] = inv;
            if (amax_out) amax_out[r] = amax;
        }
    }
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, scale)));
}

}  // namespace
