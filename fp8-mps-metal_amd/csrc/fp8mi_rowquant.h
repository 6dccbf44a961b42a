// The shared part of the row-quantising kernels (fp8mi_rowwise.hip, fp8mi_actquant.hip, fp8mi_normquant.hip).  A producer differs in how a
// lane obtains the fp32 values y of its 16-byte pieces; everything after that point, and the choice of a kernel form, is here:
//   - a piece: unpacking it, its encoders, the reductions (DPP inside a row of 16 lanes, readlane across; row_max / row_sum over the
//     waves of a row through LDS);
//   - one scale per row (QS = an ENC value): scale_of_amax (fp8mi_encode.h), the expressions in double precision; row_scale, lane 0's scale broadcast
//     (and published: the rowwise quantiser); publish_row, the publication by one lane (the fused producers);
//   - the local recipes, which hold nothing across a row: one scale per 128 columns (QS = kQGroup) and one E8M0 byte per 32 columns
//     with e4m3 or e2m1 elements (QS = kQMx8 / kQMx4), behind local_piece (a 16-byte piece per lane) and local_pair (the any-alignment
//     form: two columns per lane);
//   - the output side of a launch is a QuantOut (fp8mi_common.h); scale_row<QS> gives its scales their type;
//   - host: the launch ladder (row_rung, launch_row_reg / launch_row_loop) and dispatch_qs (dispatch_int / dispatch_in: fp8mi_common.h).
// The element steps of the local recipes that the stand-alone kernels of fp8mi_cast.hip use as well are in fp8mi_mx.h (mx_factor, mx_scaled,
// mx_e2m1) and fp8mi_encode.h (group_quotient, group_quant1).
#pragma once

#include "fp8mi_common.h"
#include "fp8mi_encode.h"
#include "fp8mi_mx.h"
#define FP8MI_MXEXP_FN FP8MI_DEVICE
#include "fp8mi_mx_exponent.h"

namespace {

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

// maximum / sum over the W waves of a row (every lane of every wave takes part and ends with the same value; the sum adds the waves
// in wave order); `lds` holds W floats that nothing else uses
template <int W>
FP8MI_DEVICE float row_max(float m, float *lds, int wave, int lane)
{
    m = wave_max(m);
    if (W > 1) {
        if (lane == 0) lds[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < W; ++w) m = fmaxf(m, lds[w]);
    }
    return m;
}

template <int W>
FP8MI_DEVICE float row_sum(float v, float *lds, int wave, int lane)
{
    v = wave_sum(v);
    if (W > 1) {
        if (lane == 0) lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < W; ++w) v = v + lds[w];
    }
    return v;
}

// the row's scale, evaluated by lane 0 alone and broadcast; `publish`: this wave also writes the row's inverse scale to scales[slot]
// (and amax to amax_out[r])
template <int ENC>
FP8MI_DEVICE float row_scale(float amax, int lane, bool publish, float *__restrict__ scales, int64_t slot, float *__restrict__ amax_out, int64_t r)
{
    float scale = 1.0f;
    if (lane == 0) {
        float inv;
        scale_of_amax<ENC>(amax, scale, inv);
        if (publish) {
            scales[slot] = inv;
            if (amax_out) amax_out[r] = amax;
        }
    }
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, scale)));
}

// the same publication on its own, by ONE lane of the row (the fused producers: the broadcast scale above then needs no double precision
// in the waves that do not publish, and the registers of the division are not live while a row's y is held)
template <int ENC>
FP8MI_DEVICE void publish_row(float amax, float *__restrict__ scales, int64_t slot, float *__restrict__ amax_out, int64_t r)
{
    float scale, inv;
    scale_of_amax<ENC>(amax, scale, inv);
    scales[slot] = inv;
    if (amax_out) amax_out[r] = amax;
}

constexpr int kQGroup = 3;   // QS template argument: FP8MI_ENC_REFERENCE (0), FP8MI_ENC_RNE (1), kEncE5M2 (2): one scale per row; or this

// ---- FP8MI_QSCALE_GROUP128: the recipe of quantize_blockwise_kernel on |y|'s bit patterns (a NaN is larger than every number) ----
template <int CTRL>
FP8MI_DEVICE uint32_t dpp_umax(uint32_t x)   // every lane of the wave is active wherever this is called
{
    const int y = __builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
    return max(x, (uint32_t)y);
}

FP8MI_DEVICE uint32_t row16_umax(uint32_t v)   // all 16 lanes of a DPP row: the four DPP steps of wave_max
{
    v = dpp_umax<0xB1>(v);
    v = dpp_umax<0x4E>(v);
    v = dpp_umax<0x141>(v);
    return dpp_umax<0x140>(v);
}

FP8MI_DEVICE uint32_t wave_umax(uint32_t v)
{
    v = row16_umax(v);
    const uint32_t r0 = __builtin_amdgcn_readlane((int)v, 0), r1 = __builtin_amdgcn_readlane((int)v, 16), r2 = __builtin_amdgcn_readlane((int)v, 32),
                   r3 = __builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}

FP8MI_DEVICE uint32_t abs_bits(float y) { return __float_as_uint(y) & 0x7FFFFFFFu; }

FP8MI_DEVICE float group_scale(uint32_t amax_bits)
{
    const float d = __uint_as_float(amax_bits) / 448.0f;
    return amax_bits > 0x7F800000u ? __uint_as_float(0x7FC00000u) : (d == 0.0f ? 1.0f : d);
}

FP8MI_DEVICE uint32_t group_quant4(float y0, float y1, float y2, float y3, float s)
{
    const float q0 = group_quotient(y0, s), q1 = group_quotient(y1, s), q2 = group_quotient(y2, s), q3 = group_quotient(y3, s);
    const uint32_t w = encode4<FP8MI_ENC_RNE>(q0, q1, q2, q3);   // a NaN comes out as 0x7F with the NaN's sign bit: the recipe stores 0x7F
    const uint32_t nan_sign = (q0 != q0 ? 0x80u : 0u) | (q1 != q1 ? 0x8000u : 0u) | (q2 != q2 ? 0x800000u : 0u) | (q3 != q3 ? 0x80000000u : 0u);
    return w & ~nan_sign;
}

// the KPER encoded bytes of a piece (w1: the second four of a 16-bit piece), and their store as piece v of an output row
template <int QS, int KPER>
FP8MI_DEVICE void piece_words(const float (&y)[8], float scale, uint32_t &w0, uint32_t &w1)
{
    w1 = 0u;
    if (QS == kQGroup) {
        w0 = group_quant4(y[0], y[1], y[2], y[3], scale);
        if (KPER == 8) w1 = group_quant4(y[4], y[5], y[6], y[7], scale);
    } else {
        w0 = quant4<QS == kQGroup ? FP8MI_ENC_RNE : QS>(y[0], y[1], y[2], y[3], scale);
        if (KPER == 8) w1 = quant4<QS == kQGroup ? FP8MI_ENC_RNE : QS>(y[4], y[5], y[6], y[7], scale);
    }
}

template <int KPER>
FP8MI_DEVICE void store_words(uint32_t w0, uint32_t w1, uint8_t *orow, int64_t v)
{
    if (KPER == 4)
        __builtin_nontemporal_store(w0, (uint32_t *)orow + v);
    else
        __builtin_nontemporal_store(u32x2{w0, w1}, (u32x2 *)orow + v);
}

template <int QS, int KPER>
FP8MI_DEVICE void store_piece(const float (&y)[8], float scale, uint8_t *orow, int64_t v)
{
    uint32_t w0, w1;
    piece_words<QS, KPER>(y, scale, w0, w1);
    store_words<KPER>(w0, w1, orow, v);
}

// the group's scale from this lane's piece (every lane of the wave takes part), published by the lane that owns the group's first piece
template <int KPER>
FP8MI_DEVICE float piece_group_scale(const float (&y)[8], int lane, bool in_row, int64_t v, float *__restrict__ srow, int64_t s_sk)
{
    constexpr int kGpp = 128 / KPER;   // pieces per group: 16 lanes (one DPP row) or 32
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < KPER; ++k) m = max(m, abs_bits(y[k]));
    m = row16_umax(m);
    if (KPER == 4) m = max(m, (uint32_t)__shfl_xor((int)m, 16, 64));
    const float s = group_scale(m);
    if (in_row && (lane & (kGpp - 1)) == 0) srow[(v / kGpp) * s_sk] = s;
    return s;
}

// ---- MX outputs (FP8MI_MX_FP8 / FP8MI_MX_FP4): the recipes of quantize_mxfp8_kernel / quantize_mxfp4_kernel (fp8mi_cast.hip) on y --------
// One E8M0 byte per 32 columns.  A block is 32 / KPER adjacent lanes of one piece (4 for 16-bit input, 8 for fp32) - or, in the
// any-alignment looping forms, the 16 lanes of a DPP row with two columns each.  cols is a multiple of 32, so no block is split
// between lanes inside the row and lanes past it.  The exponent comes from mx_rceil_biased (fp8mi_mx_exponent.h: integer arithmetic,
// proven equal to mx_exponent's double log2 over every float); the factor, the clamp and the element encoders are the recipes' own.
constexpr int kQMx8 = 4, kQMx4 = 5;   // QS template arguments: kQMx8 + FP8MI_MX_FP8 / FP8MI_MX_FP4
constexpr int kMxPad = 1, kMxWord = 2;   // scale flags: the row has room for round_up(cols / 32, 4) bytes; and its rows are 4-byte aligned

template <int QS>
FP8MI_DEVICE uint32_t mx_block_exponent(uint32_t amax_bits)   // amax_bits: the unsigned maximum of |y|'s bit patterns (a NaN is the largest)
{
    if (amax_bits > 0x7F800000u) return 0xFFu;
    const float d = __uint_as_float(amax_bits) / (QS == kQMx4 ? 6.0f : 448.0f);   // the IEEE division of the recipe
    return mx_rceil_biased(__float_as_uint(d));
}

template <int CTRL>
FP8MI_DEVICE uint32_t dpp_or(uint32_t x)   // every lane of the wave is active wherever this is called
{
    return x | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
}

// The KPER elements of a piece encoded with the block's exponent - MXFP8: KPER bytes (w1: the second four of a 16-bit piece); MXFP4: KPER
// nibbles in w0, the even column in the low one - and their store as piece v of an output row: 8 / 4 bytes (MXFP8), 4 / 2 bytes (MXFP4).
// Two halves, as piece_words / store_words: the scatter-quantiser encodes once and stores k times.
template <int QS, int KPER>
FP8MI_DEVICE void piece_words_mx(const float (&y)[8], uint32_t e, uint32_t &w0, uint32_t &w1)
{
    const float f = mx_factor(e);
    w1 = 0u;
    if (QS == kQMx4) {
        uint32_t w = 0u;
#pragma unroll
        for (int k = 0; k < KPER; ++k) w |= mx_e2m1(y[k], f) << (4 * k);
        w0 = w;
    } else {
        w0 = encode4<FP8MI_ENC_RNE>(mx_scaled(y[0], f, 448.0f), mx_scaled(y[1], f, 448.0f), mx_scaled(y[2], f, 448.0f),
                                    mx_scaled(y[3], f, 448.0f));   // a NaN comes out as 0x7F with its sign bit, as the recipe has it
        if (KPER == 8)
            w1 = encode4<FP8MI_ENC_RNE>(mx_scaled(y[4], f, 448.0f), mx_scaled(y[5], f, 448.0f), mx_scaled(y[6], f, 448.0f),
                                        mx_scaled(y[7], f, 448.0f));
    }
}

template <int QS, int KPER>
FP8MI_DEVICE void store_words_mx(uint32_t w0, uint32_t w1, uint8_t *orow, int64_t v)
{
    if (QS == kQMx4) {
        if (KPER == 4)
            __builtin_nontemporal_store((uint16_t)w0, (uint16_t *)orow + v);
        else
            __builtin_nontemporal_store(w0, (uint32_t *)orow + v);
    } else {
        store_words<KPER>(w0, w1, orow, v);
    }
}

template <int QS, int KPER>
FP8MI_DEVICE void store_piece_mx(const float (&y)[8], uint32_t e, uint8_t *orow, int64_t v)
{
    uint32_t w0, w1;
    piece_words_mx<QS, KPER>(y, e, w0, w1);
    store_words_mx<QS, KPER>(w0, w1, orow, v);
}

// Piece v of a row (nv pieces), every lane of the wave taking part: the block's exponent over its 4 or 8 lanes, the elements, and the
// scale bytes.  Four blocks are 16 (32) adjacent lanes: where one of them is in the row, the ones past it are the pad bytes
// cols / 32 .. round_up(cols / 32, 4) - 1 and get 0x7F (2^0) if the row has room (kMxPad).  kMxWord: the four bytes of a DPP row are
// gathered into one dword store (fp32 input: the two bytes of a DPP row into one 2-byte store); otherwise one byte per block.
template <int QS, int KPER>
FP8MI_DEVICE void mx_piece(const float (&y)[8], int lane, int64_t v, int64_t nv, uint8_t *orow, uint8_t *srow, int sflags)
{
    constexpr int kBl = 32 / KPER;   // lanes per block
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < KPER; ++k) m = max(m, abs_bits(y[k]));
    m = dpp_umax<0xB1>(m);                     // quad_perm [1, 0, 3, 2]
    m = dpp_umax<0x4E>(m);                     // quad_perm [2, 3, 0, 1]
    if (kBl == 8) m = dpp_umax<0x141>(m);      // row_half_mirror
    const uint32_t e = mx_block_exponent<QS>(m);
    const bool in_row = v < nv;
    if (in_row) store_piece_mx<QS, KPER>(y, e, orow, v);
    const bool live = (v & ~(int64_t)(4 * kBl - 1)) < nv;   // this lane's four blocks hold a block of the row
    const uint32_t byte = in_row ? e : 0x7Fu;
    const int64_t b = v / kBl;
    if (sflags & kMxWord) {
        if (KPER == 8) {
            uint32_t w = byte << (8 * ((lane >> 2) & 3));
            w = dpp_or<0x141>(w);   // quads 0 | 1 and 2 | 3 ...
            w = dpp_or<0x140>(w);   // ... and all four (row_mirror)
            if (live && (lane & 15) == 0) *(uint32_t *)(srow + b) = w;
        } else {
            uint32_t w = byte << (8 * ((lane >> 3) & 1));
            w = dpp_or<0x140>(w);
            if (live && (lane & 15) == 0) *(uint16_t *)(srow + b) = (uint16_t)w;
        }
    } else if ((lane & (kBl - 1)) == 0 && (in_row || ((sflags & kMxPad) && live))) {
        srow[b] = (uint8_t)byte;
    }
}

// The any-alignment form: lane l of a wave holds the columns c0 = 128 cb + 2 l and c0 + 1 of a 128-column step, a block is the 16
// lanes of a DPP row; byte stores (one byte per lane for MXFP4), the step's four scale bytes as one dword where kMxWord allows.
template <int QS>
FP8MI_DEVICE void mx_pair(float y0, float y1, int lane, bool in_row, int64_t c0, uint8_t *orow, uint8_t *srow, int sflags)
{
    const uint32_t e = mx_block_exponent<QS>(row16_umax(max(abs_bits(y0), abs_bits(y1))));
    const float f = mx_factor(e);
    if (in_row) {
        if (QS == kQMx4) {
            orow[c0 >> 1] = (uint8_t)(mx_e2m1(y0, f) | (mx_e2m1(y1, f) << 4));
        } else {
            orow[c0] = (uint8_t)encode_rne_bits(__float_as_uint(mx_scaled(y0, f, 448.0f)));
            orow[c0 + 1] = (uint8_t)encode_rne_bits(__float_as_uint(mx_scaled(y1, f, 448.0f)));
        }
    }
    const uint32_t byte = in_row ? e : 0x7Fu;
    if (sflags & kMxWord) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)byte, 0) | ((uint32_t)__builtin_amdgcn_readlane((int)byte, 16) << 8) |
                           ((uint32_t)__builtin_amdgcn_readlane((int)byte, 32) << 16) | ((uint32_t)__builtin_amdgcn_readlane((int)byte, 48) << 24);
        if (lane == 0) *(uint32_t *)(srow + (c0 >> 5)) = w;
    } else if ((lane & 15) == 0 && (in_row || (sflags & kMxPad))) {
        srow[c0 >> 5] = (uint8_t)byte;
    }
}

// the GROUP128 counterpart (the layout of quantize_blockwise_kernel): a wave is one group; n of the lane's two columns are in the row
FP8MI_DEVICE void group_pair(float y0, float y1, int lane, int n, int64_t c0, uint8_t *orow, float *srow, int64_t s_sk)
{
    const float s = group_scale(wave_umax(max(abs_bits(y0), abs_bits(y1))));
    if (n > 0) orow[c0] = (uint8_t)group_quant1(y0, s);
    if (n > 1) orow[c0 + 1] = (uint8_t)group_quant1(y1, s);
    if (lane == 0) srow[(c0 >> 7) * s_sk] = s;
}

// ---- the output side of a producer (QuantOut) -------------------------------------------------------------------------------------
template <int QS>
using ScaleT = std::conditional_t<QS == kQMx8 || QS == kQMx4, uint8_t, float>;

template <int QS>
FP8MI_DEVICE ScaleT<QS> *scale_row(const QuantOut &q, int64_t r) { return (ScaleT<QS> *)q.scales + r * q.s_sr; }

// a local recipe (QS >= kQGroup) on piece v of a row of nv pieces, every lane of the wave taking part (a piece past the row: zeros)
template <int QS, int KPER>
FP8MI_DEVICE void local_piece(const QuantOut &q, const float (&y)[8], int lane, int64_t v, int64_t nv, uint8_t *orow, ScaleT<QS> *srow)
{
    if constexpr (QS == kQGroup) {
        const float s = piece_group_scale<KPER>(y, lane, v < nv, v, srow, q.s_sk);
        if (v < nv) store_piece<QS, KPER>(y, s, orow, v);
    } else {
        mx_piece<QS, KPER>(y, lane, v, nv, orow, srow, q.mx_flags);
    }
}

// ... and on the columns c0, c0 + 1 of the any-alignment form, n (0 .. 2; MX: 0 or 2) of them in the row
template <int QS>
FP8MI_DEVICE void local_pair(const QuantOut &q, float y0, float y1, int lane, int n, int64_t c0, uint8_t *orow, ScaleT<QS> *srow)
{
    if constexpr (QS == kQGroup)
        group_pair(y0, y1, lane, n, c0, orow, srow, q.s_sk);
    else
        mx_pair<QS>(y0, y1, lane, n != 0, c0, orow, srow, q.mx_flags);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the scale flags of a launch
inline int mx_scale_flags(const void *scales, int64_t rows, int64_t cols, int64_t ld_s)
{
    const int64_t nb = cols / 32;
    if (ld_s < (nb + 3) / 4 * 4) return 0;
    return kMxPad | ((((uintptr_t)scales & 3u) == 0 && (rows == 1 || ld_s % 4 == 0)) ? kMxWord : 0);
}

// The launch ladder.  A register-resident kernel holds 8 pieces per lane (NV; the rowwise quantiser, which holds them as loaded, has an
// NV = 2 form for short rows): one wave per row up to 8 pieces per lane of ONE wave that holds the row, four waves up to 32, eight (fp32
// input only) up to 64; rows beyond kRowMaxRegCols columns take the looping form, as does whatever the caller finds misaligned.
constexpr int kRowLoopBlock = 256;       // threads of a looping kernel: one workgroup per row
constexpr int kRowMaxRegCols = 16384;
constexpr int64_t kRowMaxRows = 0x7FFFFFFF;   // a row (or four) per workgroup along grid.x

inline bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

struct RowRung {
    int w, nv;   // waves per row and pieces per lane of the register-resident form; w == 0: the looping form
};

inline RowRung row_rung(int64_t cols, int kPer, bool is_f32, bool has_nv2 = false)
{
    const int64_t pieces = (cols / kPer + 63) / 64;
    if (cols > kRowMaxRegCols) return {0, 0};
    if (pieces <= 2 && has_nv2) return {1, 2};
    if (pieces <= 8) return {1, 8};
    if (pieces <= 32) return {4, 8};
    if (is_f32 && pieces <= 64) return {8, 8};   // fp32 rows of 8193 .. 16384 columns
    return {0, 0};
}

// W == 1: four rows per workgroup; W >= 4: one row per workgroup
template <int W, typename... K, typename... A>
int launch_row_reg(void (*kernel)(K...), int64_t rows, hipStream_t s, A... args)
{
    return fp8mi_launch<K...>(kernel, dim3((unsigned)(W == 1 ? (rows + 3) / 4 : rows)), dim3(W == 1 ? 256 : 64 * W), s, args...);
}

template <typename... K, typename... A>
int launch_row_loop(void (*kernel)(K...), int64_t rows, hipStream_t s, A... args)
{
    return fp8mi_launch<K...>(kernel, dim3((unsigned)rows), dim3(kRowLoopBlock), s, args...);
}

template <typename F>
int dispatch_qs(int qs, F &&f) { return dispatch_int<kQGroup, kQMx8, kQMx4, kEncE5M2, FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(qs, f); }

}  // namespace
