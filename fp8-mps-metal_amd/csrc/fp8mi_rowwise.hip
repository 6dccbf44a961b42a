// Per-row dynamic FP8 quantisation (one scale per row: per token for activations, per output channel for weights) and its
// dequantisation, for gfx950.  fp8mi_quantize applied to every row on its own, in ONE launch: no workspace, no atomics, no
// host sync.  No counterpart in the reference, whose fp8_quantize is per tensor (fp8_mps_native.py:158-190).
//
//   amax_r  = max_c |float32(in[r, c])|                         (NaNs ignored, as amax_kernel's fmaxf; 0 for an empty row)
//   scale_r = amax_r > 0 ? FMAX / (double)amax_r : 1            (rounded to fp32; FMAX = 448 for e4m3, 57344 for e5m2)
//   inv_r   = amax_r > 0 ? float(1 / (FMAX / (double)amax_r)) : 1
//   e4m3: out[r, c] = enc<mode>(float32(in[r, c]) * scale_r);   e5m2: out[r, c] = e5m2_rne(clamp(float32(in[r, c]) * scale_r, +-57344))
//
// A row of up to 16384 elements is read from HBM ONCE: every lane loads 16-byte pieces (one contiguous KiB per wave
// instruction, as encode_kernel), keeps them in VGPRs as loaded (NV pieces = 4 NV registers) across the reduction, and encodes
// from those registers.  Short rows: one wave per row, four rows per workgroup, reduced with DPP and readlane only.  Long rows:
// W waves per row, one row per workgroup, the waves' maxima meet in LDS behind one barrier.  Rows beyond 16384 elements, and
// rows whose base or leading dimensions do not allow the 16-byte loads, take the looping form: one workgroup per row, the row
// read twice (the second time from L2: a row is tens of KiB).
// The double-precision division of the scale runs once per wave, in lane 0, and is broadcast with readfirstlane.
// The reductions, the scale, the encoders and the launch ladder are fp8mi_rowquant.h's, shared with the fused producers; what is this
// file's own is that the register-resident form holds the pieces as loaded, not as fp32 - hence its NV = 2 rung.

#include "fp8mi_rowquant.h"

namespace {

// Register-resident form.  W waves share a row; wave w of the row owns the pieces 64 (w + W j) + lane, j < NV: each of its load
// instructions reads one contiguous KiB.  Needs 16-byte aligned rows (base and ld_in), kPer-byte aligned output rows and
// cols <= 64 W NV kPer.  The last cols % kPer elements of a row go through lanes 0.. of the row's first wave, one each.
template <int IN, int ENC, int NV, int W>
__global__ __launch_bounds__(W >= 4 ? 64 * W : 256) void quantize_rowwise_reg_kernel(const void *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in,
                                                                                      uint8_t *__restrict__ out, int64_t ld_out,
                                                                                      float *__restrict__ inv_scales, float *__restrict__ amax_out)
{
    static_assert(W == 1 || W >= 4, "one wave per row (four rows per workgroup) or one row per workgroup");
    constexpr int kPer = InVec<IN>::kPer;
    constexpr int kEsz = IN == FP8MI_F32 ? 4 : 2;
    __shared__ float lds_m[W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = W == 1 ? 0 : wave;
    const int64_t r = W == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
    if (r >= rows) return;   // wave-uniform, and only where a wave is a row (W == 1: no barrier below)
    const uint8_t *rowp = (const uint8_t *)in + r * ld_in * kEsz;
    const u32x4 *in4 = (const u32x4 *)rowp;
    uint8_t *orow = out + r * ld_out;
    const int64_t nv = cols / kPer;
    const int tail = (int)(cols - nv * kPer);

    u32x4 raw[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * (wr + W * j);
        raw[j] = v < nv ? __builtin_nontemporal_load(in4 + v) : u32x4{0u, 0u, 0u, 0u};
    }
    const bool has_tail = wr == 0 && lane < tail;
    const float t = has_tail ? InVec<IN>::load1(rowp, nv * kPer + lane) : 0.0f;

    float m = fabsf(t);
    m = fmaxf(0.0f, m);   // a NaN tail element is ignored like any other
#pragma unroll
    for (int j = 0; j < NV; ++j) m = piece_amax<IN>(raw[j], m);
    m = row_max<W>(m, lds_m, wave, lane);
    const float scale = row_scale<ENC>(m, lane, wr == 0, inv_scales, r, amax_out, r);

#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * (wr + W * j);
        if (v < nv) quant_piece<IN, ENC>(raw[j], scale, orow, v);
    }
    if (has_tail) orow[nv * kPer + lane] = (uint8_t)quant1<ENC>(t, scale);
}

// Looping form: one workgroup per row, any length.  VEC: 16-byte pieces (the alignment of the register form), four in flight per
// lane in the amax pass; otherwise one element per lane and step, any alignment.  The second pass re-reads the row.
template <int IN, int ENC, bool VEC>
__global__ __launch_bounds__(kRowLoopBlock) void quantize_rowwise_loop_kernel(const void *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in,
                                                                              uint8_t *__restrict__ out, int64_t ld_out, float *__restrict__ inv_scales,
                                                                              float *__restrict__ amax_out)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2, U = 4, kWaves = kRowLoopBlock / 64;
    __shared__ float lds_m[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = blockIdx.x;
    const uint8_t *rowp = (const uint8_t *)in + r * ld_in * kEsz;
    const u32x4 *in4 = (const u32x4 *)rowp;
    uint8_t *orow = out + r * ld_out;
    const int64_t nv = VEC ? cols / kPer : 0;

    float m = 0.0f;
    int64_t v = threadIdx.x;
    for (; v + (U - 1) * kRowLoopBlock < nv; v += U * kRowLoopBlock) {
        u32x4 w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = in4[v + u * kRowLoopBlock];
#pragma unroll
        for (int u = 0; u < U; ++u) m = piece_amax<IN>(w[u], m);
    }
    for (; v < nv; v += kRowLoopBlock) m = piece_amax<IN>(in4[v], m);
    for (int64_t c = nv * kPer + threadIdx.x; c < cols; c += kRowLoopBlock) m = fmaxf(m, fabsf(InVec<IN>::load1(rowp, c)));
    m = row_max<kWaves>(m, lds_m, wave, lane);
    const float scale = row_scale<ENC>(m, lane, wave == 0, inv_scales, r, amax_out, r);

    for (v = threadIdx.x; v < nv; v += kRowLoopBlock) quant_piece<IN, ENC>(__builtin_nontemporal_load(in4 + v), scale, orow, v);
    for (int64_t c = nv * kPer + threadIdx.x; c < cols; c += kRowLoopBlock) orow[c] = (uint8_t)quant1<ENC>(InVec<IN>::load1(rowp, c), scale);
}

// ---- dequant: out[r, c] = cast(float(dec(in[r, c])) * scales[r]), the product in fp32 rounded once, then RNE to out_dtype -----
// (the rule of dequant_blockwise_kernel / dequant_e5m2_kernel; OCP decode: NaN bytes give NaN)
template <bool E5M2>
FP8MI_DEVICE float dequant1(uint32_t byte, float s)
{
    float v = decode_fmt(byte, E5M2) * s;
    asm("" : "+v"(v));   // the fp32 product is rounded first: fused with an f16 conversion (v_fma_mix) it would be rounded once, to f16
    return v;
}

// streaming form: 16 bytes in per lane (one contiguous KiB per wave instruction), 32 or 64 bytes out as 16-byte pieces;
// needs cols % 16 == 0 and 16-byte aligned rows of `in` and `out`.  nvr = cols / 16 pieces per row.
template <int OUT, bool E5M2>
__global__ __launch_bounds__(256) void dequant_rowwise_kernel(const uint8_t *__restrict__ in, int64_t rows, int64_t nvr, int64_t ld_in,
                                                              const float *__restrict__ scales, void *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * nvr) return;
    const int64_t r = g / nvr, v = g - r * nvr;
    const u32x4 w = __builtin_nontemporal_load((const u32x4 *)(in + r * ld_in) + v);
    const float s = scales[r];
    float f[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = w[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[4 * q + k] = dequant1<E5M2>((x >> (8 * k)) & 0xFFu, s);
    }
    if (OUT == FP8MI_F32) {
        f32x4 *o = (f32x4 *)out + g * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) __builtin_nontemporal_store(f32x4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]}, o + q);
    } else {
        u32x4 *o = (u32x4 *)out + g * 2;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            __builtin_nontemporal_store(u32x4{pack16<OUT>(f[8 * h], f[8 * h + 1]), pack16<OUT>(f[8 * h + 2], f[8 * h + 3]),
                                              pack16<OUT>(f[8 * h + 4], f[8 * h + 5]), pack16<OUT>(f[8 * h + 6], f[8 * h + 7])}, o + h);
    }
}

// any shape and alignment: one element per lane
template <int OUT, bool E5M2>
__global__ __launch_bounds__(256) void dequant_rowwise_scalar_kernel(const uint8_t *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in,
                                                                     const float *__restrict__ scales, void *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * cols) return;
    const int64_t r = g / cols, c = g - r * cols;
    store_from_float(out, g, dequant1<E5M2>(in[r * ld_in + c], scales[r]), OUT);
}

template <int IN, int ENC>
int launch_quantize_rowwise(const void *in, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, float *inv_scales, float *amax,
                            hipStream_t s)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2;
    if (rows > kRowMaxRows) return FP8MI_E_UNSUPPORTED;
    const bool vec = aligned_to(in, 16) && aligned_to(out, kPer) && (rows == 1 || ((ld_in * kEsz) % 16 == 0 && ld_out % kPer == 0));
    const RowRung g = vec ? row_rung(cols, kPer, IN == FP8MI_F32, true) : RowRung{0, 0};
#define FP8MI_RW_REG(NV, W) launch_row_reg<W>(quantize_rowwise_reg_kernel<IN, ENC, NV, W>, rows, s, in, rows, cols, ld_in, out, ld_out, inv_scales, amax)
    if (g.w == 1) return g.nv == 2 ? FP8MI_RW_REG(2, 1) : FP8MI_RW_REG(8, 1);
    if (g.w == 4) return FP8MI_RW_REG(8, 4);
    if constexpr (IN == FP8MI_F32)
        if (g.w == 8) return FP8MI_RW_REG(8, 8);
#undef FP8MI_RW_REG
    if (vec) return launch_row_loop(quantize_rowwise_loop_kernel<IN, ENC, true>, rows, s, in, rows, cols, ld_in, out, ld_out, inv_scales, amax);
    return launch_row_loop(quantize_rowwise_loop_kernel<IN, ENC, false>, rows, s, in, rows, cols, ld_in, out, ld_out, inv_scales, amax);
}

template <int OUT, bool E5M2>
int launch_dequant_rowwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const float *scales, void *out, hipStream_t s)
{
    const bool vec = cols % 16 == 0 && aligned_to(in, 16) && aligned_to(out, 16) && (rows == 1 || ld_in % 16 == 0);
    if (vec) return fp8mi_launch_items(dequant_rowwise_kernel<OUT, E5M2>, rows * (cols / 16), 256, 256, s, in, rows, cols / 16, ld_in, scales, out);
    return fp8mi_launch_items(dequant_rowwise_scalar_kernel<OUT, E5M2>, rows * cols, 256, 256, s, in, rows, cols, ld_in, scales, out);
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers (called from fp8mi_api.hip, which has validated the arguments)
// ---------------------------------------------------------------------------
int fp8mi_launch_quantize_rowwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, float *inv_scales,
                                  float *amax, int out_format, int mode, hipStream_t s)
{
    if (rows == 0) return 0;
    // (cols == 0 still launches: every row publishes inv_scale = 1 and amax = 0 and touches no data)
    const int enc = out_format == FP8MI_FMT_E5M2 ? kEncE5M2 : (mode == FP8MI_ENC_REFERENCE ? FP8MI_ENC_REFERENCE : FP8MI_ENC_RNE);
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<kEncE5M2, FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(enc, [&](auto enc_t) {
            return launch_quantize_rowwise<decltype(in_t)::value, decltype(enc_t)::value>(in, rows, cols, ld_in, out, ld_out, inv_scales, amax, s);
        });
    });
}

int fp8mi_launch_dequant_rowwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const float *scales, int in_format, void *out, int out_dtype,
                                 hipStream_t s)
{
    return dispatch_in(out_dtype, [&](auto out_t) {
        return dispatch_int<FP8MI_FMT_E5M2, FP8MI_FMT_E4M3>(in_format, [&](auto fmt_t) {
            return launch_dequant_rowwise<decltype(out_t)::value, decltype(fmt_t)::value == FP8MI_FMT_E5M2>(in, rows, cols, ld_in, scales, out, s);
        });
    });
}
