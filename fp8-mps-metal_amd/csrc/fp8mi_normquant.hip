// Fused RMSNorm / LayerNorm (+ residual add, affine parameters, adaLN modulation) + FP8 quantisation for gfx950: the producer of the
// FIRST GEMM's activation operand of a transformer block in ONE launch - no workspace, no atomics, no host sync.  The contract is the
// formula of include/fp8mi.h (fp8mi_norm_quantize): every operation below is one individually rounded fp32 operation, nothing is
// fused, and y is handed to the quantising tail of fp8mi_rowquant.h, shared with fp8mi_act_quantize: one scale per row (row_max,
// row_scale, publish_row), or a local recipe - GROUP128, or for fp8mi_norm_quantize_mx MXFP8 / MXFP4 - in a single quantising pass
// (local_piece / local_pair).  This file is how a lane obtains y; which kernel form a launch takes is that header's ladder.
//
//   h = x                          or, with a residual, h = in_dtype(x + res), stored to h_out and widened again
//   RMS:    d = h,        rstd = 1 / sqrt(sum d^2 / cols + eps)
//   LAYER:  d = h - mean, rstd the same;  mean = sum h / cols          (two passes: never E[h^2] - mean^2)
//   y = ((d * rstd) [* w] [+ b]) [* (1 + sc) + sh]
//
// The sums: every lane adds its own elements in order, the 64 lanes of a wave meet in wave_sum's tree (DPP inside a row of 16 lanes,
// then the four rows), the waves of a row in LDS behind one barrier, added in wave order by every wave alike - so all of them hold the
// SAME mean and rstd, the values written to mean_out / rstd_out.
//
// Register-resident form: 16-byte nontemporal loads of x (and of the residual), h HELD in fp32
// across both statistics passes (8 VGPRs per 16-bit piece), overwritten by d and then by y; the amax reduction and the encode run from
// those registers.  One wave per row (four rows per workgroup), or W waves per row.  The parameter vectors and modulation rows are shared by many
// rows and sit in L2: plain cached loads, 16 bytes (32 for fp32 parameters of 16-bit input) per piece.
// Looping form: one workgroup per row, any length.  VEC: 16-byte pieces (the alignment of the register form); otherwise a wave takes
// 128 columns per step, lane l its columns 2l and 2l + 1, at any alignment.  The row is read once per pass: sum, (LAYER) sum of
// squares, (ROW) amax, encode.  With a residual the first pass stores h and the later ones read it back from h_out - every lane the
// elements it wrote itself, so no fence is needed and h_out may be the residual's own buffer.
//
// weight / bias / modulation / residual and the parameters' type are wave-uniform run-time flags, not template arguments.

#include "fp8mi_rowquant.h"

#pragma clang fp contract(off)   // the contract is one rounding per operation: no multiply may be fused into the add that follows it

namespace {

constexpr int kNqNV = 8;   // 16-byte pieces per lane of the register-resident form

template <int IN>
FP8MI_DEVICE float round_in(float v)   // round to nearest even to the input type, widened again
{
    if (IN == FP8MI_F16) return (float)(_Float16)v;
    if (IN == FP8MI_BF16) return (float)(__bf16)v;
    return v;
}

template <int IN>
FP8MI_DEVICE uint32_t bits16(float h)   // the 16 bits of a value round_in<IN> returned
{
    if (IN == FP8MI_F16) return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)h);
    return __float_as_uint(h) >> 16;
}

template <int IN>
FP8MI_DEVICE u32x4 pack(const float (&h)[8])   // values round_in<IN> returned -> the 16-byte piece
{
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (IN == FP8MI_F32)
            o[q] = __float_as_uint(h[q]);
        else
            o[q] = bits16<IN>(h[2 * q]) | (bits16<IN>(h[2 * q + 1]) << 16);
    }
    return o;
}

// kPer parameters from column c on (16-byte aligned): of the input's type, or fp32
template <int IN>
FP8MI_DEVICE void load_params(const void *p, int64_t c, bool f32, float (&f)[8])
{
    if (IN == FP8MI_F32 || f32) {
        const u32x4 *q = (const u32x4 *)((const float *)p + c);
        const u32x4 lo = q[0];
        f[0] = __uint_as_float(lo[0]); f[1] = __uint_as_float(lo[1]); f[2] = __uint_as_float(lo[2]); f[3] = __uint_as_float(lo[3]);
        if (InVec<IN>::kPer == 8) {
            const u32x4 hi = q[1];
            f[4] = __uint_as_float(hi[0]); f[5] = __uint_as_float(hi[1]); f[6] = __uint_as_float(hi[2]); f[7] = __uint_as_float(hi[3]);
        }
    } else {
        unpack<IN>(*(const u32x4 *)((const uint16_t *)p + c), f);
    }
}

// the element's value from d: the third step of the contract, one rounding per operation
FP8MI_DEVICE float norm_value(float d, float rstd, bool hw, float w, bool hb, float b, bool hm, float sc, float sh)
{
    float z = d * rstd;
    if (hw) z = z * w;
    if (hb) z = z + b;
    if (hm) {
        const float t = 1.0f + sc;
        z = z * t;
        z = z + sh;
    }
    return z;
}

// y of the kPer elements from column c on (row r's modulation row is g); d -> y in place
template <int IN>
FP8MI_DEVICE void piece_norm(const NqArgs &a, int64_t g, int64_t c, float rstd, float (&d)[8])
{
    constexpr int kPer = InVec<IN>::kPer;
    const bool f32 = a.param_dtype == FP8MI_F32, hw = a.weight != nullptr, hb = a.bias != nullptr, hm = a.mod_scale != nullptr;
    float w[8], b[8], sc[8], sh[8];
    if (hw) load_params<IN>(a.weight, c, f32, w);
    if (hb) load_params<IN>(a.bias, c, f32, b);
    if (hm) {
        load_params<IN>(a.mod_scale, g * a.ld_mod + c, f32, sc);
        load_params<IN>(a.mod_shift, g * a.ld_mod + c, f32, sh);
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) d[k] = norm_value(d[k], rstd, hw, hw ? w[k] : 0.0f, hb, hb ? b[k] : 0.0f, hm, hm ? sc[k] : 0.0f, hm ? sh[k] : 0.0f);
}

FP8MI_DEVICE float elem_norm(const NqArgs &a, int64_t g, int64_t c, float rstd, float d)   // one element, any alignment
{
    const bool hw = a.weight != nullptr, hb = a.bias != nullptr, hm = a.mod_scale != nullptr;
    const float w = hw ? load_as_float(a.weight, c, a.param_dtype) : 0.0f, b = hb ? load_as_float(a.bias, c, a.param_dtype) : 0.0f;
    const float sc = hm ? load_as_float(a.mod_scale, g * a.ld_mod + c, a.param_dtype) : 0.0f;
    const float sh = hm ? load_as_float(a.mod_shift, g * a.ld_mod + c, a.param_dtype) : 0.0f;
    return norm_value(d, rstd, hw, w, hb, b, hm, sc, sh);
}

FP8MI_DEVICE float rstd_of(float sumsq, int64_t cols, float eps)
{
    const float v = sumsq / (float)cols + eps;
    return 1.0f / sqrtf(v);
}

// Register-resident form.  W waves share a row; wave w of the row owns the pieces 64 (w + W j) + lane, j < kNqNV.  Needs 16-byte aligned
// rows of x, the residual, h_out and the parameters, kPer-byte aligned output rows, cols a multiple of kPer and cols <= 64 W kNqNV kPer.
template <int IN, int NORM, int QS, int W>
__global__ __launch_bounds__(W >= 4 ? 64 * W : 256) void norm_quant_reg_kernel(const NqArgs a)
{
    static_assert(W == 1 || W >= 4, "one wave per row (four rows per workgroup) or one row per workgroup");
    constexpr int kPer = InVec<IN>::kPer, NV = kNqNV;
    constexpr int kEsz = IN == FP8MI_F32 ? 4 : 2;
    __shared__ float lds_a[W], lds_b[W], lds_m[W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = W == 1 ? 0 : wave;
    const int64_t r = W == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
    if (r >= a.rows) return;   // wave-uniform, and only where a wave is a row (W == 1: no barrier below)
    const u32x4 *x4 = (const u32x4 *)((const uint8_t *)a.in + r * a.ld_in * kEsz);
    const u32x4 *r4 = (const u32x4 *)((const uint8_t *)a.residual + r * a.ld_res * kEsz);
    u32x4 *h4 = (u32x4 *)((uint8_t *)a.h_out + r * a.ld_h * kEsz);
    uint8_t *orow = a.q.out + r * a.q.ld_out;
    const int64_t nv = a.cols / kPer;
    const bool has_res = a.residual != nullptr;
    const u32x4 zero{0u, 0u, 0u, 0u};

    // 1. h
    float h[NV][8];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * (wr + W * j);
        unpack<IN>(v < nv ? __builtin_nontemporal_load(x4 + v) : zero, h[j]);
        if (has_res) {
            float f[8];
            unpack<IN>(v < nv ? __builtin_nontemporal_load(r4 + v) : zero, f);
#pragma unroll
            for (int k = 0; k < kPer; ++k) h[j][k] = round_in<IN>(h[j][k] + f[k]);
            if (v < nv) h4[v] = pack<IN>(h[j]);
        }
    }

    // 2. the row's statistics; h becomes d
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int k = 0; k < kPer; ++k) s = s + (NORM == FP8MI_NORM_LAYER ? h[j][k] : h[j][k] * h[j][k]);   // a piece past the row is zeros
    }
    s = row_sum<W>(s, lds_a, wave, lane);
    float mean = 0.0f;
    if (NORM == FP8MI_NORM_LAYER) {
        mean = s / (float)a.cols;
        s = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool in_row = lane + 64 * (int64_t)(wr + W * j) < nv;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                h[j][k] = in_row ? h[j][k] - mean : 0.0f;
                s = s + h[j][k] * h[j][k];
            }
        }
        s = row_sum<W>(s, lds_b, wave, lane);
    }
    const float rstd = rstd_of(s, a.cols, a.eps);
    if (wr == 0 && lane == 0 && a.cols > 0) {
        if (NORM == FP8MI_NORM_LAYER && a.mean_out) a.mean_out[r] = mean;
        if (a.rstd_out) a.rstd_out[r] = rstd;
    }

    // 3. y, in place; 4. the quantising tail on it
    const int64_t g = a.mod_scale ? r / a.rows_per_mod : 0;
    if constexpr (QS >= kQGroup) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * (wr + W * j);
            if (64 * (int64_t)(wr + W * j) >= nv) break;   // wave-uniform: none of this wave's lanes has a piece here
            if (v < nv) piece_norm<IN>(a, g, v * kPer, rstd, h[j]);   // (a piece past the row stays zeros)
            local_piece<QS, kPer>(a.q, h[j], lane, v, nv, orow, scale_row<QS>(a.q, r));
        }
    } else {
        float m = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * (wr + W * j);
            if (v < nv) piece_norm<IN>(a, g, v * kPer, rstd, h[j]);
#pragma unroll
            for (int k = 0; k < kPer; ++k) m = fmaxf(m, fabsf(h[j][k]));   // fmaxf drops NaN operands
        }
        m = row_max<W>(m, lds_m, wave, lane);
        const float scale = row_scale<QS>(m, lane, false, nullptr, 0, nullptr, r);
        if (wr == 0 && lane == 0) publish_row<QS>(m, scale_row<QS>(a.q, r), 0, a.q.amax, r);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * (wr + W * j);
            if (v < nv) store_piece<QS, kPer>(h[j], scale, orow, v);
        }
    }
}

// What one lane handles in one step of the looping form.  VEC: the kPer elements of piece 64 (wave + 4 i) + lane; otherwise the
// columns 2 lane and 2 lane + 1 of group wave + 4 i (the layout of quantize_blockwise_kernel).  The same in every pass.
template <int IN, bool VEC>
struct Span {
    static constexpr int kN = VEC ? InVec<IN>::kPer : 2;
    static constexpr int kEsz = IN == FP8MI_F32 ? 4 : 2;

    // h of the n (0 .. kN; VEC: 0 or kN) elements from column c on; the rest zeros.  FIRST: the pass that forms and stores h
    template <bool FIRST>
    static FP8MI_DEVICE void load_h(const NqArgs &a, int64_t r, int64_t c, int n, float (&h)[8])
    {
        const uint8_t *xrow = (const uint8_t *)a.in + r * a.ld_in * kEsz;
        const uint8_t *rrow = (const uint8_t *)a.residual + r * a.ld_res * kEsz;
        uint8_t *hrow = (uint8_t *)a.h_out + r * a.ld_h * kEsz;
        const bool has_res = a.residual != nullptr;
#pragma unroll
        for (int k = 0; k < kN; ++k) h[k] = 0.0f;
        if (n == 0) return;
        if (VEC) {
            if (has_res && !FIRST) {
                unpack<IN>(*(const u32x4 *)(hrow + c * kEsz), h);
                return;
            }
            unpack<IN>(__builtin_nontemporal_load((const u32x4 *)(xrow + c * kEsz)), h);
            if (has_res) {
                float f[8];
                unpack<IN>(__builtin_nontemporal_load((const u32x4 *)(rrow + c * kEsz)), f);
#pragma unroll
                for (int k = 0; k < kN; ++k) h[k] = round_in<IN>(h[k] + f[k]);
                *(u32x4 *)(hrow + c * kEsz) = pack<IN>(h);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kN; ++k) {
                if (k >= n) break;
                if (has_res && !FIRST) {
                    h[k] = InVec<IN>::load1(hrow, c + k);
                    continue;
                }
                h[k] = InVec<IN>::load1(xrow, c + k);
                if (has_res) {
                    h[k] = round_in<IN>(h[k] + InVec<IN>::load1(rrow, c + k));
                    if (IN == FP8MI_F32)
                        ((float *)hrow)[c + k] = h[k];
                    else
                        ((uint16_t *)hrow)[c + k] = (uint16_t)bits16<IN>(h[k]);
                }
            }
        }
    }

    // h -> y in place (n elements; the rest stay zeros)
    template <int NORM>
    static FP8MI_DEVICE void to_y(const NqArgs &a, int64_t g, int64_t c, int n, float mean, float rstd, float (&h)[8])
    {
        if (n == 0) return;
        if (VEC) {
            if (NORM == FP8MI_NORM_LAYER) {
#pragma unroll
                for (int k = 0; k < kN; ++k) h[k] = h[k] - mean;
            }
            piece_norm<IN>(a, g, c, rstd, h);
        } else {
#pragma unroll
            for (int k = 0; k < kN; ++k) {
                if (k >= n) break;
                h[k] = elem_norm(a, g, c + k, rstd, NORM == FP8MI_NORM_LAYER ? h[k] - mean : h[k]);
            }
        }
    }
};

// Looping form: one workgroup per row, any length (see the head of the file).
template <int IN, int NORM, int QS, bool VEC>
__global__ __launch_bounds__(kRowLoopBlock) void norm_quant_loop_kernel(const NqArgs a)
{
    using S = Span<IN, VEC>;
    constexpr int kN = S::kN, kWaves = kRowLoopBlock / 64;
    constexpr int kStep = VEC ? kN * 64 : 128;   // columns a wave takes per step
    __shared__ float lds_a[kWaves], lds_b[kWaves], lds_m[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = blockIdx.x, cols = a.cols;
    uint8_t *orow = a.q.out + r * a.q.ld_out;
    // this lane's span in the step that starts at column c0 (wave-uniform): its first column and how many of its elements are in the row
#define FP8MI_NQ_SPAN(c0)                                  \
    const int64_t c = (c0) + (int64_t)lane * kN;          \
    const int n = VEC ? (c < cols ? kN : 0) : (int)(c + 1 < cols ? 2 : (c < cols ? 1 : 0))

    // the sums (with a residual: h is formed and stored here)
    float s = 0.0f;
    for (int64_t c0 = (int64_t)wave * kStep; c0 < cols; c0 += (int64_t)kWaves * kStep) {
        FP8MI_NQ_SPAN(c0);
        float h[8];
        S::template load_h<true>(a, r, c, n, h);
#pragma unroll
        for (int k = 0; k < kN; ++k) s = s + (NORM == FP8MI_NORM_LAYER ? h[k] : h[k] * h[k]);
    }
    s = row_sum<kWaves>(s, lds_a, wave, lane);
    float mean = 0.0f;
    if (NORM == FP8MI_NORM_LAYER) {
        mean = s / (float)cols;
        s = 0.0f;
        for (int64_t c0 = (int64_t)wave * kStep; c0 < cols; c0 += (int64_t)kWaves * kStep) {
            FP8MI_NQ_SPAN(c0);
            float h[8];
            S::template load_h<false>(a, r, c, n, h);
#pragma unroll
            for (int k = 0; k < kN; ++k) {
                const float d = k < n ? h[k] - mean : 0.0f;
                s = s + d * d;
            }
        }
        s = row_sum<kWaves>(s, lds_b, wave, lane);
    }
    const float rstd = rstd_of(s, cols, a.eps);
    if (threadIdx.x == 0 && cols > 0) {
        if (NORM == FP8MI_NORM_LAYER && a.mean_out) a.mean_out[r] = mean;
        if (a.rstd_out) a.rstd_out[r] = rstd;
    }
    const int64_t g = a.mod_scale ? r / a.rows_per_mod : 0;

    if constexpr (QS >= kQGroup) {   // a single pass: every step holds whole groups and blocks
        for (int64_t c0 = (int64_t)wave * kStep; c0 < cols; c0 += (int64_t)kWaves * kStep) {
            FP8MI_NQ_SPAN(c0);
            float y[8];
            S::template load_h<false>(a, r, c, n, y);
            S::template to_y<NORM>(a, g, c, n, mean, rstd, y);
            if constexpr (VEC)
                local_piece<QS, kN>(a.q, y, lane, c / kN, cols / kN, orow, scale_row<QS>(a.q, r));
            else
                local_pair<QS>(a.q, y[0], y[1], lane, n, c, orow, scale_row<QS>(a.q, r));
        }
    } else {
        float m = 0.0f;
        for (int64_t c0 = (int64_t)wave * kStep; c0 < cols; c0 += (int64_t)kWaves * kStep) {
            FP8MI_NQ_SPAN(c0);
            float y[8];
            S::template load_h<false>(a, r, c, n, y);
            S::template to_y<NORM>(a, g, c, n, mean, rstd, y);
#pragma unroll
            for (int k = 0; k < kN; ++k) m = fmaxf(m, fabsf(y[k]));   // fmaxf drops NaN operands
        }
        m = row_max<kWaves>(m, lds_m, wave, lane);
        const float scale = row_scale<QS>(m, lane, false, nullptr, 0, nullptr, r);
        if (threadIdx.x == 0) publish_row<QS>(m, scale_row<QS>(a.q, r), 0, a.q.amax, r);
        for (int64_t c0 = (int64_t)wave * kStep; c0 < cols; c0 += (int64_t)kWaves * kStep) {
            FP8MI_NQ_SPAN(c0);
            float y[8];
            S::template load_h<false>(a, r, c, n, y);
            S::template to_y<NORM>(a, g, c, n, mean, rstd, y);
            if (VEC) {
                if (n) store_piece<QS, kN>(y, scale, orow, c / kN);
            } else {
                if (n > 0) orow[c] = (uint8_t)quant1<QS>(y[0], scale);
                if (n > 1) orow[c + 1] = (uint8_t)quant1<QS>(y[1], scale);
            }
        }
    }
#undef FP8MI_NQ_SPAN
}

template <int IN, int NORM, int QS>
int launch_norm_quant(const NqArgs &a, hipStream_t s)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2;
    constexpr int kOutAl = QS == kQMx4 ? kPer / 2 : kPer;   // bytes a lane stores per piece
    if (a.rows > kRowMaxRows) return FP8MI_E_UNSUPPORTED;
    const int64_t psz = a.param_dtype == FP8MI_F32 ? 4 : 2;
    const bool one = a.rows == 1, one_mod = a.rows <= a.rows_per_mod;
    bool vec = aligned_to(a.in, 16) && aligned_to(a.q.out, kOutAl) && (one || ((a.ld_in * kEsz) % 16 == 0 && a.q.ld_out % kOutAl == 0)) &&
               a.cols % kPer == 0;
    if (a.residual)
        vec = vec && aligned_to(a.residual, 16) && aligned_to(a.h_out, 16) && (one || ((a.ld_res * kEsz) % 16 == 0 && (a.ld_h * kEsz) % 16 == 0));
    vec = vec && aligned_to(a.weight, 16) && aligned_to(a.bias, 16);
    if (a.mod_scale) vec = vec && aligned_to(a.mod_scale, 16) && aligned_to(a.mod_shift, 16) && (one_mod || (a.ld_mod * psz) % 16 == 0);
    const int w = vec ? row_rung(a.cols, kPer, IN == FP8MI_F32).w : 0;
    static_assert(kNqNV == 8, "row_rung's thresholds are for 8 pieces per lane");
    if (w == 1) return launch_row_reg<1>(norm_quant_reg_kernel<IN, NORM, QS, 1>, a.rows, s, a);
    if (w == 4) return launch_row_reg<4>(norm_quant_reg_kernel<IN, NORM, QS, 4>, a.rows, s, a);
    if constexpr (IN == FP8MI_F32)
        if (w == 8) return launch_row_reg<8>(norm_quant_reg_kernel<IN, NORM, QS, 8>, a.rows, s, a);
    if (vec) return launch_row_loop(norm_quant_loop_kernel<IN, NORM, QS, true>, a.rows, s, a);
    return launch_row_loop(norm_quant_loop_kernel<IN, NORM, QS, false>, a.rows, s, a);
}

int launch_norm_quant_any(const NqArgs &a, int in_dtype, int norm, int qs, hipStream_t s)
{
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_NORM_LAYER, FP8MI_NORM_RMS>(norm, [&](auto norm_t) {
            return dispatch_qs(qs, [&](auto qs_t) { return launch_norm_quant<decltype(in_t)::value, decltype(norm_t)::value, decltype(qs_t)::value>(a, s); });
        });
    });
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers (called from fp8mi_api.hip, which has validated the arguments)
// ---------------------------------------------------------------------------
int fp8mi_launch_norm_quantize(const NqArgs &a, int in_dtype, int norm, int scale_mode, int out_format, int mode, hipStream_t s)
{
    if (a.rows == 0) return 0;
    if (scale_mode == FP8MI_QSCALE_GROUP128 && a.cols == 0) return 0;
    // (FP8MI_QSCALE_ROW with cols == 0 still launches: every row publishes inv_scale = 1 and amax = 0 and touches nothing else)
    const int qs = scale_mode == FP8MI_QSCALE_GROUP128 ? kQGroup : (out_format == FP8MI_FMT_E5M2 ? kEncE5M2 : mode);
    return launch_norm_quant_any(a, in_dtype, norm, qs, s);
}

int fp8mi_launch_norm_quantize_mx(const NqArgs &a, int in_dtype, int norm, int mx_format, hipStream_t s)
{
    if (a.rows == 0 || a.cols == 0) return 0;
    NqArgs b = a;
    b.q.mx_flags = mx_scale_flags(a.q.scales, a.rows, a.cols, a.q.s_sr);
    return launch_norm_quant_any(b, in_dtype, norm, mx_format == FP8MI_MX_FP4 ? kQMx4 : kQMx8, s);
}
