// Fused activation (+ gate product) + FP8 quantisation for gfx950: the producer of an FP8 GEMM's activation operand in ONE launch - no
// workspace, no atomics, no host sync.  The streaming form of fp8mi_quantize_rowwise (FP8MI_QSCALE_ROW) and of
// fp8mi_quantize_blockwise(block_rows = 1) (FP8MI_QSCALE_GROUP128) applied to
//
//   y[r, c] = act(x[r, c])                              ungated: in is (rows, cols)
//   y[r, c] = act(x[r, c]) * x[r, cols + c]             gated:   in is (rows, 2 cols), [gate | up] as h.chunk(2, -1)
//
// with everything in fp32 on the widened input and y never rounded to the input type:
//   none       y = x  (gated: the one fp32 product gate * up)
//   silu       g sigma(g)
//   gelu_tanh  0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3)))  =  g sigma(2 sqrt(2/pi) (g + 0.044715 g^3))
//   gelu_erf   0.5 g (1 + erf(g / sqrt 2))                      =  0.5 g erfc(-g / sqrt 2)
// The right-hand forms are what is evaluated: they do not cancel in the negative tail, where 1 + tanh and 1 + erf lose every digit.
// sigma(w) = 1 / (1 + 2^-|t|) (times 2^-|t| for w < 0) with t = w log2(e): one v_exp_f32 and one v_rcp_f32.  t is carried as an
// unevaluated sum t + t_lo (the residuals of its products, by FMA) and 2^t_lo is applied as 1 + ln2 t_lo: the exponent's rounding
// error would otherwise be |t| 2^-24 RELATIVE in a result whose row holds nothing but large negative gates - past the 2^-18 the
// scales are held to.  2^-|t| below 2^-126 is flushed by v_exp_f32: |y| below about 1e-36 becomes -0.
//
// This file is how a lane obtains y; what happens to y, and which kernel form a launch takes, is fp8mi_rowquant.h's.
// Register-resident form: 16-byte nontemporal loads of gate and up, one contiguous KiB per wave instruction each.  One scale per row:
// y is HELD in fp32 (8 VGPRs per 16-bit piece) across the reduction, so the activation is evaluated once per element, and the encode
// runs from those registers.  One wave per row (four rows per workgroup), or W waves per row whose maxima meet in LDS behind one barrier.  The
// local recipes (GROUP128; the MX outputs of fp8mi_act_quantize_mx) need neither LDS nor the hold: a group or block is a few adjacent
// lanes of a piece, and every piece is reduced, scaled and stored on its own (local_piece).
// Looping form: one workgroup per row, any length; 16-byte pieces, or single elements at any alignment.  One scale per row reads the
// row twice and evaluates the activation twice; the local recipes are a single pass.

#include "fp8mi_rowquant.h"

#pragma clang fp contract(off)   // the residuals below are differences of a product and its rounded value: nothing may be fused

namespace {

// a double as an unevaluated sum of two floats
constexpr float hi_of(double x) { return (float)x; }
constexpr float lo_of(double x) { return (float)(x - (double)(float)x); }

constexpr double kLog2e = 1.4426950408889634074;
constexpr double kLn2 = 0.69314718055994530942;
constexpr double kGeluA = 2.0 * 0.79788456080286535588 * kLog2e;   // 2 sqrt(2/pi) log2(e)
constexpr double kGeluB = kGeluA * 0.044715;
constexpr double kRsqrt2 = 0.70710678118654752440;

// sigma(w), w = (t + t_lo) ln2
FP8MI_DEVICE float sigmoid_exp2(float t, float t_lo)
{
    const bool pos = t > 0.0f;
    const float a = -fabsf(t), a_lo = pos ? -t_lo : t_lo;
    const float ex = __builtin_amdgcn_exp2f(a);
    const float e = __builtin_fmaf(ex, (float)kLn2 * a_lo, ex);
    const float r = __builtin_amdgcn_rcpf(1.0f + e);   // 1 + e is in [1, 2]
    return pos ? r : e * r;
}

template <int ACT>
FP8MI_DEVICE float act1(float g)
{
    if (ACT == FP8MI_ACT_NONE) return g;
    // the exponent is taken from the gate clamped to +-1e4, where every sigma / erfc below has long saturated: an infinite gate
    // then gives inf * 1 or inf * 0 as the formulas do, not the NaN of inf - inf in a residual
    const float c = __builtin_amdgcn_fmed3f(g, -1.0e4f, 1.0e4f);
    float y;
    if (ACT == FP8MI_ACT_SILU) {
        const float t = c * hi_of(kLog2e);
        float t_lo = __builtin_fmaf(c, hi_of(kLog2e), -t);
        t_lo = __builtin_fmaf(c, lo_of(kLog2e), t_lo);
        y = g * sigmoid_exp2(t, t_lo);
    } else if (ACT == FP8MI_ACT_GELU_TANH) {
        // t = g (A + B g^2) to about 2^-45: g^2, B g^2 and the product with g as (value, residual) pairs
        const float s = c * c, s_lo = __builtin_fmaf(c, c, -s);
        const float q = hi_of(kGeluB) * s;
        float q_lo = __builtin_fmaf(hi_of(kGeluB), s, -q);
        q_lo = __builtin_fmaf(hi_of(kGeluB), s_lo, q_lo);
        q_lo = __builtin_fmaf(lo_of(kGeluB), s, q_lo);
        const float p = q + hi_of(kGeluA);
        // exact while q >= A (|g| > 4.7: where |t| is large and the residual matters); below, off by an ulp of p at most, |t| < 23
        float p_lo = hi_of(kGeluA) - (p - q);
        p_lo = p_lo + (q_lo + lo_of(kGeluA));
        const float t = c * p;
        float t_lo = __builtin_fmaf(c, p, -t);
        t_lo = __builtin_fmaf(c, p_lo, t_lo);
        y = g * sigmoid_exp2(t, t_lo);
    } else {
        // 0.5 g erfc(x), x = -g / sqrt 2 with its residual d; erfc(x + d) = erfc(x) (1 - 2 x d) in the tail x > 0, where
        // d/dx ln erfc(x) -> -2x; for x <= 0 erfc is flat to first order in d
        const float x = c * -hi_of(kRsqrt2);
        float d = __builtin_fmaf(c, -hi_of(kRsqrt2), -x);
        d = __builtin_fmaf(c, -lo_of(kRsqrt2), d);
        const float fac = __builtin_fmaf(-2.0f * fmaxf(x, 0.0f), d, 1.0f);
        y = (0.5f * g) * (erfcf(x) * fac);
    }
    return g != g ? g : y;   // a NaN gate stays the NaN it was
}

template <int ACT, bool GATED>
FP8MI_DEVICE float act_y(float g, float u)
{
    const float a = act1<ACT>(g);
    return GATED ? a * u : a;   // one fp32 multiply
}

template <bool GATED>
FP8MI_DEVICE float act_y_rt(int act, float g, float u)   // the looping forms choose the activation at run time (wave-uniform)
{
    switch (act) {
    case FP8MI_ACT_SILU: return act_y<FP8MI_ACT_SILU, GATED>(g, u);
    case FP8MI_ACT_GELU_TANH: return act_y<FP8MI_ACT_GELU_TANH, GATED>(g, u);
    case FP8MI_ACT_GELU_ERF: return act_y<FP8MI_ACT_GELU_ERF, GATED>(g, u);
    default: return act_y<FP8MI_ACT_NONE, GATED>(g, u);
    }
}

// y of piece v of a row: the 16 bytes of the gate (and of the up value) -> kPer floats
template <int IN, int ACT, bool GATED>
FP8MI_DEVICE void piece_y(const u32x4 &g, const u32x4 &u, float (&y)[8])
{
    float fg[8], fu[8];
    unpack<IN>(g, fg);
    if (GATED) unpack<IN>(u, fu);
#pragma unroll
    for (int k = 0; k < InVec<IN>::kPer; ++k) y[k] = act_y<ACT, GATED>(fg[k], GATED ? fu[k] : 0.0f);
}

template <int IN, bool GATED>
FP8MI_DEVICE void piece_y_rt(int act, const u32x4 &g, const u32x4 &u, float (&y)[8])
{
    float fg[8], fu[8];
    unpack<IN>(g, fg);
    if (GATED) unpack<IN>(u, fu);
#pragma unroll
    for (int k = 0; k < InVec<IN>::kPer; ++k) y[k] = act_y_rt<GATED>(act, fg[k], GATED ? fu[k] : 0.0f);
}

// one element of y, any alignment
template <int IN, bool GATED>
FP8MI_DEVICE float elem_y_rt(int act, const uint8_t *rowp, int64_t cols, int64_t c)
{
    return act_y_rt<GATED>(act, InVec<IN>::load1(rowp, c), GATED ? InVec<IN>::load1(rowp, cols + c) : 0.0f);
}

// Register-resident form.  W waves share a row; wave w of the row owns the pieces 64 (w + W j) + lane, j < NV.  Needs 16-byte aligned
// rows (base and ld_in), a 16-byte aligned up half (cols a multiple of kPer) when gated, kPer-byte aligned output rows and
// cols <= 64 W NV kPer.  Ungated with one scale per row: the last cols % kPer elements go through lanes 0.. of the row's first wave,
// one each; the other modes are launched with cols % kPer == 0 only.
template <int IN, int ACT, bool GATED, int QS, int NV, int W>
__global__ __launch_bounds__(W >= 4 ? 64 * W : 256) void act_quant_reg_kernel(const void *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in,
                                                                               const QuantOut q)
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
    const u32x4 *g4 = (const u32x4 *)rowp, *u4 = (const u32x4 *)(rowp + cols * kEsz);
    uint8_t *orow = q.out + r * q.ld_out;
    const int64_t nv = cols / kPer;
    const u32x4 zero{0u, 0u, 0u, 0u};

    u32x4 rg[NV], ru[GATED ? NV : 1];
    if (!GATED) ru[0] = zero;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * (wr + W * j);
        rg[j] = v < nv ? __builtin_nontemporal_load(g4 + v) : zero;
        if (GATED) ru[j] = v < nv ? __builtin_nontemporal_load(u4 + v) : zero;
    }

    if constexpr (QS >= kQGroup) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * (wr + W * j);
            if (64 * (int64_t)(wr + W * j) >= nv) break;   // wave-uniform: none of this wave's lanes has a piece here
            float y[8];
            piece_y<IN, ACT, GATED>(rg[j], ru[GATED ? j : 0], y);   // a piece past the row is zeros: act(0) = 0, 0 * 0 = 0
            local_piece<QS, kPer>(q, y, lane, v, nv, orow, scale_row<QS>(q, r));
        }
    } else {
        float y[NV][8];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (64 * (int64_t)(wr + W * j) < nv) {
                piece_y<IN, ACT, GATED>(rg[j], ru[GATED ? j : 0], y[j]);
            } else {
#pragma unroll
                for (int k = 0; k < kPer; ++k) y[j][k] = 0.0f;
            }
        }
        const bool has_tail = !GATED && wr == 0 && lane < (int)(cols - nv * kPer);
        const float t = has_tail ? act1<ACT>(InVec<IN>::load1(rowp, nv * kPer + lane)) : 0.0f;

        float m = fabsf(t);
        m = fmaxf(0.0f, m);   // a NaN tail element is ignored like any other
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
            for (int k = 0; k < kPer; ++k) m = fmaxf(m, fabsf(y[j][k]));   // fmaxf drops NaN operands
        }
        m = row_max<W>(m, lds_m, wave, lane);
        const float scale = row_scale<QS>(m, lane, false, nullptr, 0, nullptr, r);
        if (wr == 0 && lane == 0) publish_row<QS>(m, scale_row<QS>(q, r), 0, q.amax, r);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * (wr + W * j);
            if (v < nv) store_piece<QS, kPer>(y[j], scale, orow, v);
        }
        if (has_tail) orow[nv * kPer + lane] = (uint8_t)quant1<QS>(t, scale);
    }
}

// Looping form: one workgroup per row, any length.  VEC: 16-byte pieces (the alignment of the register form), a wave takes 64
// consecutive pieces per step - whole groups and blocks.  Otherwise any alignment: the local recipes take 128 columns per wave and
// step, lane l its columns 2l and 2l + 1 (local_pair); one scale per row takes one element per lane and step.  One scale per row is two
// passes: the second re-reads the row and evaluates the activation again.
template <int IN, bool GATED, int QS, bool VEC>
__global__ __launch_bounds__(kRowLoopBlock) void act_quant_loop_kernel(const void *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in, int act,
                                                                       const QuantOut q)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2, kWaves = kRowLoopBlock / 64;
    __shared__ float lds_m[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = blockIdx.x;
    const uint8_t *rowp = (const uint8_t *)in + r * ld_in * kEsz;
    const u32x4 *g4 = (const u32x4 *)rowp, *u4 = (const u32x4 *)(rowp + cols * kEsz);
    uint8_t *orow = q.out + r * q.ld_out;
    const int64_t nv = VEC ? cols / kPer : 0;
    const u32x4 zero{0u, 0u, 0u, 0u};

    if constexpr (QS >= kQGroup) {
        if (VEC) {
            for (int64_t v0 = 64 * wave; v0 < nv; v0 += kRowLoopBlock) {   // wave-uniform bound: every lane reaches the DPP steps
                const int64_t v = v0 + lane;
                float y[8];
                piece_y_rt<IN, GATED>(act, v < nv ? __builtin_nontemporal_load(g4 + v) : zero, GATED && v < nv ? __builtin_nontemporal_load(u4 + v) : zero, y);
                local_piece<QS, kPer>(q, y, lane, v, nv, orow, scale_row<QS>(q, r));
            }
        } else {
            for (int64_t cb = wave; cb < (cols + 127) / 128; cb += kWaves) {
                const int64_t c0 = cb * 128 + 2 * lane;
                const int n = c0 + 1 < cols ? 2 : (c0 < cols ? 1 : 0);
                const float y0 = n > 0 ? elem_y_rt<IN, GATED>(act, rowp, cols, c0) : 0.0f;
                const float y1 = n > 1 ? elem_y_rt<IN, GATED>(act, rowp, cols, c0 + 1) : 0.0f;
                local_pair<QS>(q, y0, y1, lane, n, c0, orow, scale_row<QS>(q, r));
            }
        }
    } else {
        float m = 0.0f;
        for (int64_t v = threadIdx.x; v < nv; v += kRowLoopBlock) {
            float y[8];
            piece_y_rt<IN, GATED>(act, g4[v], GATED ? u4[v] : zero, y);
#pragma unroll
            for (int k = 0; k < kPer; ++k) m = fmaxf(m, fabsf(y[k]));
        }
        for (int64_t c = nv * kPer + threadIdx.x; c < cols; c += kRowLoopBlock) m = fmaxf(m, fabsf(elem_y_rt<IN, GATED>(act, rowp, cols, c)));
        m = row_max<kWaves>(m, lds_m, wave, lane);
        const float scale = row_scale<QS>(m, lane, false, nullptr, 0, nullptr, r);
        if (threadIdx.x == 0) publish_row<QS>(m, scale_row<QS>(q, r), 0, q.amax, r);

        for (int64_t v = threadIdx.x; v < nv; v += kRowLoopBlock) {
            float y[8];
            piece_y_rt<IN, GATED>(act, __builtin_nontemporal_load(g4 + v), GATED ? __builtin_nontemporal_load(u4 + v) : zero, y);
            store_piece<QS, kPer>(y, scale, orow, v);
        }
        for (int64_t c = nv * kPer + threadIdx.x; c < cols; c += kRowLoopBlock)
            orow[c] = (uint8_t)quant1<QS>(elem_y_rt<IN, GATED>(act, rowp, cols, c), scale);
    }
}

struct AqArgs {
    const void *in;
    int64_t rows, cols, ld_in;
    int act;
    QuantOut q;
    hipStream_t s;
};

template <int IN, int ACT, bool GATED, int QS>
int launch_act_quant(const AqArgs &a)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2;
    constexpr bool kWhole = GATED || QS >= kQGroup;   // these forms take whole pieces only
    constexpr int kOutAl = QS == kQMx4 ? kPer / 2 : kPer;   // bytes a lane stores per piece
    if (a.rows > kRowMaxRows) return FP8MI_E_UNSUPPORTED;
    const bool vec = aligned_to(a.in, 16) && aligned_to(a.q.out, kOutAl) && (a.rows == 1 || ((a.ld_in * kEsz) % 16 == 0 && a.q.ld_out % kOutAl == 0)) &&
                     (!kWhole || a.cols % kPer == 0);
    const int w = vec ? row_rung(a.cols, kPer, IN == FP8MI_F32).w : 0;
#define FP8MI_AQ_REG(W) launch_row_reg<W>(act_quant_reg_kernel<IN, ACT, GATED, QS, 8, W>, a.rows, a.s, a.in, a.rows, a.cols, a.ld_in, a.q)
    if (w == 1) return FP8MI_AQ_REG(1);
    if (w == 4) return FP8MI_AQ_REG(4);
    if constexpr (IN == FP8MI_F32)
        if (w == 8) return FP8MI_AQ_REG(8);
#undef FP8MI_AQ_REG
    if (vec) return launch_row_loop(act_quant_loop_kernel<IN, GATED, QS, true>, a.rows, a.s, a.in, a.rows, a.cols, a.ld_in, a.act, a.q);
    return launch_row_loop(act_quant_loop_kernel<IN, GATED, QS, false>, a.rows, a.s, a.in, a.rows, a.cols, a.ld_in, a.act, a.q);
}

int launch_act_quant_any(const AqArgs &a, int in_dtype, bool gated, int qs)
{
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<1, 0>(gated, [&](auto gated_t) {
            return dispatch_int<FP8MI_ACT_SILU, FP8MI_ACT_GELU_TANH, FP8MI_ACT_GELU_ERF, FP8MI_ACT_NONE>(a.act, [&](auto act_t) {
                return dispatch_qs(qs, [&](auto qs_t) {
                    return launch_act_quant<decltype(in_t)::value, decltype(act_t)::value, decltype(gated_t)::value != 0, decltype(qs_t)::value>(a);
                });
            });
        });
    });
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers (called from fp8mi_api.hip, which has validated the arguments; `act` without FP8MI_ACT_GATED)
// ---------------------------------------------------------------------------
int fp8mi_launch_act_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, int gated, uint8_t *out, int64_t ld_out,
                              float *scales, int64_t s_stride_row, int64_t s_stride_k, float *amax, int scale_mode, int out_format, int mode, hipStream_t s)
{
    if (rows == 0) return 0;
    if (scale_mode == FP8MI_QSCALE_GROUP128 && cols == 0) return 0;
    // (FP8MI_QSCALE_ROW with cols == 0 still launches: every row publishes inv_scale = 1 and amax = 0 and touches no data)
    const int qs = scale_mode == FP8MI_QSCALE_GROUP128 ? kQGroup : (out_format == FP8MI_FMT_E5M2 ? kEncE5M2 : mode);
    return launch_act_quant_any({in, rows, cols, ld_in, act, {out, ld_out, scales, s_stride_row, s_stride_k, 0, amax}, s}, in_dtype, gated != 0, qs);
}

int fp8mi_launch_act_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, int gated, uint8_t *out, int64_t ld_out,
                                 uint8_t *scales, int64_t ld_s, int mx_format, hipStream_t s)
{
    if (rows == 0 || cols == 0) return 0;
    const int qs = mx_format == FP8MI_MX_FP4 ? kQMx4 : kQMx8;
    return launch_act_quant_any({in, rows, cols, ld_in, act, {out, ld_out, scales, ld_s, 0, mx_scale_flags(scales, rows, cols, ld_s), nullptr}, s}, in_dtype,
                                gated != 0, qs);
}
