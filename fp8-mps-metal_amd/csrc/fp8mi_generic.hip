// Shape- and alignment-agnostic FP8 scaled matmul: one wave64 per output
// element, byte loads, exact byte-wise reference decode (fp8_matmul.metal:19-40).
// It exists so that EVERY problem the reference accepts (any K, any leading
// dimension, unaligned views - fp8_mps_native.py:55-60 only asks for
// contiguity) has a device path; the tuned kernels take over whenever their
// alignment preconditions hold.  Same epilogue as the other kernels.

#include "fp8mi_common.h"

namespace {

constexpr int kWavesPerBlock = 4;

// fmt = a_format + 2 * b_format (0 = e4m3 x e4m3); a separate argument: MMParams is the kernarg of every tensorwise kernel.  An e5m2
// byte decodes exactly (the high byte of an IEEE half); every e5m2 / e4m3 product is exact in fp32 or overflows to the inf IEEE gives.
__global__ __launch_bounds__(kWavesPerBlock * 64) void generic_kernel(MMParams p, int fmt)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t m = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (n >= p.N || m >= p.M) return;  // wave-uniform
    const uint8_t *a = p.A + m * p.lda;
    const uint8_t *b = p.B + n * p.ldb;
    float s = 0.0f;
    if (fmt != 0) {   // OCP semantics only (the API rejects FP8MI_NAN_ZERO with an e5m2 operand)
        const int ea = fmt & 1, eb = (fmt >> 1) & 1;
        for (int64_t k = lane; k < p.K; k += 64) s += decode_fmt(a[k], ea) * decode_fmt(b[k], eb);
    } else if (p.nan_zero) {
        for (int64_t k = lane; k < p.K; k += 64) s += decode_ref(a[k]) * decode_ref(b[k]);
    } else {
        for (int64_t k = lane; k < p.K; k += 64) {
            // OCP semantics: let the hardware convert produce NaN for 0x7F / 0xFF
            float fa = __builtin_amdgcn_cvt_f32_fp8((int)a[k], 0);
            float fb = __builtin_amdgcn_cvt_f32_fp8((int)b[k], 0);
            s += fa * fb;
        }
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float sa = p.sa_row ? p.scale_a[m] : p.scale_a[0];
        const float sb = p.sb_row ? p.scale_b[n] : p.scale_b[0];
        const float bias = p.bias ? load_as_float(p.bias, p.transposed ? m : n, p.bias_dtype) : 0.0f;
        const float sr = p.scale_result ? p.scale_result[0] : 1.0f;
        store_from_float(p.C, m * p.ldc + n,
                         epilogue_value(s, sa, sb, p.bias != nullptr, bias, p.scale_result != nullptr, sr, p.transposed != 0), p.out_dtype);
    }
}

}  // namespace

int fp8mi_launch_generic(const MMParams &p, hipStream_t s, int fmt)
{
    const int64_t gx = (p.N + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t gy = p.M < 65535 ? p.M : 65535;
    const int64_t gz = (p.M + 65534) / 65535;
    if (gx > 0x7FFFFFFF || gz > 65535) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch(generic_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kWavesPerBlock * 64), s, p, fmt);
}

// ---- block-scaled (MXFP8) form -------------------------------------------------------------------------------------
// The same one-wave-per-output structure, every product taken exactly and scaled by 2^(sa - 127) 2^(sb - 127) of its 32-K block
// (ldexp: one rounding, subnormal results included), summed in IEEE fp32.  A scale byte 0xFF (E8M0 NaN) makes its block NaN.
// The any-alignment fallback of fp8mi_scaled_mm_mxfp8, and its exact reference in the tests.
namespace {

__global__ __launch_bounds__(kWavesPerBlock * 64) void generic_mxfp8_kernel(MMParams p, MxScales sc)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t m = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (n >= p.N || m >= p.M) return;  // wave-uniform
    const uint8_t *a = p.A + m * p.lda;
    const uint8_t *b = p.B + n * p.ldb;
    const uint8_t *sa = sc.sx + m * sc.ld_sx;
    const uint8_t *sb = sc.sw + n * sc.ld_sw;
    float s = 0.0f;
    for (int64_t k = lane; k < p.K; k += 64) {
        const float fa = p.nan_zero ? decode_ref(a[k]) : __builtin_amdgcn_cvt_f32_fp8((int)a[k], 0);
        const float fb = p.nan_zero ? decode_ref(b[k]) : __builtin_amdgcn_cvt_f32_fp8((int)b[k], 0);
        const int ea = sa[k >> 5], eb = sb[k >> 5];
        const float t = (ea == 0xFF || eb == 0xFF) ? __uint_as_float(0x7FC00000u) : __builtin_ldexpf(fa * fb, ea + eb - 254);
        s += t;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float bias = p.bias ? load_as_float(p.bias, p.transposed ? m : n, p.bias_dtype) : 0.0f;
        const float sr = p.scale_result ? p.scale_result[0] : 1.0f;
        store_from_float(p.C, m * p.ldc + n, epilogue_value(s, 1.0f, 1.0f, p.bias != nullptr, bias, p.scale_result != nullptr, sr, p.transposed != 0),
                         p.out_dtype);
    }
}

}  // namespace

int fp8mi_launch_generic_mxfp8(const MMParams &p, const MxScales &sc, hipStream_t s)
{
    const int64_t gx = (p.N + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t gy = p.M < 65535 ? p.M : 65535;
    const int64_t gz = (p.M + 65534) / 65535;
    if (gx > 0x7FFFFFFF || gz > 65535) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch(generic_mxfp8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kWavesPerBlock * 64), s, p, sc);
}

// ---- MXFP4 form ----------------------------------------------------------------------------------------------------
// generic_mxfp8_kernel with e2m1 operands: p.K counts elements (two per byte, the even k in the low nibble), p.lda / p.ldb bytes.
// Every product is exact in fp32, scaled by 2^(sa - 127) 2^(sb - 127) with one rounding and summed in IEEE fp32; a scale
// byte 0xFF makes its block NaN.  e2m1 has no NaN: nan_zero does not apply.
namespace {

__global__ __launch_bounds__(kWavesPerBlock * 64) void generic_mxfp4_kernel(MMParams p, MxScales sc)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t m = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (n >= p.N || m >= p.M) return;  // wave-uniform
    const uint8_t *a = p.A + m * p.lda;
    const uint8_t *b = p.B + n * p.ldb;
    const uint8_t *sa = sc.sx + m * sc.ld_sx;
    const uint8_t *sb = sc.sw + n * sc.ld_sw;
    float s = 0.0f;
    for (int64_t k = lane; k < p.K; k += 64) {
        const int sh = 4 * (int)(k & 1);
        const float fa = e2m1_value((uint32_t)a[k >> 1] >> sh);
        const float fb = e2m1_value((uint32_t)b[k >> 1] >> sh);
        const int ea = sa[k >> 5], eb = sb[k >> 5];
        const float t = (ea == 0xFF || eb == 0xFF) ? __uint_as_float(0x7FC00000u) : __builtin_ldexpf(fa * fb, ea + eb - 254);
        s += t;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float bias = p.bias ? load_as_float(p.bias, p.transposed ? m : n, p.bias_dtype) : 0.0f;
        const float sr = p.scale_result ? p.scale_result[0] : 1.0f;
        store_from_float(p.C, m * p.ldc + n, epilogue_value(s, 1.0f, 1.0f, p.bias != nullptr, bias, p.scale_result != nullptr, sr, p.transposed != 0),
                         p.out_dtype);
    }
}

}  // namespace

int fp8mi_launch_generic_mxfp4(const MMParams &p, const MxScales &sc, hipStream_t s)
{
    const int64_t gx = (p.N + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t gy = p.M < 65535 ? p.M : 65535;
    const int64_t gz = (p.M + 65534) / 65535;
    if (gx > 0x7FFFFFFF || gz > 65535) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch(generic_mxfp4_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kWavesPerBlock * 64), s, p, sc);
}

// ---- MXW4A8 form ---------------------------------------------------------------------------------------------------
// e4m3 A bytes against e2m1 B_nk codes (two per byte, the even k in the low nibble): p.K counts elements, p.lda / p.ldb bytes.  Every
// product is exact in fp32 (a multiple of 2^-10 below 2^12), scaled by 2^(sa - 127) 2^(sb - 127) with one rounding and summed in IEEE
// fp32; a scale byte 0xFF makes its block NaN.  Only A has NaN encodings: nan_zero reads its bytes 0x7F / 0xFF as zero.
namespace {

__global__ __launch_bounds__(kWavesPerBlock * 64) void generic_mxw4a8_kernel(MMParams p, MxScales sc)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t m = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (n >= p.N || m >= p.M) return;  // wave-uniform
    const uint8_t *a = p.A + m * p.lda;
    const uint8_t *b = p.B + n * p.ldb;
    const uint8_t *sa = sc.sx + m * sc.ld_sx;
    const uint8_t *sb = sc.sw + n * sc.ld_sw;
    float s = 0.0f;
    for (int64_t k = lane; k < p.K; k += 64) {
        const float fa = p.nan_zero ? decode_ref(a[k]) : __builtin_amdgcn_cvt_f32_fp8((int)a[k], 0);
        const float fb = e2m1_value((uint32_t)b[k >> 1] >> (4 * (int)(k & 1)));
        const int ea = sa[k >> 5], eb = sb[k >> 5];
        const float t = (ea == 0xFF || eb == 0xFF) ? __uint_as_float(0x7FC00000u) : __builtin_ldexpf(fa * fb, ea + eb - 254);
        s += t;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float bias = p.bias ? load_as_float(p.bias, p.transposed ? m : n, p.bias_dtype) : 0.0f;
        const float sr = p.scale_result ? p.scale_result[0] : 1.0f;
        store_from_float(p.C, m * p.ldc + n, epilogue_value(s, 1.0f, 1.0f, p.bias != nullptr, bias, p.scale_result != nullptr, sr, p.transposed != 0),
                         p.out_dtype);
    }
}

}  // namespace

int fp8mi_launch_generic_mxw4a8(const MMParams &p, const MxScales &sc, hipStream_t s)
{
    const int64_t gx = (p.N + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t gy = p.M < 65535 ? p.M : 65535;
    const int64_t gz = (p.M + 65534) / 65535;
    if (gx > 0x7FFFFFFF || gz > 65535) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch(generic_mxw4a8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kWavesPerBlock * 64), s, p, sc);
}

// ---- blockwise form ------------------------------------------------------------------------------------------------
// One wave per output, as above.  Lane l sums the exact products of 128-k block b = l (then l + 64, ...) in k order in IEEE fp32
// (P_b; the last block may be partial), and takes its scale product sa(m, b) * sb(n, b) rounded to fp32; the wave then folds the
// blocks in block order, acc = fma(P_b, sa * sb, acc) - the ring kernels' fold, with exact block sums.  K = 0 reads no scale.
namespace {

__global__ __launch_bounds__(kWavesPerBlock * 64) void generic_blockwise_kernel(MMParams p, BwScales sc)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t m = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (n >= p.N || m >= p.M) return;  // wave-uniform
    const uint8_t *a = p.A + m * p.lda;
    const uint8_t *b = p.B + n * p.ldb;
    const float *sa = sc.sa + (m >> sc.sh_a) * sc.sa_sr;
    const float *sb = sc.sb + (n >> sc.sh_b) * sc.sb_sr;
    float acc = 0.0f;
    for (int64_t b0 = 0; b0 < sc.nkb; b0 += 64) {
        const int64_t blk = b0 + lane;
        float pb = 0.0f, s = 0.0f;
        if (blk < sc.nkb) {
            const int64_t k1 = min(blk * 128 + 128, p.K);
            for (int64_t k = blk * 128; k < k1; ++k) {
                const float fa = p.nan_zero ? decode_ref(a[k]) : __builtin_amdgcn_cvt_f32_fp8((int)a[k], 0);
                const float fb = p.nan_zero ? decode_ref(b[k]) : __builtin_amdgcn_cvt_f32_fp8((int)b[k], 0);
                pb += fa * fb;   // the product is exact in fp32
            }
            s = sa[blk * sc.sa_sk] * sb[blk * sc.sb_sk];
        }
        const int cnt = (int)min((int64_t)64, sc.nkb - b0);
        for (int i = 0; i < cnt; ++i) {
            const float pi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pb), i));
            const float si = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), i));
            acc = __builtin_fmaf(pi, si, acc);
        }
    }
    if (lane == 0) {
        const float bias = p.bias ? load_as_float(p.bias, p.transposed ? m : n, p.bias_dtype) : 0.0f;
        const float sr = p.scale_result ? p.scale_result[0] : 1.0f;
        store_from_float(p.C, m * p.ldc + n, epilogue_value(acc, 1.0f, 1.0f, p.bias != nullptr, bias, p.scale_result != nullptr, sr, p.transposed != 0),
                         p.out_dtype);
    }
}

}  // namespace

int fp8mi_launch_generic_blockwise(const MMParams &p, const BwScales &sc, hipStream_t s)
{
    const int64_t gx = (p.N + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t gy = p.M < 65535 ? p.M : 65535;
    const int64_t gz = (p.M + 65534) / 65535;
    if (gx > 0x7FFFFFFF || gz > 65535) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch(generic_blockwise_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kWavesPerBlock * 64), s, p, sc);
}
