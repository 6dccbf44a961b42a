// Elementwise FP8 e4m3fn casts for gfx950: dequant (fp8 -> f16/f32/bf16),
// encode (f32/f16/bf16 -> fp8), amax, and the device-side scale derivation of
// the amax-scaled quantiser.  All are HBM-bound streaming kernels: 16 bytes of
// fp8 per lane per step, dwordx4 loads and stores, grid-stride over at most
// 2048 workgroups so the launch fills the 256 CUs without a long block queue.
//
// Reference kernels replaced: fp8_to_half_kernel (fp8_matmul.metal:215-223),
// float_to_fp8_kernel (:228-236); reference math restated: decode :19-40,
// encode :44-92.

#include "fp8mi_common.h"
#include "fp8mi_encode.h"   // encode_bits / encode4 / InVec / encode_e5m2_bits / scale_of_amax / group_quant1
#include "fp8mi_mx.h"       // pow2_f32 / mx_exponent / mx_factor / mx_scaled / mx_e2m1

namespace {

constexpr int kBlock = 128;  // (128 / 256 / 512 / 1024 threads: 2^30 fp32 encode 922 / 967 / 932 / 931 us, dequant 595 / 605 / 609 / 610 us)
// One pass per workgroup up to 2^30 threads (a grid-stride loop only beyond that): with the grid capped at 2048
// workgroups the 2^30-element casts ran at 4.6-4.7 TB/s, with one-shot workgroups (262,144 of them for the fp32
// encode) at 5.8 (encode) / 5.3 (dequant) TB/s - the dispatcher keeps the memory pipes fuller than a long loop does.
constexpr int kMaxGrid = 1 << 22;
constexpr int kDequantUnroll = 1;
#ifndef FP8MI_CAST_UNROLL
#define FP8MI_CAST_UNROLL 4  // 16-byte loads in flight per lane in the vector cast kernels
#endif

// ---------------------------------------------------------------------------
// decode: four packed fp8 bytes -> four halves (two packed dwords), exact.
// Bit trick: fp8 [s eeee mmm] placed at half bits [15 | 13:7] is the half
// 2^(e-15)(1+m/8) (or the half-subnormal m/8 * 2^-14 for e == 0); multiplying
// by 2^8 rebiases it to the e4m3 value 2^(e-7)(1+m/8) (m/8 * 2^-6).  NaN
// patterns become +0.0 first (fp8_matmul.metal:21).
// ---------------------------------------------------------------------------
FP8MI_DEVICE uint32_t fp8x2_to_half2_bits(uint32_t x /* bytes at [15:8] and [31:24] */)
{
    uint32_t t = x & 0x7F007F00u;
    uint32_t h = (x & 0x80008000u) | (t >> 1);
    uint32_t m = (t + 0x01000100u) & 0x80008000u;  // bit15 of a half set iff its byte is NaN
    m = m | (m - (m >> 15));                       // 0xFFFF per NaN half
    return h & ~m;
}

FP8MI_DEVICE void decode4_half(uint32_t w, f16x2 &lo, f16x2 &hi)
{
    uint32_t a = __builtin_amdgcn_perm(0u, w, 0x010c000cu);  // (b0 << 8) | (b1 << 24)
    uint32_t b = __builtin_amdgcn_perm(0u, w, 0x030c020cu);  // (b2 << 8) | (b3 << 24)
    const f16x2 k256 = {(_Float16)256.0f, (_Float16)256.0f};
    lo = __builtin_bit_cast(f16x2, fp8x2_to_half2_bits(a)) * k256;
    hi = __builtin_bit_cast(f16x2, fp8x2_to_half2_bits(b)) * k256;
}

// one byte -> half, same bit trick (a true f16 multiply keeps the sign of -0.0)
FP8MI_DEVICE _Float16 decode1_half(uint32_t b)
{
    const uint16_t hb = (uint16_t)fp8x2_to_half2_bits((b & 0xFFu) << 8);
    return __builtin_bit_cast(_Float16, hb) * (_Float16)256.0f;
}

template <int OUT>
struct OutVec;  // 16 output elements

template <>
struct OutVec<FP8MI_F16> {
    static FP8MI_DEVICE void store(void *out, int64_t i16, const f16x2 (&h)[8])
    {
        u32x4 *o = (u32x4 *)out + i16 * 2;
        u32x4 v0, v1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v0[j] = __builtin_bit_cast(uint32_t, h[j]);
            v1[j] = __builtin_bit_cast(uint32_t, h[4 + j]);
        }
        o[0] = v0;
        o[1] = v1;
    }
    static FP8MI_DEVICE void store1(void *out, int64_t i, _Float16 v) { ((_Float16 *)out)[i] = v; }
};

template <>
struct OutVec<FP8MI_F32> {
    static FP8MI_DEVICE void store(void *out, int64_t i16, const f16x2 (&h)[8])
    {
        f32x4 *o = (f32x4 *)out + i16 * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 v = {(float)h[2 * j][0], (float)h[2 * j][1], (float)h[2 * j + 1][0], (float)h[2 * j + 1][1]};
            o[j] = v;
        }
    }
    static FP8MI_DEVICE void store1(void *out, int64_t i, _Float16 v) { ((float *)out)[i] = (float)v; }
};

template <>
struct OutVec<FP8MI_BF16> {
    static FP8MI_DEVICE uint32_t pack(f16x2 h)
    {
        __bf16 a = (__bf16)(float)h[0], b = (__bf16)(float)h[1];
        return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
    }
    static FP8MI_DEVICE void store(void *out, int64_t i16, const f16x2 (&h)[8])
    {
        u32x4 *o = (u32x4 *)out + i16 * 2;
        u32x4 v0, v1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v0[j] = pack(h[j]);
            v1[j] = pack(h[4 + j]);
        }
        o[0] = v0;
        o[1] = v1;
    }
    static FP8MI_DEVICE void store1(void *out, int64_t i, _Float16 v) { ((__bf16 *)out)[i] = (__bf16)(float)v; }
};

// in/out 16-byte aligned: 16 fp8 bytes per lane per load (1 KiB per load
// instruction), the lane's 16 outputs stored as 16-byte pieces; 4 loads in
// flight per lane; n16 = count / 16 full vectors, then a scalar tail.
template <int OUT>
__global__ __launch_bounds__(kBlock) void dequant_kernel(const uint8_t *__restrict__ in, void *__restrict__ out,
                                                            const float *__restrict__ scale, int64_t count)
{
    const bool has_scale = scale != nullptr;
    _Float16 s = has_scale ? (_Float16)scale[0] : (_Float16)1.0f;
    const f16x2 s2 = {s, s};
    const int64_t n16 = count >> 4;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const u32x4 *in4 = (const u32x4 *)in;
    // ONE 16-byte piece per lane and pass (round 3, tools/probes/copy_sweep.hip: the memory instructions of this kernel alone - 16 B in, 2 x 16 B out
    // per lane - move 6.07 TB/s as one pass per workgroup and 5.28 TB/s in round 2's shape of 4 pieces per lane on a quarter of the workgroups)
    constexpr int kUn = kDequantUnroll;
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n16; i0 += stride * kUn) {
        u32x4 w[kUn];
#pragma unroll
        for (int u = 0; u < kUn; ++u) {
            const int64_t i = i0 + u * stride;
            w[u] = i < n16 ? __builtin_nontemporal_load(in4 + i) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kUn; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= n16) break;
            f16x2 h[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) decode4_half(w[u][j], h[2 * j], h[2 * j + 1]);
            if (has_scale) {
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = h[j] * s2;
            }
            OutVec<OUT>::store(out, i, h);
        }
    }
    if (blockIdx.x == 0) {
        int64_t i = (n16 << 4) + threadIdx.x;
        if (i < count) {
            _Float16 v = decode1_half(in[i]);
            if (has_scale) v = v * s;
            OutVec<OUT>::store1(out, i, v);
        }
    }
}

// unaligned fallback: one element per lane per step
template <int OUT>
__global__ __launch_bounds__(kBlock) void dequant_scalar_kernel(const uint8_t *__restrict__ in, void *__restrict__ out,
                                                                 const float *__restrict__ scale, int64_t count)
{
    const bool has_scale = scale != nullptr;
    _Float16 s = has_scale ? (_Float16)scale[0] : (_Float16)1.0f;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        _Float16 v = decode1_half(in[i]);
        if (has_scale) v = v * s;
        OutVec<OUT>::store1(out, i, v);
    }
}


// in/out 16-byte aligned.  Lane l loads the 16 bytes at 16 l of each KiB piece of
// the input (one contiguous KiB per load instruction) = kPer elements, and
// stores their kPer bytes at kPer * l (256 / 512 contiguous bytes per store
// instruction); 4 pieces per lane are in flight.
// FROM_AMAX: `prescale` points at {amax, inv_scale}: every thread derives the scale from
// amax (read-only here; scale_of_amax: 448 / amax in double, 1 for amax == 0), thread 0 of workgroup 0 publishes
// float(1 / scale) in slot 1 (fp8_mps_native.py:189) - the amax-scaled quantiser without a separate scale kernel.
template <int ENC>
FP8MI_DEVICE float prescale_of(float amax, const float *prescale)
{
    const float ps = scale_of_amax<ENC>(amax);
    if (blockIdx.x == 0 && threadIdx.x == 0) ((float *)prescale)[1] = inv_scale_of_amax<ENC>(amax);
    return ps;
}

template <int IN>
constexpr int kEncodeUnroll = IN == FP8MI_F32 ? 1 : 2;

template <int IN, int MODE, bool FROM_AMAX = false>
__global__ __launch_bounds__(kBlock) void encode_kernel(const void *__restrict__ in, uint8_t *__restrict__ out,
                                                         const float *__restrict__ prescale, int64_t count)
{
    // vectors in flight per lane (the grid covers 16 elements per lane): measured at 2^30 fp32 elements
    // 1 / 2 / 4 / 8 = 6.1 / 5.9 / 5.7 / 5.5 TB/s, at 50 M bf16 elements 3.8 / 4.3 / 4.2 / 3.6
    constexpr int kPer = InVec<IN>::kPer, kUn = kEncodeUnroll<IN>;
    const bool has_ps = prescale != nullptr;
    float ps = has_ps ? prescale[0] : 1.0f;
    if (FROM_AMAX) {
        const float amax = ps;
        ps = scale_of_amax<MODE>(amax);
        if (blockIdx.x == 0 && threadIdx.x == 0) ((float *)prescale)[1] = inv_scale_of_amax<MODE>(amax);
    }
    const int64_t nv = count / kPer;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < nv; i0 += stride * kUn) {
        float f[kUn][8];
#pragma unroll
        for (int u = 0; u < kUn; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < nv) InVec<IN>::loadv(in, i, f[u]);
        }
#pragma unroll
        for (int u = 0; u < kUn; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= nv) break;
            if (has_ps) {
#pragma unroll
                for (int j = 0; j < kPer; ++j) f[u][j] = f[u][j] * ps;  // float32 multiply, as `inp * scale` (fp8_mps_native.py:179)
            }
            const uint32_t w0 = encode4<MODE>(f[u][0], f[u][1], f[u][2], f[u][3]);
            // streaming stores: the bytes are written once and not read back here (copy_sweep.hip, this kernel's memory shape: 6.63 TB/s
            // with nt stores against 6.33 with the default policy)
            if (kPer == 4) {
                __builtin_nontemporal_store(w0, (uint32_t *)out + i);
            } else {
                const uint32_t w1 = encode4<MODE>(f[u][4], f[u][5], f[u][6], f[u][7]);
                __builtin_nontemporal_store(u32x2{w0, w1}, (u32x2 *)out + i);
            }
        }
    }
    if (blockIdx.x == 0) {
        int64_t i = nv * kPer + threadIdx.x;
        if (i < count) {
            float v = InVec<IN>::load1(in, i);
            if (has_ps) v = v * ps;
            out[i] = (uint8_t)encode_bits<MODE>(v);
        }
    }
}

template <int IN, int MODE, bool FROM_AMAX = false>
__global__ __launch_bounds__(kBlock) void encode_scalar_kernel(const void *__restrict__ in, uint8_t *__restrict__ out,
                                                                const float *__restrict__ prescale, int64_t count)
{
    const bool has_ps = prescale != nullptr;
    float ps = has_ps ? prescale[0] : 1.0f;
    if (FROM_AMAX) {
        const float amax = ps;
        ps = scale_of_amax<MODE>(amax);
        if (blockIdx.x == 0 && threadIdx.x == 0) ((float *)prescale)[1] = inv_scale_of_amax<MODE>(amax);
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        float v = InVec<IN>::load1(in, i);
        if (has_ps) v = v * ps;
        out[i] = (uint8_t)encode_bits<MODE>(v);
    }
}

// ---------------------------------------------------------------------------
// amax: |x| max as float bits through atomicMax on the (non-negative) pattern
// ---------------------------------------------------------------------------
// amax runs few, fat workgroups (1024 threads, <= 512 of them): every workgroup ends in one same-address atomic,
// and those serialise at ~10 ns each - 1536 workgroups finishing together cost ~15 us on a 25 MB tensor
constexpr int kAmaxBlock = 1024;
constexpr int kAmaxMaxGrid = 512;

template <int IN>
__global__ __launch_bounds__(kAmaxBlock) void amax_kernel(const void *__restrict__ in, uint32_t *__restrict__ out_bits,
                                                       int64_t count, int vec_ok)
{
    // like the encode kernel: every wave-instruction reads one contiguous KiB (lane l -> 16 B at 16 l), four of them
    // in flight per lane (the first version read 16 consecutive elements per lane: 25-50 % of each line per
    // instruction and one batch in flight - 0.9 TB/s on a 25 MB activation tensor)
    constexpr int P = InVec<IN>::kPer;   // elements per 16-byte vector
    constexpr int U = FP8MI_CAST_UNROLL;
    float m = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * kAmaxBlock;
    const int64_t nv = vec_ok ? count / P : 0;
    int64_t i = (int64_t)blockIdx.x * kAmaxBlock + threadIdx.x;
    for (; i + (U - 1) * stride < nv; i += U * stride) {
        float f[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) InVec<IN>::loadv(in, i + u * stride, f[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < P; ++j) m = fmaxf(m, fabsf(f[u][j]));  // fmaxf drops NaN operands
    }
    for (; i < nv; i += stride) {
        float f[8];
        InVec<IN>::loadv(in, i, f);
#pragma unroll
        for (int j = 0; j < P; ++j) m = fmaxf(m, fabsf(f[j]));
    }
    for (int64_t e = nv * P + (int64_t)blockIdx.x * kAmaxBlock + threadIdx.x; e < count; e += stride)
        m = fmaxf(m, fabsf(InVec<IN>::load1(in, e)));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __shared__ float wmax[kAmaxBlock / 64];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = wmax[0];
#pragma unroll
        for (int w = 1; w < kAmaxBlock / 64; ++w) b = fmaxf(b, wmax[w]);
        // Same-address atomics serialise at the memory side (~10 ns each): 2048 workgroups finishing together cost
        // ~20 us on a 25 MB tensor.  The running maximum only grows, so a workgroup whose maximum does not exceed
        // the value it can already see has nothing to add (a stale, smaller value merely costs the atomic).
        const uint32_t mine = __float_as_uint(b);
        if (mine > __hip_atomic_load(out_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out_bits, mine);
    }
}

int grid_for(int64_t work_items)
{
    int64_t g = (work_items + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > kMaxGrid) g = kMaxGrid;
    return (int)g;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- MXFP8 (OCP microscaling: one E8M0 scale per 32 elements of a row) --------------------------------------------
// Quantize, torch's recipe (to_mxfp(x, 32, "mxfp8") of torch/testing/_internal/common_quantized.py, torchao's RCEIL), bit for bit:
//   amax = max |x| over the block (NaN if the block holds one); descale = amax / 448 (fp32 division)
//   e = 0xFF if descale is NaN, else clamp(ceil(log2(descale)), -127, 127) + 127
//   q = e4m3_rne(clamp(x * (e == 0 ? 1 : 2^(127 - e)), -448, 448))     (fp32 multiply, subnormal factors included)
// torch takes log2 in fp32, correctly rounded: just above a power of two it returns the power itself and the block saturates to
// 448 instead of stepping its scale up.  log2 in double rounded once to fp32 gives that same value.
//
// ---- MXFP4 (e2m1, two per byte; one E8M0 scale per 32 elements of a row) ------------------------------------------------
// Quantize, torch's recipe (to_mxfp(x, 32, "mxfp4") of torch/testing/_internal/common_quantized.py), bit for bit:
//   e = the RCEIL exponent of amax / 6 (as for MXFP8);  y = clamp(x * (e == 0 ? 1 : 2^(127 - e)), -6, 6)   (fp32)
//   y is rounded to bfloat16 (RNE) FIRST, and that value to e2m1 (RNE, saturating) by torchao's integer path
//   (_f32_to_floatx_unpacked); two codes per byte, the even column in the low nibble (pack_uint4).
// The double rounding is part of the recipe: 2.5 + 2^-20 is bf16 2.5, which ties to 2.0 (a single rounding gives 3.0).
// A NaN element is the bfloat16 0xFFFF that torch's CPU cast makes of every NaN; the integer path turns it into code 0xC.
//
// The factor, the clamp and the e2m1 step are fp8mi_mx.h's mx_factor / mx_scaled / mx_e2m1, shared with the fused producers.

// one thread per 32-element block: rows x nblk threads; 32 (MXFP8) or 16 (MXFP4) bytes out per block, as 16-byte stores where the output
// block is 16-byte aligned and byte by byte where it is not
template <int IN, bool FP4>
__global__ __launch_bounds__(kBlock) void quantize_mx_kernel(const void *__restrict__ in, int64_t rows, int64_t nblk, int64_t ld_in,
                                                             uint8_t *__restrict__ out, int64_t ld_out, uint8_t *__restrict__ scales, int64_t ld_s)
{
    constexpr int kWords = FP4 ? 4 : 8;   // dwords of output per block
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= rows * nblk) return;
    const int64_t r = g / nblk, b = g - r * nblk;
    const int64_t i0 = r * ld_in + b * 32;
    float x[32];
    float amax = 0.0f;
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        x[i] = InVec<IN>::load1(in, i0 + i);
        const float a = fabsf(x[i]);
        nan = nan || a != a;
        amax = a > amax ? a : amax;
    }
    const uint32_t e = mx_exponent(nan ? __uint_as_float(0x7FC00000u) : amax, FP4 ? 6.0f : 448.0f);
    const float f = mx_factor(e);
    uint32_t w[kWords];
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        uint32_t v = 0;
        if (FP4) {
#pragma unroll
            for (int k = 0; k < 8; k += 2)   // pack_uint4: odd column high, even column low
                v |= (((mx_e2m1(x[8 * j + k + 1], f) << 4) | mx_e2m1(x[8 * j + k], f)) & 0xFFu) << (4 * k);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= encode_rne_bits(__float_as_uint(mx_scaled(x[4 * j + k], f, 448.0f))) << (8 * k);
        }
        w[j] = v;
    }
    uint8_t *o = out + r * ld_out + b * (4 * kWords);
    if ((((uintptr_t)o) & 15u) == 0) {
#pragma unroll
        for (int q = 0; q < kWords / 4; ++q) ((u32x4 *)o)[q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4 * kWords; ++i) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
    scales[r * ld_s + b] = (uint8_t)e;   // a vector byte store
}

// out = dec(q) x 2^(s - 127), computed in fp32 and rounded once to out_dtype; the scale 0xFF is NaN.  MXFP8: OCP decode, NaN bytes are NaN.
// MXFP4: dec is the e2m1 value of the column's nibble; cols count elements
template <int OUT, bool FP4>
__global__ __launch_bounds__(kBlock) void dequant_mx_kernel(const uint8_t *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in,
                                                            const uint8_t *__restrict__ scales, int64_t ld_s, void *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= rows * cols) return;
    const int64_t r = g / cols, c = g - r * cols;
    const uint32_t sb = scales[r * ld_s + (c >> 5)];
    const float d = FP4 ? e2m1_value((uint32_t)in[r * ld_in + (c >> 1)] >> (4 * (int)(c & 1))) : __builtin_amdgcn_cvt_f32_fp8((int)in[r * ld_in + c], 0);
    // 2^(s - 127) is an exact fp32 (2^-127 a subnormal): one multiply, one rounding (only below 2^-126 or above the fp32 range)
    const float v = sb == 0xFFu ? __uint_as_float(0x7FC00000u) : d * pow2_f32((int)sb - 127);
    store_from_float(out, g, v, OUT);
}

// ---- blockwise (fp32 scale per block of 1 or 128 rows x 128 columns) ------------------------------------------------------
// Quantize (tests/blockwise_ref.py restates it with torch CPU ops):
//   amax = max |x| over the block, widened to fp32 (NaN if the block holds a NaN);  s = amax / 448 (IEEE), s = 1 when that
//   quotient is 0: an all-zero block, or an f32 amax so small (below about 448 x 2^-150) that the division underflows
//   q = e4m3_rne(clamp(x / s, -448, 448)) (IEEE division);  a NaN quotient (a NaN in the block, or inf / inf) is stored as 0x7F
// The scale written is s, the dequantisation scale _scaled_mm consumes (a NaN scale as the quiet NaN 0x7FC00000).
// One wave per block: lane l owns columns 2l and 2l + 1 of every row of the block; amax first, then the quotients (quotient, clamp and
// byte: fp8mi_encode.h's group_quant1, shared with the fused producers' GROUP128 form).
template <int IN>
__global__ __launch_bounds__(256) void quantize_blockwise_kernel(const void *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in, int sh,
                                                                 int64_t ncb, uint8_t *__restrict__ out, int64_t ld_out, float *__restrict__ scales,
                                                                 int64_t s_sr, int64_t s_sk)
{
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t rb = blk / ncb, cb = blk - rb * ncb;
    if (rb >= ((rows + (1 << sh) - 1) >> sh)) return;   // wave-uniform
    const int64_t r0 = rb << sh, r1 = min(r0 + (1 << sh), rows);
    const int64_t c0 = cb * 128 + 2 * lane;
    const bool in0 = c0 < cols, in1 = c0 + 1 < cols;
    float amax = 0.0f;
    bool nan = false;
    for (int64_t r = r0; r < r1; ++r) {
        const float x0 = in0 ? InVec<IN>::load1(in, r * ld_in + c0) : 0.0f, x1 = in1 ? InVec<IN>::load1(in, r * ld_in + c0 + 1) : 0.0f;
        const float a0 = fabsf(x0), a1 = fabsf(x1);
        nan = nan || a0 != a0 || a1 != a1;
        amax = a0 > amax ? a0 : amax;
        amax = a1 > amax ? a1 : amax;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    nan = __ballot(nan) != 0;
    const float s = nan ? __uint_as_float(0x7FC00000u) : (amax / 448.0f == 0.0f ? 1.0f : amax / 448.0f);
    for (int64_t r = r0; r < r1; ++r) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!(h ? in1 : in0)) continue;
            const int64_t c = c0 + h;
            out[r * ld_out + c] = (uint8_t)group_quant1(InVec<IN>::load1(in, r * ld_in + c), s);   // a vector byte store
        }
    }
    if (lane == 0) scales[rb * s_sr + cb * s_sk] = s;
}

// out = dec(q) x s of its block (OCP decode: NaN bytes are NaN), the product in fp32 rounded once, then to out_dtype
template <int OUT>
__global__ __launch_bounds__(kBlock) void dequant_blockwise_kernel(const uint8_t *__restrict__ in, int64_t rows, int64_t cols, int64_t ld_in, int sh,
                                                                   const float *__restrict__ scales, int64_t s_sr, int64_t s_sk, void *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= rows * cols) return;
    const int64_t r = g / cols, c = g - r * cols;
    const float d = __builtin_amdgcn_cvt_f32_fp8((int)in[r * ld_in + c], 0);
    float v = d * scales[(r >> sh) * s_sr + (c >> 7) * s_sk];
    asm("" : "+v"(v));   // the fp32 product is rounded first: fused with an f16 conversion (v_fma_mix) it would be rounded once, to f16
    store_from_float(out, g, v, OUT);
}

// ---- OCP e5m2 (torch.float8_e5m2) casts ----------------------------------------------------------------------------

// FROM_AMAX: `prescale` points at {amax, inv_scale} (fp8mi_quantize_e5m2): scale = 57344 / amax evaluated in double (1 when amax is 0),
// the scaled value clamped to +-57344 (a NaN stays NaN), and thread 0 publishes float(1 / scale) in slot 1
template <int IN, bool FROM_AMAX>
__global__ __launch_bounds__(kBlock) void encode_e5m2_kernel(const void *__restrict__ in, uint8_t *__restrict__ out, const float *__restrict__ prescale,
                                                              int64_t count)
{
    const bool has_ps = prescale != nullptr;
    float ps = has_ps ? prescale[0] : 1.0f;
    if (FROM_AMAX) {
        const float amax = ps;
        ps = scale_of_amax<kEncE5M2>(amax);
        if (blockIdx.x == 0 && threadIdx.x == 0) ((float *)prescale)[1] = inv_scale_of_amax<kEncE5M2>(amax);
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        float v = InVec<IN>::load1(in, i);
        if (has_ps) {
            v = v * ps;   // float32 multiply, rounded before the encode
            asm("" : "+v"(v));
        }
        if (FROM_AMAX) v = v > 57344.0f ? 57344.0f : (v < -57344.0f ? -57344.0f : v);
        out[i] = (uint8_t)encode_e5m2_bits(v);
    }
}

// out = cast(float(dec(b)) * scale): the product in fp32 rounded once, then to out_dtype (scale NULL: no multiply); inf and NaN stay
template <int OUT>
__global__ __launch_bounds__(kBlock) void dequant_e5m2_kernel(const uint8_t *__restrict__ in, void *__restrict__ out, const float *__restrict__ scale,
                                                               int64_t count)
{
    const bool has_s = scale != nullptr;
    const float sc = has_s ? scale[0] : 1.0f;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        float v = decode_e5m2(in[i]);
        if (has_s) {
            v = v * sc;
            asm("" : "+v"(v));   // rounded to fp32 first: fused with an f16 conversion (v_fma_mix) it would be rounded once, to f16
        }
        store_from_float(out, i, v, OUT);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers (called from fp8mi_api.hip)
// ---------------------------------------------------------------------------
// (the run-time dtypes, modes and formats reach the templates through dispatch_in / dispatch_int, the 2-D grids through fp8mi_launch_items)

int fp8mi_launch_dequant(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, hipStream_t s)
{
    if (count == 0) return 0;
    const bool vec = aligned16(in) && aligned16(out);
    const int grid = grid_for(vec ? (count >> 4) / kDequantUnroll : count);  // vector kernel: 16 bytes per lane per pass
    return dispatch_in(out_dtype, [&](auto out_t) {
        return vec ? fp8mi_launch(dequant_kernel<decltype(out_t)::value>, dim3(grid), dim3(kBlock), s, in, out, scale, count)
                   : fp8mi_launch(dequant_scalar_kernel<decltype(out_t)::value>, dim3(grid), dim3(kBlock), s, in, out, scale, count);
    });
}

template <bool FROM_AMAX>
static int launch_encode(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, int mode, hipStream_t s)
{
    const bool vec = aligned16(in) && aligned16(out);
    // 16 elements per lane: 16-bit inputs in one pass of 2 vectors, fp32 in 4 passes of one (measured best: a million
    // one-vector workgroups instead reach only 5.1 TB/s)
    const int grid = grid_for(vec ? (count >> 4) + 1 : count);
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            return vec ? fp8mi_launch(encode_kernel<decltype(in_t)::value, decltype(mode_t)::value, FROM_AMAX>, dim3(grid), dim3(kBlock), s, in, out, prescale, count)
                       : fp8mi_launch(encode_scalar_kernel<decltype(in_t)::value, decltype(mode_t)::value, FROM_AMAX>, dim3(grid), dim3(kBlock), s, in, out, prescale, count);
        });
    });
}

int fp8mi_launch_encode(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, int mode, hipStream_t s)
{
    if (count == 0) return 0;
    return launch_encode<false>(in, in_dtype, out, prescale, count, mode, s);
}

int fp8mi_launch_amax(const void *in, int in_dtype, float *out, int64_t count, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    if (count == 0) return 0;
    const int vec = aligned16(in) ? 1 : 0;
    // one 16-byte vector per lane and iteration, FP8MI_CAST_UNROLL of them in flight
    const int per = in_dtype == FP8MI_F32 ? 4 : 8;
    const int64_t items = vec ? (count / per + FP8MI_CAST_UNROLL - 1) / FP8MI_CAST_UNROLL + 1 : count;
    int64_t grid = (items + kAmaxBlock - 1) / kAmaxBlock;
    grid = grid < 1 ? 1 : (grid > kAmaxMaxGrid ? kAmaxMaxGrid : grid);
    return dispatch_in(in_dtype, [&](auto in_t) {
        return fp8mi_launch(amax_kernel<decltype(in_t)::value>, dim3((unsigned)grid), dim3(kAmaxBlock), s, in, (uint32_t *)out, count, vec);
    });
}

int fp8mi_launch_quantize(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, int mode, hipStream_t s)
{
    // scales[0] <- amax (atomicMax over the input), then one encode launch that derives
    // scale = 448 / amax per thread and publishes scales[1] = 1 / scale
    int rc = fp8mi_launch_amax(in, in_dtype, scales, count, s);
    if (rc) return rc;
    // (count == 0 still launches one workgroup: it publishes inv_scale = 1 and touches no data)
    return launch_encode<true>(in, in_dtype, out, scales, count, mode, s);
}

int fp8mi_launch_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, uint8_t *scales,
                             int64_t ld_s, int mx_format, hipStream_t s)
{
    const int64_t nblk = cols / 32;
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_MX_FP4, FP8MI_MX_FP8>(mx_format, [&](auto fmt_t) {
            return fp8mi_launch_items(quantize_mx_kernel<decltype(in_t)::value, decltype(fmt_t)::value == FP8MI_MX_FP4>, rows * nblk, kBlock, kBlock, s, in, rows, nblk,
                                      ld_in, out, ld_out, scales, ld_s);
        });
    });
}

int fp8mi_launch_dequant_mx(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const uint8_t *scales, int64_t ld_s, void *out, int out_dtype,
                            int mx_format, hipStream_t s)
{
    return dispatch_in(out_dtype, [&](auto out_t) {
        return dispatch_int<FP8MI_MX_FP4, FP8MI_MX_FP8>(mx_format, [&](auto fmt_t) {
            return fp8mi_launch_items(dequant_mx_kernel<decltype(out_t)::value, decltype(fmt_t)::value == FP8MI_MX_FP4>, rows * cols, kBlock, kBlock, s, in, rows, cols,
                                      ld_in, scales, ld_s, out);
        });
    });
}

int fp8mi_launch_quantize_blockwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, uint8_t *out,
                                    int64_t ld_out, float *scales, int64_t s_sr, int64_t s_sk, hipStream_t s)
{
    const int sh = block_rows == 128 ? 7 : 0;
    const int64_t nrb = (rows + block_rows - 1) / block_rows, ncb = (cols + 127) / 128;
    return dispatch_in(in_dtype, [&](auto in_t) {   // four waves (blocks) per workgroup
        return fp8mi_launch_items(quantize_blockwise_kernel<decltype(in_t)::value>, nrb * ncb, 4, 256, s, in, rows, cols, ld_in, sh, ncb, out, ld_out, scales, s_sr,
                                  s_sk);
    });
}

int fp8mi_launch_dequant_blockwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, const float *scales, int64_t s_sr,
                                   int64_t s_sk, void *out, int out_dtype, hipStream_t s)
{
    const int sh = block_rows == 128 ? 7 : 0;
    return dispatch_in(out_dtype, [&](auto out_t) {
        return fp8mi_launch_items(dequant_blockwise_kernel<decltype(out_t)::value>, rows * cols, kBlock, kBlock, s, in, rows, cols, ld_in, sh, scales, s_sr, s_sk,
                                  out);
    });
}

// ---- e5m2 casts ----
template <bool FROM_AMAX>
static int launch_encode_e5m2(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, hipStream_t s)
{
    const int grid = grid_for((count + 3) / 4);   // grid-stride, a few elements per thread
    return dispatch_in(in_dtype, [&](auto in_t) {
        return fp8mi_launch(encode_e5m2_kernel<decltype(in_t)::value, FROM_AMAX>, dim3(grid), dim3(kBlock), s, in, out, prescale, count);
    });
}

int fp8mi_launch_encode_e5m2(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, hipStream_t s)
{
    if (count == 0) return 0;
    return launch_encode_e5m2<false>(in, in_dtype, out, prescale, count, s);
}

int fp8mi_launch_dequant_e5m2(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, hipStream_t s)
{
    if (count == 0) return 0;
    const int grid = grid_for((count + 3) / 4);
    return dispatch_in(out_dtype, [&](auto out_t) {
        return fp8mi_launch(dequant_e5m2_kernel<decltype(out_t)::value>, dim3(grid), dim3(kBlock), s, in, out, scale, count);
    });
}

int fp8mi_launch_quantize_e5m2(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, hipStream_t s)
{
    // scales[0] <- amax, then one encode launch that derives scale = 57344 / amax per thread and publishes scales[1] = 1 / scale
    // (count == 0 still launches one workgroup: it publishes inv_scale = 1 and touches no data)
    const int rc = fp8mi_launch_amax(in, in_dtype, scales, count, s);
    if (rc) return rc;
    return launch_encode_e5m2<true>(in, in_dtype, out, scales, count, s);
}
