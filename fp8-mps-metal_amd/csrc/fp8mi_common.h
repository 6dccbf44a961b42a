// Shared device helpers for the fp8mi kernels (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/fp8mi.h"

typedef float    f32x2  __attribute__((ext_vector_type(2)));
typedef float    f32x4  __attribute__((ext_vector_type(4)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));
typedef int      i32x4  __attribute__((ext_vector_type(4)));
typedef int      i32x8  __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2  __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4  __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2  __attribute__((ext_vector_type(2)));

#define FP8MI_DEVICE __device__ __forceinline__

// ---------------------------------------------------------------------------
// epilogue parameters shared by the GEMV / GEMM / generic kernels
// ---------------------------------------------------------------------------
struct MMParams {
    const uint8_t *A;      // (M,K) row-major bytes
    const uint8_t *B;      // (N,K) row-major bytes
    void *C;               // (M,N) out_dtype
    const float *scale_a;  // [1] or [M]
    const float *scale_b;  // [1] or [N]
    const void *bias;      // nullptr or [N] bias_dtype
    const float *scale_result;  // nullptr or [1]
    int64_t M, N, K;
    int64_t lda, ldb, ldc;
    int sa_row, sb_row;    // 0 per-tensor, 1 per-row
    int out_dtype, bias_dtype;
    int transposed;        // 1: the caller computes C^T = B . A^T (sharded linear): bias runs along M (bias[m]) and the epilogue
                           //    multiplies by scale_b first, then scale_a - the bits of the untransposed fused epilogue
    int nan_zero;          // 1: NaN bytes decode to 0 (reference), 0: propagate
    int debug;             // diagnostic builds only (FP8MI_STAMP): ablation bits, else 0
    int split;             // GEMM tile kernels: number of K ranges per tile (1 = no split-K)
    uint8_t *ws;           // split-K workspace (tile counters, then fp32 partial tiles) or nullptr
    int64_t ws_bytes;
};

constexpr int kWsCounterBytes = 4096;

// The block-scaled (MXFP8) GEMMs' scales: E8M0 bytes (2^(s - 127); 0xFF NaN), one per 32 K of a row, row-major, ld_s* bytes
// apart.  sx: the rows of A (M), sw: the rows of B_nk (N).  A separate argument - MMParams is the kernarg of every tensorwise kernel.
struct MxScales {
    const uint8_t *sx, *sw;
    int64_t ld_sx, ld_sw;
};  // 1024 tile counters, zero between launches

// The blockwise ("1x128 / 128x128") GEMMs' scales: fp32, one per 128 k of a block of 1 or 128 rows,
// sa(m, b) = sa[(m >> sh_a) * sa_sr + b * sa_sk] (strides in floats, >= 0), the same for sb with the rows of B_nk (N).
struct BwScales {
    const float *sa, *sb;
    int64_t sa_sr, sa_sk, sb_sr, sb_sk;
    int64_t nkb;        // ceil(K / 128): the blocks along K
    int sh_a, sh_b;     // log2 of the rows that share a scale: 0 or 7
};

// What every row-quantising producer writes (fp8mi_rowquant.h): the encoded rows and their scales.  `scales` is fp32 for one scale per
// row (row r at r * s_sr) or per 128 columns (group k of row r at r * s_sr + k * s_sk), E8M0 bytes for the MX outputs (block k of row r
// at r * s_sr + k; s_sk unused); scale_row<QS> is the one place that gives it its type.
struct QuantOut {
    uint8_t *out;
    int64_t ld_out;
    void *scales;
    int64_t s_sr, s_sk;   // strides in scales (elements of their own type), >= 0
    int mx_flags;         // MX outputs: mx_scale_flags; else 0
    float *amax;          // one scale per row: nullptr or [rows]
};

// The arguments of the fused normalisation + quantisation kernels (fp8mi_normquant.hip), validated by fp8mi_norm_quantize: their kernarg.
struct NqArgs {
    const void *in;
    int64_t rows, cols, ld_in;
    float eps;
    const void *weight, *bias, *mod_scale, *mod_shift;   // nullptr or [cols]; nullptr or (ceil(rows / rows_per_mod), cols)
    int64_t ld_mod, rows_per_mod;
    int param_dtype;
    const void *residual;   // not __restrict__: h_out may be this buffer
    int64_t ld_res;
    void *h_out;
    int64_t ld_h;
    QuantOut q;
    float *mean_out, *rstd_out;
};

// Kernel arguments arrive through the kernarg segment, which the runtime may keep in HOST memory (a scalar load from it
// is a PCIe round trip, ~1.5 us; HIP_FORCE_DEV_KERNARG=1 moves it to HBM, ~0.5 us).  Left alone, hipcc loads the fields
// lazily - the GEMM had four dependent load-and-wait groups ahead of its first DMA and another in the epilogue, 4.6 us
// from kernel entry to the K loop (in-kernel stamps, profiles/r02_stamps.txt).  pin_params() makes every field opaque at
// kernel entry: all scalar loads issue as ONE clause with one wait, and the values then live in SGPRs (the compiler
// cannot re-derive them from the kernarg pointer later).
#define FP8MI_PIN_S(x) asm volatile("" : "+s"(x))
FP8MI_DEVICE MMParams pin_params(const MMParams &p)
{
    MMParams q = p;
    FP8MI_PIN_S(q.A); FP8MI_PIN_S(q.B); FP8MI_PIN_S(q.C); FP8MI_PIN_S(q.scale_a); FP8MI_PIN_S(q.scale_b);
    FP8MI_PIN_S(q.bias); FP8MI_PIN_S(q.scale_result);
    FP8MI_PIN_S(q.M); FP8MI_PIN_S(q.N); FP8MI_PIN_S(q.K); FP8MI_PIN_S(q.lda); FP8MI_PIN_S(q.ldb); FP8MI_PIN_S(q.ldc);
    FP8MI_PIN_S(q.sa_row); FP8MI_PIN_S(q.sb_row); FP8MI_PIN_S(q.out_dtype); FP8MI_PIN_S(q.bias_dtype);
    FP8MI_PIN_S(q.transposed); FP8MI_PIN_S(q.nan_zero); FP8MI_PIN_S(q.split); FP8MI_PIN_S(q.ws); FP8MI_PIN_S(q.ws_bytes);
    return q;
}

// One float at a wave-uniform address (a pointer that is a kernel argument: the per-tensor scales).  Through the constant address
// space it is ONE s_load_dword per wave; as `p[0]` on the generic pointer it is a flat_load_dword of 64 equal addresses that sits in
// the vector-memory queue ahead of the operand loads, counts in vmcnt AND lgkmcnt, and - because a flat load's return order is not
// the vector loads' - makes hipcc wait for vmcnt(0) where it next needs any loaded value.  The scalar cache is invalidated at kernel
// start, so a value the previous kernel of the stream wrote (fp8mi_quantize -> fp8mi_scaled_mm) is seen; nothing may write it
// while this kernel runs.
FP8MI_DEVICE float load_uniform_f32(const float *p) { return *(const __attribute__((address_space(4))) float *)p; }

// Cache policy of the GEMM kernels' C stores (compile-time knob for A/B builds; the product value is the default below):
//   0 default (write-back)   1 nt (streaming)   2 sc0 sc1 (system scope: written THROUGH the XCD's L2)   3 sc0 sc1 nt   4 sc1   5 sc1 nt
// The end of a kernel is an agent-scope release, which on this 8-L2 part means a write-back of every dirty line of
// every L2: stores that are written through leave nothing for it.
#ifndef FP8MI_CSTORE
#define FP8MI_CSTORE 1
#endif
constexpr int kCStoreAux = FP8MI_CSTORE == 0 ? 0 : FP8MI_CSTORE == 1 ? 2 : FP8MI_CSTORE == 2 ? 17 : FP8MI_CSTORE == 3 ? 19 : FP8MI_CSTORE == 4 ? 16 : 18;
FP8MI_DEVICE void store_c16(u32x4 q, void *ptr)   // one 16-byte piece of C
{
#if FP8MI_CSTORE == 0
    *(u32x4 *)ptr = q;
#elif FP8MI_CSTORE == 1
    __builtin_nontemporal_store(q, (u32x4 *)ptr);
#elif FP8MI_CSTORE == 2
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(ptr), "v"(q) : "memory");
#elif FP8MI_CSTORE == 3
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(ptr), "v"(q) : "memory");
#elif FP8MI_CSTORE == 4
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(ptr), "v"(q) : "memory");
#else
    asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(ptr), "v"(q) : "memory");
#endif
}

// SWAR scrub: zero every byte of w whose low 7 bits are all ones (the two
// e4m3fn NaN patterns 0x7F / 0xFF), i.e. the reference's decode rule
// "NaN -> 0.0" (fp8_matmul.metal:21) applied to four packed bytes.
FP8MI_DEVICE uint32_t scrub_nan4(uint32_t w)
{
    uint32_t n = ~(w | 0x80808080u);            // NaN byte -> 0x00, else 0x01..0x7F
    uint32_t m = ~((n + 0x7F7F7F7Fu) | 0x7F7F7F7Fu);  // 0x80 where the byte of n is zero
    m = m | (m - (m >> 7));                     // 0xFF where NaN
    return w & ~m;
}

// true if any of the four bytes is a NaN pattern
FP8MI_DEVICE bool has_nan4(uint32_t w)
{
    uint32_t n = ~(w | 0x80808080u);
    return (~((n + 0x7F7F7F7Fu) | 0x7F7F7F7Fu)) != 0u;
}

// one byte -> float, reference semantics (fp8_matmul.metal:19-40): used by the
// slow paths only; the hot kernels decode with v_cvt_pk_f32_fp8 / MFMA.
// Built from bits, with no float multiply on the signed value: hipcc fuses
// `x * 2^k` followed by a conversion into v_fma_mix*(x, 2^k, +0), and
// (-0 * c) + (+0) is +0 - the sign of 0x80 (-0.0, metal:39) would be lost.
FP8MI_DEVICE float decode_ref(uint32_t b)
{
    const uint32_t mag = b & 0x7Fu;
    if (mag == 0x7Fu) return 0.0f;
    const uint32_t sign = (b & 0x80u) << 24;
    uint32_t bits;
    if (mag >= 8u) bits = (mag << 20) + (120u << 23);           // normal: rebias 7 -> 127
    else bits = __float_as_uint((float)mag * 0x1p-9f);           // subnormal: m * 2^-9 (>= 0, exact)
    return __uint_as_float(bits | sign);
}

// OCP e5m2 byte -> float, exact: the byte is the high byte of an IEEE half (inf 0x7C / 0xFC, NaN 0x7D-0x7F / 0xFD-0xFF, subnormals)
FP8MI_DEVICE float decode_e5m2(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)((b & 0xFFu) << 8)); }
// one byte of either format -> float, OCP semantics (e4m3 NaN bytes give NaN)
FP8MI_DEVICE float decode_fmt(uint32_t b, int e5m2) { return e5m2 ? decode_e5m2(b) : __builtin_amdgcn_cvt_f32_fp8((int)b, 0); }

// OCP e2m1 (fp4) code c (low 4 bits) -> value: 0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives (no NaN, no inf)
FP8MI_DEVICE float e2m1_value(uint32_t c)
{
    const uint32_t e = (c >> 1) & 3u, m = c & 1u;
    const float v = e == 0 ? 0.5f * (float)m : (float)((2u + m) << (e - 1)) * 0.5f;
    return (c & 8u) ? -v : v;
}

FP8MI_DEVICE float load_as_float(const void *p, int64_t i, int dtype)
{
    if (dtype == FP8MI_F32) return ((const float *)p)[i];
    if (dtype == FP8MI_F16) return (float)((const _Float16 *)p)[i];
    return (float)((const __bf16 *)p)[i];
}

FP8MI_DEVICE void store_from_float(void *p, int64_t i, float v, int dtype)
{
    if (dtype == FP8MI_F32) ((float *)p)[i] = v;
    else if (dtype == FP8MI_F16) ((_Float16 *)p)[i] = (_Float16)v;
    else ((__bf16 *)p)[i] = (__bf16)v;
}

// two floats -> two f16 / bf16 values (RNE) in one dword, the first in the low half
template <int OUT>
FP8MI_DEVICE uint32_t pack16(float a, float b)
{
    if (OUT == FP8MI_F16) {
        const _Float16 x = (_Float16)a, y = (_Float16)b;
        return (uint32_t)__builtin_bit_cast(uint16_t, x) | ((uint32_t)__builtin_bit_cast(uint16_t, y) << 16);
    }
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (uint32_t)__builtin_bit_cast(uint16_t, x) | ((uint32_t)__builtin_bit_cast(uint16_t, y) << 16);
}

// The reference epilogue, in its order (fp8_matmul.metal:144-146 then
// fp8_mps_patch.py:94-104): (sum * sa) * sb, + bias, * scale_result, cast.
FP8MI_DEVICE float epilogue_value(float sum, float sa, float sb, bool has_bias, float bias,
                                  bool has_sr, float sr, bool transposed = false)
{
    float r = transposed ? (sum * sb) * sa : (sum * sa) * sb;
    if (has_bias) r = r + bias;
    if (has_sr) r = r * sr;
    return r;
}

// wave64 all-lanes sum.  Four DPP adds inside each row of 16 lanes (quad swaps, then the two mirrors: every lane of a row ends with
// the row's sum), then the four row sums are read out as scalars.  (The generic `__shfl_xor` butterfly compiles to six DEPENDENT
// ds_bpermute_b32 + s_waitcnt pairs - ~100 cycles each - per reduced value: 24 of them in series sat in the tail of every workgroup
// of the 4-row vec-mat, ~1 us of config C1's 5.2 us.)
template <int CTRL>
FP8MI_DEVICE float dpp_add(float x)   // x + (x of the lane the DPP control selects; 0 where that lane is inactive)
{
    const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false);
    return x + __builtin_bit_cast(float, y);
}

// sum over aligned groups of P = 2 / 4 / 8 / 16 adjacent lanes (every lane of a group ends with the group's sum)
template <int P>
FP8MI_DEVICE float group_sum(float v)
{
    static_assert(P == 1 || P == 2 || P == 4 || P == 8 || P == 16, "a power of two inside a row of 16 lanes");
    if (P >= 2) v = dpp_add<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    if (P >= 4) v = dpp_add<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    if (P >= 8) v = dpp_add<0x141>(v);   // row_half_mirror: lane i <- lane 7 - i of its half row
    if (P >= 16) v = dpp_add<0x140>(v);  // row_mirror: lane i <- lane 15 - i of its row
    return v;
}

FP8MI_DEVICE float wave_sum(float v)
{
    v = group_sum<16>(v);
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)),
                r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// Per-dispatch timing hook (fp8mi_profile_begin / _end in the C ABI): while a profile is open on the calling thread
// every kernel launch carries its own start/stop event pair, filled from the dispatch packet's timestamps - the same
// clock rocprofv3 --kernel-trace reads.  Outside a profile this is a plain launch.
bool fp8mi_next_profile_events(hipEvent_t *start, hipEvent_t *stop);

// Launch with the status of THIS launch (hipGetLastError() would report - and clear - any earlier error on the thread).
template <typename... KArgs>
int fp8mi_launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t s, KArgs... args)
{
    void *argv[] = {(void *)&args...};
    hipEvent_t e0, e1;
    if (fp8mi_next_profile_events(&e0, &e1))
        return (int)hipExtLaunchKernel((const void *)kernel, grid, block, argv, 0, s, e0, e1, 0);
    return (int)hipLaunchKernel((const void *)kernel, grid, block, argv, 0, s);
}

// The launch of a per-element 2-D kernel: n work items, `per_group` of them to a workgroup of `threads` threads along grid.x.  Nothing to do
// for an empty problem; a grid past 2^31 - 1 workgroups is refused.
template <typename... K, typename... A>
int fp8mi_launch_items(void (*kernel)(K...), int64_t n, int per_group, int threads, hipStream_t s, A... args)
{
    if (n == 0) return 0;
    const int64_t grid = (n + per_group - 1) / per_group;
    if (grid > 0x7FFFFFFF) return FP8MI_E_UNSUPPORTED;
    return fp8mi_launch<K...>(kernel, dim3((unsigned)grid), dim3(threads), s, args...);
}

// The run-time enums of a launcher as template arguments: f(std::integral_constant<int, V>) for the V of the list that equals v (the last one if none does)
template <int V, int... Rest, typename F>
int dispatch_int(int v, F &&f)
{
    if constexpr (sizeof...(Rest) == 0)
        return f(std::integral_constant<int, V>{});
    else
        return v == V ? f(std::integral_constant<int, V>{}) : dispatch_int<Rest...>(v, f);
}

template <typename F>
int dispatch_in(int in_dtype, F &&f) { return dispatch_int<FP8MI_F32, FP8MI_F16, FP8MI_BF16>(in_dtype, f); }

// compute units of the current device (cached per device; the dispatch heuristics scale with it)
int fp8mi_cu_count();

// launchers implemented in the .hip files (host side, internal linkage by name)
// `fmt` of the tensorwise launchers: a_format + 2 * b_format (FP8MI_FMT_*); 0 = e4m3 x e4m3.  fmt != 0 instances have OCP semantics only
// (the API layer guarantees p.nan_zero == 0): no NaN scrub, no redo pass.
int fp8mi_launch_gemv(const MMParams &p, bool fp32_only, hipStream_t s, int fmt = 0);
int fp8mi_launch_gemv_variant(const MMParams &p, int id, hipStream_t s);  // diagnostic library only
bool fp8mi_gemv_supported(const MMParams &p);
int fp8mi_launch_gemv_mx(const MMParams &p, hipStream_t s, int fmt = 0);   // 2 <= M <= 8, the vec-mat's structure
bool fp8mi_gemv_mx_supported(const MMParams &p);
int fp8mi_launch_gemv_mx_variant(const MMParams &p, int id, hipStream_t s);  // diagnostic library only
int fp8mi_launch_gemm(const MMParams &p, int variant, hipStream_t s, int fmt = 0);
int fp8mi_choose_gemm_variant(const MMParams &p);   // the tile kernel AUTO picks (host-only)
bool fp8mi_gemm_supported(const MMParams &p);
int fp8mi_launch_gemm256(const MMParams &p, int variant, hipStream_t s);   // fp8mi_gemm256.hip: whole 256x256 tiles, hand-scheduled loop
int fp8mi_launch_gemm256_fmt(const MMParams &p, int variant, hipStream_t s, int fmt);   // ... with an e5m2 operand (fmt = 1..3; variants 0 and 1000)
bool fp8mi_gemm256_supported(const MMParams &p);
int fp8mi_launch_generic(const MMParams &p, hipStream_t s, int fmt = 0);
int fp8mi_launch_generic_mxfp8(const MMParams &p, const MxScales &sc, hipStream_t s);   // any alignment; IEEE fp32 sums
int fp8mi_launch_gemm_mxfp8(const MMParams &p, const MxScales &sc, int variant, hipStream_t s);   // the ring tiles' block-scaled forms
bool fp8mi_gemm_mxfp8_supported(const MMParams &p, const MxScales &sc);
int fp8mi_choose_gemm_mxfp8_variant(const MMParams &p);   // host-only: AUTO of every block-scaled family (MXFP4: p at its byte depth K / 2)
int fp8mi_launch_generic_mxfp4(const MMParams &p, const MxScales &sc, hipStream_t s);   // p.K = logical K (elements); lda / ldb bytes
int fp8mi_launch_gemm_mxfp4(const MMParams &p, const MxScales &sc, int variant, hipStream_t s);   // p.K, lda, ldb in bytes (K / 2)
bool fp8mi_gemm_mxfp4_supported(const MMParams &p, const MxScales &sc);
// MXW4A8 (e4m3 A x e2m1 B_nk): the generic kernel counts p.K in elements; the ring tiles take p.K and ldb in W bytes (K / 2), lda in X bytes
int fp8mi_launch_generic_mxw4a8(const MMParams &p, const MxScales &sc, hipStream_t s);
int fp8mi_launch_gemm_mxw4a8(const MMParams &p, const MxScales &sc, int variant, hipStream_t s);
bool fp8mi_gemm_mxw4a8_supported(const MMParams &p, const MxScales &sc);
int fp8mi_launch_gemm_grouped_mxw4a8(const MMParams &p, const MxScales &sc, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb, int variant,
                                     hipStream_t s);
int fp8mi_launch_generic_blockwise(const MMParams &p, const BwScales &sc, hipStream_t s);   // any alignment; exact block sums in IEEE fp32
int fp8mi_launch_gemm_blockwise(const MMParams &p, const BwScales &sc, int variant, hipStream_t s);   // the ring tiles' blockwise forms
bool fp8mi_gemm_blockwise_supported(const MMParams &p, const BwScales &sc);
// the ring tiles' grouped forms (p: the whole (M_total, N, K) problem with B, scale_b and bias at expert 0; sc: nullptr, or the blockwise scales)
int fp8mi_launch_gemm_grouped(const MMParams &p, const BwScales *sc, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb, int variant,
                              hipStream_t s);
// ... and their MXFP8 / MXFP4 forms (fp4: p.K, lda, ldb and stride_b in bytes; sc.sw at expert 0, stride_sb bytes between the experts' scales)
int fp8mi_launch_gemm_grouped_mx(const MMParams &p, const MxScales &sc, bool fp4, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb,
                                 int variant, hipStream_t s);
int fp8mi_choose_gemm_grouped_variant(const MMParams &p, int G);   // host-only: AUTO of the grouped forms
int64_t fp8mi_gemm_grouped_workgroups(const MMParams &p, int G, int variant);   // host-only: the launch grid of a ring tile's grouped form (-1: no such tile)
int fp8mi_launch_skinny(const MMParams &p, hipStream_t s, int fmt = 0);
int fp8mi_launch_gemm_pc(const MMParams &p, int variant, hipStream_t s);  // diagnostic library only
bool fp8mi_skinny_supported(const MMParams &p);
