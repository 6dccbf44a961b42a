// extern "C" surface of libfp8mi.so: argument validation, kernel selection,
// error reporting.  See include/fp8mi.h for the contract of every entry point
// and the reference interface each one replaces.

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <vector>

#include "fp8mi_common.h"
#include "fp8mi_dispatch.h"
#include "fp8mi_moe_route.h"
#include "fp8mi_moe_gate.h"
#include "fp8mi_attn.h"

int fp8mi_launch_moe_gate(const void *logits, int dtype, int64_t T, int G, int64_t ld, const float *bias, int k, int scoring, int renormalize, float scale,
                          int n_group, int topk_group, int group_score, int32_t *ids, float *weights, hipStream_t s);
int fp8mi_launch_kv_cache_append(const void *k, const void *v, int dtype, int64_t T, int Hkv, int D, int64_t ld_k, int64_t ld_v, uint8_t *k_cache,
                                 uint8_t *v_cache, int64_t num_blocks, int block_size, const void *slot_mapping, int slot_bytes, const float *k_scale,
                                 const float *v_scale, int scale_head, int mode, hipStream_t s);
int fp8mi_launch_paged_attention(const void *q, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, int Hkv, int D,
                                 int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size, const int32_t *block_table,
                                 int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len, const float *k_scale, const float *v_scale,
                                 int scale_head, float softmax_scale, int splits, void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s);
int fp8mi_launch_moe_route(const void *ids, int id_bytes, int64_t n, int G, int32_t *offs, int32_t *row_of, int32_t *src_of_row, void *workspace,
                           hipStream_t s);
int fp8mi_launch_moe_scatter_quantize(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                      int64_t rows_out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k, int scale_mode,
                                      int mode, hipStream_t s);
int fp8mi_launch_moe_scatter_quantize_mx(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                         int64_t rows_out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format, hipStream_t s);
int fp8mi_launch_moe_combine(const void *y, int y_dtype, int64_t rows, int64_t N, int64_t ld_y, const int32_t *row_of, const float *weights, int64_t T,
                             int k, void *out, int out_dtype, int64_t ld_out, hipStream_t s);
int fp8mi_launch_dequant(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, hipStream_t s);
int fp8mi_launch_encode(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, int mode,
                        hipStream_t s);
int fp8mi_launch_amax(const void *in, int in_dtype, float *out, int64_t count, hipStream_t s);
int fp8mi_launch_quantize(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, int mode,
                          hipStream_t s);
int fp8mi_launch_encode_e5m2(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, hipStream_t s);
int fp8mi_launch_dequant_e5m2(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, hipStream_t s);
int fp8mi_launch_quantize_e5m2(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, hipStream_t s);
int fp8mi_launch_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, uint8_t *scales,
                             int64_t ld_s, int mx_format, hipStream_t s);
int fp8mi_launch_dequant_mx(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const uint8_t *scales, int64_t ld_s, void *out, int out_dtype,
                            int mx_format, hipStream_t s);
int fp8mi_launch_quantize_blockwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, uint8_t *out,
                                    int64_t ld_out, float *scales, int64_t s_sr, int64_t s_sk, hipStream_t s);
int fp8mi_launch_dequant_blockwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, const float *scales, int64_t s_sr,
                                   int64_t s_sk, void *out, int out_dtype, hipStream_t s);
int fp8mi_launch_quantize_rowwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, float *inv_scales,
                                  float *amax, int out_format, int mode, hipStream_t s);
int fp8mi_launch_act_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, int gated, uint8_t *out, int64_t ld_out,
                              float *scales, int64_t s_stride_row, int64_t s_stride_k, float *amax, int scale_mode, int out_format, int mode, hipStream_t s);
int fp8mi_launch_dequant_rowwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const float *scales, int in_format, void *out, int out_dtype,
                                 hipStream_t s);
int fp8mi_launch_norm_quantize(const NqArgs &a, int in_dtype, int norm, int scale_mode, int out_format, int mode, hipStream_t s);
int fp8mi_launch_act_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, int gated, uint8_t *out, int64_t ld_out,
                                 uint8_t *scales, int64_t ld_s, int mx_format, hipStream_t s);
int fp8mi_launch_norm_quantize_mx(const NqArgs &a, int in_dtype, int norm, int mx_format, hipStream_t s);

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_result(int rc, const char *what)
{
    if (rc > 0) return fail(rc, "%s: %s", what, hipGetErrorString((hipError_t)rc));
    if (rc < 0) return fail(rc, "%s: unsupported problem for the selected kernel", what);
    return 0;
}

struct ProfileState {
    std::vector<hipEvent_t> ev;  // start0, stop0, start1, stop1, ...
    int used = 0;
    bool on = false;
};
thread_local ProfileState g_prof;

bool dtype_ok(int d) { return d == FP8MI_F32 || d == FP8MI_F16 || d == FP8MI_BF16; }
bool format_ok(int f) { return f == FP8MI_FMT_E4M3 || f == FP8MI_FMT_E5M2; }
bool encode_mode_ok(int m) { return m == FP8MI_ENC_REFERENCE || m == FP8MI_ENC_RNE; }
bool act_ok(int fn) { return fn == FP8MI_ACT_NONE || fn == FP8MI_ACT_SILU || fn == FP8MI_ACT_GELU_TANH || fn == FP8MI_ACT_GELU_ERF; }

// ---- the prologue the four fp8mi_scaled_mm_* entry points share ----------------------------------------------------------------------
// Each entry point runs these steps in its own order, with its own checks between them: the order decides the return code of a call with
// two faults, so a step that sits elsewhere in one family is a separate function rather than a reordered entry point.
struct GemmCall {
    const char *fn;   // the entry point's name, for the messages
    const uint8_t *A, *B;
    void *C;
    const void *bias;
    const float *scale_result;
    int64_t M, N, K, lda, ldb, ldc;
    int out_dtype, bias_dtype, nan_mode, split_k;
    void *workspace;
    int64_t workspace_bytes;
};

int check_dims(const GemmCall &c)
{
    if (c.M < 0 || c.N < 0 || c.K < 0)
        return fail(FP8MI_E_SHAPE, "%s: negative dimension (M=%lld N=%lld K=%lld)", c.fn, (long long)c.M, (long long)c.N, (long long)c.K);
    return 0;
}

// NULL pointers, then leading dimensions.  `scales`: both scale pointers are there; they are needed whatever K is (tensorwise) or only when
// K > 0 (`scales_with_k`, the block-scaled families).  k_row: bytes of K in an operand row; lds_ok: the family's own strides hold (MX: ld_sa / ld_sb).
// k_row_a: bytes of K in a row of A where they differ from B's (MXW4A8: K against K / 2); -1: k_row
int check_pointers_and_lds(const GemmCall &c, bool scales, bool scales_with_k, int64_t k_row, bool lds_ok = true, int64_t k_row_a = -1)
{
    if (!c.C || (!scales_with_k && !scales))
        return fail(FP8MI_E_NULL, "%s: C%s must not be NULL", c.fn, scales_with_k ? "" : " / scale_a / scale_b");
    if (c.K > 0 && (!c.A || !c.B || (scales_with_k && !scales)))
        return fail(FP8MI_E_NULL, "%s: A / B%s must not be NULL when K > 0", c.fn, scales_with_k ? " / scale_a / scale_b" : "");
    if (c.lda < (k_row_a < 0 ? k_row : k_row_a) || c.ldb < k_row || c.ldc < c.N || !lds_ok)
        return fail(FP8MI_E_SHAPE, "%s: leading dimension too small (lda=%lld ldb=%lld ldc=%lld%s)", c.fn, (long long)c.lda, (long long)c.ldb,
                    (long long)c.ldc, lds_ok ? "" : "; ld_sa / ld_sb below K / 32");
    return 0;
}

int check_dtypes_and_nan_mode(const GemmCall &c)
{
    if (!dtype_ok(c.out_dtype) || (c.bias && !dtype_ok(c.bias_dtype & ~FP8MI_EPILOGUE_TRANSPOSED)))
        return fail(FP8MI_E_ENUM, "%s: unknown out_dtype / bias_dtype", c.fn);
    if ((c.nan_mode | 1) != 1) return fail(FP8MI_E_ENUM, "%s: unknown nan mode", c.fn);
    return 0;
}

// The kernel argument of an entry point that runs on the ring tiles only: AUTO, GENERIC where the entry point has a generic form, or a ring
// tile; `form` names the family in the message ("block-scaled", "grouped")
int check_ring_tile_kernel(const GemmCall &c, int kernel, const char *form, bool generic)
{
    switch (kernel) {
    case FP8MI_KERNEL_AUTO:
    case FP8MI_KERNEL_GEMM_128: case FP8MI_KERNEL_GEMM_128x64: case FP8MI_KERNEL_GEMM_64x128:
    case FP8MI_KERNEL_GEMM_64x64: case FP8MI_KERNEL_GEMM_32x64: case FP8MI_KERNEL_GEMM_32x32: case FP8MI_KERNEL_GEMM_128D:
        return 0;
    case FP8MI_KERNEL_GENERIC:
        if (generic) return 0;
        [[fallthrough]];
    case FP8MI_KERNEL_GEMV: case FP8MI_KERNEL_GEMV_FP32: case FP8MI_KERNEL_GEMV_MX: case FP8MI_KERNEL_SKINNY:
    case FP8MI_KERNEL_GEMM_256: case FP8MI_KERNEL_GEMM_256W: case FP8MI_KERNEL_GEMM_256x128W:
        return fail(FP8MI_E_UNSUPPORTED, "%s: kernel %d has no %s form", c.fn, kernel, form);
    default:
        return fail(FP8MI_E_ENUM, "%s: unknown kernel id %d", c.fn, kernel);
    }
}

// split_k, then the kernel argument of a block-scaled entry point: AUTO, GENERIC or a ring tile that has a block-scaled form
int check_split_and_block_scaled_kernel(const GemmCall &c, int kernel, const char *form)
{
    if (c.split_k < 0) return fail(FP8MI_E_ENUM, "%s: split_k must be >= 0", c.fn);
    return check_ring_tile_kernel(c, kernel, form, true);
}

// The kernels' parameters of a checked call.  k: the depth the kernel counts (MXFP4's ring tiles: bytes).  The block-scaled families pass no
// per-tensor scales: the shared epilogue's factors are then 1 (sa_row = sb_row = 0, never loaded).
MMParams mm_params(const GemmCall &c, int64_t k, const float *scale_a = nullptr, const float *scale_b = nullptr, int sa_row = 0, int sb_row = 0)
{
    MMParams p = {};
    p.A = c.A; p.B = c.B; p.C = c.C;
    p.scale_a = scale_a; p.scale_b = scale_b; p.bias = c.bias; p.scale_result = c.scale_result;
    p.M = c.M; p.N = c.N; p.K = k; p.lda = c.lda; p.ldb = c.ldb; p.ldc = c.ldc;
    p.sa_row = sa_row; p.sb_row = sb_row;
    p.out_dtype = c.out_dtype;
    p.bias_dtype = c.bias_dtype & ~FP8MI_EPILOGUE_TRANSPOSED;
    p.transposed = (c.bias_dtype & FP8MI_EPILOGUE_TRANSPOSED) ? 1 : 0;
    p.nan_zero = c.nan_mode == FP8MI_NAN_ZERO;
    p.debug = 0;
    // an unusable workspace (misaligned, smaller than the counter block): behave as if none was given
    const bool ws = c.workspace && (((uintptr_t)c.workspace) & 15u) == 0 && c.workspace_bytes >= FP8MI_WS_COUNTER_BYTES;
    p.split = ws ? c.split_k : 1;
    p.ws = ws ? (uint8_t *)c.workspace : nullptr;
    p.ws_bytes = ws ? c.workspace_bytes : 0;
    return p;
}

// The routing of a block-scaled call: a forced ring tile on a problem the ring tiles do not take (`ring` false) is an error that says what
// they need; GENERIC, and AUTO on such a problem, run the generic kernel.
template <class Ring, class Generic>
int route_block_scaled(int kernel, bool ring, const char *needs, Ring &&run_ring, Generic &&run_generic)
{
    if (kernel != FP8MI_KERNEL_AUTO && kernel != FP8MI_KERNEL_GENERIC && !ring) return fail(FP8MI_E_UNSUPPORTED, "%s", needs);
    return (kernel == FP8MI_KERNEL_GENERIC || !ring) ? run_generic() : run_ring();
}

// ---- the steps the stand-alone casts and quantisers share ---------------------------------------------------------------------------------
// As with the GEMM families, each entry point runs them in its own order, which decides the return code of a call with two faults
// (tests/golden/cast_frontend_c.json holds every pair): the flat casts end an empty call before they look at pointers and enums and report a
// NULL pointer ahead of a bad enum; the 2-D ones check sizes, leading dimensions and enums first, then the empty problem, then the pointers.
struct CastCall {
    const char *fn;       // the entry point's name, for the messages
    int64_t rows, cols;   // a flat cast: rows = 1, cols = count
};
struct EnumArg {
    bool ok;
    const char *what;
    int value;
};

int check_sizes(const CastCall &c)
{
    return c.rows < 0 || c.cols < 0 ? fail(FP8MI_E_SHAPE, "%s: negative size or count (%lld x %lld)", c.fn, (long long)c.rows, (long long)c.cols) : 0;
}
// ok: every leading dimension reaches the recipe's minimum for c.cols, and no scale stride is negative
int check_lds(const CastCall &c, bool ok, const char *detail = "")
{
    return ok ? 0 : fail(FP8MI_E_SHAPE, "%s: leading dimension too small or negative scale stride%s", c.fn, detail);
}
int check_enum(const CastCall &c, const EnumArg &e) { return e.ok ? 0 : fail(FP8MI_E_ENUM, "%s: unknown %s %d", c.fn, e.what, e.value); }
int check_pointers(const CastCall &c, bool ok) { return ok ? 0 : fail(FP8MI_E_NULL, "%s: NULL pointer", c.fn); }

// A flat cast over `count` elements: the count, the empty call (unless it launches all the same: the amax-scaled quantisers publish
// amax = 0 and inv_scale = 1), the pointers, the dtype, the encode mode - then the launch.
template <class Launch>
int flat_cast(const char *fn, int64_t count, bool empty_launches, bool pointers, const char *dtype_name, int dtype, int encode_mode, Launch &&launch)
{
    const CastCall c{fn, 1, count};
    if (int rc = check_sizes(c)) return rc;
    if (count == 0 && !empty_launches) return 0;
    if (int rc = check_pointers(c, pointers)) return rc;
    if (int rc = check_enum(c, {dtype_ok(dtype), dtype_name, dtype})) return rc;
    if (int rc = check_enum(c, {encode_mode_ok(encode_mode), "encode_mode", encode_mode})) return rc;
    return hip_result(launch(), fn);
}

// A 2-D cast: the sizes, the width the recipe refuses (width_fault: nullptr, or what is wrong with cols), the leading dimensions and scale strides,
// the enums in the order given, the empty problem, the pointers - then the launch.
template <class Launch>
int cast_2d(const char *fn, int64_t rows, int64_t cols, const char *width_fault, bool lds_ok, std::initializer_list<EnumArg> enums, bool pointers,
            Launch &&launch)
{
    const CastCall c{fn, rows, cols};
    if (int rc = check_sizes(c)) return rc;
    if (width_fault) return fail(FP8MI_E_SHAPE, "%s: cols=%lld %s", fn, (long long)cols, width_fault);
    if (int rc = check_lds(c, lds_ok)) return rc;
    for (const EnumArg &e : enums)
        if (int rc = check_enum(c, e)) return rc;
    if (rows == 0 || cols == 0) return 0;
    if (int rc = check_pointers(c, pointers)) return rc;
    return hip_result(launch(), fn);
}

// ---- the steps the six fused producers share (activation, normalisation, MoE scatter in front of the quantising tail) ---------------------
// What a call writes, as the e4m3 form and the MX form of an entry point give it.  Every check that depends on it is written once over it, so
// the two forms of a producer are one function; each producer lists the steps in its own order (DESIGN.md 5.19 has what differs).
struct QuantTarget {
    CastCall c;                    // c.rows: the rows read (the scatter forms: T tokens)
    bool mx;                       // an MX form: cols % 32, E8M0 scales ld_s apart, rows of cols / 2 bytes for e2m1
    int kind;                      // FP8MI_QSCALE_* (e4m3 forms), FP8MI_MX_* (MX forms)
    int64_t ld_out, s_sr, s_sk;    // the scales' strides; MX: s_sr = ld_s, s_sk = 0
    int out_format, encode_mode;   // e4m3 forms only
    float *amax;
    bool fp4() const { return mx && kind == FP8MI_MX_FP4; }
    // nothing to write without columns - except one float32 scale per row (FP8MI_QSCALE_ROW), which every row still publishes as 1
    bool no_columns() const { return c.cols == 0 && (mx || kind != FP8MI_QSCALE_ROW); }
    bool pointers(const void *in, const void *out, const void *scales) const { return scales && (c.cols == 0 || (in && out)); }
};

// The sizes, the width an MX recipe refuses, the leading dimensions and scale strides (own_lds: the producer's own), the enums - the producer's
// `own` (act, norm), the scale kind, in_dtype, `param` (the norm forms' param_dtype), an e4m3 form's out_format and encode mode - and the
// pairings of those that an e4m3 form does not take.
int check_quant_target(const QuantTarget &q, bool own_lds, const char *ld_detail, const EnumArg *own, int in_dtype, const EnumArg *param = nullptr)
{
    const CastCall &c = q.c;
    if (int rc = check_sizes(c)) return rc;
    if (q.mx && c.cols % 32 != 0) return fail(FP8MI_E_SHAPE, "%s: cols=%lld is not a multiple of 32", c.fn, (long long)c.cols);
    const bool scale_lds = q.mx ? q.s_sr >= c.cols / 32 : (q.s_sr >= 0 && q.s_sk >= 0);
    if (int rc = check_lds(c, own_lds && q.ld_out >= (q.fp4() ? c.cols / 2 : c.cols) && scale_lds, ld_detail)) return rc;
    const EnumArg kind = q.mx ? EnumArg{q.kind == FP8MI_MX_FP8 || q.kind == FP8MI_MX_FP4, "mx_format", q.kind}
                              : EnumArg{q.kind == FP8MI_QSCALE_ROW || q.kind == FP8MI_QSCALE_GROUP128, "scale_mode", q.kind};
    const EnumArg in{dtype_ok(in_dtype), "in_dtype", in_dtype}, fmt{q.mx || format_ok(q.out_format), "out_format", q.out_format},
        enc{q.mx || encode_mode_ok(q.encode_mode), "encode mode", q.encode_mode};
    for (const EnumArg *e : {own, &kind, &in, param, &fmt, &enc})
        if (e)
            if (int rc = check_enum(c, *e)) return rc;
    if (q.mx) return 0;
    if (q.out_format == FP8MI_FMT_E5M2 && q.encode_mode != FP8MI_ENC_RNE)
        return fail(FP8MI_E_UNSUPPORTED, "%s: e5m2 has OCP semantics only (encode_mode must be FP8MI_ENC_RNE)", c.fn);
    if (q.kind == FP8MI_QSCALE_GROUP128 && (q.out_format != FP8MI_FMT_E4M3 || q.encode_mode != FP8MI_ENC_RNE || q.amax))
        return fail(FP8MI_E_UNSUPPORTED, "%s: FP8MI_QSCALE_GROUP128 is e4m3 / FP8MI_ENC_RNE only and has no per-row amax output", c.fn);
    return 0;
}

}  // namespace

bool fp8mi_next_profile_events(hipEvent_t *start, hipEvent_t *stop)
{
    ProfileState &ps = g_prof;
    if (!ps.on || (size_t)(2 * ps.used + 1) >= ps.ev.size()) return false;
    *start = ps.ev[2 * ps.used];
    *stop = ps.ev[2 * ps.used + 1];
    ++ps.used;
    return true;
}

int fp8mi_cu_count()
{
    static int cache[64];  // 0 = not asked yet; benign race: every thread writes the same value
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cache[dev];
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return n;
}

// The kernel the automatic dispatch runs for a problem: the cheapest by the cost model of fp8mi_dispatch.h (host-only arithmetic on shapes,
// strides, alignment and the CU count; exported as fp8mi_choose_kernel, tested on the CPU against measured times).
static int choose_kernel(const MMParams &p) { return fp8mi_dispatch::choose(p, (double)fp8mi_cu_count()); }

extern "C" {

int fp8mi_profile_begin(int max_launches)
{
    if (max_launches <= 0) return fail(FP8MI_E_SHAPE, "fp8mi_profile_begin: max_launches must be positive");
    ProfileState &ps = g_prof;
    if (ps.on) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_profile_begin: a profile is already open on this thread");
    while (ps.ev.size() < (size_t)max_launches * 2) {
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return fail((int)rc, "hipEventCreate: %s", hipGetErrorString(rc));
        ps.ev.push_back(e);
    }
    ps.used = 0;
    ps.on = true;
    return 0;
}

int fp8mi_profile_end(float *ms_out, int cap)
{
    ProfileState &ps = g_prof;
    if (!ps.on) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_profile_end: no profile open on this thread");
    ps.on = false;
    const int n = ps.used;
    if (n > 0) {
        hipError_t rc = hipEventSynchronize(ps.ev[2 * (n - 1) + 1]);
        if (rc != hipSuccess) return fail((int)rc, "hipEventSynchronize: %s", hipGetErrorString(rc));
    }
    for (int i = 0; i < n && i < cap && ms_out; ++i) {
        float ms = 0.0f;
        hipError_t rc = hipEventElapsedTime(&ms, ps.ev[2 * i], ps.ev[2 * i + 1]);
        if (rc != hipSuccess) return fail((int)rc, "hipEventElapsedTime: %s", hipGetErrorString(rc));
        ms_out[i] = ms;
    }
    return n;
}

int fp8mi_version(void) { return FP8MI_VERSION; }

const char *fp8mi_last_error(void) { return g_err; }

int fp8mi_device_info(int device, fp8mi_device_info_t *out)
{
    if (!out) return fail(FP8MI_E_NULL, "fp8mi_device_info: out is NULL");
    hipDeviceProp_t pr;
    hipError_t e = hipGetDeviceProperties(&pr, device);
    if (e != hipSuccess) return fail((int)e, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    memset(out, 0, sizeof(*out));
    out->compute_units = pr.multiProcessorCount;
    out->clock_khz = pr.clockRate;
    out->memory_clock_khz = pr.memoryClockRate;
    out->memory_bus_bits = pr.memoryBusWidth;
    out->l2_bytes = pr.l2CacheSize;
    out->lds_bytes_per_cu = (int)pr.maxSharedMemoryPerMultiProcessor;
    out->wavefront_size = pr.warpSize;
    out->total_memory = (int64_t)pr.totalGlobalMem;
    strncpy(out->arch, pr.gcnArchName, sizeof(out->arch) - 1);
    strncpy(out->name, pr.name, sizeof(out->name) - 1);
    return 0;
}

int64_t fp8mi_scaled_mm_workspace_bytes(void)
{
    // counters + room for the fp32 partial tiles of every split the library takes on its own, on any of the split-capable ring tiles
    // (128x64 / 64x128: 32 KiB per workgroup; 64x64 16 KiB, 32x64 8 KiB, 32x32 4 KiB; 128x128 64 KiB): tiles x slices stays within one
    // workgroup per CU, 256 x 32 KiB at most; twice that leaves room for forced splits (split_k > 0).  A split whose partials do not fit
    // the caller's workspace is clamped to the largest slice count that does (resolve_split, fp8mi_gemm_epi.h).
    return (int64_t)FP8MI_WS_COUNTER_BYTES + 2 * 256 * (int64_t)(128 * 64 * 4);
}

int fp8mi_workspace_reset(void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!workspace) return fail(FP8MI_E_NULL, "fp8mi_workspace_reset: workspace is NULL");
    if (workspace_bytes < FP8MI_WS_COUNTER_BYTES) return fail(FP8MI_E_SHAPE, "fp8mi_workspace_reset: workspace smaller than the counter block");
    hipError_t e = hipMemsetAsync(workspace, 0, FP8MI_WS_COUNTER_BYTES, (hipStream_t)stream);
    if (e != hipSuccess) return fail((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
    return 0;
}

int fp8mi_scaled_mm_ex(const uint8_t *A, const uint8_t *B_nk, void *C, const float *scale_a, const float *scale_b,
                       const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda,
                       int64_t ldb, int64_t ldc, int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype,
                       int nan_mode, int kernel, void *stream)
{
    return fp8mi_scaled_mm_ws(A, B_nk, C, scale_a, scale_b, bias, scale_result, M, N, K, lda, ldb, ldc, scale_a_mode,
                              scale_b_mode, out_dtype, bias_dtype, nan_mode, kernel, 1, nullptr, 0, stream);
}

int fp8mi_scaled_mm_ws(const uint8_t *A, const uint8_t *B_nk, void *C, const float *scale_a, const float *scale_b,
                       const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda,
                       int64_t ldb, int64_t ldc, int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype,
                       int nan_mode, int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream)
{
    return fp8mi_scaled_mm_fmt(A, B_nk, C, scale_a, scale_b, bias, scale_result, M, N, K, lda, ldb, ldc, scale_a_mode, scale_b_mode, out_dtype,
                               bias_dtype, nan_mode, kernel, split_k, workspace, workspace_bytes, FP8MI_FMT_E4M3, FP8MI_FMT_E4M3, stream);
}

int fp8mi_scaled_mm_fmt(const uint8_t *A, const uint8_t *B_nk, void *C, const float *scale_a, const float *scale_b,
                        const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda,
                        int64_t ldb, int64_t ldc, int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype,
                        int nan_mode, int kernel, int split_k, void *workspace, int64_t workspace_bytes, int a_format, int b_format,
                        void *stream)
{
    if ((a_format | 1) != 1 || (b_format | 1) != 1)
        return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_fmt: unknown operand format (a_format=%d b_format=%d)", a_format, b_format);
    const int fmt = a_format + 2 * b_format;   // 0 = e4m3 x e4m3: every path below is fp8mi_scaled_mm_ws's
    const GemmCall c{"fp8mi_scaled_mm", A, B_nk, C, bias, scale_result, M, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, split_k,
                     workspace, workspace_bytes};
    if (int rc = check_dims(c)) return rc;
    if (M == 0 || N == 0) return 0;
    if (int rc = check_pointers_and_lds(c, scale_a && scale_b, false, K)) return rc;
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if ((scale_a_mode | 1) != 1 || (scale_b_mode | 1) != 1) return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm: unknown scale mode");
    if (fmt != 0 && nan_mode != FP8MI_NAN_PROPAGATE)
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_scaled_mm_fmt: an e5m2 operand has OCP semantics only (nan_mode must be FP8MI_NAN_PROPAGATE)");
    if (split_k < 0) return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_ws: split_k must be >= 0");

    MMParams p = mm_params(c, K, scale_a, scale_b, scale_a_mode, scale_b_mode);
#ifdef FP8MI_DIAG
    if (const char *e = getenv("FP8MI_DEBUG")) p.debug = atoi(e);   // diagnostic library only: timing-only ablation bits
#endif
    hipStream_t s = (hipStream_t)stream;

    if (kernel == FP8MI_KERNEL_AUTO) {
        kernel = choose_kernel(p);   // (every id it returns passes its own envelope check below)
        // The generic kernel is the device path of last resort (one wave per OUTPUT ELEMENT, byte loads): correct for every problem the reference
        // accepts (fp8_mps_native.py:55-60 only asks for contiguity), and orders of magnitude slower than the tile kernels.  A large problem that
        // lands on it - K, lda or ldb not a multiple of 16, or a base pointer that is not 16-byte aligned (a sliced weight view) - says so ONCE per
        // process on stderr (FP8MI_QUIET=1 silences it); the Python op layer pads such operands into aligned copies instead (fp8_mi355x_native.py).
        if (kernel == FP8MI_KERNEL_GENERIC && K > 0 && ((double)N * (double)K >= 1048576.0 || (double)M * (double)K >= 1048576.0)) {
            static std::atomic<bool> told{false};
            if (!told.exchange(true)) {
                const char *q = getenv("FP8MI_QUIET");
                if (!(q && q[0] == '1'))
                    fprintf(stderr, "[fp8mi] note: M=%lld N=%lld K=%lld (lda=%lld ldb=%lld, A %% 16 = %d, B %% 16 = %d) runs on the GENERIC kernel: the MFMA "
                                    "kernels need K, lda and ldb to be multiples of 16 and 16-byte aligned operands. Pad K with zero bytes / align the rows "
                                    "(fp8_mi355x_native.fp8_scaled_mm does so by itself). This note is printed once.\n",
                            (long long)M, (long long)N, (long long)K, (long long)lda, (long long)ldb, (int)((uintptr_t)A & 15), (int)((uintptr_t)B_nk & 15));
            }
        }
    }
    switch (kernel) {
    case FP8MI_KERNEL_GEMV:
        if (!fp8mi_gemv_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "gemv kernel needs M == 1, K %% 16 == 0, 16-byte aligned rows");
        return hip_result(fp8mi_launch_gemv(p, false, s, fmt), "gemv");
    case FP8MI_KERNEL_GEMV_MX:
        if (!fp8mi_gemv_mx_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "few-rows kernel needs 2 <= M <= 8, K <= 16384, K %% 16 == 0, 16-byte aligned rows");
        return hip_result(fp8mi_launch_gemv_mx(p, s, fmt), "gemv-mx");
    case FP8MI_KERNEL_GEMV_FP32:
        if (!fp8mi_gemv_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "gemv kernel needs M == 1, K %% 16 == 0, 16-byte aligned rows");
        return hip_result(fp8mi_launch_gemv(p, true, s, fmt), "gemv-fp32");
    case FP8MI_KERNEL_SKINNY:
        if (!fp8mi_skinny_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "skinny kernel needs 1 <= M <= 64, K %% 16 == 0, 16-byte aligned rows");
        return hip_result(fp8mi_launch_skinny(p, s, fmt), "skinny");
    case FP8MI_KERNEL_GEMM_128:
    case FP8MI_KERNEL_GEMM_128x64:
    case FP8MI_KERNEL_GEMM_256:
    case FP8MI_KERNEL_GEMM_64x128:
    case FP8MI_KERNEL_GEMM_64x64:
    case FP8MI_KERNEL_GEMM_32x64:
    case FP8MI_KERNEL_GEMM_32x32:
    case FP8MI_KERNEL_GEMM_128D:
        if (K <= 0 || !fp8mi_gemm_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "MFMA gemm kernel needs K > 0, K %% 16 == 0 and 16-byte aligned rows");
        return hip_result(fp8mi_launch_gemm(p, kernel, s, fmt), "gemm");
    case FP8MI_KERNEL_GEMM_256W:
        if (!fp8mi_gemm256_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "256x256 one-wave-per-SIMD kernel needs K >= 256 (> 256 with a K tail), N a multiple of 16 bytes of output, 16-byte aligned rows, no split-K");
        return hip_result(fmt ? fp8mi_launch_gemm256_fmt(p, 0, s, fmt) : fp8mi_launch_gemm256(p, 0, s), "gemm256");
    case FP8MI_KERNEL_GEMM_256x128W:
        if (!fp8mi_gemm256_supported(p)) return fail(FP8MI_E_UNSUPPORTED, "256x128 one-wave-per-SIMD kernel needs K >= 256 (> 256 with a K tail), N a multiple of 16 bytes of output, 16-byte aligned rows, no split-K");
        return hip_result(fmt ? fp8mi_launch_gemm256_fmt(p, 1000, s, fmt) : fp8mi_launch_gemm256(p, 1000, s), "gemm256x128");
    case FP8MI_KERNEL_GENERIC:
        return hip_result(fp8mi_launch_generic(p, s, fmt), "generic");
    default:
        if (fmt != 0) return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_fmt: unknown kernel id %d", kernel);   // (the diagnostic variants are e4m3 only)
#ifdef FP8MI_DIAG
        if (kernel >= 80 && kernel <= 119 && fp8mi_gemm256_supported(p)) return hip_result(fp8mi_launch_gemm256(p, kernel - 80, s), "gemm256-variant");
        if (kernel >= 190 && kernel <= 199 && fp8mi_gemm256_supported(p)) return hip_result(fp8mi_launch_gemm256(p, 1000 + kernel - 190, s), "gemm256x128-variant");
        if (kernel >= 70 && kernel <= 77 && fp8mi_gemv_mx_supported(p)) return hip_result(fp8mi_launch_gemv_mx_variant(p, kernel, s), "gemv-mx-variant");
        if (((kernel >= 40 && kernel <= 69) || (kernel >= 160 && kernel <= 189)) && fp8mi_gemv_supported(p)) return hip_result(fp8mi_launch_gemv_variant(p, kernel, s), "gemv-variant");
#endif
#ifdef FP8MI_DIAG  // diagnostic library only: schedule variants of the ring kernel (7..13, 30..37), the producer / consumer kernel
                   // (15..24) and its timing-only ablations (201..207)
        if (K > 0 && fp8mi_gemm_supported(p)) {
            if ((kernel >= 7 && kernel <= 13) || (kernel >= 30 && kernel <= 39) || (kernel >= 120 && kernel <= 159)) return hip_result(fp8mi_launch_gemm(p, kernel, s), "gemm-variant");
            if ((kernel >= 15 && kernel <= 29) || (kernel >= 200 && kernel < 220)) return hip_result(fp8mi_launch_gemm_pc(p, kernel, s), "gemm-pc");
        }
#endif
        return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_ex: unknown kernel id %d", kernel);
    }
}

static bool shape_args_ok(int64_t M, int64_t N, int64_t K, int out_dtype, int split_k)
{
    return M >= 0 && N >= 0 && K >= 0 && dtype_ok(out_dtype) && split_k >= 0;
}

// the scales of a shape-only question: aligned, never dereferenced
static const uintptr_t kFakeScaleA = 0x50000, kFakeScaleB = 0x60000;

static MxScales shape_only_mx_scales(int64_t K)
{
    MxScales sc;
    sc.sx = (const uint8_t *)kFakeScaleA; sc.sw = (const uint8_t *)kFakeScaleB;
    sc.ld_sx = sc.ld_sw = (K / 32 + 3) / 4 * 4;
    return sc;
}

static MMParams shape_only_params(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace, int split_k)
{
    MMParams p = {};
    p.A = (const uint8_t *)(uintptr_t)0x10000; p.B = (const uint8_t *)(uintptr_t)0x20000; p.C = (void *)(uintptr_t)0x30000;   // aligned, never dereferenced
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.out_dtype = out_dtype;
    p.nan_zero = 1;
    p.split = has_workspace ? split_k : 1;
    p.ws = has_workspace ? (uint8_t *)(uintptr_t)0x40000 : nullptr;
    p.ws_bytes = has_workspace ? fp8mi_scaled_mm_workspace_bytes() : 0;
    return p;
}

int fp8mi_choose_kernel(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace,
                        int split_k)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k)) return FP8MI_E_ENUM;
    return choose_kernel(shape_only_params(M, N, K, lda, ldb, ldc, out_dtype, has_workspace, split_k));
}

double fp8mi_predict_kernel_us(int kernel, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace,
                               int split_k, int compute_units)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k)) return -1.0;
    const MMParams p = shape_only_params(M, N, K, lda, ldb, ldc, out_dtype, has_workspace, split_k);
    return fp8mi_dispatch::predict_us(p, kernel, compute_units > 0 ? (double)compute_units : (double)fp8mi_cu_count());
}

int fp8mi_scaled_mm(const uint8_t *A, const uint8_t *B_nk, void *C, const float *scale_a, const float *scale_b,
                    const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda,
                    int64_t ldb, int64_t ldc, int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype,
                    int nan_mode, void *stream)
{
    return fp8mi_scaled_mm_ex(A, B_nk, C, scale_a, scale_b, bias, scale_result, M, N, K, lda, ldb, ldc, scale_a_mode,
                              scale_b_mode, out_dtype, bias_dtype, nan_mode, FP8MI_KERNEL_AUTO, stream);
}

int fp8mi_dequant(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, void *stream)
{
    return flat_cast("fp8mi_dequant", count, false, in && out, "out_dtype", out_dtype, FP8MI_ENC_RNE,
                     [&] { return fp8mi_launch_dequant(in, out, scale, count, out_dtype, (hipStream_t)stream); });
}

int fp8mi_dequant_f16(const uint8_t *in, void *out, const float *scale_or_null, int64_t count, int out_dtype, void *stream)
{
    return fp8mi_dequant(in, out, scale_or_null, count, out_dtype, stream);   // SURVEY.md 8(b)'s name for the same entry point
}

int fp8mi_encode(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, int encode_mode, void *stream)
{
    return flat_cast("fp8mi_encode", count, false, in && out, "in_dtype", in_dtype, encode_mode,
                     [&] { return fp8mi_launch_encode(in, in_dtype, out, prescale, count, encode_mode, (hipStream_t)stream); });
}

int fp8mi_amax(const void *in, int in_dtype, float *out, int64_t count, void *stream)
{
    return flat_cast("fp8mi_amax", count, true, out && (count == 0 || in), "in_dtype", in_dtype, FP8MI_ENC_RNE,
                     [&] { return fp8mi_launch_amax(in, in_dtype, out, count, (hipStream_t)stream); });
}

int fp8mi_quantize(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, int encode_mode, void *stream)
{
    return flat_cast("fp8mi_quantize", count, true, scales && (count == 0 || (in && out)), "in_dtype", in_dtype, encode_mode,
                     [&] { return fp8mi_launch_quantize(in, in_dtype, out, scales, count, encode_mode, (hipStream_t)stream); });
}

// ---- e5m2 casts -------------------------------------------------------------------------------------------------------

int fp8mi_encode_e5m2(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, void *stream)
{
    return flat_cast("fp8mi_encode_e5m2", count, false, in && out, "in_dtype", in_dtype, FP8MI_ENC_RNE,
                     [&] { return fp8mi_launch_encode_e5m2(in, in_dtype, out, prescale, count, (hipStream_t)stream); });
}

int fp8mi_dequant_e5m2(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, void *stream)
{
    return flat_cast("fp8mi_dequant_e5m2", count, false, in && out, "out_dtype", out_dtype, FP8MI_ENC_RNE,
                     [&] { return fp8mi_launch_dequant_e5m2(in, out, scale, count, out_dtype, (hipStream_t)stream); });
}

int fp8mi_quantize_e5m2(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, void *stream)
{
    return flat_cast("fp8mi_quantize_e5m2", count, true, scales && (count == 0 || (in && out)), "in_dtype", in_dtype, FP8MI_ENC_RNE,
                     [&] { return fp8mi_launch_quantize_e5m2(in, in_dtype, out, scales, count, (hipStream_t)stream); });
}

// ---- MXFP8 (block-scaled) entry points ------------------------------------------------------------------------------

int fp8mi_scaled_mm_mxfp8(const uint8_t *A, const uint8_t *B_nk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                          int64_t ld_sb, const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                          int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel, int split_k, void *workspace,
                          int64_t workspace_bytes, void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_mxfp8", A, B_nk, C, bias, scale_result, M, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, split_k,
                     workspace, workspace_bytes};
    if (int rc = check_dims(c)) return rc;
    if (K % 32 != 0) return fail(FP8MI_E_SHAPE, "fp8mi_scaled_mm_mxfp8: K=%lld is not a multiple of the 32-element scale block", (long long)K);
    if (M == 0 || N == 0) return 0;
    if (int rc = check_pointers_and_lds(c, scale_a && scale_b, true, K, ld_sa >= K / 32 && ld_sb >= K / 32)) return rc;
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if (int rc = check_split_and_block_scaled_kernel(c, kernel, "block-scaled")) return rc;

    const MMParams p = mm_params(c, K);
    MxScales sc;
    sc.sx = scale_a; sc.sw = scale_b; sc.ld_sx = ld_sa; sc.ld_sw = ld_sb;
    hipStream_t s = (hipStream_t)stream;
    return route_block_scaled(kernel, K > 0 && fp8mi_gemm_mxfp8_supported(p, sc),
                              "block-scaled MFMA gemm kernel needs K > 0, 16-byte aligned operand rows, ld_sa / ld_sb multiples of 4 and 4-byte aligned scales",
                              [&] { return hip_result(fp8mi_launch_gemm_mxfp8(p, sc, kernel, s), "gemm-mxfp8"); },
                              [&] { return hip_result(fp8mi_launch_generic_mxfp8(p, sc, s), "generic-mxfp8"); });
}

int fp8mi_choose_kernel_mxfp8(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace, int split_k)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k) || K % 32 != 0) return FP8MI_E_ENUM;
    const MMParams p = shape_only_params(M, N, K, lda, ldb, ldc, out_dtype, has_workspace, split_k);
    if (K == 0 || !fp8mi_gemm_mxfp8_supported(p, shape_only_mx_scales(K))) return FP8MI_KERNEL_GENERIC;
    return fp8mi_choose_gemm_mxfp8_variant(p);
}

int fp8mi_quantize_mxfp8(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out,
                         uint8_t *scales, int64_t ld_s, void *stream)
{
    return cast_2d("fp8mi_quantize_mxfp8", rows, cols, cols % 32 ? "is not a multiple of 32" : nullptr, ld_in >= cols && ld_out >= cols && ld_s >= cols / 32,
                   {{dtype_ok(in_dtype), "in_dtype", in_dtype}}, in && out && scales,
                   [&] { return fp8mi_launch_quantize_mx(in, in_dtype, rows, cols, ld_in, out, ld_out, scales, ld_s, FP8MI_MX_FP8, (hipStream_t)stream); });
}

int fp8mi_dequant_mxfp8(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const uint8_t *scales, int64_t ld_s, void *out,
                        int out_dtype, void *stream)
{
    return cast_2d("fp8mi_dequant_mxfp8", rows, cols, nullptr, ld_in >= cols && ld_s >= (cols + 31) / 32, {{dtype_ok(out_dtype), "out_dtype", out_dtype}},
                   in && scales && out,
                   [&] { return fp8mi_launch_dequant_mx(in, rows, cols, ld_in, scales, ld_s, out, out_dtype, FP8MI_MX_FP8, (hipStream_t)stream); });
}

// ---- MXFP4 (e2m1 x e2m1, block-scaled) entry points -----------------------------------------------------------------
// K, M, N, rows and cols count elements; lda, ldb, ld_out and ld_in of the fp4 data count bytes (two elements each).

int fp8mi_scaled_mm_mxfp4(const uint8_t *A, const uint8_t *B_nk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                          int64_t ld_sb, const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                          int64_t ldc, int out_dtype, int bias_dtype, int kernel, int split_k, void *workspace, int64_t workspace_bytes,
                          void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_mxfp4", A, B_nk, C, bias, scale_result, M, N, K, lda, ldb, ldc, out_dtype, bias_dtype,
                     FP8MI_NAN_PROPAGATE /* e2m1 has no NaN encoding */, split_k, workspace, workspace_bytes};
    if (int rc = check_dims(c)) return rc;
    if (K % 32 != 0) return fail(FP8MI_E_SHAPE, "fp8mi_scaled_mm_mxfp4: K=%lld is not a multiple of the 32-element scale block", (long long)K);
    if (M == 0 || N == 0) return 0;
    if (int rc = check_pointers_and_lds(c, scale_a && scale_b, true, K / 2, ld_sa >= K / 32 && ld_sb >= K / 32)) return rc;   // (lda, ldb in bytes)
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if (int rc = check_split_and_block_scaled_kernel(c, kernel, "MXFP4")) return rc;

    // the ring kernels take the operands as bytes (K / 2 per row); the generic kernel counts elements
    MMParams p = mm_params(c, K / 2);
    MxScales sc;
    sc.sx = scale_a; sc.sw = scale_b; sc.ld_sx = ld_sa; sc.ld_sw = ld_sb;
    hipStream_t s = (hipStream_t)stream;
    return route_block_scaled(kernel, K > 0 && fp8mi_gemm_mxfp4_supported(p, sc),
                              "MXFP4 MFMA gemm kernel needs K > 0, 16-byte aligned operand rows, ld_sa / ld_sb multiples of 4 and 4-byte aligned scales",
                              [&] { return hip_result(fp8mi_launch_gemm_mxfp4(p, sc, kernel, s), "gemm-mxfp4"); },
                              [&] { p.K = K; return hip_result(fp8mi_launch_generic_mxfp4(p, sc, s), "generic-mxfp4"); });
}

int fp8mi_choose_kernel_mxfp4(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace, int split_k)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k) || K % 32 != 0) return FP8MI_E_ENUM;
    const MMParams p = shape_only_params(M, N, K / 2, lda, ldb, ldc, out_dtype, has_workspace, split_k);
    if (K == 0 || !fp8mi_gemm_mxfp4_supported(p, shape_only_mx_scales(K))) return FP8MI_KERNEL_GENERIC;
    return fp8mi_choose_gemm_mxfp8_variant(p);   // the MXFP8 choice priced at the operands' byte depth K / 2
}

// ---- MXW4A8 (e4m3 A x e2m1 B_nk, block-scaled) --------------------------------------------------------
// K, M and N count elements; lda counts A's bytes (>= K), ldb B's (>= K / 2).  fp8mi_scaled_mm_mxfp8's steps in its order.

int fp8mi_scaled_mm_mxw4a8(const uint8_t *A, const uint8_t *B_nk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                           int64_t ld_sb, const void *bias, const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                           int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel, int split_k, void *workspace,
                           int64_t workspace_bytes, void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_mxw4a8", A, B_nk, C, bias, scale_result, M, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, split_k,
                     workspace, workspace_bytes};
    if (int rc = check_dims(c)) return rc;
    if (K % 32 != 0) return fail(FP8MI_E_SHAPE, "fp8mi_scaled_mm_mxw4a8: K=%lld is not a multiple of the 32-element scale block", (long long)K);
    if (M == 0 || N == 0) return 0;
    if (int rc = check_pointers_and_lds(c, scale_a && scale_b, true, K / 2, ld_sa >= K / 32 && ld_sb >= K / 32, K)) return rc;
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if (int rc = check_split_and_block_scaled_kernel(c, kernel, "MXW4A8")) return rc;

    // the ring kernels count K in W bytes (K / 2; an X row holds twice as many); the generic kernel counts elements
    MMParams p = mm_params(c, K / 2);
    MxScales sc;
    sc.sx = scale_a; sc.sw = scale_b; sc.ld_sx = ld_sa; sc.ld_sw = ld_sb;
    hipStream_t s = (hipStream_t)stream;
    return route_block_scaled(kernel, K > 0 && fp8mi_gemm_mxw4a8_supported(p, sc),
                              "MXW4A8 MFMA gemm kernel needs K > 0, 16-byte aligned operand rows, ld_sa / ld_sb multiples of 4 and 4-byte aligned scales",
                              [&] { return hip_result(fp8mi_launch_gemm_mxw4a8(p, sc, kernel, s), "gemm-mxw4a8"); },
                              [&] { p.K = K; return hip_result(fp8mi_launch_generic_mxw4a8(p, sc, s), "generic-mxw4a8"); });
}

int fp8mi_choose_kernel_mxw4a8(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int has_workspace, int split_k)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k) || K % 32 != 0) return FP8MI_E_ENUM;
    const MMParams p = shape_only_params(M, N, K / 2, lda, ldb, ldc, out_dtype, has_workspace, split_k);
    if (K == 0 || !fp8mi_gemm_mxw4a8_supported(p, shape_only_mx_scales(K))) return FP8MI_KERNEL_GENERIC;
    return fp8mi_choose_gemm_mxfp8_variant(p);   // the MXFP8 choice priced at the weights' byte depth K / 2
}

int fp8mi_quantize_mxfp4(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out,
                         uint8_t *scales, int64_t ld_s, void *stream)
{
    return cast_2d("fp8mi_quantize_mxfp4", rows, cols, cols % 32 ? "is not a multiple of 32" : nullptr,
                   ld_in >= cols && ld_out >= cols / 2 && ld_s >= cols / 32, {{dtype_ok(in_dtype), "in_dtype", in_dtype}}, in && out && scales,
                   [&] { return fp8mi_launch_quantize_mx(in, in_dtype, rows, cols, ld_in, out, ld_out, scales, ld_s, FP8MI_MX_FP4, (hipStream_t)stream); });
}

int fp8mi_dequant_mxfp4(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const uint8_t *scales, int64_t ld_s, void *out,
                        int out_dtype, void *stream)
{
    return cast_2d("fp8mi_dequant_mxfp4", rows, cols, cols % 2 ? "is odd (two elements per byte)" : nullptr, ld_in >= cols / 2 && ld_s >= (cols + 31) / 32,
                   {{dtype_ok(out_dtype), "out_dtype", out_dtype}}, in && scales && out,
                   [&] { return fp8mi_launch_dequant_mx(in, rows, cols, ld_in, scales, ld_s, out, out_dtype, FP8MI_MX_FP4, (hipStream_t)stream); });
}

// ---- blockwise (fp32 scale per 128 k of a row or a 128-row block) entry points ----------------------------------------

static bool block_ok(int b) { return b == FP8MI_BLOCK_1 || b == FP8MI_BLOCK_128; }

static BwScales bw_scales(const float *sa, int64_t sa_sr, int64_t sa_sk, int block_a, const float *sb, int64_t sb_sr, int64_t sb_sk, int block_b,
                          int64_t K)
{
    BwScales sc;
    sc.sa = sa; sc.sb = sb;
    sc.sa_sr = sa_sr; sc.sa_sk = sa_sk; sc.sb_sr = sb_sr; sc.sb_sk = sb_sk;
    sc.nkb = (K + 127) / 128;
    sc.sh_a = block_a == FP8MI_BLOCK_128 ? 7 : 0;
    sc.sh_b = block_b == FP8MI_BLOCK_128 ? 7 : 0;
    return sc;
}

int fp8mi_scaled_mm_blockwise(const uint8_t *A, const uint8_t *B_nk, void *C, const float *scale_a, int64_t sa_stride_row, int64_t sa_stride_k,
                              int block_a, const float *scale_b, int64_t sb_stride_row, int64_t sb_stride_k, int block_b, const void *bias,
                              const float *scale_result, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                              int bias_dtype, int nan_mode, int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_blockwise", A, B_nk, C, bias, scale_result, M, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, split_k,
                     workspace, workspace_bytes};
    if (int rc = check_dims(c)) return rc;
    if (sa_stride_row < 0 || sa_stride_k < 0 || sb_stride_row < 0 || sb_stride_k < 0)
        return fail(FP8MI_E_SHAPE, "fp8mi_scaled_mm_blockwise: negative scale stride");
    if (!block_ok(block_a) || !block_ok(block_b))
        return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_blockwise: block_a / block_b must be 1 or 128 (got %d, %d)", block_a, block_b);
    if (M == 0 || N == 0) return 0;
    if (int rc = check_pointers_and_lds(c, scale_a && scale_b, true, K)) return rc;
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if (int rc = check_split_and_block_scaled_kernel(c, kernel, "blockwise")) return rc;

    const MMParams p = mm_params(c, K);
    const BwScales sc = bw_scales(scale_a, sa_stride_row, sa_stride_k, block_a, scale_b, sb_stride_row, sb_stride_k, block_b, K);
    hipStream_t s = (hipStream_t)stream;
    return route_block_scaled(kernel, K > 0 && fp8mi_gemm_blockwise_supported(p, sc),
                              "blockwise MFMA gemm kernel needs K > 0, K % 16 == 0, 16-byte aligned operand rows, 4-byte aligned scales and scale extents below 2 GiB",
                              [&] { return hip_result(fp8mi_launch_gemm_blockwise(p, sc, kernel, s), "gemm-blockwise"); },
                              [&] { return hip_result(fp8mi_launch_generic_blockwise(p, sc, s), "generic-blockwise"); });
}

int fp8mi_choose_kernel_blockwise(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, int block_a, int block_b,
                                  int has_workspace, int split_k)
{
    if (!shape_args_ok(M, N, K, out_dtype, split_k) || !block_ok(block_a) || !block_ok(block_b)) return FP8MI_E_ENUM;
    const MMParams p = shape_only_params(M, N, K, lda, ldb, ldc, out_dtype, has_workspace, split_k);
    // torch's outer-dim-major layout: (rows, K/128) with stride (1, rows)
    const BwScales sc = bw_scales((const float *)kFakeScaleA, 1, (M + block_a - 1) / block_a, block_a, (const float *)kFakeScaleB, 1,
                                  (N + block_b - 1) / block_b, block_b, K);
    if (K == 0 || M == 0 || N == 0 || !fp8mi_gemm_blockwise_supported(p, sc)) return FP8MI_KERNEL_GENERIC;
    return fp8mi_choose_gemm_mxfp8_variant(p);
}

// ---- grouped (MoE) entry points: one launch over rows sorted by expert ---------------------------------------------

// What the two grouped entry points check alike, in the GemmCall order (c.M is M_total); `scales`: both scale pointers are there.
// Returns 1 for the no-op (M_total = 0 or N = 0), 0 to go on, a negative code otherwise.
// k_row: bytes of K in an operand row (-1: c.K); lds_ok: the family's own strides hold (MX: ld_sa / ld_sb).
// k_row_a: bytes of K in a row of A where they differ from B's (MXW4A8); -1: k_row
static int check_grouped(const GemmCall &c, bool scales, const int32_t *offs, int G, int64_t stride_b, int kernel, int64_t k_row = -1, bool lds_ok = true,
                         int64_t k_row_a = -1)
{
    if (k_row < 0) k_row = c.K;
    if (int rc = check_dims(c)) return rc;
    if (G < 1) return fail(FP8MI_E_SHAPE, "%s: G=%d groups; at least one is needed", c.fn, G);
    if (stride_b < 0) return fail(FP8MI_E_SHAPE, "%s: negative stride_b", c.fn);
    if (c.M == 0 || c.N == 0) return 1;
    if (int rc = check_pointers_and_lds(c, scales, false, k_row, lds_ok, k_row_a)) return rc;
    if (!offs) return fail(FP8MI_E_NULL, "%s: offs must not be NULL", c.fn);
    if (stride_b < (c.N - 1) * c.ldb + k_row)
        return fail(FP8MI_E_SHAPE, "%s: stride_b=%lld is smaller than one expert's (N, K) rows", c.fn, (long long)stride_b);
    if (int rc = check_dtypes_and_nan_mode(c)) return rc;
    if (int rc = check_ring_tile_kernel(c, kernel, "grouped", false)) return rc;
    if (c.bias_dtype & FP8MI_EPILOGUE_TRANSPOSED)
        return fail(FP8MI_E_UNSUPPORTED, "%s: bias_dtype carries FP8MI_EPILOGUE_TRANSPOSED, which the grouped forms do not have", c.fn);
    if (G > 1024) return fail(FP8MI_E_UNSUPPORTED, "%s: G=%d groups; at most 1024", c.fn, G);
    if (c.K == 0) return fail(FP8MI_E_UNSUPPORTED, "%s: K = 0 (the grouped forms run on the ring tiles only)", c.fn);
    return 0;
}

// The ring tiles' conditions on the grouped operands, then AUTO and the slot grid of the resolved tile
static int check_grouped_ring(const char *fn, const MMParams &p, int G, int64_t stride_b, int &kernel)
{
    if (!fp8mi_gemm_supported(p) || (stride_b % 16) != 0)
        return fail(FP8MI_E_UNSUPPORTED, "%s: the ring tiles need K, lda, ldb and stride_b multiples of 16, 16-byte aligned A / B_gnk, lda and ldb below 2^22", fn);
    if (kernel == FP8MI_KERNEL_AUTO) kernel = fp8mi_choose_gemm_grouped_variant(p, G);
    const int64_t wgs = fp8mi_gemm_grouped_workgroups(p, G, kernel);
    if (wgs < 0 || wgs > 0x7FFFFFFF)
        return fail(FP8MI_E_UNSUPPORTED, "%s: the slot grid (M_total / BM + G m-tile slots x n-tiles) of M_total=%lld G=%d N=%lld on kernel %d exceeds 2^31 - 1 workgroups",
                    fn, (long long)p.M, G, (long long)p.N, kernel);
    return 0;
}

int fp8mi_scaled_mm_grouped(const uint8_t *A, const uint8_t *B_gnk, void *C, const float *scale_a, const float *scale_b, const void *bias,
                            const float *scale_result, const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                            int64_t stride_b, int64_t ldc, int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype, int nan_mode, int kernel,
                            void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_grouped", A, B_gnk, C, bias, scale_result, M_total, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, 1, nullptr, 0};
    if (int rc = check_grouped(c, scale_a && scale_b, offs, G, stride_b, kernel)) return rc < 0 ? rc : 0;
    if ((scale_a_mode | 1) != 1 || (scale_b_mode | 1) != 1) return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_grouped: unknown scale mode");
    const MMParams p = mm_params(c, K, scale_a, scale_b, scale_a_mode, scale_b_mode);
    if (int rc = check_grouped_ring(c.fn, p, G, stride_b, kernel)) return rc;
    return hip_result(fp8mi_launch_gemm_grouped(p, nullptr, offs, G, stride_b, 0, kernel, (hipStream_t)stream), "gemm-grouped");
}

int fp8mi_scaled_mm_grouped_blockwise(const uint8_t *A, const uint8_t *B_gnk, void *C, const float *scale_a, int64_t sa_stride_row, int64_t sa_stride_k,
                                      int block_a, const float *scale_b, int64_t sb_stride_row, int64_t sb_stride_k, int64_t sb_stride_expert, int block_b,
                                      const void *bias, const float *scale_result, const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K,
                                      int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel,
                                      void *stream)
{
    const GemmCall c{"fp8mi_scaled_mm_grouped_blockwise", A, B_gnk, C, bias, scale_result, M_total, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode,
                     1, nullptr, 0};
    if (int rc = check_dims(c)) return rc;
    if (sa_stride_row < 0 || sa_stride_k < 0 || sb_stride_row < 0 || sb_stride_k < 0 || sb_stride_expert < 0)
        return fail(FP8MI_E_SHAPE, "fp8mi_scaled_mm_grouped_blockwise: negative scale stride");
    if (!block_ok(block_a) || !block_ok(block_b))
        return fail(FP8MI_E_ENUM, "fp8mi_scaled_mm_grouped_blockwise: block_a / block_b must be 1 or 128 (got %d, %d)", block_a, block_b);
    if (int rc = check_grouped(c, scale_a && scale_b, offs, G, stride_b, kernel)) return rc < 0 ? rc : 0;
    if (block_a != FP8MI_BLOCK_1)
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_scaled_mm_grouped_blockwise: block_a must be FP8MI_BLOCK_1 (group starts are not 128-aligned)");
    const MMParams p = mm_params(c, K);
    const BwScales sc = bw_scales(scale_a, sa_stride_row, sa_stride_k, block_a, scale_b, sb_stride_row, sb_stride_k, block_b, K);
    if (int rc = check_grouped_ring(c.fn, p, G, stride_b, kernel)) return rc;
    if (!fp8mi_gemm_blockwise_supported(p, sc))
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_scaled_mm_grouped_blockwise: the ring tiles need 4-byte aligned scales and scale extents below 2 GiB");
    return hip_result(fp8mi_launch_gemm_grouped(p, &sc, offs, G, stride_b, sb_stride_expert, kernel, (hipStream_t)stream), "gemm-grouped-blockwise");
}

// The two grouped choosers.  k_row: the operands' byte depth (MXFP4: K / 2), which is what the cost model prices.
static int choose_kernel_grouped(bool args_ok, int G, int64_t M_total, int64_t N, int64_t K, int64_t k_row, int64_t lda, int64_t ldb, int64_t ldc,
                                 int out_dtype)
{
    if (!shape_args_ok(M_total, N, K, out_dtype, 1) || G < 1 || !args_ok) return FP8MI_E_ENUM;
    const MMParams p = shape_only_params(M_total, N, k_row, lda, ldb, ldc, out_dtype, 0, 1);
    if (G > 1024 || K == 0 || M_total == 0 || N == 0 || !fp8mi_gemm_supported(p)) return FP8MI_E_UNSUPPORTED;
    return fp8mi_choose_gemm_grouped_variant(p, G);
}

int fp8mi_choose_kernel_grouped(int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype)
{
    return choose_kernel_grouped(true, G, M_total, N, K, K, lda, ldb, ldc, out_dtype);
}

// ---- grouped MXFP8 / MXFP4: fp8mi_scaled_mm_grouped with E8M0 block scales applied inside the MFMAs ------------------
// fp4: K counts elements; lda, ldb and stride_b count bytes (two elements each), as in fp8mi_scaled_mm_mxfp4.
// w4a8 (fp4 is then true of B alone): lda counts A's e4m3 bytes, as in fp8mi_scaled_mm_mxw4a8.
static int scaled_mm_grouped_mx(const char *fn, bool fp4, bool w4a8, const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa,
                                const uint8_t *scale_b, int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result,
                                const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b,
                                int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel, void *stream)
{
    const GemmCall c{fn, A, B_gnk, C, bias, scale_result, M_total, N, K, lda, ldb, ldc, out_dtype, bias_dtype, nan_mode, 1, nullptr, 0};
    if (int rc = check_dims(c)) return rc;
    if (K % 32 != 0) return fail(FP8MI_E_SHAPE, "%s: K=%lld is not a multiple of the 32-element scale block", fn, (long long)K);
    if (stride_sb < 0) return fail(FP8MI_E_SHAPE, "%s: negative stride_sb", fn);
    const int64_t k_row = fp4 ? K / 2 : K, nb = K / 32;
    if (int rc = check_grouped(c, scale_a && scale_b, offs, G, stride_b, kernel, k_row, ld_sa >= nb && ld_sb >= nb, w4a8 ? K : -1)) return rc < 0 ? rc : 0;
    if (stride_sb < (N - 1) * ld_sb + nb)
        return fail(FP8MI_E_SHAPE, "%s: stride_sb=%lld is smaller than one expert's (N, K/32) scale rows", fn, (long long)stride_sb);
    MMParams p = mm_params(c, k_row);
    MxScales sc;
    sc.sx = scale_a; sc.sw = scale_b; sc.ld_sx = ld_sa; sc.ld_sw = ld_sb;
    if ((ld_sa % 4) != 0 || (ld_sb % 4) != 0 || (stride_sb % 4) != 0 || (((uintptr_t)scale_a | (uintptr_t)scale_b) & 3u) != 0)
        return fail(FP8MI_E_UNSUPPORTED, "%s: the ring tiles need ld_sa, ld_sb and stride_sb multiples of 4 and 4-byte aligned scales "
                                         "(ld_sa=%lld ld_sb=%lld stride_sb=%lld)", fn, (long long)ld_sa, (long long)ld_sb, (long long)stride_sb);
    if (int rc = check_grouped_ring(fn, p, G, stride_b, kernel)) return rc;
    if (w4a8) return hip_result(fp8mi_launch_gemm_grouped_mxw4a8(p, sc, offs, G, stride_b, stride_sb, kernel, (hipStream_t)stream), "gemm-grouped-mxw4a8");
    return hip_result(fp8mi_launch_gemm_grouped_mx(p, sc, fp4, offs, G, stride_b, stride_sb, kernel, (hipStream_t)stream),
                      fp4 ? "gemm-grouped-mxfp4" : "gemm-grouped-mxfp8");
}

int fp8mi_scaled_mm_grouped_mxfp8(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                                  int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result, const int32_t *offs, int G,
                                  int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc, int out_dtype,
                                  int bias_dtype, int nan_mode, int kernel, void *stream)
{
    return scaled_mm_grouped_mx("fp8mi_scaled_mm_grouped_mxfp8", false, false, A, B_gnk, C, scale_a, ld_sa, scale_b, ld_sb, stride_sb, bias, scale_result, offs, G,
                                M_total, N, K, lda, ldb, stride_b, ldc, out_dtype, bias_dtype, nan_mode, kernel, stream);
}

int fp8mi_scaled_mm_grouped_mxfp4(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                                  int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result, const int32_t *offs, int G,
                                  int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc, int out_dtype,
                                  int bias_dtype, int kernel, void *stream)
{
    return scaled_mm_grouped_mx("fp8mi_scaled_mm_grouped_mxfp4", true, false, A, B_gnk, C, scale_a, ld_sa, scale_b, ld_sb, stride_sb, bias, scale_result, offs, G,
                                M_total, N, K, lda, ldb, stride_b, ldc, out_dtype, bias_dtype, FP8MI_NAN_PROPAGATE /* e2m1 has no NaN encoding */, kernel,
                                stream);
}

int fp8mi_scaled_mm_grouped_mxw4a8(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b,
                                   int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result, const int32_t *offs, int G,
                                   int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc, int out_dtype,
                                   int bias_dtype, int nan_mode, int kernel, void *stream)
{
    return scaled_mm_grouped_mx("fp8mi_scaled_mm_grouped_mxw4a8", true, true, A, B_gnk, C, scale_a, ld_sa, scale_b, ld_sb, stride_sb, bias, scale_result, offs,
                                G, M_total, N, K, lda, ldb, stride_b, ldc, out_dtype, bias_dtype, nan_mode, kernel, stream);
}

// priced at the weights' byte depth K / 2; fp8mi_gemm_supported sees lda and ldb as they are (each a multiple of 16)
int fp8mi_choose_kernel_grouped_mxw4a8(int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype)
{
    return choose_kernel_grouped(K % 32 == 0, G, M_total, N, K, K / 2, lda, ldb, ldc, out_dtype);
}

int fp8mi_choose_kernel_grouped_mx(int mx_format, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype)
{
    return choose_kernel_grouped(K % 32 == 0 && (mx_format == FP8MI_MX_FP8 || mx_format == FP8MI_MX_FP4), G, M_total, N, K,
                                 mx_format == FP8MI_MX_FP4 ? K / 2 : K, lda, ldb, ldc, out_dtype);
}

int fp8mi_quantize_blockwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, uint8_t *out, int64_t ld_out,
                             float *scales, int64_t s_stride_row, int64_t s_stride_k, void *stream)
{
    return cast_2d("fp8mi_quantize_blockwise", rows, cols, nullptr, ld_in >= cols && ld_out >= cols && s_stride_row >= 0 && s_stride_k >= 0,
                   {{block_ok(block_rows), "block_rows (1 or 128)", block_rows}, {dtype_ok(in_dtype), "in_dtype", in_dtype}}, in && out && scales, [&] {
                       return fp8mi_launch_quantize_blockwise(in, in_dtype, rows, cols, ld_in, block_rows, out, ld_out, scales, s_stride_row, s_stride_k,
                                                              (hipStream_t)stream);
                   });
}

int fp8mi_dequant_blockwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, int block_rows, const float *scales, int64_t s_stride_row,
                            int64_t s_stride_k, void *out, int out_dtype, void *stream)
{
    return cast_2d("fp8mi_dequant_blockwise", rows, cols, nullptr, ld_in >= cols && s_stride_row >= 0 && s_stride_k >= 0,
                   {{block_ok(block_rows), "block_rows (1 or 128)", block_rows}, {dtype_ok(out_dtype), "out_dtype", out_dtype}}, in && scales && out, [&] {
                       return fp8mi_launch_dequant_blockwise(in, rows, cols, ld_in, block_rows, scales, s_stride_row, s_stride_k, out, out_dtype,
                                                             (hipStream_t)stream);
                   });
}

// ---- per-row dynamic quantisation (fp8mi_rowwise.hip) ---------------------------------------------------------------------------
int fp8mi_quantize_rowwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, uint8_t *out, int64_t ld_out, float *inv_scales,
                           float *amax, int out_format, int encode_mode, void *stream)
{
    // its own order of the steps: an unsupported pair of enums behind the enums, and cols == 0 launches (every row publishes inv_scale = 1 and amax = 0)
    const CastCall c{"fp8mi_quantize_rowwise", rows, cols};
    if (int rc = check_sizes(c)) return rc;
    if (int rc = check_lds(c, ld_in >= cols && ld_out >= cols)) return rc;
    for (const EnumArg &e : {EnumArg{dtype_ok(in_dtype), "in_dtype", in_dtype}, EnumArg{format_ok(out_format), "out_format", out_format},
                             EnumArg{encode_mode_ok(encode_mode), "encode_mode", encode_mode}})
        if (int rc = check_enum(c, e)) return rc;
    if (out_format == FP8MI_FMT_E5M2 && encode_mode != FP8MI_ENC_RNE)
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_quantize_rowwise: e5m2 has OCP semantics only (encode_mode must be FP8MI_ENC_RNE)");
    if (rows == 0) return 0;
    if (int rc = check_pointers(c, inv_scales && (cols == 0 || (in && out)))) return rc;
    return hip_result(fp8mi_launch_quantize_rowwise(in, in_dtype, rows, cols, ld_in, out, ld_out, inv_scales, amax, out_format, encode_mode,
                                                    (hipStream_t)stream), c.fn);
}

int fp8mi_dequant_rowwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const float *scales, int in_format, void *out, int out_dtype,
                          void *stream)
{
    return cast_2d("fp8mi_dequant_rowwise", rows, cols, nullptr, ld_in >= cols, {{format_ok(in_format), "in_format", in_format}, {dtype_ok(out_dtype), "out_dtype", out_dtype}},
                   in && scales && out,
                   [&] { return fp8mi_launch_dequant_rowwise(in, rows, cols, ld_in, scales, in_format, out, out_dtype, (hipStream_t)stream); });
}

// ---- fused activation (+ gate product) + quantisation, e4m3 and MXFP8 / MXFP4 output (fp8mi_actquant.hip) ------------------------------------
static int act_quantize(const QuantTarget &q, const void *in, int in_dtype, int64_t ld_in, int act, uint8_t *out, void *scales, void *stream)
{
    const CastCall &c = q.c;
    const int gated = (act & FP8MI_ACT_GATED) != 0, fn = act & ~FP8MI_ACT_GATED;
    const EnumArg act_arg{act_ok(fn), "act", act};
    if (int rc = check_quant_target(q, ld_in >= (gated ? 2 * c.cols : c.cols), gated ? " (gated: the input has 2 cols columns)" : "", &act_arg, in_dtype))
        return rc;
    if (c.rows == 0 || q.no_columns()) return 0;
    if (int rc = check_pointers(c, q.pointers(in, out, scales))) return rc;
    hipStream_t s = (hipStream_t)stream;
    return hip_result(q.mx ? fp8mi_launch_act_quantize_mx(in, in_dtype, c.rows, c.cols, ld_in, fn, gated, out, q.ld_out, (uint8_t *)scales, q.s_sr, q.kind, s)
                           : fp8mi_launch_act_quantize(in, in_dtype, c.rows, c.cols, ld_in, fn, gated, out, q.ld_out, (float *)scales, q.s_sr, q.s_sk, q.amax,
                                                       q.kind, q.out_format, q.encode_mode, s),
                      c.fn);
}

int fp8mi_act_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, uint8_t *out, int64_t ld_out, float *scales,
                       int64_t s_stride_row, int64_t s_stride_k, float *amax, int scale_mode, int out_format, int encode_mode, void *stream)
{
    return act_quantize({{"fp8mi_act_quantize", rows, cols}, false, scale_mode, ld_out, s_stride_row, s_stride_k, out_format, encode_mode, amax}, in,
                        in_dtype, ld_in, act, out, scales, stream);
}

int fp8mi_act_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act, uint8_t *out, int64_t ld_out, uint8_t *scales,
                          int64_t ld_s, int mx_format, void *stream)
{
    return act_quantize({{"fp8mi_act_quantize_mx", rows, cols}, true, mx_format, ld_out, ld_s, 0, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, nullptr}, in, in_dtype,
                        ld_in, act, out, scales, stream);
}

// ---- fused RMSNorm / LayerNorm + quantisation, e4m3 and MXFP8 / MXFP4 output (fp8mi_normquant.hip) ----------------------------------------
// a: the kernels' arguments as the entry point received them (a.q from the QuantTarget; the MX launcher adds the scale flags)
static int norm_quantize(const QuantTarget &q, const NqArgs &a, int in_dtype, int norm, void *stream)
{
    const CastCall &c = q.c;
    const bool mod = a.mod_scale || a.mod_shift, res = a.residual || a.h_out;
    if (mod && a.rows_per_mod < 1) return fail(FP8MI_E_SHAPE, "%s: rows_per_mod must be at least 1 (got %lld)", c.fn, (long long)a.rows_per_mod);
    const EnumArg norm_arg{norm == FP8MI_NORM_RMS || norm == FP8MI_NORM_LAYER, "norm", norm}, param{dtype_ok(a.param_dtype), "param_dtype", a.param_dtype};
    if (int rc = check_quant_target(q, a.ld_in >= c.cols && (!res || (a.ld_res >= c.cols && a.ld_h >= c.cols)) && (!mod || a.ld_mod >= c.cols),
                                    "", &norm_arg, in_dtype, &param))
        return rc;
    if (a.param_dtype != in_dtype && a.param_dtype != FP8MI_F32)
        return fail(FP8MI_E_UNSUPPORTED, "%s: param_dtype must be in_dtype or FP8MI_F32 (got %d with in_dtype %d)", c.fn, a.param_dtype, in_dtype);
    if (norm == FP8MI_NORM_RMS && a.mean_out) return fail(FP8MI_E_UNSUPPORTED, "%s: FP8MI_NORM_RMS has no mean (mean_out must be NULL)", c.fn);
    if (c.rows == 0) return 0;
    // its own order: the pointers that come in pairs are looked at for a call without columns too
    if ((a.mod_scale == nullptr) != (a.mod_shift == nullptr)) return fail(FP8MI_E_NULL, "%s: mod_scale and mod_shift come together (one is NULL)", c.fn);
    if ((a.residual == nullptr) != (a.h_out == nullptr)) return fail(FP8MI_E_NULL, "%s: residual and h_out come together (one is NULL)", c.fn);
    if (q.no_columns()) return 0;
    if (int rc = check_pointers(c, q.pointers(a.in, a.q.out, a.q.scales))) return rc;
    hipStream_t s = (hipStream_t)stream;
    return hip_result(q.mx ? fp8mi_launch_norm_quantize_mx(a, in_dtype, norm, q.kind, s)
                           : fp8mi_launch_norm_quantize(a, in_dtype, norm, q.kind, q.out_format, q.encode_mode, s), c.fn);
}

int fp8mi_norm_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int norm, float eps, const void *weight, const void *bias,
                        const void *mod_scale, const void *mod_shift, int64_t ld_mod, int64_t rows_per_mod, int param_dtype, const void *residual,
                        int64_t ld_res, void *h_out, int64_t ld_h, uint8_t *out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k,
                        float *amax, int scale_mode, int out_format, int encode_mode, float *mean_out, float *rstd_out, void *stream)
{
    return norm_quantize({{"fp8mi_norm_quantize", rows, cols}, false, scale_mode, ld_out, s_stride_row, s_stride_k, out_format, encode_mode, amax},
                         {in, rows, cols, ld_in, eps, weight, bias, mod_scale, mod_shift, ld_mod, rows_per_mod, param_dtype, residual, ld_res, h_out, ld_h,
                          {out, ld_out, scales, s_stride_row, s_stride_k, 0, amax}, mean_out, rstd_out},
                         in_dtype, norm, stream);
}

int fp8mi_norm_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int norm, float eps, const void *weight, const void *bias,
                           const void *mod_scale, const void *mod_shift, int64_t ld_mod, int64_t rows_per_mod, int param_dtype, const void *residual,
                           int64_t ld_res, void *h_out, int64_t ld_h, uint8_t *out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format,
                           float *mean_out, float *rstd_out, void *stream)
{
    return norm_quantize({{"fp8mi_norm_quantize_mx", rows, cols}, true, mx_format, ld_out, ld_s, 0, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, nullptr},
                         {in, rows, cols, ld_in, eps, weight, bias, mod_scale, mod_shift, ld_mod, rows_per_mod, param_dtype, residual, ld_res, h_out, ld_h,
                          {out, ld_out, scales, ld_s, 0, 0, nullptr}, mean_out, rstd_out},
                         in_dtype, norm, stream);
}

// ---- MoE routing: expert sort, scatter-quantise, combine (fp8mi_moe.hip) ------------------------------------------------------------
static int check_route_sizes(const char *fn, int64_t n, int G)
{
    if (n < 0) return fail(FP8MI_E_SHAPE, "%s: negative size (n=%lld)", fn, (long long)n);
    if (G < 1) return fail(FP8MI_E_SHAPE, "%s: G=%d experts; at least one is needed", fn, G);
    if (G > kMoeRouteMaxExperts) return fail(FP8MI_E_UNSUPPORTED, "%s: G=%d experts; at most %d are supported", fn, G, kMoeRouteMaxExperts);
    if (n > 0x7FFFFFFFll) return fail(FP8MI_E_UNSUPPORTED, "%s: n=%lld assignments; rows are int32", fn, (long long)n);
    return 0;
}

int64_t fp8mi_moe_route_workspace_bytes(int64_t n, int G)
{
    if (const int rc = check_route_sizes("fp8mi_moe_route_workspace_bytes", n, G)) return rc;
    return fp8mi_moe_route_ws_bytes(n, G);
}

int fp8mi_moe_route(const void *ids, int id_bytes, int64_t n, int G, int32_t *offs, int32_t *row_of, int32_t *src_of_row, void *workspace,
                    int64_t workspace_bytes, void *stream)
{
    if (const int rc = check_route_sizes("fp8mi_moe_route", n, G)) return rc;
    if (id_bytes != 4 && id_bytes != 8) return fail(FP8MI_E_ENUM, "fp8mi_moe_route: ids of %d bytes; int32 (4) or int64 (8) are taken", id_bytes);
    if (workspace_bytes < 0) return fail(FP8MI_E_SHAPE, "fp8mi_moe_route: negative workspace_bytes");
    if (n == 0) return 0;
    if (!ids || !offs || !row_of) return fail(FP8MI_E_NULL, "fp8mi_moe_route: NULL pointer");
    const int64_t need = fp8mi_moe_route_ws_bytes(n, G);
    if (need > 0 && !workspace) return fail(FP8MI_E_NULL, "fp8mi_moe_route: NULL workspace (n=%lld needs %lld bytes)", (long long)n, (long long)need);
    if (workspace_bytes < need)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_route: workspace of %lld bytes; n=%lld G=%d needs %lld (fp8mi_moe_route_workspace_bytes)",
                    (long long)workspace_bytes, (long long)n, G, (long long)need);
    if (((uintptr_t)ids & (uintptr_t)(id_bytes - 1)) || (((uintptr_t)offs | (uintptr_t)row_of | (uintptr_t)src_of_row | (uintptr_t)workspace) & 3u))
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_route: ids, offs, row_of, src_of_row and the workspace must be aligned to their element size");
    return hip_result(fp8mi_launch_moe_route(ids, id_bytes, n, G, offs, row_of, src_of_row, workspace, (hipStream_t)stream), "moe-route");
}

// the scatter-quantise, e4m3 and MXFP8 / MXFP4 output; q.c.rows: T.  Its own order: the cols envelope behind the enums and the pairings
static int moe_scatter_quantize(const QuantTarget &q, const void *in, int in_dtype, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                int64_t rows_out, void *scales, void *stream)
{
    const CastCall &c = q.c;
    if (k < 0 || rows_out < 0) return fail(FP8MI_E_SHAPE, "%s: negative size (k=%d rows_out=%lld)", c.fn, k, (long long)rows_out);
    if (int rc = check_quant_target(q, ld_in >= c.cols, "", nullptr, in_dtype)) return rc;
    if (q.out_format != FP8MI_FMT_E4M3) return fail(FP8MI_E_UNSUPPORTED, "%s: e4m3 only (there is no grouped GEMM that takes e5m2)", c.fn);
    if ((!q.mx && c.cols % 16 != 0) || c.cols > 16384)
        return fail(FP8MI_E_UNSUPPORTED, "%s: cols=%lld; a multiple of %d up to 16384 is needed (there is no generic form)", c.fn, (long long)c.cols,
                    q.mx ? 32 : 16);
    if (c.rows == 0 || k == 0 || q.no_columns()) return 0;
    if (int rc = check_pointers(c, row_of && q.pointers(in, out, scales))) return rc;
    const int64_t esz = in_dtype == FP8MI_F32 ? 4 : 2;
    const uintptr_t oal = q.fp4() ? 4 : 8;   // the widest store of a piece: 8 e4m3 bytes, 8 e2m1 nibbles
    if (((uintptr_t)in & 15u) || ((uintptr_t)out & (oal - 1)) || ((uintptr_t)row_of & 3u) || (!q.mx && ((uintptr_t)scales & 3u)) ||
        (c.rows > 1 && (ld_in * esz) % 16 != 0) || (rows_out > 1 && q.ld_out % (int64_t)oal != 0))
        return fail(FP8MI_E_UNSUPPORTED, "%s: in and ld_in must allow 16-byte loads, out and ld_out %d-byte stores (ld_in=%lld elements of %lld bytes, "
                                         "ld_out=%lld)", c.fn, (int)oal, (long long)ld_in, (long long)esz, (long long)q.ld_out);
    hipStream_t s = (hipStream_t)stream;
    return hip_result(q.mx ? fp8mi_launch_moe_scatter_quantize_mx(in, in_dtype, c.rows, c.cols, ld_in, row_of, k, out, rows_out, q.ld_out, (uint8_t *)scales,
                                                                  q.s_sr, q.kind, s)
                           : fp8mi_launch_moe_scatter_quantize(in, in_dtype, c.rows, c.cols, ld_in, row_of, k, out, rows_out, q.ld_out, (float *)scales, q.s_sr,
                                                               q.s_sk, q.kind, q.encode_mode, s),
                      c.fn);
}

int fp8mi_moe_scatter_quantize(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                               int64_t rows_out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k, int scale_mode,
                               int out_format, int encode_mode, void *stream)
{
    return moe_scatter_quantize({{"fp8mi_moe_scatter_quantize", T, cols}, false, scale_mode, ld_out, s_stride_row, s_stride_k, out_format, encode_mode, nullptr},
                                in, in_dtype, ld_in, row_of, k, out, rows_out, scales, stream);
}

int fp8mi_moe_scatter_quantize_mx(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                  int64_t rows_out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format, void *stream)
{
    return moe_scatter_quantize({{"fp8mi_moe_scatter_quantize_mx", T, cols}, true, mx_format, ld_out, ld_s, 0, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, nullptr}, in,
                                in_dtype, ld_in, row_of, k, out, rows_out, scales, stream);
}

int fp8mi_moe_combine(const void *y, int y_dtype, int64_t rows, int64_t N, int64_t ld_y, const int32_t *row_of, const float *weights, int64_t T, int k,
                      void *out, int out_dtype, int64_t ld_out, void *stream)
{
    if (rows < 0 || N < 0 || T < 0 || k < 0) return fail(FP8MI_E_SHAPE, "fp8mi_moe_combine: negative size");
    if (ld_y < N || ld_out < N)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_combine: leading dimension too small (N=%lld ld_y=%lld ld_out=%lld)", (long long)N, (long long)ld_y,
                    (long long)ld_out);
    if (!dtype_ok(y_dtype)) return fail(FP8MI_E_ENUM, "fp8mi_moe_combine: unknown y_dtype %d", y_dtype);
    if (!dtype_ok(out_dtype)) return fail(FP8MI_E_ENUM, "fp8mi_moe_combine: unknown out_dtype %d", out_dtype);
    if (T == 0 || N == 0) return 0;
    if (!out || (k > 0 && !row_of) || (k > 0 && rows > 0 && !y)) return fail(FP8MI_E_NULL, "fp8mi_moe_combine: NULL pointer");
    const uintptr_t ysz = y_dtype == FP8MI_F32 ? 4 : 2, osz = out_dtype == FP8MI_F32 ? 4 : 2;
    if (((uintptr_t)y & (ysz - 1)) || ((uintptr_t)out & (osz - 1)) || (((uintptr_t)row_of | (uintptr_t)weights) & 3u))
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_combine: y, out, row_of and weights must be aligned to their element size");
    return hip_result(fp8mi_launch_moe_combine(y, y_dtype, rows, N, ld_y, row_of, weights, T, k, out, out_dtype, ld_out, (hipStream_t)stream), "moe-combine");
}

// ---- the MoE gate (fp8mi_moe_gate.hip) ----------------------------------------------------------------------------------------------------
int fp8mi_moe_gate(const void *logits, int dtype, int64_t T, int G, int64_t ld, const float *bias, int k, int scoring, int renormalize, float scale,
                   int n_group, int topk_group, int group_score, int32_t *ids, float *weights, void *stream)
{
    if (T < 0) return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: negative size (T=%lld)", (long long)T);
    if (G < 1) return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: G=%d experts; at least one is needed", G);
    if (k < 1 || k > G) return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: k=%d of G=%d experts; 1 <= k <= G is needed", k, G);
    if (ld < G) return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: leading dimension too small (G=%d ld=%lld)", G, (long long)ld);
    if (n_group < 1 || G % n_group != 0)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: n_group=%d; a positive divisor of G=%d is needed", n_group, G);
    const int gs = G / n_group;
    if (topk_group < 1 || topk_group > n_group)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: topk_group=%d of n_group=%d groups; 1 <= topk_group <= n_group is needed", topk_group, n_group);
    if ((int64_t)k > (int64_t)topk_group * gs)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: k=%d; topk_group=%d groups of %d experts hold fewer", k, topk_group, gs);
    if (!dtype_ok(dtype)) return fail(FP8MI_E_ENUM, "fp8mi_moe_gate: unknown dtype %d", dtype);
    if (scoring != FP8MI_GATE_SOFTMAX && scoring != FP8MI_GATE_SIGMOID) return fail(FP8MI_E_ENUM, "fp8mi_moe_gate: unknown scoring %d", scoring);
    if (group_score != FP8MI_GATE_GROUP_MAX && group_score != FP8MI_GATE_GROUP_TOP2)
        return fail(FP8MI_E_ENUM, "fp8mi_moe_gate: unknown group_score %d", group_score);
    if (group_score == FP8MI_GATE_GROUP_TOP2 && n_group > 1 && gs < 2)
        return fail(FP8MI_E_SHAPE, "fp8mi_moe_gate: group_score FP8MI_GATE_GROUP_TOP2 needs groups of two experts or more (G=%d n_group=%d)", G, n_group);
    if (G > kMoeGateMaxExperts) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: G=%d experts; at most %d are supported", G, kMoeGateMaxExperts);
    if (k > kMoeGateMaxK) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: k=%d; at most FP8MI_MOE_GATE_MAX_K = %d are supported", k, kMoeGateMaxK);
    if (n_group > kMoeGateMaxGroups) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: n_group=%d; at most %d groups are supported", n_group, kMoeGateMaxGroups);
    if (T > 0x7FFFFFFFll / k) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: T k = %lld x %d assignments; rows are int32", (long long)T, k);
    if (!(scale - scale == 0.0f)) return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: scale is not finite");
    if (T == 0) return 0;
    if (!logits || !ids || !weights) return fail(FP8MI_E_NULL, "fp8mi_moe_gate: NULL pointer (logits, ids or weights)");
    const uintptr_t esz = dtype == FP8MI_F32 ? 4 : 2;
    if (((uintptr_t)logits & (esz - 1)) || (((uintptr_t)bias | (uintptr_t)ids | (uintptr_t)weights) & 3u))
        return fail(FP8MI_E_UNSUPPORTED, "fp8mi_moe_gate: logits, bias, ids and weights must be aligned to their element size");
    return hip_result(fp8mi_launch_moe_gate(logits, dtype, T, G, ld, bias, k, scoring, renormalize, scale, n_group, topk_group, group_score, ids, weights,
                                            (hipStream_t)stream), "moe-gate");
}

// ---- the FP8 paged KV cache and decode attention (fp8mi_kvcache.hip, fp8mi_attn_decode.hip) ----------------------------------------------
static_assert(kAttnMaxGroup == FP8MI_ATTN_MAX_GROUP && kAttnMaxSplits == FP8MI_ATTN_MAX_SPLITS, "include/fp8mi.h exports these");

static int check_cache_geometry(const char *fn, int Hkv, int D, int64_t num_blocks, int block_size)
{
    if (Hkv < 1) return fail(FP8MI_E_SHAPE, "%s: Hkv=%d KV heads; at least one is needed", fn, Hkv);
    if (num_blocks < 0) return fail(FP8MI_E_SHAPE, "%s: negative size (num_blocks=%lld)", fn, (long long)num_blocks);
    if (!fp8mi_attn_head_dim_ok(D)) return fail(FP8MI_E_SHAPE, "%s: D=%d; the head dimension is 64 or 128", fn, D);
    if (!fp8mi_attn_block_size_ok(block_size)) return fail(FP8MI_E_SHAPE, "%s: block_size=%d; 16, 32, 64 or 128 is needed", fn, block_size);
    return 0;
}

static bool kv_scale_mode_ok(int m) { return m == FP8MI_KV_SCALE_TENSOR || m == FP8MI_KV_SCALE_HEAD; }

int fp8mi_kv_cache_append(const void *k, const void *v, int dtype, int64_t T, int Hkv, int D, int64_t ld_k, int64_t ld_v, uint8_t *k_cache,
                          uint8_t *v_cache, int64_t num_blocks, int block_size, const void *slot_mapping, int slot_bytes, const float *k_scale,
                          const float *v_scale, int scale_mode, int encode_mode, void *stream)
{
    const char *fn = "fp8mi_kv_cache_append";
    if (T < 0) return fail(FP8MI_E_SHAPE, "%s: negative size (T=%lld)", fn, (long long)T);
    if (int rc = check_cache_geometry(fn, Hkv, D, num_blocks, block_size)) return rc;
    if (ld_k < (int64_t)Hkv * D || ld_v < (int64_t)Hkv * D)
        return fail(FP8MI_E_SHAPE, "%s: leading dimension too small (Hkv D=%lld ld_k=%lld ld_v=%lld)", fn, (long long)Hkv * D, (long long)ld_k, (long long)ld_v);
    if (!dtype_ok(dtype)) return fail(FP8MI_E_ENUM, "%s: unknown dtype %d", fn, dtype);
    if (!kv_scale_mode_ok(scale_mode)) return fail(FP8MI_E_ENUM, "%s: unknown scale_mode %d", fn, scale_mode);
    if (!encode_mode_ok(encode_mode)) return fail(FP8MI_E_ENUM, "%s: unknown encode_mode %d", fn, encode_mode);
    if (slot_bytes != 4 && slot_bytes != 8) return fail(FP8MI_E_ENUM, "%s: slot_bytes=%d; slots are int32 (4) or int64 (8)", fn, slot_bytes);
    if (T > (1ll << 40) / ((int64_t)Hkv * D)) return fail(FP8MI_E_UNSUPPORTED, "%s: T Hkv D = %lld x %d x %d elements; fewer than 2^40 are supported", fn, (long long)T, Hkv, D);
    if (T == 0) return 0;
    if (!k || !v || !k_cache || !v_cache || !slot_mapping || !k_scale || !v_scale) return fail(FP8MI_E_NULL, "%s: NULL pointer", fn);
    const uintptr_t esz = dtype == FP8MI_F32 ? 4 : 2;
    if ((((uintptr_t)k | (uintptr_t)v) & (esz - 1)) || (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15u) || ((uintptr_t)slot_mapping & (uintptr_t)(slot_bytes - 1)) ||
        (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3u))
        return fail(FP8MI_E_UNSUPPORTED, "%s: k, v, slot_mapping and the scales must be aligned to their element size, the caches to 16 bytes", fn);
    return hip_result(fp8mi_launch_kv_cache_append(k, v, dtype, T, Hkv, D, ld_k, ld_v, k_cache, v_cache, num_blocks, block_size, slot_mapping, slot_bytes, k_scale,
                                                   v_scale, scale_mode == FP8MI_KV_SCALE_HEAD, encode_mode, (hipStream_t)stream), "kv-cache-append");
}

int64_t fp8mi_paged_attention_workspace_bytes(int64_t B, int Hq, int D, int num_splits)
{
    if (B < 0 || Hq < 1 || !fp8mi_attn_head_dim_ok(D) || num_splits < 0 || num_splits > kAttnMaxSplits) return 0;
    if (num_splits == 0)   // the most the library chooses for any Hkv (Hq / Hkv <= 16) and any max_seq_len
        num_splits = fp8mi_attn_auto_splits(B, Hq, (Hq + kAttnMaxGroup - 1) / kAttnMaxGroup, D, INT64_MAX / 2, INT64_MAX, fp8mi_cu_count());
    return fp8mi_attn_workspace_bytes(B, Hq, D, num_splits);
}

}  // extern "C"

// fp8mi_paged_attention_decode and fp8mi_paged_attention_varlen: one set of argument checks and one split choice.  `varlen` = false is the
// decode entry - one query row per sequence, rows = B, cu_seqlens_q and max_q_len unused; true: rows = T query rows dealt to B sequences.
static int paged_attention(const char *fn, const char *what, bool varlen, const void *q, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q,
                           int64_t max_q_len, int Hq, int Hkv, int D, int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks,
                           int block_size, const int32_t *block_table, int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len,
                           const float *k_scale, const float *v_scale, int scale_mode, float softmax_scale, int num_splits, void *workspace,
                           int64_t workspace_bytes, void *out, int out_dtype, int64_t ld_out, void *stream)
{
    if (varlen && (rows < 0 || max_q_len < 0))
        return fail(FP8MI_E_SHAPE, "%s: negative size (T=%lld max_q_len=%lld)", fn, (long long)rows, (long long)max_q_len);
    if (B < 0 || max_blocks < 0 || max_seq_len < 0 || workspace_bytes < 0)
        return fail(FP8MI_E_SHAPE, "%s: negative size (B=%lld max_blocks=%lld max_seq_len=%lld workspace_bytes=%lld)", fn, (long long)B, (long long)max_blocks,
                    (long long)max_seq_len, (long long)workspace_bytes);
    if (int rc = check_cache_geometry(fn, Hkv, D, num_blocks, block_size)) return rc;
    if (Hq < 1 || Hq % Hkv != 0) return fail(FP8MI_E_SHAPE, "%s: Hq=%d query heads; a positive multiple of Hkv=%d is needed", fn, Hq, Hkv);
    if (ld_q < (int64_t)Hq * D || ld_out < (int64_t)Hq * D || ld_bt < max_blocks)
        return fail(FP8MI_E_SHAPE, "%s: leading dimension too small (Hq D=%lld ld_q=%lld ld_out=%lld; max_blocks=%lld ld_bt=%lld)", fn, (long long)Hq * D,
                    (long long)ld_q, (long long)ld_out, (long long)max_blocks, (long long)ld_bt);
    if (num_splits < 0) return fail(FP8MI_E_SHAPE, "%s: num_splits=%d; 0 (chosen here) or a positive count is needed", fn, num_splits);
    if (!dtype_ok(q_dtype) || !dtype_ok(out_dtype)) return fail(FP8MI_E_ENUM, "%s: unknown q_dtype %d / out_dtype %d", fn, q_dtype, out_dtype);
    if (!kv_scale_mode_ok(scale_mode)) return fail(FP8MI_E_ENUM, "%s: unknown scale_mode %d", fn, scale_mode);
    if (Hq / Hkv > kAttnMaxGroup) return fail(FP8MI_E_UNSUPPORTED, "%s: Hq / Hkv = %d; at most FP8MI_ATTN_MAX_GROUP = %d query heads share a KV head", fn, Hq / Hkv, kAttnMaxGroup);
    if (num_splits > kAttnMaxSplits) return fail(FP8MI_E_UNSUPPORTED, "%s: num_splits=%d; at most FP8MI_ATTN_MAX_SPLITS = %d", fn, num_splits, kAttnMaxSplits);
    if (!(softmax_scale - softmax_scale == 0.0f)) return fail(FP8MI_E_UNSUPPORTED, "%s: softmax_scale is not finite", fn);
    if (max_blocks > (1ll << 40) / block_size) return fail(FP8MI_E_UNSUPPORTED, "%s: max_blocks=%lld; fewer than 2^40 positions are supported", fn, (long long)max_blocks);
    if (varlen && rows > 0x7FFFFFFFll / Hq) return fail(FP8MI_E_UNSUPPORTED, "%s: T Hq = %lld x %d query rows; fewer than 2^31 are supported", fn, (long long)rows, Hq);
    const bool ws_usable = workspace && ((uintptr_t)workspace & 15u) == 0;
    if (num_splits > 1 && (!ws_usable || workspace_bytes < fp8mi_attn_workspace_bytes(rows, Hq, D, num_splits)))
        return fail(FP8MI_E_UNSUPPORTED, "%s: num_splits=%d needs a 16-byte aligned workspace of %lld bytes (fp8mi_paged_attention_workspace_bytes)", fn, num_splits,
                    (long long)fp8mi_attn_workspace_bytes(rows, Hq, D, num_splits));
    if (B == 0 || (varlen && (rows == 0 || max_q_len == 0))) return 0;
    if (!q || !k_cache || !v_cache || !block_table || !seq_lens || !k_scale || !v_scale || !out || (varlen && !cu_seqlens_q)) return fail(FP8MI_E_NULL, "%s: NULL pointer", fn);
    const uintptr_t qsz = q_dtype == FP8MI_F32 ? 4 : 2, osz = out_dtype == FP8MI_F32 ? 4 : 2;
    if (((uintptr_t)q & (qsz - 1)) || ((uintptr_t)out & (osz - 1)) || (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15u) ||
        (((uintptr_t)block_table | (uintptr_t)seq_lens | (uintptr_t)k_scale | (uintptr_t)v_scale | (uintptr_t)(varlen ? cu_seqlens_q : nullptr)) & 3u))
        return fail(FP8MI_E_UNSUPPORTED, "%s: q, out, block_table, seq_lens%s and the scales must be aligned to their element size, the caches to 16 bytes", fn,
                    varlen ? ", cu_seqlens_q" : "");
    if (varlen && max_q_len > rows) max_q_len = rows;   // no sequence owns more rows than there are
    // the decode entry is the one-token case of both rules below: max_q_len = 1 is one tile, and the split choice of B rows, a token each, is
    // fp8mi_attn_auto_splits's
    const int64_t tiles = fp8mi_attn_q_tiles(max_q_len, Hq, Hkv);
    const int splits = num_splits > 0 ? num_splits
                                      : fp8mi_attn_auto_splits_varlen(rows, B, max_q_len, Hq, Hkv, D, max_seq_len, ws_usable ? workspace_bytes : 0, fp8mi_cu_count());
    if (B * Hkv > 0x7FFFFFFFll / tiles || B * Hkv * tiles > 0x7FFFFFFFll / splits)
        return varlen ? fail(FP8MI_E_UNSUPPORTED, "%s: B Hkv ceil(max_q_len / TQ) num_splits = %lld x %d x %lld x %d workgroups; fewer than 2^31 are supported", fn,
                             (long long)B, Hkv, (long long)tiles, splits)
                      : fail(FP8MI_E_UNSUPPORTED, "%s: B Hkv num_splits = %lld x %d x %d workgroups; fewer than 2^31 are supported", fn, (long long)B, Hkv, splits);
    return hip_result(fp8mi_launch_paged_attention(q, q_dtype, rows, B, varlen ? cu_seqlens_q : nullptr, max_q_len, Hq, Hkv, D, ld_q, k_cache, v_cache, num_blocks,
                                                   block_size, block_table, ld_bt, max_blocks, seq_lens, max_seq_len, k_scale, v_scale,
                                                   scale_mode == FP8MI_KV_SCALE_HEAD, softmax_scale, splits, workspace, out, out_dtype, ld_out, (hipStream_t)stream),
                      what);
}

extern "C" {

int fp8mi_paged_attention_decode(const void *q, int q_dtype, int64_t B, int Hq, int Hkv, int D, int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache,
                                 int64_t num_blocks, int block_size, const int32_t *block_table, int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens,
                                 int64_t max_seq_len, const float *k_scale, const float *v_scale, int scale_mode, float softmax_scale, int num_splits,
                                 void *workspace, int64_t workspace_bytes, void *out, int out_dtype, int64_t ld_out, void *stream)
{
    return paged_attention("fp8mi_paged_attention_decode", "paged-attention-decode", false, q, q_dtype, B, B, nullptr, 1, Hq, Hkv, D, ld_q, k_cache, v_cache, num_blocks,
                           block_size, block_table, ld_bt, max_blocks, seq_lens, max_seq_len, k_scale, v_scale, scale_mode, softmax_scale, num_splits, workspace,
                           workspace_bytes, out, out_dtype, ld_out, stream);
}

int fp8mi_paged_attention_varlen_splits(int64_t T, int64_t B, int64_t max_q_len, int Hq, int Hkv, int D, int64_t max_seq_len, int64_t workspace_bytes)
{
    if (T < 0 || B < 0 || max_q_len < 0 || max_seq_len < 0 || workspace_bytes < 0 || Hkv < 1 || Hq < 1 || Hq % Hkv != 0 || Hq / Hkv > kAttnMaxGroup ||
        !fp8mi_attn_head_dim_ok(D))
        return 0;
    if (T == 0 || B == 0 || max_q_len == 0) return 1;
    return fp8mi_attn_auto_splits_varlen(T, B, max_q_len < T ? max_q_len : T, Hq, Hkv, D, max_seq_len, workspace_bytes, fp8mi_cu_count());
}

int fp8mi_paged_attention_varlen(const void *q, int q_dtype, int64_t T, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, int Hkv, int D,
                                 int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size, const int32_t *block_table,
                                 int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len, const float *k_scale, const float *v_scale,
                                 int scale_mode, float softmax_scale, int num_splits, void *workspace, int64_t workspace_bytes, void *out, int out_dtype,
                                 int64_t ld_out, void *stream)
{
    return paged_attention("fp8mi_paged_attention_varlen", "paged-attention-varlen", true, q, q_dtype, T, B, cu_seqlens_q, max_q_len, Hq, Hkv, D, ld_q, k_cache, v_cache,
                           num_blocks, block_size, block_table, ld_bt, max_blocks, seq_lens, max_seq_len, k_scale, v_scale, scale_mode, softmax_scale, num_splits,
                           workspace, workspace_bytes, out, out_dtype, ld_out, stream);
}

}  // extern "C"
