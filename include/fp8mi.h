/*
 * fp8mi - MI355X (gfx950) FP8 (e4m3fn; e5m2 through the *_fmt / *_e5m2 entry points) scaled-matmul and cast kernels, C ABI.
 *
 * This is the drop-in boundary of the build: a shared library
 * (fp8-mps-metal_amd/libfp8mi.so) with plain-C entry points - device pointers,
 * sizes and a HIP stream; no torch or C++ types - that a host binds with
 * ctypes / cgo / JNI.  It is the MI355X-native counterpart of the reference's
 * pybind11 module `fp8_metal` (fp8_bridge.cpp:361-371) and of the four kernel
 * launch sites of fp8_mps_native.py, but pointer-level: nothing is staged
 * through the CPU, nothing is allocated, nothing synchronises.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the current HIP device unless said
 *     otherwise; `stream` is a hipStream_t passed as void* (NULL = default);
 *   - every call only ENQUEUES work on `stream` and returns; it never blocks,
 *     never allocates, and is safe to capture into a HIP graph;
 *   - return value 0 = ok; negative = argument error (FP8MI_E_*); positive =
 *     a hipError_t from the launch.  fp8mi_last_error() returns a
 *     thread-local, human-readable message for the last non-zero return;
 *   - the compute entry points keep no state (no globals besides that message
 *     and a per-device cache of the CU count), so calls are re-entrant from any
 *     thread.  The two measurement hooks at the end of this header
 *     (fp8mi_profile_begin / _end) DO keep per-thread state - an event pool and
 *     an "a profile is open" flag that every launch on that thread consults;
 *     they exist for bench.py and are not meant for production call paths;
 *   - all element counts are 64-bit (the reference's `uint count`,
 *     fp8_matmul.metal:218,231, caps at 2^32-1).
 *
 * Semantics are the REFERENCE's (audiohacking/fp8-mps-metal), not OCP/torch's,
 * wherever they differ; the non-default modes give the OCP behaviour:
 *   decode: NaN bytes 0x7F/0xFF -> +0.0              (fp8_matmul.metal:21)
 *   encode: clamp-not-carry, flush below 2^-9, saturate to 0x7E, -0.0 -> 0x00
 *                                                    (fp8_matmul.metal:44-92)
 */
#ifndef FP8MI_H
#define FP8MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP8MI_VERSION 0x000400 /* 0.4.0: + fp8mi_predict_kernel_us (the dispatch is one cost model), + fp8mi_act_quantize; 0.3.0: + fp8mi_workspace_reset, FP8MI_EPILOGUE_TRANSPOSED, kernel ids GEMV_FP32 / GEMV_MX / GEMM_256W */

/* element types of non-fp8 operands */
enum { FP8MI_F32 = 0, FP8MI_F16 = 1, FP8MI_BF16 = 2 };

/* OR into `bias_dtype`: the caller computes the TRANSPOSED product C^T = B . A^T (what a
 * rank of an N-column-sharded linear does, so that its block of the output is contiguous:
 * the weight shard is passed as `A`, the activations as `B_nk`).  The epilogue then
 * multiplies by scale_b first and scale_a second and takes bias[m] (M elements, per
 * output row) - bit for bit what the untransposed fused epilogue
 * ((acc * s_activation) * s_weight + bias[weight row]) would have stored. */
#define FP8MI_EPILOGUE_TRANSPOSED 0x100

/* scale layouts */
enum { FP8MI_SCALE_TENSOR = 0, /* one float                               */
       FP8MI_SCALE_ROW = 1 };  /* one float per row of A (M) / of B (N)   */

/* what a NaN byte (0x7F / 0xFF) in A or B means */
enum { FP8MI_NAN_ZERO = 0,       /* reference: decodes to +0.0 (fp8_matmul.metal:21)   */
       FP8MI_NAN_PROPAGATE = 1 };/* OCP / torch: NaN, poisons its dot products        */

/* float -> fp8 rounding/saturation rules */
enum { FP8MI_ENC_REFERENCE = 0,  /* fp8_matmul.metal:44-92 (see header comment)        */
       FP8MI_ENC_RNE = 1 };      /* OCP round-to-nearest-even, overflow -> NaN (torch) */

/* kernel selection for fp8mi_scaled_mm_ex (testing / benchmarking) */
enum { FP8MI_KERNEL_AUTO = 0,
       FP8MI_KERNEL_GEMV = 1,      /* M == 1 wavefront-reduced vec-mat (fp32 FMA for K <= 4096, matrix core above) */
       FP8MI_KERNEL_GEMM_128 = 2,  /* 128x128x128 LDS-tiled fp8 MFMA (mid sizes)      */
       FP8MI_KERNEL_GENERIC = 3,   /* any shape / alignment, one wave per output      */
       FP8MI_KERNEL_GEMM_256 = 4,  /* 256x256x128 LDS-tiled fp8 MFMA (large M,N)      */
       FP8MI_KERNEL_GEMM_128x64 = 5, /* 128x64x128 tile (few tiles: one per CU)       */
       FP8MI_KERNEL_SKINNY = 6,    /* 1 <= M <= 64 weight-streaming MFMA              */
       FP8MI_KERNEL_GEMM_64x128 = 14, /* 64x128x128 tile (M <= 64, deep K)            */
       FP8MI_KERNEL_GEMV_FP32 = 18,  /* M == 1, IEEE fp32 accumulation at every K     */
       FP8MI_KERNEL_GEMV_MX = 19,    /* 2 <= M <= 8 on the vec-mat's weight-streaming structure */
       FP8MI_KERNEL_GEMM_256W = 20, /* 256x256 tile, one wave per SIMD, hand-scheduled K loop: any M, N (a multiple of 4 fp32 / 8 half columns), K >= 256 (K % 16 == 0; a partial last K-step since round 3) */
       FP8MI_KERNEL_GEMM_256x128W = 21, /* the same on 256x128 tiles (shapes that give 256x256 tiles less than a round) */
       FP8MI_KERNEL_GEMM_64x64 = 22,  /* 64x64x128 tile, 8 waves (33 <= M <= 64 against deep K, and up to M = 128 while the tile grid is small; with split-K) */
       FP8MI_KERNEL_GEMM_32x64 = 23,  /* 32x64x128 tile, 4 waves (9 <= M <= 32: the decode regime; with split-K) */
       FP8MI_KERNEL_GEMM_32x32 = 24,  /* 32x32x128 tile, 2 waves (M <= 32 against K, N <= 8192: N / 32 tiles fill the chip with fewer K slices) */
       FP8MI_KERNEL_GEMM_128D = 25 }; /* 128x128x128 tile on a DEEP ring (4 x 32 KiB, one workgroup per CU): shapes that give at most one 128x128 tile per CU */
/* Other ids exist only in the diagnostic build of the library (libfp8mi_diag.so:
 * schedule variants, the producer/consumer kernel and its ablations, kept for
 * A/B timing - tools/README.md); the product library rejects them. */

/* error codes (negative returns) */
enum { FP8MI_OK = 0,
       FP8MI_E_NULL = -1,     /* required pointer is NULL                  */
       FP8MI_E_SHAPE = -2,    /* negative size or leading dim too small    */
       FP8MI_E_ENUM = -3,     /* unknown dtype / mode / kernel             */
       FP8MI_E_UNSUPPORTED = -4 /* forced kernel cannot run this problem   */ };

/*
 * C[m,n] = cast( ((sum_k dec(A[m,k]) * dec(B[n,k])) * sa * sb + bias[n]) * scale_result )
 *
 * Replaces: fp8_scaled_matmul_kernel (fp8_matmul.metal:99-147),
 *           fp8_scaled_vecmat_kernel (fp8_matmul.metal:155-210), their launch
 *           sites fp8_mps_native.py:41-95 / fp8_bridge.cpp:165-259, the kernel
 *           choice fp8_scaled_mm_auto (fp8_mps_native.py:193-210) and the three
 *           elementwise passes of the epilogue in fp8_mps_patch.py:94-104
 *           (fused here, same order: + bias, * scale_result, cast).
 *
 * A        (M,K) fp8 e4m3fn bytes, row-major, leading dimension lda >= K
 * B_nk     (N,K) fp8 e4m3fn bytes, row-major (i.e. torch's column-major
 *          `other` (K,N) seen through .t()), leading dimension ldb >= K
 * C        (M,N) out_dtype, row-major, leading dimension ldc >= N (elements)
 * scale_a  float[1] (FP8MI_SCALE_TENSOR) or float[M] (FP8MI_SCALE_ROW)
 * scale_b  float[1] or float[N]
 * bias     NULL or [N] of bias_dtype ([M] with FP8MI_EPILOGUE_TRANSPOSED);  scale_result NULL or float[1]
 * Accumulators are float32.  On the matrix-core kernels (M > 1; M == 1 with K > 4096) the
 * sum inside an instruction is the gfx950 fp8 MFMA's: exact products, addends more than
 * ~2^13 below the largest of their group of 8 truncated (|err| <= 1e-3 sum|a||b| worst
 * case, ~2e-5 rms on random data, exact on operands within a 2^12 product range) - two
 * orders of magnitude inside the reference's own 4 % gate.  FP8MI_KERNEL_GEMV_FP32 and
 * FP8MI_KERNEL_GENERIC accumulate in IEEE fp32 like the reference's kernels
 * (fp8_matmul.metal:116-141, 177-199).  M == 0 or N == 0 is a no-op; K == 0 writes the
 * epilogue of a zero sum.
 */
int fp8mi_scaled_mm(const uint8_t *A, const uint8_t *B_nk, void *C,
                    const float *scale_a, const float *scale_b,
                    const void *bias, const float *scale_result,
                    int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    int scale_a_mode, int scale_b_mode,
                    int out_dtype, int bias_dtype, int nan_mode,
                    void *stream);

/* Same, with the kernel forced (FP8MI_KERNEL_*); FP8MI_E_UNSUPPORTED if the
 * forced kernel cannot run the problem (e.g. GEMV with M != 1). */
int fp8mi_scaled_mm_ex(const uint8_t *A, const uint8_t *B_nk, void *C,
                       const float *scale_a, const float *scale_b,
                       const void *bias, const float *scale_result,
                       int64_t M, int64_t N, int64_t K,
                       int64_t lda, int64_t ldb, int64_t ldc,
                       int scale_a_mode, int scale_b_mode,
                       int out_dtype, int bias_dtype, int nan_mode,
                       int kernel, void *stream);

/*
 * Split-K.  When M x N yields far fewer output tiles than the device has CUs (small M,
 * deep K: the decode / small-batch regime) the tile kernels can cut K into
 * `split_k` slices, one workgroup per (tile, slice); the slices' fp32 partial
 * tiles meet in `workspace`, and the last workgroup of a tile to finish adds
 * them in slice order (run-to-run reproducible) and runs the fused epilogue.
 * No counterpart in the reference (its kernels are one thread per output,
 * fp8_matmul.metal:99-147).
 *
 * workspace        device buffer, 16-byte aligned, used by ONE launch at a time
 *                  (launches on one stream may share it; concurrent streams
 *                  need their own).  Its first FP8MI_WS_COUNTER_BYTES bytes
 *                  (the tiles' arrival counters) must be zero before the first
 *                  launch that uses it - fp8mi_workspace_reset() - and every
 *                  launch that completes leaves them zero.  A launch that is
 *                  ABORTED mid-flight (device fault) can leave a counter
 *                  non-zero, and later launches on that workspace would then
 *                  mis-reduce silently: reset the workspace as part of any
 *                  error recovery.  NULL: never split.
 * workspace_bytes  its size; fp8mi_scaled_mm_workspace_bytes() is enough for
 *                  every problem the library would split on its own.  A
 *                  workspace that is too small silently disables the split.
 * split_k          0: library decides; 1: no split; > 1: that many slices
 *                  (clamped to the largest count K and the workspace allow).
 * fp8mi_scaled_mm / _ex are this call with workspace == NULL.
 */
#define FP8MI_WS_COUNTER_BYTES 4096
int64_t fp8mi_scaled_mm_workspace_bytes(void);
/* Enqueue a memset of the counter block (FP8MI_WS_COUNTER_BYTES at the head of
 * `workspace`) on `stream`: once after allocating a workspace, and after any
 * aborted launch.  Graph-capturable (a memset node). */
int fp8mi_workspace_reset(void *workspace, int64_t workspace_bytes, void *stream);
int fp8mi_scaled_mm_ws(const uint8_t *A, const uint8_t *B_nk, void *C,
                       const float *scale_a, const float *scale_b,
                       const void *bias, const float *scale_result,
                       int64_t M, int64_t N, int64_t K,
                       int64_t lda, int64_t ldb, int64_t ldc,
                       int scale_a_mode, int scale_b_mode,
                       int out_dtype, int bias_dtype, int nan_mode,
                       int kernel, int split_k,
                       void *workspace, int64_t workspace_bytes,
                       void *stream);

/*
 * Operand element formats of fp8mi_scaled_mm_fmt: the two OCP FP8 types.  e5m2 (torch.float8_e5m2: 1-5-2, bias 15, the high byte
 * of an IEEE half) is the gradient type of FP8 training recipes and the weight type of fp8_e5m2 checkpoints.
 */
enum { FP8MI_FMT_E4M3 = 0, FP8MI_FMT_E5M2 = 1 };

/*
 * fp8mi_scaled_mm_ws with the element format of each operand: A (M,K) holds a_format bytes, B_nk (N,K) b_format bytes; all four
 * pairs run on every kernel family (the matrix-core kernels set the MFMA's per-operand format code, at the same instruction
 * rate; the fp32 paths decode e5m2 exactly).  No counterpart in the reference, which decodes e5m2 bytes as e4m3
 * (fp8_mps_patch.py:65).
 *   - a_format == b_format == FP8MI_FMT_E4M3: exactly fp8mi_scaled_mm_ws (same kernels, same bits).
 *   - with an FP8MI_FMT_E5M2 operand the semantics are OCP / IEEE only: nan_mode must be FP8MI_NAN_PROPAGATE
 *     (FP8MI_E_UNSUPPORTED otherwise).  e5m2 has inf (0x7C / 0xFC) and NaN (0x7D-0x7F / 0xFD-0xFF) encodings; they propagate as
 *     the arithmetic produces them (inf * 0 and inf - inf are NaN), e4m3 NaN bytes of the other operand likewise, and no
 *     NaN-scrub or redo pass exists in these kernel instances.
 *   - an unknown format returns FP8MI_E_ENUM.  Every argument check runs before any HIP call.
 *   - kernel forcing, split_k / workspace and FP8MI_EPILOGUE_TRANSPOSED keep their meaning.  FP8MI_KERNEL_AUTO uses the cost model
 *     of fp8mi_choose_kernel unchanged: the format does not enter the price, and the model is NOT fitted to e5m2 timings
 *     (profiles/e5m2_timing.txt has the measured ratios).
 * Accuracy: the matrix-core sum is the same instruction's (truncation ~2^-13 below the largest addend of a group of 8,
 * profiles/mfma_numerics_e5m2.txt), but e5m2 products span 2^-32 .. 2^31.6, so "exact within a 2^12 product range" covers less
 * of the format than it does for e4m3; the fp32 paths (generic, GEMV_FP32, vec-mat at K <= 4096) sum exact products in IEEE fp32.
 */
int fp8mi_scaled_mm_fmt(const uint8_t *A, const uint8_t *B_nk, void *C,
                        const float *scale_a, const float *scale_b,
                        const void *bias, const float *scale_result,
                        int64_t M, int64_t N, int64_t K,
                        int64_t lda, int64_t ldb, int64_t ldc,
                        int scale_a_mode, int scale_b_mode,
                        int out_dtype, int bias_dtype, int nan_mode,
                        int kernel, int split_k,
                        void *workspace, int64_t workspace_bytes,
                        int a_format, int b_format,
                        void *stream);

/*
 * e5m2 casts (OCP / torch semantics; no counterpart in the reference).
 *
 * fp8mi_encode_e5m2: out[i] = e5m2_rne(float32(in[i]) * prescale)   (prescale NULL = no multiply; the product is rounded to fp32
 *   first).  Byte for byte torch's CPU `x.to(torch.float8_e5m2)`: round to nearest even, finite overflow (|v| >= 61440) -> +-inf
 *   (0x7C / 0xFC), NaN -> 0x7F with the input's sign bit, -0.0 -> 0x80, subnormals down to 2^-16.
 * fp8mi_dequant_e5m2: out[i] = cast(float(dec(in[i])) * scale)      (scale NULL = no multiply): the product is formed in fp32,
 *   rounded once, then rounded to out_dtype (RNE); inf and NaN are preserved.
 * fp8mi_quantize_e5m2: amax-scaled quantisation on the device (two kernels, no host sync), as fp8mi_quantize:
 *   amax = max|in| (NaNs ignored); scale = amax > 0 ? 57344 / amax : 1 (evaluated in double)
 *   out[i] = e5m2_rne(clamp(float32(in[i]) * float32(scale), -57344, 57344))   (a NaN stays NaN: 0x7F / 0xFF)
 *   scales[0] = amax, scales[1] = float32(1 / scale); `scales` is float[2] device memory owned by the caller.
 */
int fp8mi_encode_e5m2(const void *in, int in_dtype, uint8_t *out, const float *prescale, int64_t count, void *stream);
int fp8mi_dequant_e5m2(const uint8_t *in, void *out, const float *scale, int64_t count, int out_dtype, void *stream);
int fp8mi_quantize_e5m2(const void *in, int in_dtype, uint8_t *out, float *scales, int64_t count, void *stream);

/*
 * out[i] = cast( half(dec(in[i])) * half(scale) )      (scale NULL = no multiply)
 *
 * Replaces: fp8_to_half_kernel (fp8_matmul.metal:215-223) + the separate
 *           `output * scale.to(float16)` pass of fp8_dequantize
 *           (fp8_mps_native.py:98-124; fp8_bridge.cpp:265-306).  The product
 *           is formed in float16 exactly as there; out_dtype F32/BF16 then
 *           widens/rounds that half (the reference's `.to(dtype)`,
 *           fp8_mps_patch.py:219-221).
 */
int fp8mi_dequant(const uint8_t *in, void *out, const float *scale,
                  int64_t count, int out_dtype, void *stream);

/* The same entry point under the name SURVEY.md 8(b) item 2 gives it (the half output of fp8_to_half_kernel is the
 * default use; out_dtype still selects F16 / F32 / BF16).  Two deviations from 8(b) as written, both on purpose:
 * the symbol was shortened to fp8mi_dequant (this alias keeps the contract's name linkable), and every leading
 * dimension / count in this header is int64_t where 8(b) says `int` (a (M,K) slab of a > 2 GiB buffer needs it). */
int fp8mi_dequant_f16(const uint8_t *in, void *out, const float *scale_or_null,
                      int64_t count, int out_dtype, void *stream);

/*
 * out[i] = enc( float32(in[i]) * prescale )            (prescale NULL = no multiply)
 *
 * Replaces: float_to_fp8_kernel (fp8_matmul.metal:228-236) and its launch in
 *           fp8_encode (fp8_mps_native.py:127-155; value-preserving, used by
 *           .to()/.copy_(), fp8_mps_patch.py:191,283); with `prescale` also
 *           the `inp * scale` pass of fp8_quantize (fp8_mps_native.py:179).
 *           f16/bf16 inputs are widened in-kernel (the reference converts to
 *           float32 first, fp8_mps_native.py:142).
 */
int fp8mi_encode(const void *in, int in_dtype, uint8_t *out, const float *prescale,
                 int64_t count, int encode_mode, void *stream);

/* *out = max_i |in[i]| as float32 (0 for count == 0; NaNs are ignored).
 * Replaces: `inp.abs().max().item()` of fp8_quantize (fp8_mps_native.py:174)
 * without the host read-back. */
int fp8mi_amax(const void *in, int in_dtype, float *out, int64_t count, void *stream);

/*
 * Amax-scaled quantisation, entirely on the device (no host sync, two kernels):
 *   amax = max|in|; scale = amax > 0 ? 448/amax : 1   (evaluated in double)
 *   out[i] = enc(float32(in[i]) * float32(scale));  scales[0] = amax,
 *   scales[1] = float32(1/scale)  (the inverse scale _scaled_mm consumes)
 * Replaces: fp8_quantize (fp8_mps_native.py:158-190; fp8_bridge.cpp:312-356).
 * `scales` is float[2] device memory owned by the caller.
 */
int fp8mi_quantize(const void *in, int in_dtype, uint8_t *out, float *scales,
                   int64_t count, int encode_mode, void *stream);

typedef struct fp8mi_device_info {
    int compute_units;       /* multiProcessorCount                       */
    int clock_khz;           /* max engine clock                          */
    int memory_clock_khz;
    int memory_bus_bits;
    int l2_bytes;
    int lds_bytes_per_cu;    /* maxSharedMemoryPerMultiProcessor          */
    int wavefront_size;
    int64_t total_memory;
    char arch[64];           /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    char name[128];
} fp8mi_device_info_t;

/* Host-side query of HIP device `device` (for the roofline harness). */
int fp8mi_device_info(int device, fp8mi_device_info_t *out);

/*
 * Per-dispatch kernel timing for the measurement harness (bench.py).  Between
 * fp8mi_profile_begin(n) and fp8mi_profile_end() every kernel this library
 * launches FROM THE CALLING THREAD carries its own start/stop HIP event pair
 * filled from the dispatch packet's timestamps (hipExtLaunchKernelGGL) - the
 * clock rocprofv3 --kernel-trace reads - up to n launches.  _end() waits for
 * the last profiled launch, writes up to `cap` durations (milliseconds, launch
 * order) to the HOST array ms_out and returns how many launches were timed (or
 * a negative error).  Not for use inside graph capture.  No reference
 * counterpart: the reference times with time.perf_counter() around
 * torch.mps.synchronize() (test_fp8_metal.py:248-255).
 */
int fp8mi_profile_begin(int max_launches);
int fp8mi_profile_end(float *ms_out, int cap);

int fp8mi_version(void);
const char *fp8mi_last_error(void);

/* Which kernel FP8MI_KERNEL_AUTO runs for a problem of this shape (host-only; pointers are assumed 16-byte aligned):
 * returns an FP8MI_KERNEL_* id, or a negative error for an invalid argument.  For tests and for callers that want to log
 * the dispatch; no counterpart in the reference (its choice is `M == 1` in fp8_mps_native.py:193-210). */
int fp8mi_choose_kernel(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                        int has_workspace, int split_k);

/* The dispatch's cost model itself (round 4; host-only): the time in microseconds it predicts for `kernel` on this problem on a device of
 * `compute_units` CUs (0 = the current device's), or a negative value when the kernel does not take the problem or is not offered for it
 * (FP8MI_KERNEL_GEMV / _GENERIC / _AUTO are not priced: M = 1 is a rule, the generic kernel the last resort).  fp8mi_choose_kernel returns
 * the id with the smallest prediction.  For tests (tests/golden/dispatch_times_cold_*.json) and for callers that log the dispatch. */
double fp8mi_predict_kernel_us(int kernel, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                               int has_workspace, int split_k, int compute_units);

/*
 * MXFP8: OCP microscaling block-scaled GEMM (no counterpart in the reference, which has per-tensor scales only).
 *
 * C[m,n] = cast( (sum_b 2^(sa[m,b]-127) * 2^(sb[n,b]-127) * sum_{k in block b} dec(A[m,k]) * dec(B[n,k]) + bias[n]) * scale_result )
 *
 * Blocks b are 32 consecutive k.  scale_a / scale_b are E8M0 bytes (torch.float8_e8m0fnu: 2^(s-127), 0xFF = NaN), row-major
 * (M, K/32) / (N, K/32) with leading dimensions ld_sa / ld_sb (bytes; >= K/32).  The matrix-core kernels read the scales in
 * 4-byte K-steps: they take ld_sa, ld_sb multiples of 4 and 4-byte aligned scale pointers (torch's padded layout,
 * round_up(K/32, 4) per row), and then read every row up to its ld bytes; otherwise AUTO runs the generic kernel.
 * K must be a multiple of 32 (FP8MI_E_SHAPE otherwise).  On the matrix-core kernels each block is summed by the
 * v_mfma_scale_f32_16x16x128_f8f6f4 instruction with its scales applied in the instruction (same accuracy note as
 * fp8mi_scaled_mm); FP8MI_KERNEL_GENERIC scales every exact product with one rounding and sums in IEEE fp32.
 * Scale 0x00 is 2^-127.  Scale 0xFF (NaN) makes every output that sums its block NaN - on the matrix-core kernels
 * (profiles/mxfp8_scale_map.txt) and on the generic one alike.  NaN data bytes follow nan_mode as in fp8mi_scaled_mm.
 * Finite scaled sums can overflow fp32 to inf (and inf - inf is NaN): unlike the tensorwise GEMM, a NaN output need not
 * mean a NaN byte.
 * kernel: FP8MI_KERNEL_AUTO (the cheapest block-scaled ring tile by the tensorwise cost model; generic as the last resort),
 * FP8MI_KERNEL_GEMM_{128, 128x64, 64x128, 64x64, 32x64, 32x32, 128D} or FP8MI_KERNEL_GENERIC.  The vec-mat, few-rows,
 * skinny, 256x256 and one-wave-per-SIMD kernels have no block-scaled form: FP8MI_E_UNSUPPORTED.  split_k / workspace as in
 * fp8mi_scaled_mm_ws (slices are cut on 128-k boundaries).  FP8MI_EPILOGUE_TRANSPOSED in bias_dtype keeps its meaning.
 * Every argument check runs before any HIP call.
 */
int fp8mi_scaled_mm_mxfp8(const uint8_t *A, const uint8_t *B_nk, void *C,
                          const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b, int64_t ld_sb,
                          const void *bias, const float *scale_result,
                          int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                          int out_dtype, int bias_dtype, int nan_mode,
                          int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream);

/* Which kernel FP8MI_KERNEL_AUTO of fp8mi_scaled_mm_mxfp8 runs for this shape (host-only; operands 16-byte aligned, scales in
 * torch's padded layout); a negative error for an invalid argument. */
int fp8mi_choose_kernel_mxfp8(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                              int has_workspace, int split_k);

/*
 * MXFP8 quantisation of a (rows, cols) f32 / f16 / bf16 matrix (row stride ld_in elements; cols % 32 == 0): e4m3 bytes
 * out (rows, cols; ld_out) and E8M0 scales (rows, cols/32; ld_s), byte for byte torch's recipe
 * (torch.testing._internal.common_quantized.to_mxfp(x, 32, "mxfp8"), torchao's RCEIL):
 *   amax = max|x| of the block (NaN if it holds one); descale = amax / 448 (fp32)
 *   e = descale is NaN ? 0xFF : clamp(ceil(log2f(descale)), -127, 127) + 127     (log2f correctly rounded)
 *   q = rne_e4m3(clamp(x * (e == 0 ? 1 : 2^(127-e)), -448, 448))
 */
int fp8mi_quantize_mxfp8(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in,
                         uint8_t *out, int64_t ld_out, uint8_t *scales, int64_t ld_s, void *stream);

/* out[r,c] = cast(dec(in[r,c]) * 2^(scales[r, c/32] - 127)), out contiguous (rows, cols) of out_dtype; OCP decode
 * (NaN bytes and scale 0xFF give NaN), the product in fp32 rounded once, then to out_dtype. */
int fp8mi_dequant_mxfp8(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in,
                        const uint8_t *scales, int64_t ld_s, void *out, int out_dtype, void *stream);

/*
 * MXFP4: OCP microscaling GEMM with e2m1 (fp4) operands, both sides (no counterpart in the reference).
 *
 * C[m,n] = cast( (sum_b 2^(sa[m,b]-127) * 2^(sb[n,b]-127) * sum_{k in block b} e2m1(A[m,k]) * e2m1(B[n,k]) + bias[n]) * scale_result )
 *
 * A (M, K) and B_nk (N, K) hold two e2m1 codes per byte (torch.float4_e2m1fn_x2): element k of a row is the low nibble of
 * byte k/2 when k is even, the high nibble when odd.  K, M and N count ELEMENTS; lda and ldb count BYTES (>= K/2).  Scales
 * as in fp8mi_scaled_mm_mxfp8: E8M0 bytes, (M, K/32) / (N, K/32) row-major, ld_sa / ld_sb >= K/32 bytes; the matrix-core
 * kernels take ld_sa, ld_sb multiples of 4 and 4-byte aligned scale pointers (torch's padded layout, both K/32 = 0 and
 * 4 mod 8 included), otherwise AUTO runs the generic kernel.  K must be a multiple of 32 (FP8MI_E_SHAPE otherwise).
 * e2m1 has no NaN or inf encoding (bytes 0x7F / 0xFF are finite values): there is no nan_mode.  Scale 0xFF makes every
 * output that sums its block NaN; scale 0x00 is 2^-127 (profiles/mxfp4_operand_map.txt).  With every scale 2^0 and
 * K <= 4096 the matrix-core result is the exact sum (every product a multiple of 0.25 up to 36); across blocks of very
 * different scales the instruction's internal sum is not exact (the probe's 2^24 + 1 + 1 gives 2^24).
 * kernel: FP8MI_KERNEL_AUTO (the MXFP8 tile choice priced at the operands' byte depth K/2 - the tensorwise cost model, not
 * fitted to fp4 timings; generic as the last resort), FP8MI_KERNEL_GEMM_{128, 128x64, 64x128, 64x64, 32x64, 32x32, 128D}
 * or FP8MI_KERNEL_GENERIC (every exact product scaled with one rounding, IEEE fp32 sums).  The vec-mat, few-rows, skinny,
 * 256x256 and one-wave-per-SIMD kernels have no MXFP4 form: FP8MI_E_UNSUPPORTED.  split_k / workspace as in
 * fp8mi_scaled_mm_ws (slices on 256-k boundaries).  FP8MI_EPILOGUE_TRANSPOSED in bias_dtype keeps its meaning.
 * Every argument check runs before any HIP call.
 */
int fp8mi_scaled_mm_mxfp4(const uint8_t *A, const uint8_t *B_nk, void *C,
                          const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b, int64_t ld_sb,
                          const void *bias, const float *scale_result,
                          int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                          int out_dtype, int bias_dtype,
                          int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream);

/* Which kernel FP8MI_KERNEL_AUTO of fp8mi_scaled_mm_mxfp4 runs for this shape (host-only; K in elements, lda / ldb in bytes,
 * operands 16-byte aligned, scales in torch's padded layout); a negative error for an invalid argument. */
int fp8mi_choose_kernel_mxfp4(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                              int has_workspace, int split_k);

/*
 * MXFP4 quantisation of a (rows, cols) f32 / f16 / bf16 matrix (row stride ld_in elements; cols % 32 == 0): e2m1 codes out
 * (rows, cols/2 bytes, the even column in the low nibble; ld_out bytes >= cols/2) and E8M0 scales (rows, cols/32; ld_s),
 * byte for byte torch's recipe (torch.testing._internal.common_quantized.to_mxfp(x, 32, "mxfp4")):
 *   amax = max|x| of the block (NaN if it holds one); e = the RCEIL exponent of amax / 6 as in fp8mi_quantize_mxfp8
 *   y = clamp(x * (e == 0 ? 1 : 2^(127-e)), -6, 6) in fp32; then y -> bfloat16 (RNE) -> e2m1 (RNE, saturating)
 * The double rounding is the recipe's (2.5 + 2^-20 -> bf16 2.5 -> 2.0).  A NaN element becomes code 0xC, what torch's
 * integer e2m1 path makes of the bfloat16 0xFFFF that its CPU cast gives every NaN; the block's scale is 0xFF.
 */
int fp8mi_quantize_mxfp4(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in,
                         uint8_t *out, int64_t ld_out, uint8_t *scales, int64_t ld_s, void *stream);

/* out[r,c] = cast(e2m1(in[r, c/2] nibble c%2) * 2^(scales[r, c/32] - 127)), out contiguous (rows, cols) of out_dtype; cols even
 * (elements), ld_in bytes >= cols/2; scale 0xFF gives NaN; the product in fp32 rounded once, then to out_dtype. */
int fp8mi_dequant_mxfp4(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in,
                        const uint8_t *scales, int64_t ld_s, void *out, int out_dtype, void *stream);

/*
 * MXW4A8: OCP microscaling GEMM of e4m3 activations against e2m1 (fp4) weights - the recipe of an MXFP4 checkpoint whose
 * activations are quantised to MXFP8 (no counterpart in the reference).
 *
 * C[m,n] = cast( (sum_b 2^(sa[m,b]-127) * 2^(sb[n,b]-127) * sum_{k in block b} e4m3(A[m,k]) * e2m1(B[n,k]) + bias[n]) * scale_result )
 *
 * A (M, K) is e4m3 bytes (fp8mi_quantize_mxfp8's), lda >= K bytes; B_nk (N, K) holds two e2m1 codes per byte
 * (fp8mi_quantize_mxfp4's: the even k in the low nibble), ldb >= K/2 bytes.  M, N and K count ELEMENTS; K must be a multiple of 32
 * (FP8MI_E_SHAPE otherwise).  Scales as in the two recipes: E8M0 bytes, (M, K/32) / (N, K/32) row-major, ld_sa / ld_sb >= K/32;
 * the matrix-core kernels take ld_sa, ld_sb multiples of 4 and 4-byte aligned scale pointers (torch's padded layout, K/32 = 0 and
 * 4 mod 8 included), lda and ldb multiples of 16 and 16-byte aligned operands; otherwise AUTO runs the generic kernel.
 * nan_mode as in fp8mi_scaled_mm_mxfp8, on A only: e2m1 has no NaN encoding, B's bytes 0x7F / 0xFF are finite values under
 * either mode.  FP8MI_NAN_ZERO reads A's bytes 0x7F / 0xFF as zero; FP8MI_NAN_PROPAGATE makes the outputs of their rows NaN.
 * Scale 0xFF makes every output that sums its block NaN under either mode; scale 0x00 is 2^-127
 * (profiles/mxw4a8_operand_map.txt).
 * kernel: FP8MI_KERNEL_AUTO (the MXFP8 tile choice priced at the WEIGHTS' byte depth K/2 - the tensorwise cost model, not fitted to
 * this recipe; generic as the last resort), FP8MI_KERNEL_GEMM_{128, 128x64, 64x128, 64x64, 32x64, 32x32, 128D} - every ring tile
 * that has the MX forms has this one; each runs one 256-k K-step per ring stage at a ring depth of its own - or
 * FP8MI_KERNEL_GENERIC (every exact product scaled with one rounding, IEEE fp32 sums).  The vec-mat, few-rows, skinny, 256x256 and
 * one-wave-per-SIMD kernels have no MXW4A8 form: FP8MI_E_UNSUPPORTED.  split_k / workspace as in fp8mi_scaled_mm_ws (slices on
 * 256-k boundaries).  FP8MI_EPILOGUE_TRANSPOSED in bias_dtype keeps its meaning.  Error codes as fp8mi_scaled_mm_mxfp8, with lda
 * checked against K and ldb against K/2.  Every argument check runs before any HIP call.
 */
int fp8mi_scaled_mm_mxw4a8(const uint8_t *A, const uint8_t *B_nk, void *C,
                           const uint8_t *scale_a, int64_t ld_sa, const uint8_t *scale_b, int64_t ld_sb,
                           const void *bias, const float *scale_result,
                           int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                           int out_dtype, int bias_dtype, int nan_mode,
                           int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream);

/* Which kernel FP8MI_KERNEL_AUTO of fp8mi_scaled_mm_mxw4a8 runs for this shape (host-only; K in elements, lda / ldb in bytes,
 * operands 16-byte aligned, scales in torch's padded layout); a negative error for an invalid argument. */
int fp8mi_choose_kernel_mxw4a8(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                               int has_workspace, int split_k);

/*
 * Blockwise ("DeepSeek-style") scaling: fp32 scales per 128 k of every row (1x128) or of every 128-row block (128x128), the
 * recipe of DeepSeek-V3 / Qwen3-FP8 checkpoints and of torch._scaled_mm's blockwise modes (no counterpart in the reference).
 *
 * C[m,n] = cast( (sum_b  sa(m,b) * sb(n,b) * P_b(m,n)  + bias[n]) * scale_result )
 *
 * P_b is the dot product over block b, k in [128b, 128b + 128); the last block may be partial (K is any value >= 0) and
 * reads block ceil(K/128) - 1.  sa(m,b) = scale_a[(m / block_a) * sa_stride_row + b * sa_stride_k], and the same with block_b
 * and the sb strides gives sb(n,b) over the rows n of B_nk.  Strides count floats and must be >= 0; any layout is read in place:
 * torch's outer-dim-major (M, K/128) with stride (1, M), plain row-major, or DeepSeek's weight_scale_inv (ceil(N/128),
 * ceil(K/128)).  block_a, block_b: FP8MI_BLOCK_1 or FP8MI_BLOCK_128, all four pairs (torch's _scaled_mm uses (1, 128) and
 * (1, 1); (128, 1) is what a caller needs with FP8MI_EPILOGUE_TRANSPOSED, which keeps its meaning).
 * Matrix-core kernels: each P_b is the MFMA's sum with unit block scales, started from zero (the accuracy note of
 * fp8mi_scaled_mm), folded into the accumulator in block order as acc = fmaf(P_b, sa*sb, acc) with sa*sb rounded to fp32.
 * They take the tensorwise alignment (K, lda, ldb multiples of 16, 16-byte aligned operands), 4-byte aligned scale pointers
 * and scale extents below 2^31 bytes; otherwise AUTO runs the generic kernel and a forced tile returns FP8MI_E_UNSUPPORTED.
 * FP8MI_KERNEL_GENERIC sums P_b over exact products in IEEE fp32 and applies the same fold.  A scale of inf or NaN, or an
 * overflowing fold, gives IEEE results; NaN bytes follow nan_mode (the NaN-detect-and-redo of the matrix-core kernels may
 * fire on a NaN that came from a scale: that costs time only, as for MXFP8).  M = 0 or N = 0 is a no-op; with K = 0 the
 * scale pointers may be NULL.
 * kernel: FP8MI_KERNEL_AUTO (the cheapest blockwise ring tile by the tensorwise cost model; generic as the last resort),
 * FP8MI_KERNEL_GEMM_{128, 128x64, 64x128, 64x64, 32x64, 32x32, 128D} or FP8MI_KERNEL_GENERIC; the vec-mat, few-rows, skinny,
 * 256x256 and one-wave-per-SIMD kernels have no blockwise form: FP8MI_E_UNSUPPORTED.  split_k / workspace as in
 * fp8mi_scaled_mm_ws (slices on 128-k boundaries).  Every argument check runs before any HIP call.
 */
/* rows of an operand that share one scale per 128 k: 1 ("1x128") or 128 ("128x128") */
enum { FP8MI_BLOCK_1 = 1, FP8MI_BLOCK_128 = 128 };

int fp8mi_scaled_mm_blockwise(const uint8_t *A, const uint8_t *B_nk, void *C,
                              const float *scale_a, int64_t sa_stride_row, int64_t sa_stride_k, int block_a,
                              const float *scale_b, int64_t sb_stride_row, int64_t sb_stride_k, int block_b,
                              const void *bias, const float *scale_result,
                              int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                              int out_dtype, int bias_dtype, int nan_mode,
                              int kernel, int split_k, void *workspace, int64_t workspace_bytes, void *stream);

/* Which kernel FP8MI_KERNEL_AUTO of fp8mi_scaled_mm_blockwise runs for this shape (host-only; operands 16-byte aligned,
 * scales in torch's outer-dim-major layout); a negative error for an invalid argument. */
int fp8mi_choose_kernel_blockwise(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype,
                                  int block_a, int block_b, int has_workspace, int split_k);

/*
 * Blockwise quantisation of a (rows, cols) f32 / f16 / bf16 matrix (row stride ld_in elements), blocks of block_rows (1 or 128)
 * x 128 columns, partial blocks at the edges: e4m3 bytes out (rows, cols; ld_out) and one fp32 scale per block at
 * scales[rb * s_stride_row + cb * s_stride_k] (the dequantisation scale _scaled_mm consumes):
 *   amax = max|x| over the block, widened to fp32 (NaN if the block holds a NaN)
 *   s = amax / 448.0f (IEEE division);  s = 1.0f when amax / 448.0f == 0.0f (an all-zero block, or an f32 amax below about
 *   448 x 2^-150 whose quotient underflows: the block's elements then round to 0 and finite input never yields NaN bytes)
 *   q = e4m3fn_rne(clamp(x / s, -448, 448))  (IEEE division; a NaN quotient - NaN input, inf / inf - is stored as 0x7F)
 */
int fp8mi_quantize_blockwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int block_rows,
                             uint8_t *out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k, void *stream);

/* out[r,c] = cast(float(dec(in[r,c])) * s(r / block_rows, c / 128)), out contiguous (rows, cols) of out_dtype; OCP decode
 * (NaN bytes give NaN), the product in fp32 rounded once, then RNE to out_dtype. */
int fp8mi_dequant_blockwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, int block_rows,
                            const float *scales, int64_t s_stride_row, int64_t s_stride_k, void *out, int out_dtype, void *stream);

/*
 * Per-row dynamic quantisation of a (rows, cols) f32 / f16 / bf16 matrix (row stride ld_in elements): fp8mi_quantize (e4m3) or
 * fp8mi_quantize_e5m2 applied to every row on its own - one scale per token for activations, per output channel for weights; the
 * scales FP8MI_SCALE_ROW of fp8mi_scaled_mm consumes.  No counterpart in the reference (its fp8_quantize is per tensor).  For row r:
 *   amax_r = max_c |float32(in[r,c])| (NaNs ignored; 0 for cols == 0);  scale_r = amax_r > 0 ? FMAX / amax_r : 1 (evaluated in double,
 *   rounded to fp32);  FMAX = 448 (FP8MI_FMT_E4M3) or 57344 (FP8MI_FMT_E5M2)
 *   e4m3: out[r,c] = enc<encode_mode>(float32(in[r,c]) * scale_r)                  (FP8MI_ENC_REFERENCE or FP8MI_ENC_RNE)
 *   e5m2: out[r,c] = e5m2_rne(clamp(float32(in[r,c]) * scale_r, -57344, 57344))    (a NaN stays NaN; encode_mode must be FP8MI_ENC_RNE:
 *         e5m2 is OCP only, FP8MI_E_UNSUPPORTED otherwise)
 *   inv_scales[r] = float32(1 / (FMAX / amax_r)), or 1;  amax[r] = amax_r when `amax` is not NULL.
 * Non-finite input behaves as in fp8mi_quantize, row by row (an inf makes the row's scale 0 and its inverse inf).
 * One kernel launch, no workspace, no atomics, no host sync (safe inside a HIP graph capture).  Rows of up to 16384 elements whose
 * base, ld_in (in bytes) and ld_out allow 16-byte loads and 4- / 8-byte stores are read from memory once; anything else is correct, slower.
 * rows == 0 is a no-op (NULL pointers accepted); cols == 0 writes inv_scales[r] = 1 and amax[r] = 0.  Every argument check runs before
 * any HIP call.
 */
int fp8mi_quantize_rowwise(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in,
                           uint8_t *out, int64_t ld_out, float *inv_scales /* [rows] */, float *amax /* [rows] or NULL */,
                           int out_format /* FP8MI_FMT_* */, int encode_mode, void *stream);

/* out[r,c] = cast(float(dec(in[r,c])) * scales[r]), out contiguous (rows, cols) of out_dtype; in_format FP8MI_FMT_*; OCP decode
 * (NaN bytes give NaN; e5m2 inf stays inf), the product in fp32 rounded once, then RNE to out_dtype. */
int fp8mi_dequant_rowwise(const uint8_t *in, int64_t rows, int64_t cols, int64_t ld_in, const float *scales /* [rows] */,
                          int in_format, void *out /* contiguous (rows, cols) */, int out_dtype, void *stream);

/*
 * Fused activation (+ gate product) + quantisation: the producer of the second GEMM's operand in an FP8 MLP, in one launch.
 * `cols` counts OUTPUT columns.  Ungated: `in` is (rows, cols) and y[r,c] = act(x[r,c]).  Gated (act | FP8MI_ACT_GATED): `in` is
 * (rows, 2 cols), ld_in >= 2 cols, the gate is column c and the up value column cols + c - h.chunk(2, -1), the [gate | up] layout of a
 * fused gate_up projection - and y[r,c] = act(gate) * up.  Everything is fp32 on the widened input; y is never rounded to the input type:
 *   FP8MI_ACT_NONE       y = x                                                   (gated: exactly fl32(gate * up))
 *   FP8MI_ACT_SILU       g / (1 + exp(-g))
 *   FP8MI_ACT_GELU_TANH  0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3)))
 *   FP8MI_ACT_GELU_ERF   0.5 g (1 + erf(g / sqrt 2))
 * the three functions to a few fp32 ulps of their exact value wherever |y| >= 1e-36 (smaller results become -0), also in the negative
 * tail, where the formulas as written cancel; the gate product is one fp32 multiply.  A NaN gate gives that NaN.
 * FP8MI_QSCALE_ROW: the recipe of fp8mi_quantize_rowwise applied to y - amax_r = max_c |y[r,c]| (NaNs ignored), scale_r = FMAX / amax_r
 *   in double (1 for amax_r == 0), out = enc(y * scale_r); out_format FP8MI_FMT_E4M3 with either encode mode, or FP8MI_FMT_E5M2 with
 *   FP8MI_ENC_RNE; scales[r * s_stride_row] = float32(1 / (FMAX / amax_r)) or 1, amax[r] = amax_r when `amax` is not NULL.
 *   cols == 0 writes 1 and 0.  (Under FP8MI_ENC_REFERENCE a result that underflowed to -0 is stored as 0x00, a tiny negative one as 0x80.)
 * FP8MI_QSCALE_GROUP128: the recipe of fp8mi_quantize_blockwise(block_rows = 1) applied to y - amax per 128 output columns (the last
 *   group partial; NaN if the group holds one), s = amax / 448.0f (1.0f where that quotient is 0), out = e4m3fn_rne(clamp(y / s, -448,
 *   448)) with the IEEE division, a NaN quotient as 0x7F; scales[r * s_stride_row + cb * s_stride_k] = s.  e4m3 / FP8MI_ENC_RNE only and
 *   `amax` must be NULL: FP8MI_E_UNSUPPORTED otherwise.
 * With FP8MI_ACT_NONE, ungated, the bytes and scales are those of fp8mi_quantize_rowwise / fp8mi_quantize_blockwise(.., 1, ..).
 * One kernel launch, no workspace, no atomics, no host sync (safe inside a HIP graph capture).  Rows of up to 16384 output columns whose
 * base and ld_in (in bytes) allow 16-byte loads - gated: also cols * element size a multiple of 16 - and whose output rows allow 4- / 8-byte
 * stores are read from memory once; anything else is correct, slower.  `out` must not alias `in`.  rows == 0 is a no-op (NULL pointers
 * accepted).  FP8MI_E_ENUM for an unknown act, scale_mode, in_dtype, out_format or encode_mode; FP8MI_E_SHAPE for a negative size or
 * stride or a leading dimension that is too small; FP8MI_E_NULL for a missing pointer.  Every argument check runs before any HIP call.
 */
enum { FP8MI_ACT_NONE = 0, FP8MI_ACT_SILU = 1, FP8MI_ACT_GELU_TANH = 2, FP8MI_ACT_GELU_ERF = 3 };
#define FP8MI_ACT_GATED 0x100 /* OR into `act` */
enum { FP8MI_QSCALE_ROW = 0, FP8MI_QSCALE_GROUP128 = 1 };

int fp8mi_act_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act,
                       uint8_t *out, int64_t ld_out,
                       float *scales, int64_t s_stride_row, int64_t s_stride_k, float *amax /* [rows], FP8MI_QSCALE_ROW only, or NULL */,
                       int scale_mode, int out_format /* FP8MI_FMT_* */, int encode_mode, void *stream);

/*
 * Fused RMSNorm / LayerNorm (+ residual add, affine parameters, adaLN modulation) + quantisation: the producer of the FIRST GEMM's
 * operand of a transformer block, in one launch.  `in` is (rows, cols) f32 / f16 / bf16 with row stride ld_in.  Every operation below is
 * ONE individually rounded fp32 operation on exactly widened inputs - fl32(.) - and nothing is fused into a multiply-add:
 *   1. h = x.  With `residual` (rows, cols) of in_dtype, row stride ld_res:  h_out[r,c] = rne_to_in_dtype(fl32(x + res)), and h is the
 *      widening of what was stored: the call equals `x + res` in in_dtype followed by the call without a residual, byte for byte.
 *      `h_out` (row stride ld_h) is required exactly when `residual` is given; it may be the residual's own buffer (in-place stream
 *      update) and must not overlap `in` or `out`.
 *   2. FP8MI_NORM_RMS:    d = h;                                      ms  = (sum_c d^2) / cols;  rstd = 1 / sqrt(ms + eps)
 *      FP8MI_NORM_LAYER:  mean = (sum_c h) / cols;  d = fl32(h - mean);  var = (sum_c d^2) / cols;  rstd = 1 / sqrt(var + eps)
 *      (two passes, never E[h^2] - mean^2).  The sums are fp32: every lane adds its own elements, the lanes meet in a tree - at least 64
 *      independent partial sums for a row of more than 64 elements.  mean and rstd are ONE fp32 value each per row: what is written to
 *      mean_out[r] / rstd_out[r] (NULL or float [rows]; mean_out with FP8MI_NORM_LAYER only) is what every element is computed with.
 *   3. z = fl32(d * rstd);  with `weight`: z = fl32(z * w[c]);  with `bias`: z = fl32(z + b[c]);  with mod_scale / mod_shift (both or
 *      neither): z = fl32(fl32(z * fl32(1 + sc[g,c])) + sh[g,c]),  g = r / rows_per_mod - adaLN's one row per image, broadcast over
 *      its rows_per_mod tokens; the two are (ceil(rows / rows_per_mod), cols) with row stride ld_mod.  y = z, never rounded to in_dtype.
 *      weight, bias, mod_scale, mod_shift share ONE param_dtype: in_dtype or FP8MI_F32 (FP8MI_E_UNSUPPORTED otherwise).
 *   4. y is quantised by FP8MI_QSCALE_ROW or FP8MI_QSCALE_GROUP128 exactly as in fp8mi_act_quantize: the same expressions, encoders, NaN
 *      rules, restrictions (GROUP128 is e4m3 / FP8MI_ENC_RNE only and takes no amax; e5m2 is FP8MI_ENC_RNE only) and cols == 0 behaviour
 *      (mean_out / rstd_out are not written for cols == 0).
 * Non-finite input: plain IEEE arithmetic decides.  A NaN in a row makes its statistics and every y of the row NaN; so does an infinity
 * under FP8MI_NORM_LAYER (mean is inf or NaN, d is -inf or NaN).  Under FP8MI_NORM_RMS a row with infinities and no NaN has ms = inf and
 * rstd = 0: its finite elements give z = 0 and the infinite ones NaN.  The recipes' NaN rules then apply; where two NaNs meet in one
 * operation the sign of the result is not specified.
 * One kernel launch, no workspace, no atomics, no host sync (safe inside a HIP graph capture).  Rows of up to 16384 columns, a multiple
 * of 16 bytes long, whose bases and leading dimensions (x, residual, h_out, parameters, modulation rows) allow 16-byte accesses and
 * whose output rows allow 4- / 8-byte stores are read from memory once; anything else is correct, slower.  rows == 0 is a no-op (NULL
 * pointers accepted).  FP8MI_E_ENUM for an unknown norm, scale_mode, in_dtype, param_dtype, out_format or encode_mode; FP8MI_E_SHAPE for
 * a negative size or stride, a leading dimension that is too small, rows_per_mod < 1 with modulation; FP8MI_E_NULL for a missing pointer,
 * one of mod_scale / mod_shift or of residual / h_out without the other included.  Every argument check runs before any HIP call.
 */
enum { FP8MI_NORM_RMS = 0, FP8MI_NORM_LAYER = 1 };

int fp8mi_norm_quantize(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int norm, float eps,
                        const void *weight /* [cols] or NULL */, const void *bias /* [cols] or NULL */,
                        const void *mod_scale, const void *mod_shift /* both or neither */, int64_t ld_mod, int64_t rows_per_mod, int param_dtype,
                        const void *residual, int64_t ld_res, void *h_out, int64_t ld_h,
                        uint8_t *out, int64_t ld_out,
                        float *scales, int64_t s_stride_row, int64_t s_stride_k, float *amax /* [rows], FP8MI_QSCALE_ROW only, or NULL */,
                        int scale_mode, int out_format /* FP8MI_FMT_* */, int encode_mode,
                        float *mean_out /* [rows], FP8MI_NORM_LAYER only, or NULL */, float *rstd_out /* [rows] or NULL */, void *stream);

/*
 * MXFP8 / MXFP4 output of the two fused producers: one launch from the activation (or the normalised hidden state) to the operand of
 * fp8mi_scaled_mm_mxfp8 / fp8mi_scaled_mm_mxfp4.  y is defined word for word as in fp8mi_act_quantize, and in steps 1 - 3 of
 * fp8mi_norm_quantize: the same fp32 expressions, gate layout, residual / h_out rule, statistics outputs and NaN / inf arithmetic; y is
 * fp32 and never rounded to the input type.  y is then quantised by the recipe of fp8mi_quantize_mxfp8 (FP8MI_MX_FP8) or
 * fp8mi_quantize_mxfp4 (FP8MI_MX_FP4) applied to y as an fp32 matrix - byte for byte torch's to_mxfp(y, 32, "mxfp8" | "mxfp4"): per block
 * of 32 columns amax (NaN if the block holds one), descale = fl32(amax / 448) or fl32(amax / 6), the RCEIL exponent
 * e = clamp(ceil(log2(descale)), -127, 127) + 127 with log2 correctly rounded to fp32 (just above a power of two it returns the power),
 * e = 0xFF for a block with a NaN; elements fl32(y * 2^(127 - e)) (factor 1 for e == 0) clamped to +-448 / +-6 and rounded to e4m3fn
 * (RNE; a NaN element is 0x7F with its sign bit), or through bfloat16 (RNE) to e2m1 (RNE, saturating; a NaN element is code 0xC).
 * `cols` counts output columns and must be a multiple of 32 (FP8MI_E_SHAPE otherwise).  FP8MI_MX_FP8: `out` is (rows, cols) bytes,
 * ld_out >= cols.  FP8MI_MX_FP4: `out` is (rows, cols / 2) bytes, the even column in the low nibble, ld_out >= cols / 2.  `scales` is
 * (rows, cols / 32) E8M0 bytes, row-major, ld_s >= cols / 32.  When ld_s >= round_up(cols / 32, 4) the bytes cols / 32 ..
 * round_up(cols / 32, 4) - 1 of every scale row are written as 0x7F (2^0): the matrix-core GEMMs read scale rows in 4-byte steps, and a
 * stray 0xFF there is a NaN.  Otherwise exactly cols / 32 bytes per row are written.  Nothing else in `out` or `scales` is touched.
 * With FP8MI_ACT_NONE, ungated, the bytes and scale bytes are those of fp8mi_quantize_mxfp8 / fp8mi_quantize_mxfp4.
 * One kernel launch, no workspace, no atomics, no host sync (safe inside a HIP graph capture).  The single-read forms need what the two
 * functions above need, with output rows that allow 8- / 4-byte (MXFP4: 4- / 2-byte) stores; scale rows that are 4-byte aligned take one
 * dword per 128 columns.  Anything else is correct, slower.  `out` and `scales` must not alias the inputs.  rows == 0 or cols == 0 is a
 * no-op that still validates enums and shapes (NULL pointers accepted).  FP8MI_E_ENUM for an unknown act / norm, mx_format, in_dtype or
 * param_dtype; FP8MI_E_SHAPE for a negative size, cols % 32 != 0, a leading dimension that is too small, rows_per_mod < 1 with
 * modulation; FP8MI_E_UNSUPPORTED for a param_dtype that is neither in_dtype nor FP8MI_F32 and for mean_out with FP8MI_NORM_RMS;
 * FP8MI_E_NULL for a missing pointer, one of mod_scale / mod_shift or of residual / h_out without the other included.  Every argument
 * check runs before any HIP call.
 */
enum { FP8MI_MX_FP8 = 0, FP8MI_MX_FP4 = 1 };   /* element format of an MX output */

int fp8mi_act_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int act,
                          uint8_t *out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format, void *stream);

int fp8mi_norm_quantize_mx(const void *in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in, int norm, float eps,
                           const void *weight /* [cols] or NULL */, const void *bias /* [cols] or NULL */,
                           const void *mod_scale, const void *mod_shift /* both or neither */, int64_t ld_mod, int64_t rows_per_mod, int param_dtype,
                           const void *residual, int64_t ld_res, void *h_out, int64_t ld_h,
                           uint8_t *out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format,
                           float *mean_out /* [rows], FP8MI_NORM_LAYER only, or NULL */, float *rstd_out /* [rows] or NULL */, void *stream);

/*
 * Grouped (mixture-of-experts) GEMM: ONE launch over tokens sorted by expert, each run of rows against its own expert's weights -
 * what torch._scaled_grouped_mm computes on its 2D x 3D layout (no counterpart in the reference).
 *
 *   A (M_total, K) e4m3fn bytes, row-major (lda);  B_gnk (G, N, K), K contiguous, rows ldb bytes apart, experts stride_b bytes
 *   apart;  C (M_total, N) out_dtype (ldc);  offs int32[G] in DEVICE memory: cumulative row ends (torch's convention).
 *
 * Group g owns rows [start_g, end_g):  start_0 = 0, start_g = end_{g-1}, end_g = clamp(offs[g], start_g, M_total); for a
 * non-decreasing offs inside [0, M_total] that is [offs[g-1], offs[g]).  The clamps are part of the definition: no content of
 * offs makes a kernel read or write outside the M_total rows of A, C and the row scales.  Empty groups are legal; rows at or
 * beyond end_{G-1} are not written.  For the rows m of group g
 *   C[m,n] = cast( ((sum_k dec(A[m,k]) dec(B[g,n,k])) * sa[m] * sb[g,n] + bias[g,n]) * scale_result )
 * with the epilogue order and NaN modes of fp8mi_scaled_mm: scale_a float[1] or float[M_total] (scale_a_mode), scale_b float[G]
 * (FP8MI_SCALE_TENSOR: one per expert) or float[G * N] (FP8MI_SCALE_ROW), bias NULL or [G, N] of bias_dtype.  A group's rows
 * equal, bit for bit, fp8mi_scaled_mm_ex on those rows with the same ring tile.
 * The host never reads offs: no sync, no workspace, no atomics, capturable into a HIP graph and replayable after offs changed.
 * The grid holds M_total / BM + G m-tile slots per n-tile (enough for any offs); surplus slots return at once.
 * kernel: FP8MI_KERNEL_AUTO or FP8MI_KERNEL_GEMM_{128, 128x64, 64x128, 64x64, 32x64, 32x32, 128D}.  There is no split-K and no
 * generic form: FP8MI_E_UNSUPPORTED for G > 1024, a slot grid beyond 2^31 - 1 workgroups, K = 0, operands the ring tiles
 * cannot read (K, lda, ldb, stride_b multiples of 16, 16-byte aligned A and B_gnk, lda and ldb below 2^22), any other kernel
 * id of fp8mi_scaled_mm, and FP8MI_EPILOGUE_TRANSPOSED.  FP8MI_E_NULL: A, B_gnk, C, scale_a, scale_b, or offs (required when
 * G > 0 and M_total > 0); FP8MI_E_SHAPE: a negative size, lda / ldb < K, ldc < N, stride_b < (N - 1) * ldb + K, G < 1;
 * FP8MI_E_ENUM: unknown modes, dtypes or kernel ids.  M_total = 0 or N = 0 is a no-op.  Every argument check runs before any
 * HIP call.
 */
int fp8mi_scaled_mm_grouped(const uint8_t *A, const uint8_t *B_gnk, void *C, const float *scale_a, const float *scale_b,
                            const void *bias, const float *scale_result, const int32_t *offs, int G,
                            int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc,
                            int scale_a_mode, int scale_b_mode, int out_dtype, int bias_dtype, int nan_mode, int kernel, void *stream);

/*
 * The blockwise form of the grouped GEMM (fp8mi_scaled_mm_blockwise per group): activation scales 1x128 over the whole
 * (M_total, ceil(K/128)) matrix, sa(m,b) = scale_a[m * sa_stride_row + b * sa_stride_k]; block_a must be FP8MI_BLOCK_1 (group
 * starts are not 128-aligned: FP8MI_E_UNSUPPORTED for FP8MI_BLOCK_128).  Weight scales per expert, block_b 1 or 128:
 * sb(g,n,b) = scale_b[g * sb_stride_expert + (n / block_b) * sb_stride_row + b * sb_stride_k].  Strides count floats, >= 0.
 * Everything else - groups, offs, bias, return codes, kernels - as fp8mi_scaled_mm_grouped; the scale pointers must be 4-byte
 * aligned and the scale extents below 2^31 bytes (FP8MI_E_UNSUPPORTED).  A group's rows equal fp8mi_scaled_mm_blockwise on
 * those rows with the same ring tile and split_k = 1, bit for bit.
 */
int fp8mi_scaled_mm_grouped_blockwise(const uint8_t *A, const uint8_t *B_gnk, void *C,
                                      const float *scale_a, int64_t sa_stride_row, int64_t sa_stride_k, int block_a,
                                      const float *scale_b, int64_t sb_stride_row, int64_t sb_stride_k, int64_t sb_stride_expert, int block_b,
                                      const void *bias, const float *scale_result, const int32_t *offs, int G,
                                      int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t stride_b, int64_t ldc,
                                      int out_dtype, int bias_dtype, int nan_mode, int kernel, void *stream);

/* Which ring tile FP8MI_KERNEL_AUTO of the grouped entry points runs (host-only): the tensorwise cost model priced at ONE
 * problem of ceil(M_total / G) rows, restricted to the seven ring tiles.  It is NOT fitted to grouped timings (it knows
 * neither the G problems that share the chip nor the surplus slots).  A negative error for an invalid argument or a shape the
 * grouped kernels do not take. */
int fp8mi_choose_kernel_grouped(int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype);

/*
 * The MXFP8 / MXFP4 forms of the grouped GEMM (fp8mi_scaled_mm_mxfp8 / _mxfp4 per group): E8M0 block scales, one byte per 32 k,
 * applied inside the scaled MFMAs.  scale_a is (M_total, K/32) bytes with row stride ld_sa; scale_b is (G, N, K/32) with ld_sb
 * bytes between rows and stride_sb bytes between experts.  For the rows m of group g
 *   C[m,n] = cast( (sum_blocks 2^(sa[m,b]-127) 2^(sb[g,n,b]-127) sum_{k in b} dec(A[m,k]) dec(B[g,n,k]) + bias[g,n]) * scale_result )
 * MXFP4: A and B_gnk hold two e2m1 codes per byte; K counts ELEMENTS, lda, ldb and stride_b count BYTES; there is no nan_mode
 * (e2m1 has no NaN encoding).  Groups, the clamps of offs, G <= 1024, the slot grid, bias [G, N], scale_result and the kernels are
 * fp8mi_scaled_mm_grouped's.  A group's rows equal, bit for bit, fp8mi_scaled_mm_mxfp8 / _mxfp4 on those rows with the same ring
 * tile and split_k = 1 (MXFP8: under either nan_mode); a group's scale reads cannot reach another group's rows or another
 * expert's scales.  No split-K, no workspace, no atomics, no generic form.
 * FP8MI_E_SHAPE: a negative size, K % 32 != 0, lda / ldb below a row's bytes, ldc < N, ld_sa / ld_sb < K / 32,
 * stride_b < (N - 1) * ldb + a row's bytes, stride_sb < (N - 1) * ld_sb + K / 32, G < 1.  FP8MI_E_UNSUPPORTED: operands the ring
 * tiles cannot read (as fp8mi_scaled_mm_grouped, on the operands' bytes); ld_sa, ld_sb or stride_sb not multiples of 4 or a scale
 * pointer not 4-byte aligned (group starts are arbitrary rows: every rebased scale base must stay 4-byte aligned); G > 1024; K = 0;
 * FP8MI_EPILOGUE_TRANSPOSED; any other kernel id of fp8mi_scaled_mm.  FP8MI_E_NULL / FP8MI_E_ENUM as fp8mi_scaled_mm_grouped.
 * M_total = 0 or N = 0 is a no-op.  Every argument check runs before any HIP call.
 */
int fp8mi_scaled_mm_grouped_mxfp8(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa,
                                  const uint8_t *scale_b, int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result,
                                  const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                  int64_t stride_b, int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel, void *stream);
int fp8mi_scaled_mm_grouped_mxfp4(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa,
                                  const uint8_t *scale_b, int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result,
                                  const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                  int64_t stride_b, int64_t ldc, int out_dtype, int bias_dtype, int kernel, void *stream);

/* Which ring tile FP8MI_KERNEL_AUTO of the two entry points above runs (host-only; mx_format FP8MI_MX_FP8 / FP8MI_MX_FP4): the
 * choice of fp8mi_choose_kernel_mxfp8 / _mxfp4 - the tensorwise cost model, MXFP4 priced at its byte depth K / 2 - for ONE problem
 * of ceil(M_total / G) rows, restricted to the seven ring tiles.  It is NOT fitted to grouped (or to MX) timings.  A negative
 * error for an invalid argument or a shape the grouped kernels do not take. */
int fp8mi_choose_kernel_grouped_mx(int mx_format, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                                   int out_dtype);

/*
 * The MXW4A8 form of the grouped GEMM (fp8mi_scaled_mm_mxw4a8 per group): A (M_total, K) e4m3 bytes, lda >= K; B_gnk (G, N, K/2)
 * bytes of two e2m1 codes, ldb >= K/2 and stride_b in BYTES; K counts elements.  Scales, groups, the clamps of offs, the slot grid,
 * bias [G, N], scale_result, the error codes (each operand's row bytes checked against its own element size) and the 4-byte
 * alignment rule of ld_sa, ld_sb and stride_sb are fp8mi_scaled_mm_grouped_mxfp8's; nan_mode as in fp8mi_scaled_mm_mxw4a8.  A
 * group's rows equal, bit for bit, fp8mi_scaled_mm_mxw4a8 on those rows with the same ring tile and split_k = 1, under either
 * nan_mode.  No split-K, no workspace, no atomics, no generic form.
 */
int fp8mi_scaled_mm_grouped_mxw4a8(const uint8_t *A, const uint8_t *B_gnk, void *C, const uint8_t *scale_a, int64_t ld_sa,
                                   const uint8_t *scale_b, int64_t ld_sb, int64_t stride_sb, const void *bias, const float *scale_result,
                                   const int32_t *offs, int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                   int64_t stride_b, int64_t ldc, int out_dtype, int bias_dtype, int nan_mode, int kernel, void *stream);

/* Which ring tile FP8MI_KERNEL_AUTO of fp8mi_scaled_mm_grouped_mxw4a8 runs (host-only): the choice of fp8mi_choose_kernel_grouped_mx
 * priced at the weights' byte depth K / 2 - not fitted to grouped, MX or mixed timings.  A negative error for an invalid argument
 * (K % 32 != 0 included) or a shape the grouped kernels do not take (lda or ldb no multiple of 16: FP8MI_E_UNSUPPORTED). */
int fp8mi_choose_kernel_grouped_mxw4a8(int G, int64_t M_total, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int out_dtype);

/*
 * MoE routing on the device: from the gate's expert ids to the sorted rows the grouped GEMMs read, and back.  Three calls; none
 * syncs the host, none uses a global atomic or leaves a result that depends on the order in which workgroups ran, all are
 * capturable into a HIP graph and replay on new ids.  Every argument check runs before any HIP call.
 *
 * fp8mi_moe_route - the stable sort by expert.  `ids` holds n = T k expert ids, row-major (assignment i = t k + j), int32
 * (id_bytes 4) or int64 (8).  Assignment i is VALID iff 0 <= ids[i] < G; any other id drops the assignment (no error: this is how
 * an expert-parallel caller masks the experts of other ranks).  A token that names an expert twice owns two rows.  Outputs, int32
 * in device memory:
 *   offs[g]       = #{valid i : ids[i] <= g}, g < G: the offs of fp8mi_scaled_mm_grouped
 *   row_of[i]     = (g ? offs[g-1] : 0) + #{i' < i : ids[i'] == ids[i]} with g = ids[i] for a valid i;  -1 for a dropped one
 *   src_of_row[r] = the i with row_of[i] == r for r < offs[G-1];  -1 for offs[G-1] <= r < n.  May be NULL.
 * n <= FP8MI_MOE_ROUTE_SINGLE_MAX is ONE launch of one workgroup and needs no workspace; a larger n is three launches (count per
 * chunk of FP8MI_MOE_ROUTE_CHUNK assignments, scan, rank) and a caller-owned workspace of fp8mi_moe_route_workspace_bytes(n, G)
 * bytes, 4-byte aligned, whose content before and after the call is of no interest.  fp8mi_moe_route_workspace_bytes is 0 for the
 * one-launch form, non-decreasing in n and G, and a negative error code for sizes fp8mi_moe_route rejects.
 * FP8MI_E_SHAPE: n < 0, G < 1, a workspace that is too small;  FP8MI_E_UNSUPPORTED: G > 1024 (the grouped GEMM's maximum),
 * n >= 2^31, a pointer not aligned to its element size;  FP8MI_E_ENUM: id_bytes other than 4 or 8;  FP8MI_E_NULL: ids, offs,
 * row_of, or the workspace where one is needed.  n == 0 is a no-op that still validates (nothing is written, offs included).
 *
 * fp8mi_moe_scatter_quantize - quantise a token once, store it k times.  `in` is (T, cols) f32 / f16 / bf16 (ld_in); for every
 * token t the row is quantised once, in registers, and its bytes and scale(s) are stored to each row row_of[t k + j], j < k, of
 * `out` (rows_out, cols) bytes (ld_out) and of `scales`.  A destination outside [0, rows_out) is skipped, -1 included: no content
 * of row_of makes the call touch memory outside `out` and `scales`.  Rows that no assignment names are not written.  e4m3 only:
 *   FP8MI_QSCALE_ROW       the bytes and the inverse scale (scales[row * s_stride_row]) of fp8mi_quantize_rowwise, either encode mode
 *   FP8MI_QSCALE_GROUP128  the bytes and scales (scales[row * s_stride_row + cb * s_stride_k]) of fp8mi_act_quantize(FP8MI_ACT_NONE,
 *                          FP8MI_QSCALE_GROUP128); FP8MI_ENC_RNE only
 * of token t, bit for bit.  Like the grouped GEMM it feeds this call has no generic form: FP8MI_E_UNSUPPORTED for cols % 16 != 0,
 * cols > 16384, `in` not 16-byte or `out` not 8-byte aligned, ld_in * element size not a multiple of 16 (T > 1), ld_out not a
 * multiple of 8 (rows_out > 1), FP8MI_FMT_E5M2.  FP8MI_E_SHAPE / _ENUM / _NULL as fp8mi_act_quantize.  T == 0 or k == 0 is a no-op.
 *
 * fp8mi_moe_scatter_quantize_mx - the same with an MX output: the bytes and E8M0 scale bytes (scales[row * ld_s + block]) of
 * fp8mi_quantize_mxfp8 (FP8MI_MX_FP8: `out` (rows_out, cols) bytes) or fp8mi_quantize_mxfp4 (FP8MI_MX_FP4: (rows_out, cols / 2)
 * bytes, the even column in the low nibble) of token t, bit for bit - a block with a NaN gets the scale 0xFF and NaN elements as
 * there.  When ld_s >= round_up(cols / 32, 4), the pad bytes cols / 32 .. round_up(cols / 32, 4) - 1 of every written scale row
 * are stored as 0x7F (2^0), so that the grouped MX GEMMs read the scales in place.  FP8MI_E_SHAPE: a negative size, cols % 32 != 0,
 * ld_in < cols, ld_out below a row's bytes, ld_s < cols / 32.  FP8MI_E_UNSUPPORTED: cols > 16384, `in` not 16-byte aligned, `out`
 * not aligned to 8 (MXFP4: 4) bytes, ld_in * element size not a multiple of 16 (T > 1), ld_out not a multiple of 8 (MXFP4: 4;
 * rows_out > 1), row_of not 4-byte aligned: there is no generic form.  T == 0, k == 0 or cols == 0 is a no-op.
 *
 * fp8mi_moe_combine - the weighted un-permute.  `y` is (rows, N) f32 / f16 / bf16 (ld_y), `weights` float [T, k] or NULL for 1,
 * `out` (T, N) of out_dtype (ld_out):  out[t,c] = cast(acc_k),  acc_0 = 0,  acc_{j+1} = fl32(acc_j + fl32(w[t,j] * float(y[row_of[t k + j], c])))
 * for j = 0 .. k-1 in that order - two individually rounded fp32 operations per assignment, never a fused multiply-add.  An
 * assignment whose row lies outside [0, rows) is skipped; a token with none gets zeros.  Every one of the T output rows is
 * written and nothing else is.  A gather without atomics: 16-byte loads where N, the bases and the leading dimensions allow, one
 * column per lane otherwise (any N).  T == 0 or N == 0 is a no-op.  FP8MI_E_SHAPE: a negative size, ld_y or ld_out < N;
 * FP8MI_E_ENUM: unknown dtypes;  FP8MI_E_NULL: out, row_of (k > 0), y (k > 0 and rows > 0);  FP8MI_E_UNSUPPORTED: a pointer not
 * aligned to its element size, N beyond 65535 * 256 lanes' worth of columns.
 */
#define FP8MI_MOE_ROUTE_CHUNK 1024      /* assignments per workgroup of the three-launch form */
#define FP8MI_MOE_ROUTE_SINGLE_MAX 1024 /* the largest n of the one-launch form */

int64_t fp8mi_moe_route_workspace_bytes(int64_t n, int G);
int fp8mi_moe_route(const void *ids, int id_bytes, int64_t n, int G, int32_t *offs /* [G] */, int32_t *row_of /* [n] */,
                    int32_t *src_of_row /* [n] or NULL */, void *workspace, int64_t workspace_bytes, void *stream);
int fp8mi_moe_scatter_quantize(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of /* [T, k] */, int k,
                               uint8_t *out, int64_t rows_out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k,
                               int scale_mode, int out_format /* FP8MI_FMT_E4M3 */, int encode_mode, void *stream);
int fp8mi_moe_scatter_quantize_mx(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of /* [T, k] */, int k,
                                  uint8_t *out, int64_t rows_out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format, void *stream);
int fp8mi_moe_combine(const void *y, int y_dtype, int64_t rows, int64_t N, int64_t ld_y, const int32_t *row_of /* [T, k] */,
                      const float *weights /* [T, k] or NULL */, int64_t T, int k, void *out, int out_dtype, int64_t ld_out, void *stream);

/*
 * fp8mi_moe_gate - the gate: from the router's logits (T, G) f32 / f16 / bf16 (ld) to the ids [T, k] and weights [T, k] that
 * fp8mi_moe_route and fp8mi_moe_combine read, in ONE launch: softmax or sigmoid scores, a selection-only bias, group-limited routing,
 * renormalisation and a scale.  No host sync, no global atomic, no workspace; capturable into a HIP graph, replays on new logits.
 * Every argument check runs before any HIP call.  Per token t, every operation an individually rounded fp32 operation unless stated:
 *   1. x_e = float(logits[t ld + e]), exact.
 *   2. the score s_e:  FP8MI_GATE_SOFTMAX  exp(x_e - m) / sum_e' exp(x_e' - m),  m = max x over all G experts (a softmax followed by
 *      a top-k, not a top-k followed by a softmax);  FP8MI_GATE_SIGMOID  1 / (1 + exp(-x_e)).
 *   3. the key:  PLAIN form (bias == NULL and n_group == 1)  key_e = x_e - both scorings are monotone in the logit, so the selection
 *      is exact and reproducible on any host;  SCORED form (anything else)  key_e = fl32(s_e + bias_e), bias_e = 0 for a NULL bias.
 *   4. the order, total on (key, index): the larger key first; every NaN above +inf and all NaNs equal (torch.topk's convention);
 *      -0.0 == +0.0; among equal keys the smaller index first.
 *   5. groups (n_group > 1; group g = the experts [g gs, (g + 1) gs), gs = G / n_group): a group's score is its first key in that
 *      order (FP8MI_GATE_GROUP_MAX) or fl32(first + second) (FP8MI_GATE_GROUP_TOP2); the topk_group groups that come first by (group
 *      score in the same order on values, then the smaller group index) stay eligible, every other expert is excluded.
 *   6. ids[t, j], j < k, is the j-th eligible expert in that order: always k distinct values in [0, G), whatever the logits hold
 *      (NaN, +-inf, all equal, all -inf) - fp8mi_moe_route never sees an id this call invented.
 *   7. weights[t, j] = s_{ids[t, j]} - the score, never the key: the bias selects and does not weight;  with renormalize != 0
 *      den = (((w_0 + w_1) + w_2) + ...) in the order j = 0 .. k-1 and w_j = w_j / (den + 1e-20f);  then w_j = fl32(w_j scale).
 * The exponential is the hardware's (exp2 of x log2 e): a relative error of a few ulp plus |argument| 2^-24 log2 e.  For a token whose
 * logits hold a NaN or an infinity the ids are as defined and the k weights are written, with unspecified values.  Exactly the T k ids
 * and T k weights are written.  Any G in [1, 1024], any ld >= G and any element-aligned base work: 16-byte loads (shorter ones where
 * a lane owns fewer bytes, G <= 128 or 256) where base, ld and G allow them, one element per load otherwise.
 * FP8MI_E_NULL: logits, ids or weights;  FP8MI_E_SHAPE: T < 0, G < 1, k < 1, k > G, ld < G, n_group < 1, G % n_group != 0,
 * topk_group outside [1, n_group], k > topk_group gs, FP8MI_GATE_GROUP_TOP2 with gs < 2 and n_group > 1;  FP8MI_E_ENUM: unknown
 * dtype, scoring or group_score;  FP8MI_E_UNSUPPORTED: G > 1024 (the grouped GEMM's maximum), k > FP8MI_MOE_GATE_MAX_K,
 * n_group > 64, T k >= 2^31, a pointer not aligned to its element size, a scale that is not finite.  T == 0 is a no-op that still
 * validates.
 */
#define FP8MI_GATE_SOFTMAX 0
#define FP8MI_GATE_SIGMOID 1
#define FP8MI_GATE_GROUP_MAX  0   /* a group's score: its largest key            (DeepSeek-V2) */
#define FP8MI_GATE_GROUP_TOP2 1   /* fl32(largest + second largest key)          (DeepSeek-V3) */
#define FP8MI_MOE_GATE_MAX_K 64

int fp8mi_moe_gate(const void *logits, int dtype /* f32 / f16 / bf16 */, int64_t T, int G, int64_t ld,
                   const float *bias /* [G] or NULL: selection only */, int k, int scoring, int renormalize, float scale,
                   int n_group, int topk_group, int group_score,
                   int32_t *ids /* [T, k] */, float *weights /* [T, k] */, void *stream);

/*
 * The FP8 paged KV cache, single-query (decode) attention over it, and its multi-token (causal, variable-length) form.
 *
 * The cache is two byte tensors of e4m3fn codes, in blocks of block_size positions (16, 32, 64 or 128), head dimension D 64 or 128:
 *   K cache  uint8 [num_blocks, Hkv, block_size, D]   a position's D channels are contiguous;
 *   V cache  uint8 [num_blocks, Hkv, D, block_size]   a channel's positions are contiguous: the product P.V sums over positions, so its
 *                                                     V operand is read in place, with no transpose.
 * Slot s of a cache is position s % block_size of block s / block_size.  k_scale and v_scale are DEQUANTISATION scales (value = byte x
 * scale, as everywhere in this header), fp32 in device memory: one value each (FP8MI_KV_SCALE_TENSOR) or one per KV head, [Hkv]
 * (FP8MI_KV_SCALE_HEAD).  They are static - calibrated by the caller; appending a token re-quantises nothing.  Both caches 16-byte aligned.
 *
 * fp8mi_kv_cache_append - ONE launch, no workspace, nothing read on the host, capturable: for every token t of k, v (T, Hkv, D) f32 /
 * f16 / bf16 (token t's heads at t ld_k / t ld_v elements: slices of a fused qkv), the bytes
 *   enc<encode_mode>(float32(k[t, h, d]) * (1.0f / k_scale_h))     (an IEEE fp32 division, then fp8mi_encode's multiply and encoder)
 * go to slot slot_mapping[t] (int32 or int64 by slot_bytes = 4 or 8, device) of the K cache and the same of v to the V cache: byte for
 * byte fp8mi_encode of the same values with prescale = 1.0f / scale.  A negative slot is padding; it and a slot at or beyond
 * num_blocks block_size store nothing.  Two tokens with one slot: either may win.
 * FP8MI_E_SHAPE: T < 0, Hkv < 1, num_blocks < 0, D not 64 / 128, block_size not 16 / 32 / 64 / 128, ld_k or ld_v < Hkv D;  FP8MI_E_ENUM:
 * unknown dtype, scale_mode, encode_mode, slot_bytes not 4 / 8;  FP8MI_E_NULL (T > 0): any pointer;  FP8MI_E_UNSUPPORTED: a pointer not
 * aligned to its element size (the caches: 16 bytes), T Hkv D at or beyond 2^40.  T == 0 is a no-op that still validates.
 *
 * fp8mi_paged_attention_decode - one query token per sequence: q (B, Hq, D) f32 / f16 / bf16 (sequence b at b ld_q elements) against the
 * positions [0, seq_lens[b]) of the blocks block_table[b ld_bt + i], i < max_blocks, names (int32); out (B, Hq, D) f32 / f16 / bf16 (ld_out).
 * Query head hq reads KV head hq / (Hq / Hkv); Hq % Hkv == 0 and Hq / Hkv <= 16.  With x_p = k_scale K[p] (decoded), y_p = v_scale V[p]:
 *   out[b, hq] = sum_p softmax_p(softmax_scale q . x_p) y_p       over p in [0, seq_lens[b]);  seq_lens[b] == 0 gives a zero row.
 * Numerics: q is rounded to e4m3 per (b, hq) row with the scale amax / 448 over D (round to nearest even) - any finite row, down to one
 * whose amax is subnormal (below 2^-64 the row is scaled by 2^64 first, so that 448 / amax stays finite; an all-zero row scores 0
 * everywhere); a q that holds an infinity or a NaN is undefined; the scores q . K are the fp8
 * MFMA's on those bytes and the cache's; the softmax is online in fp32 (base 2, the hardware's exp2), its row sum from the fp32
 * probabilities; each probability p (relative to the running maximum) is rounded to e4m3 as rne(p 2^8) - down to 2^-17 it is not flushed -
 * and P.V is the fp8 MFMA's on those bytes and the V cache's; accumulators, the merge of splits and the normalisation are fp32.  NaN
 * bytes (0x7F / 0xFF) INSIDE [0, seq_len) are NaN (OCP) and poison their row.
 * Nothing outside [0, seq_lens[b]) influences the output, whatever its bytes (NaN patterns included): not the tail of the last block,
 * not blocks the table names beyond ceil(seq_len / block_size); those table entries may be any value (-1 included) and are never
 * dereferenced.  seq_lens[b] is clamped to [0, max_blocks block_size]; a needed entry outside [0, num_blocks) reads as zeros.
 * max_seq_len is a HOST upper bound of seq_lens: it sizes the grid and the splits only, no device value is read on the host.
 * num_splits: 0 = the library chooses (1 .. 64, by B Hkv, max_seq_len and the workspace given - none: 1); 1 = one launch; n > 1 forces
 * n splits of the positions: two launches - partials (m, l, O) in fp32 in the workspace, then a combine; a split that owns no position of
 * a short sequence contributes zero.  The workspace (16-byte aligned) holds fp8mi_paged_attention_workspace_bytes(B, Hq, D, num_splits)
 * bytes (num_splits = 0: enough for whatever the library chooses; <= 1: 0); it is written and read inside the call only.
 * FP8MI_E_SHAPE: a negative size, Hkv < 1, Hq % Hkv != 0, D, block_size as above, ld_q or ld_out < Hq D, ld_bt < max_blocks, num_splits
 * < 0;  FP8MI_E_ENUM: unknown q_dtype, out_dtype, scale_mode;  FP8MI_E_UNSUPPORTED: Hq / Hkv > 16, num_splits > 256, a forced split
 * without a workspace of that size, a softmax_scale that is not finite, a misaligned pointer, B Hkv num_splits at or beyond 2^31;
 * FP8MI_E_NULL (B > 0): any pointer but the workspace.  B == 0 is a no-op that still validates.
 *
 * fp8mi_paged_attention_varlen - several query tokens per sequence, causal among themselves: speculative verification, a chunk of a prompt
 * appended to a context already in the cache ("extend"), and batches that mix such sequences with single-token ones.  q (T, Hq, D) f32 / f16 /
 * bf16 (token t at t ld_q elements: a slice of a fused qkv is read in place); cu_seqlens_q int32 [B + 1] in device memory: sequence b owns
 * the query rows [cu[b], cu[b + 1]), q_len_b = max(cu[b + 1] - cu[b], 0) of them.  seq_lens[b] is the context length INCLUDING those
 * q_len_b tokens, which the caller has appended already (fp8mi_kv_cache_append); it is clamped to [0, max_blocks block_size] as above.  The
 * cache, block_table (B, max_blocks), the scales, softmax_scale, num_splits, the workspace and out_dtype are the decode entry's; out is
 * (T, Hq, D) with ld_out.  Query token j of sequence b (row cu[b] + j) attends the positions [0, limit),
 *   limit = seq_lens[b] - q_len_b + j + 1      (causal, aligned at the END of the context: the last token sees all of it),
 * and limit <= 0 - q_len_b > seq_lens[b] makes some - gives a zero row, as seq_len == 0 does above.
 * max_q_len and max_seq_len are HOST upper bounds of q_len_b and seq_lens: they size the grid and the splits only; no device value is
 * read on the host and the call is capturable.  Rows no sequence owns (t >= cu[B]: the padding of a captured shape) are NOT written, with
 * one launch and with splits alike; nor are the rows j >= max_q_len of a sequence (max_q_len above T counts as T), nor any row outside
 * [0, T).  The other rows of such a sequence are what the call with a sufficient max_q_len gives.
 * Numerics: the decode entry's, per row - out[t] equals, BIT FOR BIT, fp8mi_paged_attention_decode on the expansion with one sequence per
 * query token (that token's q row, the sequence's table row, seq_len = max(limit, 0)), given the same max_seq_len and num_splits.
 * One workgroup takes TQ = 16 / (Hq / Hkv) tokens (integer division) of one sequence and KV head - its 16 MFMA columns are (token, head)
 * pairs - and reads the K and V bytes of a step once for all of them: the context is read once per TQ tokens, not once per token.  It is
 * still the memory-bound kernel: a long prompt chunk re-reads K / V once per TQ tokens; this is no compute-bound prefill.
 * Nothing at or beyond a row's own limit changes that row by one bit - K bytes there, NaN patterns included, and finite V bytes there -
 * with ONE exception: a NaN byte (0x7F / 0xFF) of V at a position in [limit_j, limit of the last token of j's tile) may turn row j into
 * NaN (0 x NaN is NaN in the MFMA, and the columns of a tile share one V operand).  Tiles are the tokens [i TQ, (i + 1) TQ) of a sequence.
 * Bytes at or beyond the tile's last limit are never read.
 * num_splits = 0: chosen as above with B Hkv ceil(max_q_len / TQ) workgroups (every sequence counted at max_q_len tokens: a mixed batch
 * over-counts them); cu = 0 .. B with max_q_len = 1 gives the decode entry's choice.  The workspace holds
 * fp8mi_paged_attention_workspace_bytes(T, Hq, D, num_splits) bytes: partials are per query row.
 * fp8mi_paged_attention_varlen_splits returns that choice for a 16-byte aligned workspace of workspace_bytes bytes on the current device
 * (0: a shape the entry rejects) - the num_splits to force for the same bits.
 * FP8MI_E_SHAPE: a negative size (T, B, max_q_len, max_blocks, max_seq_len, workspace_bytes), Hkv < 1, Hq % Hkv != 0, D, block_size as
 * above, ld_q or ld_out < Hq D, ld_bt < max_blocks, num_splits < 0;  FP8MI_E_ENUM: unknown q_dtype, out_dtype, scale_mode;
 * FP8MI_E_UNSUPPORTED: Hq / Hkv > 16, num_splits > 256, a forced split without a workspace of that size, a softmax_scale that is not
 * finite, a misaligned pointer, T Hq, B Hkv ceil(max_q_len / TQ) num_splits or B min(max_q_len, T) Hq (the combine's grid) at or beyond
 * 2^31;  FP8MI_E_NULL (T > 0, B > 0 and max_q_len > 0): any pointer but the workspace.  T == 0, B == 0 or max_q_len == 0 is a no-op that
 * still validates.
 */
#define FP8MI_KV_SCALE_TENSOR 0
#define FP8MI_KV_SCALE_HEAD   1
#define FP8MI_ATTN_MAX_GROUP  16    /* Hq / Hkv */
#define FP8MI_ATTN_MAX_SPLITS 256

int fp8mi_kv_cache_append(const void *k, const void *v, int dtype /* f32 / f16 / bf16 */, int64_t T, int Hkv, int D, int64_t ld_k, int64_t ld_v,
                          uint8_t *k_cache, uint8_t *v_cache, int64_t num_blocks, int block_size,
                          const void *slot_mapping /* [T] */, int slot_bytes /* 4 or 8 */,
                          const float *k_scale, const float *v_scale, int scale_mode /* FP8MI_KV_SCALE_* */, int encode_mode, void *stream);
int64_t fp8mi_paged_attention_workspace_bytes(int64_t B, int Hq, int D, int num_splits);
int fp8mi_paged_attention_decode(const void *q, int q_dtype, int64_t B, int Hq, int Hkv, int D, int64_t ld_q,
                                 const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size,
                                 const int32_t *block_table /* (B, max_blocks) */, int64_t ld_bt, int64_t max_blocks,
                                 const int32_t *seq_lens /* [B] */, int64_t max_seq_len,
                                 const float *k_scale, const float *v_scale, int scale_mode /* FP8MI_KV_SCALE_* */, float softmax_scale,
                                 int num_splits, void *workspace, int64_t workspace_bytes, void *out, int out_dtype, int64_t ld_out, void *stream);
int fp8mi_paged_attention_varlen_splits(int64_t T, int64_t B, int64_t max_q_len, int Hq, int Hkv, int D, int64_t max_seq_len, int64_t workspace_bytes);
int fp8mi_paged_attention_varlen(const void *q, int q_dtype, int64_t T, int64_t B, const int32_t *cu_seqlens_q /* [B + 1] */, int64_t max_q_len,
                                 int Hq, int Hkv, int D, int64_t ld_q,
                                 const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size,
                                 const int32_t *block_table /* (B, max_blocks) */, int64_t ld_bt, int64_t max_blocks,
                                 const int32_t *seq_lens /* [B] */, int64_t max_seq_len,
                                 const float *k_scale, const float *v_scale, int scale_mode /* FP8MI_KV_SCALE_* */, float softmax_scale,
                                 int num_splits, void *workspace, int64_t workspace_bytes, void *out, int out_dtype, int64_t ld_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FP8MI_H */
