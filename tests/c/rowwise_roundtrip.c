/*
 * Torch-free use of the per-row quantiser of the C ABI (include/fp8mi.h): a plain C host program that allocates with HIP, quantises
 * a float matrix per row (fp8mi_quantize_rowwise, e4m3 RNE and e5m2), multiplies the e4m3 bytes with fp8mi_scaled_mm under
 * FP8MI_SCALE_ROW, dequantises them (fp8mi_dequant_rowwise), and checks everything against values computed here: the amax, the
 * scales (double arithmetic rounded to float), the bytes (a nearest-value search over the format's decode table, on inputs chosen
 * away from ties) and the product (a double sum of the decoded bytes).  Built and run by tests/test_gpu_rowwise.py:
 *   gcc -D__HIP_PLATFORM_AMD__ tests/c/rowwise_roundtrip.c -I/opt/rocm/include -Iinclude -Lfp8-mps-metal_amd -lfp8mi \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o ...
 * Exit code 0 = every check passed.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fp8mi.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define CHECK_MI(x) do { int r_ = (x); if (r_ != 0) { printf("fp8mi error %d: %s (%s:%d)\n", r_, fp8mi_last_error(), __FILE__, __LINE__); return 3; } } while (0)
#define EXPECT(c) do { if (!(c)) { printf("check failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); return 1; } } while (0)

static double dec_e4m3(uint8_t b)
{
    if ((b & 0x7F) == 0x7F) return NAN;
    int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
    double v = e == 0 ? m / 8.0 * ldexp(1.0, -6) : (1 + m / 8.0) * ldexp(1.0, e - 7);
    return s ? -v : v;
}
static double dec_e5m2(uint8_t b)
{
    int s = b >> 7, e = (b >> 2) & 31, m = b & 3;
    double v = e == 31 ? (m ? NAN : INFINITY) : e == 0 ? m / 4.0 * ldexp(1.0, -14) : (1 + m / 4.0) * ldexp(1.0, e - 15);
    return s ? -v : v;
}

/* the byte whose value is nearest to v (|v| <= the format's largest finite value, not on a tie), with v's sign */
static uint8_t nearest(double v, int e5m2)
{
    int best = 0;
    double bd = INFINITY;
    for (int b = 0; b < 0x80; ++b) {
        const double d = e5m2 ? dec_e5m2((uint8_t)b) : dec_e4m3((uint8_t)b);
        if (isnan(d) || isinf(d)) continue;
        if (fabs(fabs(v) - d) < bd) { bd = fabs(fabs(v) - d); best = b; }
    }
    return (uint8_t)(best | (v < 0 ? 0x80 : 0));
}

static uint32_t rng = 20261017u;
static uint32_t next(void) { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

int main(void)
{
    /* X: M rows of K values k / 16 * 2^-(r % 9) with random signs, k in {0, 1, 2, 3, 4, 6, 8, 12, 16, 24}; one element of every row is
     * forced to -56 / 16 * 2^-(r % 9), the row's amax, so that scale = 448 / amax = 128 * 2^(r % 9) exactly and x * scale = 8 k: values with
     * one or two significant bits, exact in e4m3 and (times 128) in e5m2 - the byte search below never meets a tie */
    const int M = 72, K = 1024, N = 136, LD = K + 16;
    float *X = malloc(sizeof(float) * M * LD);
    uint8_t *W = malloc((size_t)N * K), *Q = malloc((size_t)M * K), *Q5 = malloc((size_t)M * K);
    float *C = malloc(sizeof(float) * M * N), *D = malloc(sizeof(float) * M * K);
    static const int ks[8] = {0, 1, 2, 3, 4, 6, 8, 12};          /* 8 k in {0 .. 96}: exact in both formats */
    for (int r = 0; r < M; ++r) {
        for (int c = 0; c < LD; ++c) {
            const uint32_t u = next();
            const double v = ks[u & 7] * (1 + ((u >> 3) & 1)) / 16.0 * ldexp(1.0, -(r % 9));      /* k in {0 .. 24} */
            X[r * LD + c] = (float)((u >> 4) & 1 ? -v : v);
        }
        X[r * LD + (r * 37) % K] = (float)(-56.0 / 16.0 * ldexp(1.0, -(r % 9)));                  /* the row's amax, negative */
        for (int c = K; c < LD; ++c) X[r * LD + c] = 1e30f;                                       /* padding beyond cols: never read */
    }
    for (size_t i = 0; i < (size_t)N * K; ++i) { W[i] = (uint8_t)next(); if ((W[i] & 0x7F) == 0x7F) W[i] &= 0xF7; }

    float *dX, *dinv, *damax, *dsw, *dC, *dD; uint8_t *dQ, *dW;
    CHECK_HIP(hipMalloc((void **)&dX, sizeof(float) * M * LD)); CHECK_HIP(hipMalloc((void **)&dQ, (size_t)M * K));
    CHECK_HIP(hipMalloc((void **)&dinv, sizeof(float) * M)); CHECK_HIP(hipMalloc((void **)&damax, sizeof(float) * M));
    CHECK_HIP(hipMalloc((void **)&dW, (size_t)N * K)); CHECK_HIP(hipMalloc((void **)&dsw, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dC, sizeof(float) * M * N)); CHECK_HIP(hipMalloc((void **)&dD, sizeof(float) * M * K));
    CHECK_HIP(hipMemcpy(dX, X, sizeof(float) * M * LD, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dW, W, (size_t)N * K, hipMemcpyHostToDevice));

    /* ---- quantize per row: e4m3 (RNE) and e5m2, through ld_in > cols ---- */
    float inv[72], amax[72], inv5[72];
    CHECK_MI(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, LD, dQ, K, dinv, damax, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(Q, dQ, (size_t)M * K, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(inv, dinv, sizeof inv, hipMemcpyDeviceToHost)); CHECK_HIP(hipMemcpy(amax, damax, sizeof amax, hipMemcpyDeviceToHost));
    CHECK_MI(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, LD, dQ, K, dinv, NULL, FP8MI_FMT_E5M2, FP8MI_ENC_RNE, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(Q5, dQ, (size_t)M * K, hipMemcpyDeviceToHost)); CHECK_HIP(hipMemcpy(inv5, dinv, sizeof inv5, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r) {
        double am = 0;
        for (int c = 0; c < K; ++c) am = fmax(am, fabs((double)X[r * LD + c]));
        EXPECT(amax[r] == (float)am && am == 3.5 * ldexp(1.0, -(r % 9)));
        const float scale = (float)(448.0 / am), scale5 = (float)(57344.0 / am);
        EXPECT(inv[r] == (float)(1.0 / (448.0 / am)) && inv5[r] == (float)(1.0 / (57344.0 / am)));
        for (int c = 0; c < K; ++c) {
            const float y = X[r * LD + c] * scale, y5 = X[r * LD + c] * scale5;     /* exact: small integers times powers of two */
            const uint8_t want = y == 0 ? (uint8_t)(signbit(y) ? 0x80 : 0) : nearest(y, 0), want5 = y5 == 0 ? (uint8_t)(signbit(y5) ? 0x80 : 0) : nearest(y5, 1);
            if (Q[(size_t)r * K + c] != want || Q5[(size_t)r * K + c] != want5) {
                printf("quantize[%d,%d] (%g): e4m3 got 0x%02X want 0x%02X, e5m2 got 0x%02X want 0x%02X\n", r, c, X[r * LD + c], Q[(size_t)r * K + c], want,
                       Q5[(size_t)r * K + c], want5);
                return 1;
            }
        }
    }
    /* the e5m2 mode restriction and the other argument errors come back before any launch */
    EXPECT(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, LD, dQ, K, dinv, NULL, FP8MI_FMT_E5M2, FP8MI_ENC_REFERENCE, NULL) == FP8MI_E_UNSUPPORTED);
    EXPECT(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, K - 1, dQ, K, dinv, NULL, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, LD, dQ, K, NULL, NULL, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL) == FP8MI_E_NULL);
    EXPECT(fp8mi_quantize_rowwise(dX, 5, M, K, LD, dQ, K, dinv, NULL, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL) == FP8MI_E_ENUM);
    EXPECT(fp8mi_quantize_rowwise(NULL, FP8MI_F32, 0, K, LD, NULL, K, NULL, NULL, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL) == 0);

    /* ---- scaled_mm with one scale per row of A (the quantiser's) and per row of B: AUTO, a forced tile and the generic kernel ---- */
    CHECK_MI(fp8mi_quantize_rowwise(dX, FP8MI_F32, M, K, LD, dQ, K, dinv, NULL, FP8MI_FMT_E4M3, FP8MI_ENC_RNE, NULL));   /* the e4m3 bytes again */
    float sw[136];
    for (int n = 0; n < N; ++n) sw[n] = ldexpf(1.0f + (float)(n % 4) / 4.0f, -(n % 7) - 8);
    CHECK_HIP(hipMemcpy(dsw, sw, sizeof sw, hipMemcpyHostToDevice));
    const int kernels[3] = {FP8MI_KERNEL_AUTO, FP8MI_KERNEL_GEMM_64x64, FP8MI_KERNEL_GENERIC};
    for (int ki = 0; ki < 3; ++ki) {
        CHECK_MI(fp8mi_scaled_mm_ex(dQ, dW, dC, dinv, dsw, NULL, NULL, M, N, K, K, K, N, FP8MI_SCALE_ROW, FP8MI_SCALE_ROW, FP8MI_F32, 0,
                                    FP8MI_NAN_PROPAGATE, kernels[ki], NULL));
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(C, dC, sizeof(float) * M * N, hipMemcpyDeviceToHost));
        double worst = 0;
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                double ex = 0, bound = 0;
                for (int k = 0; k < K; ++k) {
                    const double p = dec_e4m3(Q[(size_t)m * K + k]) * dec_e4m3(W[(size_t)n * K + k]);
                    ex += p; bound += fabs(p);
                }
                ex *= (double)inv[m] * sw[n]; bound *= (double)inv[m] * sw[n];
                const double r = fabs(C[(size_t)m * N + n] - ex) / (bound + 1e-300);
                if (r > worst) worst = r;
            }
        /* the existing suite's bounds (tests/e5m2_ref.py): fp32 sums of exact products, and the matrix core's truncation */
        const double tol = kernels[ki] == FP8MI_KERNEL_GENERIC ? 4e-6 : 1e-3;
        printf("scaled_mm SCALE_ROW kernel %d: max err / sum|ab| = %.3e (tol %.1e)\n", kernels[ki], worst, tol);
        EXPECT(worst <= tol);
    }

    /* ---- dequant per row: dec(q) * inv is x again where the byte was exact ---- */
    CHECK_MI(fp8mi_dequant_rowwise(dQ, M, K, K, dinv, FP8MI_FMT_E4M3, dD, FP8MI_F32, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(D, dD, sizeof(float) * M * K, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < K; ++c) {
            const float want = (float)dec_e4m3(Q[(size_t)r * K + c]) * inv[r];
            if (D[(size_t)r * K + c] != want || (double)want != (double)X[r * LD + c]) {
                printf("dequant[%d,%d]: got %g, want %g (x %g)\n", r, c, D[(size_t)r * K + c], want, X[r * LD + c]);
                return 1;
            }
        }

    printf("rowwise C ABI round trip: ok\n");
    return 0;
}
