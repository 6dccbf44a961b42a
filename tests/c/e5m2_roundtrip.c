/*
 * Torch-free use of the e5m2 entry points of the C ABI (include/fp8mi.h): a plain C host program that allocates with HIP,
 * encodes floats to e5m2 (fp8mi_encode_e5m2), multiplies e5m2 x e5m2 and e5m2 x e4m3 bytes (fp8mi_scaled_mm_fmt), dequantises
 * (fp8mi_dequant_e5m2) and quantises (fp8mi_quantize_e5m2), and checks everything against values computed here from the format's
 * definition.  Built and run by tests/test_gpu_e5m2.py:
 *   gcc -D__HIP_PLATFORM_AMD__ tests/c/e5m2_roundtrip.c -I/opt/rocm/include -Iinclude -Lfp8-mps-metal_amd -lfp8mi \
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

static double dec_e5m2(uint8_t b)
{
    int s = b >> 7, e = (b >> 2) & 31, m = b & 3;
    double v = e == 31 ? (m ? NAN : INFINITY) : e == 0 ? m / 4.0 * ldexp(1.0, -14) : (1 + m / 4.0) * ldexp(1.0, e - 15);
    return s ? -v : v;
}
static double dec_e4m3(uint8_t b)
{
    if ((b & 0x7F) == 0x7F) return NAN;
    int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
    double v = e == 0 ? m / 8.0 * ldexp(1.0, -6) : (1 + m / 8.0) * ldexp(1.0, e - 7);
    return s ? -v : v;
}

static uint32_t rng = 2024u;
static uint32_t next(void) { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

int main(void)
{
    /* ---- encode: known values ---- */
    const float xin[12] = {0.0f, -0.0f, 1.0f, -1.5f, 57344.0f, 61439.0f, 61440.0f, -1e9f, INFINITY, NAN, 1.125f, 1.375f};
    const uint8_t want[12] = {0x00, 0x80, 0x3C, 0xBE, 0x7B, 0x7B, 0x7C, 0xFC, 0x7C, 0x7F, 0x3C, 0x3E};   /* 1.125 -> 1.0 and 1.375 -> 1.5: ties to even */
    float *dx; uint8_t *dq;
    CHECK_HIP(hipMalloc((void **)&dx, sizeof xin)); CHECK_HIP(hipMalloc((void **)&dq, 12));
    CHECK_HIP(hipMemcpy(dx, xin, sizeof xin, hipMemcpyHostToDevice));
    CHECK_MI(fp8mi_encode_e5m2(dx, FP8MI_F32, dq, NULL, 12, NULL));
    uint8_t q[12];
    CHECK_HIP(hipMemcpy(q, dq, 12, hipMemcpyDeviceToHost));
    for (int i = 0; i < 12; ++i)
        if (q[i] != want[i]) { printf("encode[%d] (%g): got 0x%02X, want 0x%02X\n", i, xin[i], q[i], want[i]); return 1; }

    /* ---- dequant: all 256 bytes to float32, with a scale ---- */
    uint8_t all[256]; for (int i = 0; i < 256; ++i) all[i] = (uint8_t)i;
    uint8_t *dall; float *dout, *dscale; const float scale = 0.75f;
    CHECK_HIP(hipMalloc((void **)&dall, 256)); CHECK_HIP(hipMalloc((void **)&dout, 1024)); CHECK_HIP(hipMalloc((void **)&dscale, 8));
    CHECK_HIP(hipMemcpy(dall, all, 256, hipMemcpyHostToDevice)); CHECK_HIP(hipMemcpy(dscale, &scale, 4, hipMemcpyHostToDevice));
    CHECK_MI(fp8mi_dequant_e5m2(dall, dout, dscale, 256, FP8MI_F32, NULL));
    float out[256];
    CHECK_HIP(hipMemcpy(out, dout, 1024, hipMemcpyDeviceToHost));
    for (int i = 0; i < 256; ++i) {
        const double w = dec_e5m2((uint8_t)i) * 0.75;   /* exact in float32 */
        if (isnan(w) ? !isnan(out[i]) : (double)out[i] != w) { printf("dequant[0x%02X]: got %g, want %g\n", i, out[i], w); return 1; }
    }

    /* ---- scaled_mm_fmt: random finite bytes, e5m2 x e5m2 and e5m2 x e4m3, AUTO and a forced tile, with split-K workspace ---- */
    const int M = 72, K = 1024, N = 136;
    uint8_t *A = malloc((size_t)M * K), *B = malloc((size_t)N * K);
    float *C = malloc(sizeof(float) * M * N);
    uint8_t *dA, *dB; float *dC, *ds;
    CHECK_HIP(hipMalloc((void **)&dA, (size_t)M * K)); CHECK_HIP(hipMalloc((void **)&dB, (size_t)N * K));
    CHECK_HIP(hipMalloc((void **)&dC, sizeof(float) * M * N)); CHECK_HIP(hipMalloc((void **)&ds, 8));
    const float s1 = 1.0f / 16384.0f;
    CHECK_HIP(hipMemcpy(ds, &s1, 4, hipMemcpyHostToDevice));
    void *ws; const int64_t ws_bytes = fp8mi_scaled_mm_workspace_bytes();
    CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
    CHECK_MI(fp8mi_workspace_reset(ws, ws_bytes, NULL));
    for (int bfmt = 0; bfmt < 2; ++bfmt) {
        for (size_t i = 0; i < (size_t)M * K; ++i) { A[i] = (uint8_t)next(); if ((A[i] & 0x7C) == 0x7C) A[i] &= 0xBF; }
        for (size_t i = 0; i < (size_t)N * K; ++i) {
            B[i] = (uint8_t)next();
            if (bfmt == FP8MI_FMT_E5M2 ? (B[i] & 0x7C) == 0x7C : (B[i] & 0x7F) == 0x7F) B[i] &= 0xB7;
        }
        CHECK_HIP(hipMemcpy(dA, A, (size_t)M * K, hipMemcpyHostToDevice)); CHECK_HIP(hipMemcpy(dB, B, (size_t)N * K, hipMemcpyHostToDevice));
        const int kernels[3] = {FP8MI_KERNEL_AUTO, FP8MI_KERNEL_GEMM_64x64, FP8MI_KERNEL_GENERIC};
        for (int ki = 0; ki < 3; ++ki) {
            CHECK_MI(fp8mi_scaled_mm_fmt(dA, dB, dC, ds, ds, NULL, NULL, M, N, K, K, K, N, FP8MI_SCALE_TENSOR, FP8MI_SCALE_TENSOR, FP8MI_F32, 0,
                                         FP8MI_NAN_PROPAGATE, kernels[ki], 0, ws, ws_bytes, FP8MI_FMT_E5M2, bfmt, NULL));
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(C, dC, sizeof(float) * M * N, hipMemcpyDeviceToHost));
            double worst = 0;
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) {
                    double ex = 0, bound = 0;
                    for (int k = 0; k < K; ++k) {
                        const double p = dec_e5m2(A[(size_t)m * K + k]) * (bfmt ? dec_e5m2(B[(size_t)n * K + k]) : dec_e4m3(B[(size_t)n * K + k]));
                        ex += p; bound += fabs(p);
                    }
                    ex *= (double)s1 * s1; bound *= (double)s1 * s1;
                    const double r = fabs(C[(size_t)m * N + n] - ex) / (bound + 1e-300);
                    if (r > worst) worst = r;
                }
            const double tol = kernels[ki] == FP8MI_KERNEL_GENERIC ? 4e-6 : 1e-3;
            printf("scaled_mm_fmt e5m2 x %s kernel %d: max err / sum|ab| = %.3e (tol %.1e)\n", bfmt ? "e5m2" : "e4m3", kernels[ki], worst, tol);
            EXPECT(worst <= tol);
        }
    }
    /* argument errors come back before any launch */
    EXPECT(fp8mi_scaled_mm_fmt(dA, dB, dC, ds, ds, NULL, NULL, M, N, K, K, K, N, 0, 0, FP8MI_F32, 0, FP8MI_NAN_ZERO, FP8MI_KERNEL_AUTO, 0, NULL, 0,
                               FP8MI_FMT_E5M2, FP8MI_FMT_E4M3, NULL) == FP8MI_E_UNSUPPORTED);
    EXPECT(fp8mi_scaled_mm_fmt(dA, dB, dC, ds, ds, NULL, NULL, M, N, K, K, K, N, 0, 0, FP8MI_F32, 0, FP8MI_NAN_PROPAGATE, FP8MI_KERNEL_AUTO, 0, NULL, 0,
                               2, FP8MI_FMT_E4M3, NULL) == FP8MI_E_ENUM);

    /* ---- quantize: amax, inverse scale, bytes ---- */
    const float xq[5] = {0.5f, -2.0f, 1.0f, 0.0f, 2.0f};
    float *dxq, *dsc; uint8_t *dqq;
    CHECK_HIP(hipMalloc((void **)&dxq, sizeof xq)); CHECK_HIP(hipMalloc((void **)&dsc, 8)); CHECK_HIP(hipMalloc((void **)&dqq, 5));
    CHECK_HIP(hipMemcpy(dxq, xq, sizeof xq, hipMemcpyHostToDevice));
    CHECK_MI(fp8mi_quantize_e5m2(dxq, FP8MI_F32, dqq, dsc, 5, NULL));
    float sc[2]; uint8_t qq[5];
    CHECK_HIP(hipMemcpy(sc, dsc, 8, hipMemcpyDeviceToHost)); CHECK_HIP(hipMemcpy(qq, dqq, 5, hipMemcpyDeviceToHost));
    EXPECT(sc[0] == 2.0f && sc[1] == (float)(1.0 / (57344.0 / 2.0)));
    const uint8_t wq[5] = {0x73, 0xFB, 0x77, 0x00, 0x7B};   /* x * 28672: 14336, -57344, 28672, 0, 57344 */
    EXPECT(memcmp(qq, wq, 5) == 0);

    printf("e5m2 C ABI round trip: ok\n");
    return 0;
}
