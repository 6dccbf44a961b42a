/*
 * Torch-free use of the blockwise entry points of the C ABI (include/fp8mi.h): a plain C host program that allocates with HIP,
 * quantises a 70 x 400 float matrix with 1x128 blocks and a 200 x 400 one with 128x128 blocks (fp8mi_quantize_blockwise, through
 * ld_in > cols), multiplies them with fp8mi_scaled_mm_blockwise (AUTO, a forced tile and the generic kernel), dequantises both
 * (fp8mi_dequant_blockwise) and checks everything against values computed here.  The data is chosen so that every step but the
 * product is exact: each block's amax is 448 x 2^j, so its scale is 2^j, and every element is a small integer times 2^j, an e4m3
 * value - dequant(quant(x)) == x bit for bit.  The product is held to the bar of include/fp8mi.h against the double sum of the
 * dequantised values: |gpu - exact| <= (1e-3 + nkb 2^-23) bound on the matrix-core tiles, (128 2^-24 + nkb 2^-23) bound on the
 * generic kernel, bound = sum_k |a b|.  The argument errors of tests/test_blockwise_host.py are asked for again, with live device
 * pointers.  Built and run by tests/test_gpu_blockwise_edges.py:
 *   gcc -D__HIP_PLATFORM_AMD__ tests/c/blockwise_roundtrip.c -I/opt/rocm/include -Iinclude -Lfp8-mps-metal_amd -lfp8mi \
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

enum { M = 70, N = 200, K = 400, LD = K + 8, NKB = (K + 127) / 128, NRB_B = (N + 127) / 128 };

static uint32_t rng = 20261017u;
static uint32_t next(void) { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

static int exp_a(int r, int cb) { return r % 5 - 2 + cb % 3; }     /* the scale exponent of block (r, cb) of X: 1x128 blocks */
static int exp_b(int rb, int cb) { return rb - cb; }                /* ... of block (rb, cb) of W: 128x128 blocks */

/* rows x K values v 2^j(block), v a signed integer of {0, 1, 2, 3, 4, 6, 8, 12} x {1, 2, 4, 8}: e4m3 values.  The padding up to LD is huge. */
static void fill(float *x, int rows, int block_rows)
{
    static const int ks[8] = {0, 1, 2, 3, 4, 6, 8, 12};
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < LD; ++c) {
            const uint32_t u = next();
            const int j = block_rows == 1 ? exp_a(r, c / 128) : exp_b(r / 128, c / 128);
            const double v = ldexp((double)(ks[u & 7] << ((u >> 3) & 3)), j);
            x[r * LD + c] = c < K ? (float)((u >> 5) & 1 ? -v : v) : 1e30f;
        }
}

int main(void)
{
    float *X = malloc(sizeof(float) * M * LD), *W = malloc(sizeof(float) * N * LD);
    float *DX = malloc(sizeof(float) * M * K), *DW = malloc(sizeof(float) * N * K), *C = malloc(sizeof(float) * M * N);
    uint8_t *QX = malloc((size_t)M * K);
    float sx[M * NKB], sw[NRB_B * NKB];
    EXPECT(X && W && DX && DW && C && QX);
    fill(X, M, 1);
    fill(W, N, 128);
    /* the amax of every block: -448 x 2^j somewhere inside it (the last column block is 16 wide, the last row block 72 high) */
    for (int r = 0; r < M; ++r)
        for (int cb = 0; cb < NKB; ++cb) X[r * LD + cb * 128 + (r * 5 + cb) % 16] = (float)ldexp(-448.0, exp_a(r, cb));
    for (int rb = 0; rb < NRB_B; ++rb)
        for (int cb = 0; cb < NKB; ++cb) W[(rb * 128 + 3 + cb) * LD + cb * 128 + (rb + 2 * cb) % 16] = (float)ldexp(448.0, exp_b(rb, cb));

    float *dX, *dW, *dsx, *dsw, *dC, *dDX, *dDW;
    uint8_t *dQX, *dQW;
    CHECK_HIP(hipMalloc((void **)&dX, sizeof(float) * M * LD)); CHECK_HIP(hipMalloc((void **)&dW, sizeof(float) * N * LD));
    CHECK_HIP(hipMalloc((void **)&dQX, (size_t)M * K)); CHECK_HIP(hipMalloc((void **)&dQW, (size_t)N * K));
    CHECK_HIP(hipMalloc((void **)&dsx, sizeof sx)); CHECK_HIP(hipMalloc((void **)&dsw, sizeof sw));
    CHECK_HIP(hipMalloc((void **)&dC, sizeof(float) * M * N));
    CHECK_HIP(hipMalloc((void **)&dDX, sizeof(float) * M * K)); CHECK_HIP(hipMalloc((void **)&dDW, sizeof(float) * N * K));
    CHECK_HIP(hipMemcpy(dX, X, sizeof(float) * M * LD, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dW, W, sizeof(float) * N * LD, hipMemcpyHostToDevice));

    /* ---- quantize: X with 1x128 blocks, W with 128x128 blocks, both through ld_in > cols; row-major scales ---- */
    CHECK_MI(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, LD, FP8MI_BLOCK_1, dQX, K, dsx, NKB, 1, NULL));
    CHECK_MI(fp8mi_quantize_blockwise(dW, FP8MI_F32, N, K, LD, FP8MI_BLOCK_128, dQW, K, dsw, NKB, 1, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(sx, dsx, sizeof sx, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(sw, dsw, sizeof sw, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(QX, dQX, (size_t)M * K, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r)
        for (int cb = 0; cb < NKB; ++cb) EXPECT(sx[r * NKB + cb] == (float)ldexp(1.0, exp_a(r, cb)));
    for (int rb = 0; rb < NRB_B; ++rb)
        for (int cb = 0; cb < NKB; ++cb) EXPECT(sw[rb * NKB + cb] == (float)ldexp(1.0, exp_b(rb, cb)));
    for (int r = 0; r < M; ++r)
        for (int cb = 0; cb < NKB; ++cb) EXPECT(QX[(size_t)r * K + cb * 128 + (r * 5 + cb) % 16] == 0xFE);   /* -448 */

    /* ---- dequantize: exactly the input again ---- */
    CHECK_MI(fp8mi_dequant_blockwise(dQX, M, K, K, FP8MI_BLOCK_1, dsx, NKB, 1, dDX, FP8MI_F32, NULL));
    CHECK_MI(fp8mi_dequant_blockwise(dQW, N, K, K, FP8MI_BLOCK_128, dsw, NKB, 1, dDW, FP8MI_F32, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(DX, dDX, sizeof(float) * M * K, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(DW, dDW, sizeof(float) * N * K, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < K; ++c)
            if (DX[r * K + c] != X[r * LD + c]) { printf("X[%d,%d]: dequant(quant(x)) = %g, x = %g\n", r, c, DX[r * K + c], X[r * LD + c]); return 1; }
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < K; ++c)
            if (DW[r * K + c] != W[r * LD + c]) { printf("W[%d,%d]: dequant(quant(x)) = %g, x = %g\n", r, c, DW[r * K + c], W[r * LD + c]); return 1; }

    /* ---- the argument errors, on a live device: each comes back before any launch ---- */
#define MM(A_, B_, C_, sa_, sa_sr, sa_sk, ba, sb_, sb_sr, sb_sk, bb, M_, N_, K_, lda, ldb, ldc, out, kernel) \
    fp8mi_scaled_mm_blockwise(A_, B_, C_, sa_, sa_sr, sa_sk, ba, sb_, sb_sr, sb_sk, bb, NULL, NULL, M_, N_, K_, lda, ldb, ldc, out, FP8MI_F32, \
                              FP8MI_NAN_ZERO, kernel, 1, NULL, 0, NULL)
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, -1, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_SHAPE);
    EXPECT(MM(dQX, dQW, dC, dsx, -1, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_SHAPE);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 2, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_ENUM);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 64, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_ENUM);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K - 16, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_SHAPE);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N - 1, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_SHAPE);
    EXPECT(MM(dQX, dQW, NULL, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_NULL);
    EXPECT(MM(dQX, dQW, dC, NULL, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == FP8MI_E_NULL);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, 7, FP8MI_KERNEL_AUTO) == FP8MI_E_ENUM);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, 999) == FP8MI_E_ENUM);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_SKINNY) == FP8MI_E_UNSUPPORTED);
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M, N, K - 8, K, K, N, FP8MI_F32, FP8MI_KERNEL_GEMM_64x64) == FP8MI_E_UNSUPPORTED);  /* K % 16 */
    EXPECT(MM(dQX + 8, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, M - 1, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_GEMM_128x64) == FP8MI_E_UNSUPPORTED);
    EXPECT(MM(dQX, dQW, dC, (const float *)((const char *)dsx + 2), NKB, 1, 1, dsw, NKB, 1, 128, M, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_GEMM_64x64) == FP8MI_E_UNSUPPORTED);
    EXPECT(MM(NULL, NULL, dC, NULL, 0, 0, 1, NULL, 0, 0, 128, M, N, 0, 0, 0, N, FP8MI_F32, FP8MI_KERNEL_GEMM_64x64) == FP8MI_E_UNSUPPORTED);      /* a tile needs K > 0 */
    EXPECT(MM(dQX, dQW, dC, dsx, NKB, 1, 1, dsw, NKB, 1, 128, 0, N, K, K, K, N, FP8MI_F32, FP8MI_KERNEL_AUTO) == 0);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, -1, K, LD, 1, dQX, K, dsx, NKB, 1, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, K - 1, 1, dQX, K, dsx, NKB, 1, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, LD, 1, dQX, K - 1, dsx, NKB, 1, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, LD, 1, dQX, K, dsx, -2, 1, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, LD, 2, dQX, K, dsx, NKB, 1, NULL) == FP8MI_E_ENUM);
    EXPECT(fp8mi_quantize_blockwise(dX, 9, M, K, LD, 1, dQX, K, dsx, NKB, 1, NULL) == FP8MI_E_ENUM);
    EXPECT(fp8mi_quantize_blockwise(NULL, FP8MI_F32, M, K, LD, 1, dQX, K, dsx, NKB, 1, NULL) == FP8MI_E_NULL);
    EXPECT(fp8mi_quantize_blockwise(dX, FP8MI_F32, M, K, LD, 128, dQX, K, NULL, NKB, 1, NULL) == FP8MI_E_NULL);
    EXPECT(fp8mi_quantize_blockwise(NULL, FP8MI_F32, 0, K, LD, 1, NULL, K, NULL, NKB, 1, NULL) == 0);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, K, K - 1, 1, dsx, NKB, 1, dDX, FP8MI_F32, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, K, K, 1, dsx, NKB, -1, dDX, FP8MI_F32, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_dequant_blockwise(dQX, -1, K, K, 1, dsx, NKB, 1, dDX, FP8MI_F32, NULL) == FP8MI_E_SHAPE);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, K, K, 3, dsx, NKB, 1, dDX, FP8MI_F32, NULL) == FP8MI_E_ENUM);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, K, K, 1, dsx, NKB, 1, dDX, 9, NULL) == FP8MI_E_ENUM);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, K, K, 1, NULL, NKB, 1, dDX, FP8MI_F32, NULL) == FP8MI_E_NULL);
    EXPECT(fp8mi_dequant_blockwise(dQX, M, 0, K, 1, dsx, NKB, 1, dDX, FP8MI_F32, NULL) == 0);

    /* ---- the product: AUTO, a forced tile and the generic kernel against the double sum of the dequantised values ---- */
    double *ex = malloc(sizeof(double) * M * N), *bound = malloc(sizeof(double) * M * N);
    EXPECT(ex && bound);
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            double e = 0, b = 0;
            for (int k = 0; k < K; ++k) { const double p = (double)DX[m * K + k] * (double)DW[n * K + k]; e += p; b += fabs(p); }
            ex[m * N + n] = e; bound[m * N + n] = b;
        }
    const int kernels[3] = {FP8MI_KERNEL_AUTO, FP8MI_KERNEL_GEMM_64x64, FP8MI_KERNEL_GENERIC};
    EXPECT(fp8mi_choose_kernel_blockwise(M, N, K, K, K, N, FP8MI_F32, 1, 128, 0, 1) != FP8MI_KERNEL_GENERIC);
    for (int ki = 0; ki < 3; ++ki) {
        CHECK_HIP(hipMemset(dC, 0xFF, sizeof(float) * M * N));
        CHECK_MI(MM(dQX, dQW, dC, dsx, NKB, 1, FP8MI_BLOCK_1, dsw, NKB, 1, FP8MI_BLOCK_128, M, N, K, K, K, N, FP8MI_F32, kernels[ki]));
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(C, dC, sizeof(float) * M * N, hipMemcpyDeviceToHost));
        const double tol = (kernels[ki] == FP8MI_KERNEL_GENERIC ? 128 * ldexp(1.0, -24) : 1e-3) + NKB * ldexp(1.0, -23);
        double worst = 0;
        for (int i = 0; i < M * N; ++i) {
            const double err = fabs((double)C[i] - ex[i]);
            if (!(err <= tol * bound[i])) { printf("kernel %d C[%d,%d] = %g, exact %g, bound %g\n", kernels[ki], i / N, i % N, C[i], ex[i], bound[i]); return 1; }
            if (bound[i] > 0 && err / bound[i] > worst) worst = err / bound[i];
        }
        printf("scaled_mm_blockwise kernel %d: max err / bound = %.3e (bar %.3e)\n", kernels[ki], worst, tol);
    }

    CHECK_HIP(hipFree(dX)); CHECK_HIP(hipFree(dW)); CHECK_HIP(hipFree(dQX)); CHECK_HIP(hipFree(dQW)); CHECK_HIP(hipFree(dsx));
    CHECK_HIP(hipFree(dsw)); CHECK_HIP(hipFree(dC)); CHECK_HIP(hipFree(dDX)); CHECK_HIP(hipFree(dDW));
    printf("blockwise C ABI round trip: ok\n");
    return 0;
}
