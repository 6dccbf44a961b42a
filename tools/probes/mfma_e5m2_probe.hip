// Probe: v_mfma_scale_f32_16x16x128_f8f6f4 with e5m2 (bf8) operands - format code 1 in cbsz (first operand) and / or blgp
// (second operand) - on one wave, against a double reference on the host.  The sibling of tools/mfma_probe.hip (e4m3 only).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mfma_e5m2_probe.hip -o tools/probes/mfma_e5m2_probe && tools/probes/mfma_e5m2_probe
// For each format pair (cbsz, blgp) in (0,0) (1,0) (0,1) (1,1) it reports
//   1. operand K-map: exact small-integer data, asymmetric in row, column and k, against the map the e4m3 kernels rely on
//      (D[i][j] = sum over lane groups g and bytes t of first[lane 16 g + i][t] * second[lane 16 g + j][t]); the two operands
//      hold DIFFERENT bytes for the same values where their formats differ, so a swapped cbsz / blgp cannot match either;
//   2. accumulation: random finite bytes (max |err| / sum|ab| and rms err / rms bound) and "one big product + 127 small ones"
//      patterns - how far below the largest addend of its group a product can sit before it is lost;
//   3. inf / NaN: inf * 1, inf * 0, inf - inf, NaN * 1, -inf * 1, and that a row without special bytes stays finite.
// Ordinary IEEE values throughout: nothing here faults.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int CBSZ, int BLGP>
__global__ void k_scaled(const i32x8 *a, const i32x8 *b, f32x4 *c, int reps)
{
    int l = threadIdx.x;
    f32x4 acc = {0, 0, 0, 0};
    for (int r = 0; r < reps; ++r)
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l + 64 * r], b[l + 64 * r], acc, CBSZ, BLGP, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    c[l] = acc;
}

static double dec_e4m3(uint8_t b)
{
    if ((b & 0x7F) == 0x7F) return NAN;
    int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
    double v = e == 0 ? m / 8.0 * pow(2, -6) : (1 + m / 8.0) * pow(2, e - 7);
    return s ? -v : v;
}
static double dec_e5m2(uint8_t b)
{
    int s = b >> 7, e = (b >> 2) & 31, m = b & 3;
    double v = e == 31 ? (m ? NAN : INFINITY) : e == 0 ? m / 4.0 * pow(2, -14) : (1 + m / 4.0) * pow(2, e - 15);
    return s ? -v : v;
}
static double dec(uint8_t b, int fmt) { return fmt ? dec_e5m2(b) : dec_e4m3(b); }
static uint8_t enc(double v, int fmt)   // the byte of format fmt whose value is exactly v
{
    for (int b = 0; b < 256; ++b) {
        double d = dec((uint8_t)b, fmt);
        if (d == v && (signbit(d) == signbit(v))) return (uint8_t)b;
    }
    fprintf(stderr, "value %g is not representable in format %d\n", v, fmt);
    exit(2);
}
static bool finite_byte(uint8_t b, int fmt) { return fmt ? (b & 0x7C) != 0x7C : (b & 0x7F) != 0x7F; }

static void launch(int cb, int bl, const uint8_t *A, const uint8_t *B, int reps, float *C)
{
    size_t n = (size_t)64 * 32 * reps;
    uint8_t *dA, *dB; float *dC;
    hipMalloc(&dA, n); hipMalloc(&dB, n); hipMalloc(&dC, 64 * 16);
    hipMemcpy(dA, A, n, hipMemcpyHostToDevice); hipMemcpy(dB, B, n, hipMemcpyHostToDevice);
    const i32x8 *a = (const i32x8 *)dA, *b = (const i32x8 *)dB;
    f32x4 *c = (f32x4 *)dC;
    if (cb == 0 && bl == 0) hipLaunchKernelGGL((k_scaled<0, 0>), 1, 64, 0, 0, a, b, c, reps);
    else if (cb == 1 && bl == 0) hipLaunchKernelGGL((k_scaled<1, 0>), 1, 64, 0, 0, a, b, c, reps);
    else if (cb == 0 && bl == 1) hipLaunchKernelGGL((k_scaled<0, 1>), 1, 64, 0, 0, a, b, c, reps);
    else hipLaunchKernelGGL((k_scaled<1, 1>), 1, 64, 0, 0, a, b, c, reps);
    hipMemcpy(C, dC, 1024, hipMemcpyDeviceToHost);
    hipFree(dA); hipFree(dB); hipFree(dC);
}
// D[i][j] sits in register i % 4 of lane (i / 4) * 16 + j
static float out_of(const float *C, int i, int j) { return C[((i / 4) * 16 + j) * 4 + (i % 4)]; }
static size_t at(int r, int g, int row, int t) { return ((size_t)r * 64 + 16 * g + row) * 32 + t; }

static void compare(const char *name, int cb, int bl, const uint8_t *A, const uint8_t *B, int reps)
{
    float C[256];
    launch(cb, bl, A, B, reps, C);
    double worst = 0, se = 0, sb = 0, maxdiff = 0;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double ex = 0, bd = 0;
            for (int r = 0; r < reps; ++r)
                for (int g = 0; g < 4; ++g)
                    for (int t = 0; t < 32; ++t) {
                        double p = dec(A[at(r, g, i, t)], cb) * dec(B[at(r, g, j, t)], bl);
                        ex += p; bd += fabs(p);
                    }
            double d = fabs(out_of(C, i, j) - ex);
            if (d > maxdiff) maxdiff = d;
            if (d / (bd + 1e-300) > worst) worst = d / (bd + 1e-300);
            se += d * d; sb += bd * bd;
        }
    printf("  (cbsz %d, blgp %d) %-40s K=%5d  max|diff| %.6g  max|err|/sum|ab| %.3e  rms err / rms bound %.3e\n", cb, bl, name, 128 * reps,
           maxdiff, worst, sqrt(se / 256) / (sqrt(sb / 256) + 1e-300));
}

int main()
{
    const int pairs[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
    printf("# 1. operand K-map, exact integer data (max|diff| must be 0 if the e5m2 K-map is the e4m3 one and the format codes bind as assumed)\n");
    for (auto &pr : pairs) {
        const int cb = pr[0], bl = pr[1];
        // values exact in both formats; products <= 64, 128 of them: inside the 2^12 window in which the instruction is exact
        const double vals[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        uint8_t A[64 * 32], B[64 * 32];
        for (int g = 0; g < 4; ++g)
            for (int row = 0; row < 16; ++row)
                for (int t = 0; t < 32; ++t) {
                    const int k = 32 * g + t;
                    double va = vals[(row * 7 + k * 5 + (k >> 3)) % 8] * (((row + k) % 3 == 0) ? -1 : 1);
                    double vb = vals[(row * 3 + k * 11 + (k >> 4) + 1) % 8] * (((row * 2 + k) % 5 == 0) ? -1 : 1);
                    A[at(0, g, row, t)] = enc(va, cb);
                    B[at(0, g, row, t)] = enc(vb, bl);
                }
        compare("integers 1..8, signed, asymmetric", cb, bl, A, B, 1);
        // one-hot: a single non-zero k per row of the first operand against a ramp in the second: reads the pairing of k directly
        int bad = 0;
        for (int k0 = 0; k0 < 128; ++k0) {
            memset(A, 0, sizeof A); memset(B, 0, sizeof B);
            for (int row = 0; row < 16; ++row) A[at(0, k0 / 32, row, k0 % 32)] = enc(1, cb);
            for (int g = 0; g < 4; ++g)
                for (int row = 0; row < 16; ++row)
                    for (int t = 0; t < 32; ++t) B[at(0, g, row, t)] = enc(vals[(32 * g + t) % 8] * (1 << ((32 * g + t) / 32)), bl);   // 1..8 x 2^g
            float C[256];
            launch(cb, bl, A, B, 1, C);
            const double want = vals[k0 % 8] * (1 << (k0 / 32));
            for (int i = 0; i < 16; ++i)
                for (int j = 0; j < 16; ++j) bad += out_of(C, i, j) != (float)want;
        }
        printf("  (cbsz %d, blgp %d) one-hot k against a ramp: %d of %d outputs differ from the e4m3 pairing\n", cb, bl, bad, 128 * 256);
    }
    printf("# 2a. accumulation on random FINITE bytes of each operand's format\n");
    srand(1234);
    for (auto &pr : pairs)
        for (int reps : {1, 8, 32, 128}) {
            size_t n = (size_t)64 * 32 * reps;
            uint8_t *A = (uint8_t *)malloc(n), *B = (uint8_t *)malloc(n);
            for (size_t i = 0; i < n; ++i) {
                do A[i] = rand() & 0xFF; while (!finite_byte(A[i], pr[0]));
                do B[i] = rand() & 0xFF; while (!finite_byte(B[i], pr[1]));
            }
            compare("uniform random finite bytes", pr[0], pr[1], A, B, reps);
            free(A); free(B);
        }
    printf("# 2b. one big product (256 = 16 x 16, group 0) + 127 products of 2^-s: D[0][0] exact vs instruction\n");
    for (auto &pr : pairs)
        for (int s = 2; s <= 18; s += 2) {
            const int ea = s / 2, eb = s - ea;   // 2^-ea x 2^-eb; e4m3 reaches 2^-9, e5m2 2^-16
            if (ea > 9 || eb > 9) break;
            uint8_t A[64 * 32], B[64 * 32];
            for (int i = 0; i < 64 * 32; ++i) { A[i] = enc(pow(2, -ea), pr[0]); B[i] = enc(pow(2, -eb), pr[1]); }
            for (int l = 0; l < 16; ++l) { A[l * 32] = enc(16, pr[0]); B[l * 32] = enc(16, pr[1]); }
            float C[256];
            launch(pr[0], pr[1], A, B, 1, C);
            printf("  (cbsz %d, blgp %d) 256 + 127 x 2^-%-2d  exact %.10g  instruction %.10g  lost %.4g small products\n", pr[0], pr[1], s,
                   256 + 127 * pow(2, -s), C[0], (256 + 127 * pow(2, -s) - C[0]) / pow(2, -s));
        }
    printf("# 3. inf / NaN (e5m2 operands: 0x7C inf, 0xFC -inf, 0x7F NaN; e4m3 operand: 0x7F NaN).  D[0][0] is the row with the special byte, D[1][1] a clean row\n");
    for (auto &pr : pairs) {
        struct Case { const char *name; int a0, a1, b0, b1; };   // bytes at k = 0 and k = 1 of row 0 (first operand) / column 0 (second); -1: value 1
        const int one_a = enc(1, pr[0]), one_b = enc(1, pr[1]);
        const int inf_a = pr[0] ? 0x7C : -2, ninf_a = pr[0] ? 0xFC : -2, inf_b = pr[1] ? 0x7C : -2;
        const Case cases[] = {
            {"first: inf * 1", inf_a, 0, one_b, 0},          {"first: inf * 0", inf_a, 0, 0, 0},
            {"first: inf * 1 + (-inf) * 1", inf_a, ninf_a, one_b, one_b}, {"first: -inf * 1", ninf_a, 0, one_b, 0},
            {"first: NaN byte 0x7F * 1", 0x7F, 0, one_b, 0}, {"second: inf * 1", one_a, 0, inf_b, 0},
            {"second: inf * 0", 0, 0, inf_b, 0},              {"second: NaN byte 0x7F * 1", one_a, 0, 0x7F, 0},
        };
        for (const Case &c : cases) {
            if (c.a0 == -2 || c.a1 == -2 || c.b0 == -2) continue;   // no inf encoding in e4m3
            uint8_t A[64 * 32], B[64 * 32];
            for (int i = 0; i < 64 * 32; ++i) { A[i] = (uint8_t)one_a; B[i] = (uint8_t)one_b; }
            A[at(0, 0, 0, 0)] = (uint8_t)c.a0; A[at(0, 0, 0, 1)] = (uint8_t)c.a1;
            B[at(0, 0, 0, 0)] = (uint8_t)c.b0; B[at(0, 0, 0, 1)] = (uint8_t)c.b1;
            float C[256];
            launch(pr[0], pr[1], A, B, 1, C);
            double ex = 0;
            for (int g = 0; g < 4; ++g)
                for (int t = 0; t < 32; ++t) ex += dec(A[at(0, g, 0, t)], pr[0]) * dec(B[at(0, g, 0, t)], pr[1]);
            printf("  (cbsz %d, blgp %d) %-30s D[0][0] = %-8g (IEEE: %-8g)  D[1][1] = %g (clean row: 128)\n", pr[0], pr[1], c.name, out_of(C, 0, 0), ex,
                   out_of(C, 1, 1));
        }
    }
    return 0;
}
