// Probe: how v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands) maps its two E8M0 scale operands onto lanes, rows and K,
// and what it does with the special scale bytes.  Started from tools/mfma_probe.hip.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mxfp8_scale_probe.hip -o mxfp8_scale_probe && ./mxfp8_scale_probe
//
// Data are exact: every run holds ONE product 1.0 x 1.0 at (operand-A row i, operand-B column j, lane group g, byte t of
// the lane's 32 bytes), every other byte is +0.  Each lane's scale dword carries a distinct exponent for its lane in the
// byte op_sel selects (2^(l-32): 95 + l) and 2^40 in the other three bytes, so D[i][j] = 2^(la-32) names the lane (and
// confirms the byte) whose scale was applied to that product.  The other operand's scales are all 2^0.
// Output: for every (operand, op_sel, row, lane group): the scale lane applied to each of the group's 32 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int OPA, int OPB>
__global__ void k_one(const uint8_t *a, const uint8_t *b, const uint32_t *sa, const uint32_t *sb, float *d)
{
    const int l = threadIdx.x, w = blockIdx.x;
    i32x8 x, y;
    memcpy(&x, a + ((size_t)w * 64 + l) * 32, 32);
    memcpy(&y, b + ((size_t)w * 64 + l) * 32, 32);
    f32x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(x, y, acc, 0, 0, OPA, sa[w * 64 + l], OPB, sb[w * 64 + l]);
    for (int r = 0; r < 4; ++r) d[((size_t)w * 64 + l) * 4 + r] = acc[r];
}

// D[i][j] sits in lane (i / 4) * 16 + j, register i % 4 (shape-determined C/D map)
static float dij(const float *d, int w, int i, int j) { return d[((size_t)w * 64 + (i / 4) * 16 + j) * 4 + i % 4]; }

struct Dev {
    uint8_t *a, *b; uint32_t *sa, *sb; float *d; int n;
    explicit Dev(int waves) : n(waves)
    {
        hipMalloc(&a, (size_t)n * 2048); hipMalloc(&b, (size_t)n * 2048);
        hipMalloc(&sa, (size_t)n * 256); hipMalloc(&sb, (size_t)n * 256); hipMalloc(&d, (size_t)n * 1024);
    }
    void run(int opa, int opb, const uint8_t *A, const uint8_t *B, const uint32_t *SA, const uint32_t *SB, float *D)
    {
        hipMemcpy(a, A, (size_t)n * 2048, hipMemcpyHostToDevice); hipMemcpy(b, B, (size_t)n * 2048, hipMemcpyHostToDevice);
        hipMemcpy(sa, SA, (size_t)n * 256, hipMemcpyHostToDevice); hipMemcpy(sb, SB, (size_t)n * 256, hipMemcpyHostToDevice);
        void (*k)(const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, float *) = nullptr;
        if (opa == 0 && opb == 0) k = k_one<0, 0>; else if (opa == 1) k = k_one<1, 0>; else if (opa == 2) k = k_one<2, 0>;
        else if (opa == 3) k = k_one<3, 0>; else if (opb == 1) k = k_one<0, 1>; else if (opb == 2) k = k_one<0, 2>; else k = k_one<0, 3>;
        hipLaunchKernelGGL(k, n, 64, 0, 0, a, b, sa, sb, d);
        hipMemcpy(D, d, (size_t)n * 1024, hipMemcpyDeviceToHost);
    }
};

int main()
{
    // one wave per (row i, lane group g, byte t): 16 x 4 x 32 = 2048 waves
    const int n = 16 * 4 * 32;
    Dev dev(n);
    static uint8_t A[n * 2048], B[n * 2048];
    static uint32_t SA[n * 64], SB[n * 64], ONE[n * 64];
    static float D[n * 256];
    for (int i = 0; i < n * 64; ++i) ONE[i] = 0x7F7F7F7Fu;
    int agree_all = 1;
    for (int side = 0; side < 2; ++side) {      // 0: vary operand A's (first source's) scales, 1: operand B's
        for (int op = 0; op < 4; ++op) {
            memset(A, 0, sizeof A); memset(B, 0, sizeof B);
            for (int w = 0; w < n; ++w) {
                const int i = w / 128, g = (w / 32) % 4, t = w % 32, j = (i + 5) % 16;
                A[((size_t)w * 64 + 16 * g + i) * 32 + t] = 0x38;   // 1.0 at row i
                B[((size_t)w * 64 + 16 * g + j) * 32 + t] = 0x38;   // 1.0 at column j, same lane group and byte
                for (int l = 0; l < 64; ++l) {
                    uint32_t v = 0;
                    for (int k = 0; k < 4; ++k) v |= (uint32_t)(k == op ? 95 + l : 167) << (8 * k);
                    (side ? SB : SA)[w * 64 + l] = v;
                }
            }
            dev.run(side ? 0 : op, side ? op : 0, A, B, side ? ONE : SA, side ? SB : ONE, D);
            printf("operand %s (%s), op_sel %d: scale lane applied to byte t of lane group g, per row (col for B)\n",
                   side ? "B" : "A", side ? "X fragment in the kernels" : "W fragment in the kernels", op);
            for (int i = 0; i < 16; ++i) {
                const int j = (i + 5) % 16;
                printf("  %s%2d:", side ? "col " : "row ", side ? j : i);
                for (int g = 0; g < 4; ++g) {
                    int first = -99, same = 1;
                    for (int t = 0; t < 32; ++t) {
                        const int w = i * 128 + g * 32 + t;
                        const float v = dij(D, w, i, j);
                        const int e = (v > 0.0f && isfinite(v)) ? (int)lrint(log2(v)) : -999;
                        const int lane = e + 32;
                        if (t == 0) first = lane;
                        else if (lane != first) same = 0;
                        if (e < -32 || e > 31) agree_all = 0;
                        if (t == 0 || t == 16) printf(" g%d.t%02d->lane%3d", g, t, lane);
                    }
                    (void)same;
                    for (int t = 0; t < 32; ++t) {   // expected: block 2h + g/2 (h = t / 16), scale lane 16 x block + row
                        const int w = i * 128 + g * 32 + t;
                        const float v = dij(D, w, i, j);
                        const int lane = (v > 0.0f && isfinite(v)) ? (int)lrint(log2(v)) + 32 : -999;
                        if (lane != 16 * (2 * (t / 16) + g / 2) + (side ? j : i)) agree_all = 0;
                    }
                }
                printf("\n");
            }
        }
    }
    printf("map: byte 16h + j of lane group g is K = 64h + 16g + j (32-K block 2h + g/2); the scale of (row r, block b) is lane 16b + r's: %s\n",
           agree_all ? "HOLDS for both operands and every op_sel" : "DOES NOT HOLD (see table)");

    // K order: which bytes of two lane groups pair up is fixed by the data layout (both operands alike).  Block membership
    // is what matters for scaling: confirmed above if each lane group's 32 bytes take one scale.

    // special scale bytes, every lane the same, product 1.0 x 1.0 in (row 0, col 5, g 0, t 0)
    struct Case { const char *what; uint32_t sa, sb; uint8_t da, db; };
    const Case cases[] = {
        {"sa 0x7F sb 0x7F data 1*1", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x38, 0x38},
        {"sa 0x00 sb 0x7F data 1*1 (2^-127)", 0u, 0x7F7F7F7Fu, 0x38, 0x38},
        {"sa 0x00 sb 0x7F data 256*256 (2^-111)", 0u, 0x7F7F7F7Fu, 0x78, 0x78},
        {"sa 0x00 sb 0x00 data 256*256 (2^-238)", 0u, 0u, 0x78, 0x78},
        {"sa 0x01 sb 0x7F data 1*1 (2^-126)", 0x01010101u, 0x7F7F7F7Fu, 0x38, 0x38},
        {"sa 0xFE sb 0x7F data 1*1 (2^127)", 0xFEFEFEFEu, 0x7F7F7F7Fu, 0x38, 0x38},
        {"sa 0xFE sb 0x81 data 1*1 (2^129)", 0xFEFEFEFEu, 0x81818181u, 0x38, 0x38},
        {"sa 0xFF sb 0x7F data 1*1", 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x38, 0x38},
        {"sa 0xFF sb 0x7F data 0*0", 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x00, 0x00},
        {"sa 0x7F sb 0xFF data 0*0", 0x7F7F7F7Fu, 0xFFFFFFFFu, 0x00, 0x00},
        {"sa 0x7F sb 0x7F data NaN(0x7F)*1", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F, 0x38},
    };
    printf("special scales (all lanes alike; D[0][5], and D[1][5] whose row holds only zero bytes):\n");
    Dev one(1);
    for (const Case &c : cases) {
        memset(A, 0, 2048 * n); memset(B, 0, 2048 * n);
        for (int l = 0; l < 64; ++l) { SA[l] = c.sa; SB[l] = c.sb; }
        A[(0 * 64 + 0) * 32 + 0] = c.da;    // row 0, g 0, t 0
        B[(0 * 64 + 5) * 32 + 0] = c.db;    // col 5
        one.run(0, 0, A, B, SA, SB, D);
        printf("  %-40s D[0][5] = %-14.8g (bits %08x)  D[1][5] = %g\n", c.what, dij(D, 0, 0, 5),
               [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; }(dij(D, 0, 0, 5)), dij(D, 0, 1, 5));
    }
    return 0;
}
