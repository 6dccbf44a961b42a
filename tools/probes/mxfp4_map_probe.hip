// Probe: how v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1 (fp4) operands (format code 4 in both format fields) maps operand
// nibbles onto K and 32-K blocks, where it takes each block's E8M0 scale from, which registers it reads, what the special
// scale bytes do and how it accumulates.  Started from tools/probes/mxfp8_scale_probe.hip.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mxfp4_map_probe.hip -o mxfp4_map_probe && ./mxfp4_map_probe
//
// Operands are 8-VGPR (32-byte) fragments per lane, as the ring kernels hold them.  Bytes 0..15 of a lane (its low 4 VGPRs)
// carry the data; bytes 16..31 (the high 4 VGPRs) hold 0x77 (6.0 in both nibbles) in every run, so a product that read them
// would add 36 x scale to the output.  Position p = (lane group g, byte t, nibble n; n = 0 the low nibble) of a lane.
// Map runs: operand A holds one 1.0 (code 0x2) at p in row i; operand B holds 1.0 at EVERY position of column j (pass "all")
// or at every position but p (pass "all-but-p").  Each lane's scale dword carries 2^(2l - 64) (byte 2l + 63) in the byte op_sel
// picks and 2^40 in the other three, the other operand's scales are 2^0.  So in pass "all", D[i][j] = c x 2^(2la - 64): an even
// exponent names the scale lane la (and confirms the byte), c = 1 says exactly one B position pairs with p; pass "all-but-p"
// must give 0 (p pairs with p and with nothing else).  All output goes through plain (vector) stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// one MFMA per wave: a / b 64 lanes x 32 bytes, sa / sb one dword per lane, d 64 lanes x 4 floats
template <int OPA, int OPB>
__global__ void k_one(const uint8_t *a, const uint8_t *b, const uint32_t *sa, const uint32_t *sb, float *d)
{
    const int l = threadIdx.x, w = blockIdx.x;
    i32x8 x, y;
    memcpy(&x, a + ((size_t)w * 64 + l) * 32, 32);
    memcpy(&y, b + ((size_t)w * 64 + l) * 32, 32);
    f32x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(x, y, acc, 4, 4, OPA, sa[w * 64 + l], OPB, sb[w * 64 + l]);
    for (int r = 0; r < 4; ++r) d[((size_t)w * 64 + l) * 4 + r] = acc[r];
}

// the same MFMA written in assembly with the operands pinned to v[8:15] and v[16:23]: the instruction names only the base
// register of each operand, so this shows what the hardware itself reads when the registers above the low four hold data
__global__ void k_pinned(const uint8_t *a, const uint8_t *b, const uint32_t *sa, const uint32_t *sb, float *d)
{
    const int l = threadIdx.x, w = blockIdx.x;
    i32x8 x, y;
    memcpy(&x, a + ((size_t)w * 64 + l) * 32, 32);
    memcpy(&y, b + ((size_t)w * 64 + l) * 32, 32);
    f32x4 acc = {0, 0, 0, 0};
    asm volatile("s_nop 7\n\ts_nop 7\n\t"
                 "v_mfma_scale_f32_16x16x128_f8f6f4 %0, v[8:11], v[16:19], %0, %1, %2 op_sel_hi:[0,0,0] cbsz:4 blgp:4\n\t"
                 "s_nop 7\n\ts_nop 7\n\ts_nop 7"
                 : "+v"(acc) : "v"(sa[w * 64 + l]), "v"(sb[w * 64 + l]), "{v[8:15]}"(x), "{v[16:23]}"(y));
    for (int r = 0; r < 4; ++r) d[((size_t)w * 64 + l) * 4 + r] = acc[r];
}

// K = 128 x nsteps with unit scales: one wave, nsteps MFMAs chained through the accumulator (the ring kernels' K loop)
__global__ void k_chain(const uint8_t *a, const uint8_t *b, int nsteps, float *d)
{
    const int l = threadIdx.x;
    f32x4 acc = {0, 0, 0, 0};
    for (int s = 0; s < nsteps; ++s) {
        i32x8 x, y;
        memcpy(&x, a + ((size_t)s * 64 + l) * 32, 32);
        memcpy(&y, b + ((size_t)s * 64 + l) * 32, 32);
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(x, y, acc, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
    for (int r = 0; r < 4; ++r) d[l * 4 + r] = acc[r];
}

// D[i][j] sits in lane (i / 4) * 16 + j, register i % 4 (shape-determined C/D map)
static float dij(const float *d, int w, int i, int j) { return d[((size_t)w * 64 + (i / 4) * 16 + j) * 4 + i % 4]; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static const float kE2M1[16] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f, -0.0f, -0.5f, -1.0f, -1.5f, -2.0f, -3.0f, -4.0f, -6.0f};

// set nibble n of byte t of lane (16g + row) of wave w
static void put(uint8_t *buf, int w, int g, int row, int t, int n, uint8_t code)
{
    uint8_t &v = buf[((size_t)w * 64 + 16 * g + row) * 32 + t];
    v = (uint8_t)((v & (n ? 0x0F : 0xF0)) | (code << (4 * n)));
}

static void poison_high(uint8_t *buf, int waves)
{
    for (size_t w = 0; w < (size_t)waves * 64; ++w) memset(buf + w * 32 + 16, 0x77, 16);
}

struct Dev {
    uint8_t *a, *b; uint32_t *sa, *sb; float *d; int n;
    explicit Dev(int waves) : n(waves)
    {
        (void)hipMalloc(&a, (size_t)n * 2048); (void)hipMalloc(&b, (size_t)n * 2048);
        (void)hipMalloc(&sa, (size_t)n * 256); (void)hipMalloc(&sb, (size_t)n * 256); (void)hipMalloc(&d, (size_t)n * 1024);
    }
    hipError_t run(int opa, int opb, bool pinned, const uint8_t *A, const uint8_t *B, const uint32_t *SA, const uint32_t *SB, float *D)
    {
        hipError_t e;
        if ((e = hipMemcpy(a, A, (size_t)n * 2048, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(b, B, (size_t)n * 2048, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(sa, SA, (size_t)n * 256, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(sb, SB, (size_t)n * 256, hipMemcpyHostToDevice))) return e;
        void (*k)(const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, float *) = nullptr;
        if (pinned) k = k_pinned;
        else if (opa == 0 && opb == 0) k = k_one<0, 0>; else if (opa == 1) k = k_one<1, 0>; else if (opa == 2) k = k_one<2, 0>;
        else if (opa == 3) k = k_one<3, 0>; else if (opb == 1) k = k_one<0, 1>; else if (opb == 2) k = k_one<0, 2>; else k = k_one<0, 3>;
        hipLaunchKernelGGL(k, n, 64, 0, 0, a, b, sa, sb, d);
        if ((e = hipGetLastError())) return e;
        return hipMemcpy(D, d, (size_t)n * 1024, hipMemcpyDeviceToHost);
    }
};

int main()
{
    // one wave per (row i, lane group g, byte t, nibble n): 16 x 4 x 16 x 2 = 2048 waves
    const int n = 16 * 4 * 16 * 2;
    Dev dev(n);
    static uint8_t A[n * 2048], B[n * 2048];
    static uint32_t SA[n * 64], SB[n * 64], ONE[n * 64];
    static float D[n * 256];
    for (int i = 0; i < n * 64; ++i) ONE[i] = 0x7F7F7F7Fu;
    bool map_ok = true;
    for (int side = 0; side < 2; ++side) {      // 0: vary operand A's (first source's) scales, 1: operand B's
        for (int op = 0; op < 4; ++op) {
            for (int pass = 0; pass < (op == 0 ? 2 : 1); ++pass) {   // 0: B at every position; 1: every position but p
                memset(A, 0, sizeof A); memset(B, 0, sizeof B);
                for (int w = 0; w < n; ++w) {
                    const int i = w / 128, g = (w / 32) % 4, t = (w / 2) % 16, nb = w % 2, j = (i + 5) % 16;
                    put(A, w, g, i, t, nb, 0x2);
                    for (int g2 = 0; g2 < 4; ++g2)
                        for (int t2 = 0; t2 < 16; ++t2)
                            for (int n2 = 0; n2 < 2; ++n2)
                                if (pass == 0 || g2 != g || t2 != t || n2 != nb) put(B, w, g2, j, t2, n2, 0x2);
                    for (int l = 0; l < 64; ++l) {
                        uint32_t v = 0;
                        for (int k = 0; k < 4; ++k) v |= (uint32_t)(k == op ? 2 * l + 63 : 167) << (8 * k);
                        (side ? SB : SA)[w * 64 + l] = v;
                    }
                }
                poison_high(A, n); poison_high(B, n);
                CHECK(dev.run(side ? 0 : op, side ? op : 0, false, A, B, side ? ONE : SA, side ? SB : ONE, D));
                if (pass == 1) {
                    int nonzero = 0;
                    for (int w = 0; w < n; ++w) nonzero += dij(D, w, w / 128, (w / 128 + 5) % 16) != 0.0f;
                    printf("operand %s, pass all-but-p: %d of %d positions pair with another position%s\n", side ? "B" : "A", nonzero, n,
                           nonzero ? "  <-- UNEXPECTED" : "");
                    map_ok = map_ok && nonzero == 0;
                    continue;
                }
                printf("operand %s (%s), op_sel %d: scale lane applied at (lane group g, byte t, nibble n), per row (col for B)\n",
                       side ? "B" : "A", side ? "X fragment in the kernels" : "W fragment in the kernels", op);
                for (int i = 0; i < 16; ++i) {
                    const int j = (i + 5) % 16;
                    printf("  %s%2d:", side ? "col " : "row ", side ? j : i);
                    for (int g = 0; g < 4; ++g) {
                        for (int t = 0; t < 16; ++t)
                            for (int nb = 0; nb < 2; ++nb) {
                                const int w = i * 128 + g * 32 + t * 2 + nb;
                                const float v = dij(D, w, i, j);
                                const int e = (v > 0.0f && isfinite(v)) ? (int)lrint(log2(v)) : -999;
                                const bool pow2 = v > 0.0f && isfinite(v) && ldexp(1.0, e) == (double)v;
                                const int lane = (pow2 && (e & 1) == 0) ? (e + 64) / 2 : -1;   // odd exponent: 2 positions paired
                                if (t == 0 && nb == 0) printf(" g%d->lane%3d", g, lane);
                                if (lane != 16 * g + (side ? j : i)) map_ok = false;   // expected: block g of the 4, scale lane 16g + row
                            }
                    }
                    printf("\n");
                }
            }
        }
    }
    printf("map: nibble n of byte t of lane group g is k = 32g + 2t + n (the 32-k block g: one block per lane group, low nibble first), "
           "each position pairs with the same position of the other operand and nothing else, and the scale of (row r, block b) is the "
           "byte op_sel picks from lane 16b + r - both operands alike: %s\n", map_ok ? "HOLDS" : "DOES NOT HOLD (see table)");
    printf("registers: bytes 16..31 of every lane (the high 4 VGPRs of the 8-VGPR fragment) held 0x77 (6.0 x 6.0 = 36 per product) in "
           "every run above: %s\n", map_ok ? "never read" : "see table");

    // the same with the assembly form pinned to 8-VGPR operands (position: row 0, g 1, byte 3, low nibble; scale lanes 2^0)
    bool pinned_ok = true;
    {
        Dev one(1);
        memset(A, 0, 2048); memset(B, 0, 2048);
        for (int r = 0; r < 16; ++r) { put(A, 0, 1, r, 3, 0, 0x2); put(B, 0, 1, r, 3, 0, 0x4); }   // 1.0 x 2.0 at one position
        poison_high(A, 1); poison_high(B, 1);
        for (int l = 0; l < 64; ++l) { SA[l] = 0x7F7F7F7Fu; SB[l] = 0x7F7F7F7Fu; }
        CHECK(one.run(0, 0, true, A, B, SA, SB, D));
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) pinned_ok = pinned_ok && dij(D, 0, i, j) == 2.0f;
        printf("pinned 8-VGPR operands (v[8:15], v[16:23]; high 4 = 0x77): every D = 2.0 (1.0 x 2.0, nothing from the high registers): %s\n",
               pinned_ok ? "yes" : "NO");
    }

    // format code 4 decodes e2m1: each code of operand A at one position times 1.0
    bool dec_ok = true;
    {
        Dev one(1);
        printf("e2m1 decode (cbsz 4 / blgp 4), code: value\n ");
        for (int c = 0; c < 16; ++c) {
            memset(A, 0, 2048); memset(B, 0, 2048);
            put(A, 0, 2, 0, 7, 1, (uint8_t)c); put(B, 0, 2, 5, 7, 1, 0x2);
            poison_high(A, 1); poison_high(B, 1);
            for (int l = 0; l < 64; ++l) { SA[l] = 0x7F7F7F7Fu; SB[l] = 0x7F7F7F7Fu; }
            CHECK(one.run(0, 0, false, A, B, SA, SB, D));
            const float v = dij(D, 0, 0, 5);
            printf(" %X:%g", c, v);
            dec_ok = dec_ok && v == kE2M1[c];
        }
        printf("\n  matches the OCP e2m1 table (0x7 = 6.0, 0xF = -6.0; no NaN, no inf): %s\n", dec_ok ? "yes" : "NO");
    }

    // special scale bytes, every lane alike: products in (row 0, col 5)
    struct Case { const char *what; uint32_t sa, sb; uint8_t da, db; };
    const Case cases[] = {
        {"sa 0x7F sb 0x7F data 1*1", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x2, 0x2},
        {"sa 0x00 sb 0x7F data 1*1 (2^-127)", 0u, 0x7F7F7F7Fu, 0x2, 0x2},
        {"sa 0x00 sb 0x7F data 6*6 (36 x 2^-127)", 0u, 0x7F7F7F7Fu, 0x7, 0x7},
        {"sa 0x00 sb 0x00 data 6*6 (36 x 2^-254)", 0u, 0u, 0x7, 0x7},
        {"sa 0x01 sb 0x7F data 1*1 (2^-126)", 0x01010101u, 0x7F7F7F7Fu, 0x2, 0x2},
        {"sa 0xFE sb 0x7F data 1*1 (2^127)", 0xFEFEFEFEu, 0x7F7F7F7Fu, 0x2, 0x2},
        {"sa 0xFE sb 0x81 data 1*1 (2^129)", 0xFEFEFEFEu, 0x81818181u, 0x2, 0x2},
        {"sa 0xFF sb 0x7F data 1*1", 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x2, 0x2},
        {"sa 0xFF sb 0x7F data 0*0", 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x0, 0x0},
        {"sa 0x7F sb 0xFF data 0*0", 0x7F7F7F7Fu, 0xFFFFFFFFu, 0x0, 0x0},
        {"sa 0x7F sb 0x7F data 0xF*0x7 (-6*6)", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0xF, 0x7},
    };
    bool special_ok = true;
    printf("special scales (all lanes alike; D[0][5], and D[1][5] whose row holds only zero nibbles):\n");
    {
        Dev one(1);
        for (const Case &c : cases) {
            memset(A, 0, 2048); memset(B, 0, 2048);
            for (int l = 0; l < 64; ++l) { SA[l] = c.sa; SB[l] = c.sb; }
            put(A, 0, 0, 0, 0, 0, c.da);    // row 0, g 0, byte 0, low nibble
            put(B, 0, 0, 5, 0, 0, c.db);    // col 5
            poison_high(A, 1); poison_high(B, 1);
            CHECK(one.run(0, 0, false, A, B, SA, SB, D));
            printf("  %-40s D[0][5] = %-14.8g (bits %08x)  D[1][5] = %g\n", c.what, dij(D, 0, 0, 5), bits(dij(D, 0, 0, 5)), dij(D, 0, 1, 5));
        }
        // the claims the kernels rely on: 0xFF is NaN (also for zero data), 0x00 is 2^-127 (kept as an fp32 subnormal)
        memset(A, 0, 2048); memset(B, 0, 2048);
        put(A, 0, 0, 0, 0, 0, 0x2); put(B, 0, 0, 5, 0, 0, 0x2);
        poison_high(A, 1); poison_high(B, 1);
        for (int l = 0; l < 64; ++l) { SA[l] = 0u; SB[l] = 0x7F7F7F7Fu; }
        CHECK(one.run(0, 0, false, A, B, SA, SB, D));
        special_ok = special_ok && bits(dij(D, 0, 0, 5)) == 0x00400000u;
        for (int l = 0; l < 64; ++l) { SA[l] = 0xFFFFFFFFu; }
        CHECK(one.run(0, 0, false, A, B, SA, SB, D));
        special_ok = special_ok && isnan(dij(D, 0, 0, 5)) && isnan(dij(D, 0, 1, 5));
        printf("  scale 0xFF gives NaN, scale 0x00 gives 2^-127: %s\n", special_ok ? "yes" : "NO");
    }

    // accumulation.  (1) inside one MFMA: block 0 gives 2^24, blocks 1 and 2 give 1 each (2^24 + 2 is an fp32 value; a
    // sequential fp32 sum would round 2^24 + 1 back to 2^24).  (2) unit scales, K = 4096 (32 chained MFMAs), random codes: every
    // product is a multiple of 0.25 up to 36, every partial sum below 2^22 in magnitude, so an exact sum is one fp32 value.
    bool acc_ok = true;
    {
        Dev one(1);
        memset(A, 0, 2048); memset(B, 0, 2048);
        for (int r = 0; r < 16; ++r)
            for (int g = 0; g < 3; ++g) { put(A, 0, g, r, 0, 0, 0x2); put(B, 0, g, r, 0, 0, 0x2); }
        poison_high(A, 1); poison_high(B, 1);
        for (int l = 0; l < 64; ++l) { SA[l] = (l < 16) ? 0x97979797u : 0x7F7F7F7Fu; SB[l] = 0x7F7F7F7Fu; }   // block 0 of A: 2^24
        CHECK(one.run(0, 0, false, A, B, SA, SB, D));
        printf("accumulation inside one MFMA: 2^24 + 1 + 1 (three blocks) = %.1f (%s)\n", dij(D, 0, 0, 0),
               dij(D, 0, 0, 0) == 16777218.0f ? "the exact sum, rounded once" : "NOT the exact sum");

        const int steps = 32;   // K = 4096
        static uint8_t CA[steps * 2048], CB[steps * 2048];
        uint32_t seed = 12345u;
        auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
        for (int i = 0; i < steps * 2048; ++i) { CA[i] = (uint8_t)rnd(); CB[i] = (uint8_t)rnd(); }
        poison_high(CA, steps); poison_high(CB, steps);
        // worst case for magnitude on row 0 / col 0: every nibble 6.0 (36 x 4096 = 147456)
        for (int s = 0; s < steps; ++s)
            for (int g = 0; g < 4; ++g) { memset(CA + ((size_t)s * 64 + 16 * g) * 32, 0x77, 16); memset(CB + ((size_t)s * 64 + 16 * g) * 32, 0x77, 16); }
        uint8_t *ca, *cb; float *cd;
        CHECK(hipMalloc(&ca, sizeof CA)); CHECK(hipMalloc(&cb, sizeof CB)); CHECK(hipMalloc(&cd, 1024));
        CHECK(hipMemcpy(ca, CA, sizeof CA, hipMemcpyHostToDevice)); CHECK(hipMemcpy(cb, CB, sizeof CB, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_chain, 1, 64, 0, 0, ca, cb, steps, cd);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(D, cd, 1024, hipMemcpyDeviceToHost));
        int bad = 0;
        double maxabs = 0;
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double ex = 0;
                for (int s = 0; s < steps; ++s)
                    for (int g = 0; g < 4; ++g)
                        for (int t = 0; t < 16; ++t)
                            for (int nb = 0; nb < 2; ++nb) {
                                const uint8_t qa = (CA[((size_t)s * 64 + 16 * g + i) * 32 + t] >> (4 * nb)) & 15;
                                const uint8_t qb = (CB[((size_t)s * 64 + 16 * g + j) * 32 + t] >> (4 * nb)) & 15;
                                ex += (double)kE2M1[qa] * (double)kE2M1[qb];
                            }
                maxabs = fmax(maxabs, fabs(ex));
                bad += (double)dij(D, 0, i, j) != ex;
            }
        acc_ok = bad == 0;
        printf("accumulation, unit scales, K = 4096 (32 chained MFMAs), random codes (max |sum| %.0f): %d of 256 outputs differ from the "
               "exact sum\n", maxabs, bad);
        (void)hipFree(ca); (void)hipFree(cb); (void)hipFree(cd);
    }
    const bool all = map_ok && pinned_ok && dec_ok && special_ok && acc_ok;
    printf("probe: %s\n", all ? "ALL CLAIMS HOLD" : "SOME CLAIM FAILED");
    return all ? 0 : 1;
}
