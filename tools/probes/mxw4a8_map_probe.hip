// Probe: v_mfma_scale_f32_16x16x128_f8f6f4 with MIXED operands - e2m1 (format code 4) in the first source, e4m3 (code 0) in the
// second - as the MXW4A8 ring kernels issue it (W fragment first, X fragment second).  Does each operand keep the K map and the
// scale map that its own format has when both operands share it (profiles/mxfp4_operand_map.txt, profiles/mxfp8_scale_map.txt)?
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mxw4a8_map_probe.hip -o mxw4a8_map_probe && ./mxw4a8_map_probe
//
// Expected (the claim under test), for logical k = 0..127 of one instruction:
//   first source  (e2m1): lane group g = k / 32, byte t = (k % 32) / 2 of the lane's LOW 16 bytes, nibble n = k % 2 (low first);
//                         bytes 16..31 of the lane are not read (they hold 0x77 = 6.0 | 6.0 in every run)
//   second source (e4m3): lane group g = (k % 64) / 16, byte 16 (k / 64) + k % 16 of the lane's 32
//   scale of (row r, 32-k block b): the byte op_sel picks from lane 16 b + r, both sources alike
// Operands are 8-VGPR (32-byte) fragments per lane, as the ring kernels hold them.  All output goes through plain (vector) stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// one MFMA per wave: w / x 64 lanes x 32 bytes, sw / sx one dword per lane, d 64 lanes x 4 floats
template <int OPW, int OPX>
__global__ void k_one(const uint8_t *w, const uint8_t *x, const uint32_t *sw, const uint32_t *sx, float *d)
{
    const int l = threadIdx.x, b = blockIdx.x;
    i32x8 fw, fx;
    memcpy(&fw, w + ((size_t)b * 64 + l) * 32, 32);
    memcpy(&fx, x + ((size_t)b * 64 + l) * 32, 32);
    f32x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fx, acc, 4, 0, OPW, sw[b * 64 + l], OPX, sx[b * 64 + l]);
    for (int r = 0; r < 4; ++r) d[((size_t)b * 64 + l) * 4 + r] = acc[r];
}

// K = 128 x nsteps with unit scales: one wave, nsteps MFMAs chained through the accumulator (the ring kernels' K loop)
__global__ void k_chain(const uint8_t *w, const uint8_t *x, int nsteps, float *d)
{
    const int l = threadIdx.x;
    f32x4 acc = {0, 0, 0, 0};
    for (int s = 0; s < nsteps; ++s) {
        i32x8 fw, fx;
        memcpy(&fw, w + ((size_t)s * 64 + l) * 32, 32);
        memcpy(&fx, x + ((size_t)s * 64 + l) * 32, 32);
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fx, acc, 4, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
    for (int r = 0; r < 4; ++r) d[l * 4 + r] = acc[r];
}

// D[i][j] sits in lane (i / 4) * 16 + j, register i % 4 (shape-determined C/D map); i: row of the first source, j: of the second
static float dij(const float *d, int w, int i, int j) { return d[((size_t)w * 64 + (i / 4) * 16 + j) * 4 + i % 4]; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static const float kE2M1[16] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f, -0.0f, -0.5f, -1.0f, -1.5f, -2.0f, -3.0f, -4.0f, -6.0f};
static double e4m3(uint8_t b)   // (0x7F / 0xFF, the NaN bytes, are not asked for)
{
    const int e = (b >> 3) & 15, m = b & 7;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return (b & 0x80) ? -v : v;
}

// the expected maps: logical k of row `row` -> byte (and nibble) of wave w's operand image
static void put_w(uint8_t *buf, int w, int row, int k, uint8_t code)
{
    uint8_t &v = buf[((size_t)w * 64 + 16 * (k / 32) + row) * 32 + (k % 32) / 2];
    v = (uint8_t)((k & 1) ? ((v & 0x0F) | (code << 4)) : ((v & 0xF0) | code));
}
static void put_x(uint8_t *buf, int w, int row, int k, uint8_t byte) { buf[((size_t)w * 64 + 16 * ((k % 64) / 16) + row) * 32 + 16 * (k / 64) + k % 16] = byte; }
static void poison_high(uint8_t *buf, int waves)
{
    for (size_t l = 0; l < (size_t)waves * 64; ++l) memset(buf + l * 32 + 16, 0x77, 16);
}

struct Dev {
    uint8_t *w, *x; uint32_t *sw, *sx; float *d; int n;
    explicit Dev(int waves) : n(waves)
    {
        (void)hipMalloc(&w, (size_t)n * 2048); (void)hipMalloc(&x, (size_t)n * 2048);
        (void)hipMalloc(&sw, (size_t)n * 256); (void)hipMalloc(&sx, (size_t)n * 256); (void)hipMalloc(&d, (size_t)n * 1024);
    }
    ~Dev() { (void)hipFree(w); (void)hipFree(x); (void)hipFree(sw); (void)hipFree(sx); (void)hipFree(d); }
    hipError_t run(int opw, int opx, const uint8_t *W, const uint8_t *X, const uint32_t *SW, const uint32_t *SX, float *D)
    {
        hipError_t e;
        if ((e = hipMemcpy(w, W, (size_t)n * 2048, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(x, X, (size_t)n * 2048, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(sw, SW, (size_t)n * 256, hipMemcpyHostToDevice))) return e;
        if ((e = hipMemcpy(sx, SX, (size_t)n * 256, hipMemcpyHostToDevice))) return e;
        void (*k)(const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, float *) = nullptr;
        if (opw == 0 && opx == 0) k = k_one<0, 0>; else if (opw == 1) k = k_one<1, 0>; else if (opw == 2) k = k_one<2, 0>;
        else if (opw == 3) k = k_one<3, 0>; else if (opx == 1) k = k_one<0, 1>; else if (opx == 2) k = k_one<0, 2>; else k = k_one<0, 3>;
        hipLaunchKernelGGL(k, n, 64, 0, 0, w, x, sw, sx, d);
        if ((e = hipGetLastError())) return e;
        return hipMemcpy(D, d, (size_t)n * 1024, hipMemcpyDeviceToHost);
    }
};

int main()
{
    const int n = 128;   // one wave per logical k (operand map) or per (row, block) (scale map)
    static uint8_t W[n * 2048], X[n * 2048];
    static uint32_t SW[n * 64], SX[n * 64], ONE[n * 64];
    static float D[n * 256];
    for (int i = 0; i < n * 64; ++i) ONE[i] = 0x7F7F7F7Fu;
    Dev dev(n);

    // ---- operand map: W holds one 1.0 at logical k of row i; X holds 1.0 (0x38) in column j at k alone ("only"), or at every k but it
    // ("all-but").  "only" must give 1 and "all-but" 0: W's position k meets X's position k and nothing else, and W's high bytes are not read.
    bool map_ok = true;
    printf("operand map: wave k, W (e2m1, first source) row k %% 16 holds 1.0 at logical k, X (e4m3, second source) col (k + 5) %% 16\n");
    for (int pass = 0; pass < 2; ++pass) {
        memset(W, 0, sizeof W); memset(X, 0, sizeof X);
        for (int k = 0; k < n; ++k) {
            const int i = k % 16, j = (k + 5) % 16;
            put_w(W, k, i, k, 0x2);
            for (int k2 = 0; k2 < 128; ++k2)
                if ((pass == 0) == (k2 == k)) put_x(X, k, j, k2, 0x38);
        }
        poison_high(W, n);
        CHECK(dev.run(0, 0, W, X, ONE, ONE, D));
        int bad = 0;
        for (int k = 0; k < n; ++k) {
            const float v = dij(D, k, k % 16, (k + 5) % 16);
            if (v != (pass == 0 ? 1.0f : 0.0f)) { if (bad < 8) printf("    k %3d: D = %g\n", k, v); ++bad; }
        }
        printf("  pass %s: %d of 128 k differ from %s%s\n", pass == 0 ? "only   " : "all-but", bad, pass == 0 ? "1" : "0", bad ? "  <-- UNEXPECTED" : "");
        map_ok = map_ok && bad == 0;
    }
    printf("  W: k = 32g + 2t + n in the low 16 bytes of lane group g (high 16 bytes = 0x77 never read); X: k = 64h + 16g + j in byte 16h + j "
           "of lane group g: %s\n", map_ok ? "HOLDS" : "DOES NOT HOLD");

    // ---- scale map: wave (row i, block b): 1.0 x 1.0 at k = 32 b + 3 (W row i, X col j); lane l of the varied side carries 2^(2l - 64) in the
    // byte op_sel picks and 2^40 in the other three; the other side 2^0.  D = 2^(2 la - 64) names the scale lane la.
    bool scale_ok = true;
    for (int side = 0; side < 2; ++side) {
        printf("scale map, %s scales varied: scale lane of (row, block), op_sel 0..3\n", side ? "X (second source)" : "W (first source)");
        for (int op = 0; op < 4; ++op) {
            memset(W, 0, sizeof W); memset(X, 0, sizeof X);
            for (int w = 0; w < 64; ++w) {
                const int i = w / 4, b = w % 4, j = (i + 5) % 16;
                put_w(W, w, i, 32 * b + 3, 0x2);
                put_x(X, w, j, 32 * b + 3, 0x38);
                for (int l = 0; l < 64; ++l) {
                    uint32_t v = 0;
                    for (int q = 0; q < 4; ++q) v |= (uint32_t)(q == op ? 2 * l + 63 : 167) << (8 * q);
                    (side ? SX : SW)[w * 64 + l] = v;
                }
            }
            poison_high(W, n);
            CHECK(dev.run(side ? 0 : op, side ? op : 0, W, X, side ? ONE : SW, side ? SX : ONE, D));
            int bad = 0;
            for (int w = 0; w < 64; ++w) {
                const int i = w / 4, b = w % 4, j = (i + 5) % 16;
                const float v = dij(D, w, i, j);
                const int e = (v > 0.0f && isfinite(v)) ? (int)lrint(log2(v)) : -999;
                const bool pow2 = v > 0.0f && isfinite(v) && ldexp(1.0, e) == (double)v;
                const int lane = (pow2 && (e & 1) == 0) ? (e + 64) / 2 : -1;
                if (lane != 16 * b + (side ? j : i)) { if (bad < 8) printf("    row %2d block %d: lane %d (D = %g)\n", side ? j : i, b, lane, v); ++bad; }
            }
            printf("  op_sel %d: %d of 64 (row, block) do not take their scale from lane 16 b + row%s\n", op, bad, bad ? "  <-- UNEXPECTED" : "");
            scale_ok = scale_ok && bad == 0;
        }
    }
    printf("  scale of (row r, block b) = the byte op_sel picks from lane 16 b + r, both sources: %s\n", scale_ok ? "HOLDS" : "DOES NOT HOLD");

    // ---- special bytes (one wave; product at W row 0 / X col 5, k = 0; D[1][5] sums only zeros)
    struct Case { const char *what; uint32_t sw, sx; uint8_t dw, dx; };
    const Case cases[] = {
        {"sw 0x7F sx 0x7F  W 1.0 x X 1.0", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x2, 0x38},
        {"sw 0x00 sx 0x7F  W 1.0 x X 1.0 (2^-127)", 0u, 0x7F7F7F7Fu, 0x2, 0x38},
        {"sw 0x7F sx 0x00  W 1.0 x X 1.0 (2^-127)", 0x7F7F7F7Fu, 0u, 0x2, 0x38},
        {"sw 0xFF sx 0x7F  W 0 x X 0", 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x0, 0x00},
        {"sw 0x7F sx 0xFF  W 0 x X 0", 0x7F7F7F7Fu, 0xFFFFFFFFu, 0x0, 0x00},
        {"sw 0x7F sx 0x7F  W 6.0 (0x7) x X 448 (0x7E)", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7, 0x7E},
        {"sw 0x7F sx 0x7F  W -6.0 (0xF) x X 1.0", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0xF, 0x38},
        {"sw 0x7F sx 0x7F  W 1.0 x X byte 0x7F (NaN)", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x2, 0x7F},
        {"sw 0x7F sx 0x7F  W 0 x X byte 0xFF (NaN)", 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x0, 0xFF},
    };
    bool special_ok = true;
    printf("special bytes (all lanes' scales alike):\n");
    {
        Dev one(1);
        float got[9];
        int c = 0;
        for (const Case &cs : cases) {
            memset(W, 0, 2048); memset(X, 0, 2048);
            for (int l = 0; l < 64; ++l) { SW[l] = cs.sw; SX[l] = cs.sx; }
            put_w(W, 0, 0, 0, cs.dw);
            put_x(X, 0, 5, 0, cs.dx);
            poison_high(W, 1);
            CHECK(one.run(0, 0, W, X, SW, SX, D));
            got[c++] = dij(D, 0, 0, 5);
            printf("  %-46s D[0][5] = %-14.8g (bits %08x)  D[1][5] = %g\n", cs.what, dij(D, 0, 0, 5), bits(dij(D, 0, 0, 5)), dij(D, 0, 1, 5));
            if (c == 4 || c == 5) special_ok = special_ok && isnan(dij(D, 0, 1, 5));   // a NaN scale reaches rows of zeros too
        }
        special_ok = special_ok && got[0] == 1.0f && bits(got[1]) == 0x00400000u && bits(got[2]) == 0x00400000u && isnan(got[3]) && isnan(got[4]) &&
                     got[5] == 2688.0f && got[6] == -6.0f && isnan(got[7]) && isnan(got[8]);
        printf("  scale 0xFF gives NaN on either side, scale 0x00 is 2^-127, e2m1 0x7 / 0xF are +-6.0, X's bytes 0x7F / 0xFF are NaN (also against a "
               "zero of W): %s\n", special_ok ? "yes" : "NO");
    }

    // ---- accumulation: unit scales, K = 4096 (32 chained MFMAs), X from the e4m3 bytes that are multiples of 1/8 up to 16, W any code:
    // every product is a multiple of 1/16 up to 96 and every partial sum below 2^19, so the exact sum is one fp32 value
    bool acc_ok = true;
    {
        const int steps = 32;
        static uint8_t CW[steps * 2048], CX[steps * 2048];
        uint8_t ok_bytes[256]; int nok = 0;
        for (int b = 0; b < 256; ++b) {
            if ((b & 0x7F) == 0x7F) continue;
            const double v = e4m3((uint8_t)b);
            if (fabs(v) <= 16.0 && v * 8.0 == floor(v * 8.0)) ok_bytes[nok++] = (uint8_t)b;
        }
        uint32_t seed = 12345u;
        auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 16; };
        memset(CW, 0, sizeof CW);
        for (int s = 0; s < steps; ++s)
            for (int r = 0; r < 16; ++r)
                for (int k = 0; k < 128; ++k) {
                    put_w(CW, s, r, k, (uint8_t)(r == 0 ? 0x7 : rnd() & 15));            // row 0 / col 0: the largest magnitude, 6 x 16 x 4096
                    put_x(CX, s, r, k, r == 0 ? (uint8_t)0x58 : ok_bytes[rnd() % nok]);  // 0x58 = 16.0
                }
        poison_high(CW, steps);
        uint8_t *cw, *cx; float *cd;
        CHECK(hipMalloc(&cw, sizeof CW)); CHECK(hipMalloc(&cx, sizeof CX)); CHECK(hipMalloc(&cd, 1024));
        CHECK(hipMemcpy(cw, CW, sizeof CW, hipMemcpyHostToDevice)); CHECK(hipMemcpy(cx, CX, sizeof CX, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_chain, 1, 64, 0, 0, cw, cx, steps, cd);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(D, cd, 1024, hipMemcpyDeviceToHost));
        int bad = 0;
        double maxabs = 0;
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double ex = 0;
                for (int s = 0; s < steps; ++s)
                    for (int k = 0; k < 128; ++k) {
                        const uint8_t qw = (CW[((size_t)s * 64 + 16 * (k / 32) + i) * 32 + (k % 32) / 2] >> (4 * (k & 1))) & 15;
                        const uint8_t qx = CX[((size_t)s * 64 + 16 * ((k % 64) / 16) + j) * 32 + 16 * (k / 64) + k % 16];
                        ex += (double)kE2M1[qw] * e4m3(qx);
                    }
                maxabs = fmax(maxabs, fabs(ex));
                bad += (double)dij(D, 0, i, j) != ex;
            }
        acc_ok = bad == 0;
        printf("accumulation, unit scales, K = 4096 (32 chained MFMAs), %d usable e4m3 bytes (max |sum| %.0f): %d of 256 outputs differ from the "
               "exact sum\n", nok, maxabs, bad);
        (void)hipFree(cw); (void)hipFree(cx); (void)hipFree(cd);
    }
    const bool all = map_ok && scale_ok && special_ok && acc_ok;
    printf("probe: %s\n", all ? "ALL CLAIMS HOLD" : "SOME CLAIM FAILED");
    return all ? 0 : 1;
}
