// The position permutation of the decode attention kernel (csrc/fp8mi_attn_decode.hip), checked on exact integer data with one wave on gfx950:
// eight S^T tiles of v_mfma_scale_f32_16x16x128_f8f6f4 (K rows first source, Q second), packed four registers to a dword, ARE a lane's
// 32-byte second operand of the P.V MFMA when row m of tile t carries position 64 (t >> 2) + 16 (m >> 2) + 4 (t & 3) + (m & 3) of the
// 128-position step and the V operand is two contiguous 16-position runs (16 g .. and 64 + 16 g ..) of a [channel][position] image.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/paged_attn_perm_probe.hip -o tools/probes/paged_attn_perm_probe && tools/probes/paged_attn_perm_probe
// Data: K[pos][ch] in 0 .. 4, query q = e_q + 2 e_(q + 64) (so S[pos][q] = K[pos][q] + 2 K[pos][q + 64] <= 12, exact in e4m3 and different
// from position to position and from query to query), V[d][pos] in -4 .. 4: every sum is an integer far below 2^24.  Exits non-zero on a mismatch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                              \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

constexpr int kPos = 128, kD = 128, kScaleOne = 0x7F7F7F7F;

// (pos * 7 + (pos >> 4)) % 5 would be invariant under the exchange of bits 2..3 and 4..5 of pos - the very permutation under test - and prove nothing
static int k_val(int pos, int ch) { return (pos * 7 + ch * 3 + (pos >> 2) + (pos >> 5)) % 5; }
static int v_val(int d, int pos) { return (d * 5 + pos * 11 + (pos >> 3)) % 9 - 4; }

static uint8_t enc_small(int v)   // an integer of magnitude <= 16 as e4m3fn, exact
{
    if (v == 0) return 0;
    const uint8_t sign = v < 0 ? 0x80 : 0;
    int a = v < 0 ? -v : v, e = 0;
    while ((2 << e) <= a) ++e;
    const int mant = (a * 8 >> e) - 8;   // (a / 2^e - 1) 8: an integer for a <= 16
    return (uint8_t)(sign | ((e + 7) << 3) | mant);
}

static int perm(int t, int m) { return 64 * (t >> 2) + 16 * (m >> 2) + 4 * (t & 3) + (m & 3); }

// kc: [pos][ch] bytes; vc: [d][pos] bytes; qc: [q][ch] bytes; s_out: [t][lane][4] floats; o_out: [dt][lane][4] floats
__global__ __launch_bounds__(64) void probe(const uint8_t *kc, const uint8_t *vc, const uint8_t *qc, float *s_out, float *o_out, int natural)
{
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const u32x4 q0 = *(const u32x4 *)(qc + r * kD + 16 * g), q1 = *(const u32x4 *)(qc + r * kD + 64 + 16 * g);
    const i32x8 qf = {(int)q0[0], (int)q0[1], (int)q0[2], (int)q0[3], (int)q1[0], (int)q1[1], (int)q1[2], (int)q1[3]};
    i32x8 pf;
    for (int t = 0; t < 8; ++t) {
        const int pos = natural ? 16 * t + r : 64 * (t >> 2) + 16 * (r >> 2) + 4 * (t & 3) + (r & 3);
        const u32x4 x0 = *(const u32x4 *)(kc + pos * kD + 16 * g), x1 = *(const u32x4 *)(kc + pos * kD + 64 + 16 * g);
        const i32x8 kf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0, kScaleOne);
        for (int j = 0; j < 4; ++j) s_out[(t * 64 + lane) * 4 + j] = acc[j];
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(acc[0], acc[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(acc[2], acc[3], w, true);
        pf[t] = w;
    }
    for (int dt = 0; dt < kD / 16; ++dt) {
        const uint8_t *row = vc + (16 * dt + r) * kPos;
        const u32x4 x0 = *(const u32x4 *)(row + 16 * g), x1 = *(const u32x4 *)(row + 64 + 16 * g);
        const i32x8 vf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0, kScaleOne);
        for (int j = 0; j < 4; ++j) o_out[(dt * 64 + lane) * 4 + j] = acc[j];
    }
}

int main()
{
    static uint8_t kc[kPos * kD], vc[kD * kPos], qc[16 * kD];
    static float s_host[8 * 64 * 4], o_host[8 * 64 * 4];
    static int S[kPos][16];
    for (int p = 0; p < kPos; ++p)
        for (int c = 0; c < kD; ++c) kc[p * kD + c] = enc_small(k_val(p, c));
    for (int d = 0; d < kD; ++d)
        for (int p = 0; p < kPos; ++p) vc[d * kPos + p] = enc_small(v_val(d, p));
    for (int q = 0; q < 16; ++q)
        for (int c = 0; c < kD; ++c) qc[q * kD + c] = enc_small(c == q ? 1 : c == q + 64 ? 2 : 0);
    for (int p = 0; p < kPos; ++p)
        for (int q = 0; q < 16; ++q) S[p][q] = k_val(p, q) + 2 * k_val(p, q + 64);
    uint8_t *dk, *dv, *dq;
    float *ds, *dout;
    CHECK(hipMalloc(&dk, sizeof(kc)));
    CHECK(hipMalloc(&dv, sizeof(vc)));
    CHECK(hipMalloc(&dq, sizeof(qc)));
    CHECK(hipMalloc(&ds, sizeof(s_host)));
    CHECK(hipMalloc(&dout, sizeof(o_host)));
    CHECK(hipMemcpy(dk, kc, sizeof(kc), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dv, vc, sizeof(vc), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dq, qc, sizeof(qc), hipMemcpyHostToDevice));
    int bad_total = 0;
    for (int natural = 0; natural < 2; ++natural) {
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dk, dv, dq, ds, dout, natural);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(s_host, ds, sizeof(s_host), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(o_host, dout, sizeof(o_host), hipMemcpyDeviceToHost));
        // S^T tile t: lane (q = lane & 15, g = lane >> 4), register j is row m = 4 g + j, whose K row was loaded for position pos(t, m)
        int bad_s = 0, bad_o = 0;
        for (int t = 0; t < 8; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int m = 4 * (lane >> 4) + j, pos = natural ? 16 * t + m : perm(t, m);
                    bad_s += s_host[(t * 64 + lane) * 4 + j] != (float)S[pos][lane & 15];
                }
        // O^T tile dt: lane (q, g), register j is channel 16 dt + 4 g + j; the exact sum over ALL 128 positions
        for (int dt = 0; dt < 8; ++dt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int d = 16 * dt + 4 * (lane >> 4) + j, q = lane & 15;
                    long want = 0;
                    for (int p = 0; p < kPos; ++p) want += (long)v_val(d, p) * S[p][q];
                    bad_o += o_host[(dt * 64 + lane) * 4 + j] != (float)want;
                }
        printf("%s K rows: S^T tiles %d of 2048 values differ from K . Q^T at their positions; O^T %d of 2048 values differ from V^T . S\n",
               natural ? "natural-order (row m of tile t = position 16 t + m)" : "permuted      (row m of tile t = position perm(t, m))", bad_s, bad_o);
        if (!natural) bad_total = bad_s + bad_o;
        else if (bad_s != 0 || bad_o == 0) bad_total += 1;   // the control: S is right, but as a P operand its positions do not meet V's
    }
    printf("probe: %s\n", bad_total == 0 ? "ALL CLAIMS HOLD" : "A CLAIM FAILS");
    return bad_total == 0 ? 0 : 1;
}
