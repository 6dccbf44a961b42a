// Which lane receives which byte from gfx950's LDS transpose read ds_read_b64_tr_b8 (__builtin_amdgcn_ds_read_tr8_b64_v2i32), settled on exact
// data with one wave, for the P.V operand of the MLA decode kernel (csrc/fp8mi_attn_mla.hip).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mla_transpose_probe.hip -o tools/probes/mla_transpose_probe && tools/probes/mla_transpose_probe
// Part 1, the raw map.  Lane s hands the instruction the address of ITS 8 bytes (8 s .. 8 s + 7 of a 512-byte image).  The image is read three
// times with byte = source lane, byte = index inside the source lane's 8, and byte = 37 s + 11 k mod 251 (a value no exchange of lanes or
// bytes leaves in place): every destination (lane, byte) then names its source exactly.  Two candidate maps are tested against it, for
// destination lane i = 16 G + c, byte k:
//   A  source lane 16 G + 2 k + (c >> 3), source byte c & 7      (the 16 source lanes are 8 rows x 2 halves, the halves adjacent)
//   B  source lane 16 G + k + 8 (c >> 3), source byte c & 7      (the halves 8 lanes apart)
// The identifiers differ in every (lane, byte), so at most one candidate can hold: that is the control - data that a wrong map cannot satisfy.
// Part 2, the operand.  A [128 position][pitch] image of e4m3 integers V[pos][ch] is read with the kernel's own addressing (position map pi of
// fp8mi_attn_mla.hip) into the first operand of v_mfma_scale_f32_16x16x128_f8f6f4; the second operand is P[slot] = weights placed by the same
// map; the exact integer sums sum_pos V[pos][ch] w[pos] must come out.  Control: the same reads with the OTHER candidate's addressing must
// miss.  Exits non-zero when a claim fails.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                              \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

constexpr int kPitch = 592, kRows = 128, kCh = 32, kScaleOne = 0x7F7F7F7F;

__global__ __launch_bounds__(64) void raw_probe(const uint8_t *img, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[512];
    const int lane = threadIdx.x;
    for (int k = 0; k < 8; ++k) lds[8 * lane + k] = img[8 * lane + k];
    __syncthreads();
    const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)(lds + 8 * lane));
    for (int k = 0; k < 8; ++k) out[8 * lane + k] = (uint8_t)((uint32_t)v[k >> 2] >> (8 * (k & 3)));
}

// slot 64 h + 16 g + 8 u + e of the MFMA's contraction is position pi(...) of the step (fp8mi_attn_mla.hip)
__host__ __device__ static int pi_pos(int h, int g, int u, int e) { return (e & 3) + 4 * (g & 1) + 8 * ((g >> 1) ^ (e >> 2)) + 16 * (e >> 2) + 32 * u + 64 * h; }

// img: [128][kPitch] bytes (channels 0 .. kCh - 1 used); pw: [128 slots] e4m3 weights, one column for all 16; o_out: [kCh / 16][64][4]
__global__ __launch_bounds__(64) void operand_probe(const uint8_t *img, const uint8_t *pw, float *o_out, int map_b)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * kPitch];
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    for (int i = lane; i < kRows * kPitch / 4; i += 64) ((uint32_t *)lds)[i] = ((const uint32_t *)img)[i];
    __syncthreads();
    const int e = map_b ? (c & 7) : (c >> 1), hh = map_b ? (c >> 3) : (c & 1);   // this lane AS A SOURCE: position e of eight, channel half hh
    i32x8 pf;
    for (int w = 0; w < 8; ++w) pf[w] = ((const int *)pw)[(w >> 2) * 16 + 4 * g + (w & 3)];   // slots 64 h + 16 g + [0, 16): bytes 16 h + [0, 16)
    for (int dt = 0; dt < kCh / 16; ++dt) {
        i32x8 vf;
        for (int h = 0; h < 2; ++h)
            for (int u = 0; u < 2; ++u) {
                const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                    (__attribute__((address_space(3))) i32x2 *)(lds + pi_pos(h, g, u, e) * kPitch + 16 * dt + 8 * hh));
                vf[4 * h + 2 * u] = v[0];
                vf[4 * h + 2 * u + 1] = v[1];
            }
        const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0, kScaleOne);
        for (int j = 0; j < 4; ++j) o_out[(dt * 64 + lane) * 4 + j] = acc[j];
    }
}

static uint8_t enc_small(int v)   // an integer of magnitude <= 16 as e4m3fn, exact
{
    if (v == 0) return 0;
    const uint8_t sign = v < 0 ? 0x80 : 0;
    int a = v < 0 ? -v : v, e = 0;
    while ((2 << e) <= a) ++e;
    return (uint8_t)(sign | ((e + 7) << 3) | ((a * 8 >> e) - 8));
}
// neither is invariant under an exchange of position bits or of channel bits
static int v_val(int pos, int ch) { return (pos * 7 + ch * 5 + (pos >> 2) + (pos >> 5) + (ch >> 3)) % 9 - 4; }
static int w_val(int pos) { return (pos * 3 + (pos >> 3) + (pos >> 4)) % 5; }

int main()
{
    static uint8_t img[512], got[3][512];
    uint8_t *d_img, *d_out;
    CHECK(hipMalloc(&d_img, 512));
    CHECK(hipMalloc(&d_out, 512));
    for (int pass = 0; pass < 3; ++pass) {
        for (int s = 0; s < 64; ++s)
            for (int k = 0; k < 8; ++k) img[8 * s + k] = (uint8_t)(pass == 0 ? s : pass == 1 ? k : (37 * s + 11 * k) % 251);
        CHECK(hipMemcpy(d_img, img, 512, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(raw_probe, dim3(1), dim3(64), 0, 0, d_img, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(got[pass], d_out, 512, hipMemcpyDeviceToHost));
    }
    printf("ds_read_b64_tr_b8, lane s supplies bytes 8 s .. 8 s + 7.  destination lane: (source lane.source byte) of its bytes 0 .. 7\n");
    int bad_a = 0, bad_b = 0, bad_id = 0;
    for (int i = 0; i < 64; ++i) {
        printf("  lane %2d:", i);
        for (int k = 0; k < 8; ++k) {
            const int s = got[0][8 * i + k], sb = got[1][8 * i + k], G = i >> 4, c = i & 15;
            printf(" %2d.%d", s, sb);
            bad_id += got[2][8 * i + k] != (uint8_t)((37 * s + 11 * sb) % 251);   // the third image agrees with the two that named the source
            bad_a += !(s == 16 * G + 2 * k + (c >> 3) && sb == (c & 7));
            bad_b += !(s == 16 * G + k + 8 * (c >> 3) && sb == (c & 7));
        }
        printf("\n");
    }
    printf("raw map: candidate A misses %d of 512, candidate B misses %d of 512, third image disagrees on %d\n", bad_a, bad_b, bad_id);
    const int map_b = bad_b == 0;
    int fail = bad_id != 0 || (bad_a == 0) == (bad_b == 0);

    static uint8_t vimg[kRows * kPitch], pw[128];
    static float o_host[kCh / 16 * 64 * 4];
    for (int p = 0; p < kRows; ++p)
        for (int ch = 0; ch < kCh; ++ch) vimg[p * kPitch + ch] = enc_small(v_val(p, ch));
    for (int h = 0; h < 2; ++h)
        for (int g = 0; g < 4; ++g)
            for (int u = 0; u < 2; ++u)
                for (int e = 0; e < 8; ++e) pw[64 * h + 16 * g + 8 * u + e] = enc_small(w_val(pi_pos(h, g, u, e)));
    uint8_t *d_v, *d_p;
    float *d_o;
    CHECK(hipMalloc(&d_v, sizeof(vimg)));
    CHECK(hipMalloc(&d_p, sizeof(pw)));
    CHECK(hipMalloc(&d_o, sizeof(o_host)));
    CHECK(hipMemcpy(d_v, vimg, sizeof(vimg), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_p, pw, sizeof(pw), hipMemcpyHostToDevice));
    for (int other = 0; other < 2; ++other) {
        hipLaunchKernelGGL(operand_probe, dim3(1), dim3(64), 0, 0, d_v, d_p, d_o, other ? !map_b : map_b);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(o_host, d_o, sizeof(o_host), hipMemcpyDeviceToHost));
        int bad = 0;
        for (int dt = 0; dt < kCh / 16; ++dt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    long want = 0;
                    for (int p = 0; p < kRows; ++p) want += (long)v_val(p, 16 * dt + 4 * (lane >> 4) + j) * w_val(p);
                    bad += o_host[(dt * 64 + lane) * 4 + j] != (float)want;
                }
        printf("operand, source lanes addressed by candidate %c%s: %d of %d sums differ from sum_pos V[pos][ch] w[pos]\n", (other ? !map_b : map_b) ? 'B' : 'A',
               other ? " (control)" : "", bad, kCh / 16 * 256);
        fail |= other ? bad == 0 : bad != 0;
    }
    printf("probe: %s\n", fail ? "A CLAIM FAILS" : "ALL CLAIMS HOLD");
    return fail;
}
