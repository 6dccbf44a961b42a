// The FP8 paged KV cache's append for gfx950 (fp8mi_kv_cache_append; include/fp8mi.h has the layout): T new tokens' K and V rows
// (T, Hkv, D) f32 / f16 / bf16, each with its own row stride (slices of a fused qkv), encoded to e4m3 with static dequantisation scales and
// written to slot slot_mapping[t] of both caches, in one launch.  No workspace, nothing read on the host, capturable.
//   K cache [num_blocks, Hkv, block_size, D]: a token's D bytes are contiguous - one thread stores 4 of them as a dword;
//   V cache [num_blocks, Hkv, D, block_size]: a channel's positions are contiguous - the same thread stores its 4 channels as 4 bytes,
//   block_size apart.
// One thread per (token, head, 4 channels).  The bytes are fp8mi_encode's of the same values with prescale = 1.0f / scale: the same
// float32 product, the same encoder (encode4 of fp8mi_encode.h).  A slot below 0 or at or beyond num_blocks * block_size stores nothing.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

namespace {

constexpr int kAppendThreads = 256;

struct AppendArgs {
    const void *k, *v;
    int64_t T, ld_k, ld_v;
    int Hkv, D, bs_log2;
    int64_t slots;   // num_blocks * block_size
    uint8_t *kc, *vc;
    const void *slot_mapping;
    const float *k_scale, *v_scale;
    int scale_head;
};

template <int IN, int MODE, bool SLOT64>
__global__ __launch_bounds__(kAppendThreads) void kv_append_kernel(const AppendArgs a)
{
    const int d4n = a.D >> 2;
    const int64_t idx = (int64_t)blockIdx.x * kAppendThreads + threadIdx.x;
    const int64_t per_token = (int64_t)a.Hkv * d4n;
    if (idx >= a.T * per_token) return;
    const int64_t t = idx / per_token;
    const int rem = (int)(idx - t * per_token), h = rem / d4n, d = (rem - h * d4n) * 4;
    const int64_t slot = SLOT64 ? ((const int64_t *)a.slot_mapping)[t] : (int64_t)((const int32_t *)a.slot_mapping)[t];
    if (slot < 0 || slot >= a.slots) return;   // padding
    const int bs = 1 << a.bs_log2;
    const int64_t blk = slot >> a.bs_log2;
    const int off = (int)(slot & (bs - 1));
    const float pk = __fdiv_rn(1.0f, a.k_scale[a.scale_head ? h : 0]), pv = __fdiv_rn(1.0f, a.v_scale[a.scale_head ? h : 0]);
    const int64_t ik = t * a.ld_k + (int64_t)h * a.D + d, iv = t * a.ld_v + (int64_t)h * a.D + d;
    float fk[4], fv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        fk[j] = InVec<IN>::load1(a.k, ik + j) * pk;   // the float32 multiply of fp8mi_encode
        fv[j] = InVec<IN>::load1(a.v, iv + j) * pv;
    }
    const uint32_t wk = encode4<MODE>(fk[0], fk[1], fk[2], fk[3]), wv = encode4<MODE>(fv[0], fv[1], fv[2], fv[3]);
    const int64_t head = blk * a.Hkv + h;
    *(uint32_t *)(a.kc + ((head << a.bs_log2) + off) * a.D + d) = wk;
    uint8_t *pvc = a.vc + ((head * a.D + d) << a.bs_log2) + off;
#pragma unroll
    for (int j = 0; j < 4; ++j) pvc[(int64_t)j << a.bs_log2] = (uint8_t)(wv >> (8 * j));
}

}  // namespace

// host launcher (called from fp8mi_api.hip, which has validated the arguments)
int fp8mi_launch_kv_cache_append(const void *k, const void *v, int dtype, int64_t T, int Hkv, int D, int64_t ld_k, int64_t ld_v, uint8_t *k_cache,
                                 uint8_t *v_cache, int64_t num_blocks, int block_size, const void *slot_mapping, int slot_bytes, const float *k_scale,
                                 const float *v_scale, int scale_head, int mode, hipStream_t s)
{
    const AppendArgs a{k, v, T, ld_k, ld_v, Hkv, D, fp8mi_attn_log2(block_size), num_blocks * block_size, k_cache, v_cache, slot_mapping,
                       k_scale, v_scale, scale_head};
    const int64_t n = T * Hkv * (D / 4);
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            constexpr int IN = decltype(in_t)::value, MODE = decltype(mode_t)::value;
            if (slot_bytes == 8) return fp8mi_launch_items(kv_append_kernel<IN, MODE, true>, n, kAppendThreads, kAppendThreads, s, a);
            return fp8mi_launch_items(kv_append_kernel<IN, MODE, false>, n, kAppendThreads, kAppendThreads, s, a);
        });
    });
}
