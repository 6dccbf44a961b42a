// Rotary embedding (+ optional per-head RMSNorm) fused into the FP8 cache appends for gfx950 (fp8mi_rope_kv_cache_append,
// fp8mi_mla_rope_cache_append; include/fp8mi.h has the contract, DESIGN.md 5.27 the design).  One launch, no workspace, nothing read on the
// host, capturable.
//
// Work split.  A work item is a (token, head) row of D channels: the Hq query rows, the Hkv key rows and the Hkv value rows of a token (MLA:
// the Hq q_pe rows, the k_pe row and the 512-channel latent row).  A row is owned by D / 16 adjacent lanes, 16 elements each, held as four
// quads of 4 channels, x[4 q + r] = channel qs[q] + r.  The quads are chosen so that both partners of a rotation sit in ONE lane (lane_quads):
//   NEOX  partners (i, i + rot_dim / 2): the lane owns quads p, p + 1 of the first half and their partners - x[j] and x[j + 8] are partners;
//   GPTJ  partners (2i, 2i + 1): the lane owns 16 consecutive channels - x[2j] and x[2j + 1] are partners;
// in both, pair j of lane l uses cos[8 l + j] and sin[8 l + j], and is a rotary pair iff 8 l + j < rot_dim / 2.  The rotation needs no
// cross-lane traffic.  A lane's cosines and sines depend on its place in the row only, not on the head: a wave loads them once and keeps
// them in registers for every row it takes of that token.  The norm's sum of squares is a DPP reduction inside the row's lanes.
//
// Data movement.  When every base and stride is a multiple of 16 bytes and rot_dim of 16 (VEC), a lane's quads pair up into two 8-element
// chunks: inputs and the table are read with 16-byte loads, q_out is written with 16-byte stores, K bytes with 8-byte stores, V bytes of
// the contiguous copy and latent bytes with one 16-byte store.  Otherwise (scalar form) every element is loaded and stored on its own, a
// quad of bytes as one dword.
//
// Kernels.  Up to kRopeFlatMaxT tokens (decode): a wave is (token, 64 / (D / 16) rows), workgroups of four waves - as few, full waves as
// the rows allow; V bytes go to the V cache one at a time, block_size apart, as fp8mi_kv_cache_append stores them.  Beyond that (prefill):
// a workgroup of 16 waves owns 16 consecutive tokens.  grid.y 1 takes their query rows, grid.y 0 their key rows, one wave a token, and then
// their value rows: the 16 tokens' slots are compared on the device (a ballot) and when they are consecutive, start at a multiple of 16
// and all valid - so inside one block - the V bytes are transposed through LDS and each channel's 16 positions leave as ONE 16-byte store;
// any other pattern takes the byte stores.  Both give the same bytes.
//
// Numerics: inputs and table values widened to fp32 (exact); y_a = fl(fl(x_a c) - fl(x_b s)), y_b = fl(fl(x_b c) + fl(x_a s)) with separately
// rounded operations (no fused multiply-add); the cache bytes are encode4 of fl(y * fl(1 / scale)) - fp8mi_kv_cache_append's on y.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

#pragma clang fp contract(off)   // the rotation is individually rounded fp32 operations (written with plain operators: hipcc's __fmul_rn / __fadd_rn carry their header's contraction and fuse)

namespace {

constexpr int kFlatThreads = 256;
constexpr int kTileThreads = 64 * kRopeTileWaves;
constexpr int kTileVDwords = 4096;   // the V bytes of 16 tokens x 64 / (D / 16) heads x D channels: 16 KiB at either head dimension

FP8MI_DEVICE int64_t load_index(const void *p, int64_t i, int wide)
{
    return wide ? ((const int64_t *)p)[i] : (int64_t)((const int32_t *)p)[i];
}

// Channel starts of lane l's four quads.  A lane wholly inside the rotary channels takes quads 2l, 2l + 1 of the first half and their
// partners; a lane past them takes 16 consecutive channels; with an odd number of quads in a half (rot_dim % 16 == 8) one lane takes the
// last pair and the first two pass-through quads.  GPTJ, and rows that are not rotated (rot_dim 0): 16 consecutive channels.
template <int STYLE>
FP8MI_DEVICE void lane_quads(int l, int rot_dim, int (&qs)[4])
{
    const int hq = rot_dim >> 3;   // quads in half the rotary channels
    qs[0] = 16 * l; qs[1] = 16 * l + 4; qs[2] = 16 * l + 8; qs[3] = 16 * l + 12;
    if (STYLE == FP8MI_ROPE_NEOX && 2 * l < hq) {
        qs[0] = 8 * l;
        qs[2] = 8 * l + 4 * hq;
        if (2 * l + 1 < hq) {
            qs[1] = 8 * l + 4;
            qs[3] = 8 * l + 4 + 4 * hq;
        } else {
            qs[1] = 16 * l + 8;   // the first two quads past the rotary channels: 8 hq = 16 l + 8 here
        }
    }
}

// eight elements at element index e of a tensor of dtype IN (a 16-byte aligned address) -> f[O .. O + 8)
template <int IN, int O, int N>
FP8MI_DEVICE void load8(const void *p, int64_t e, float (&f)[N])
{
    if (IN == FP8MI_F32) {
        const f32x4 lo = __builtin_nontemporal_load((const f32x4 *)((const float *)p + e)), hi = __builtin_nontemporal_load((const f32x4 *)((const float *)p + e + 4));
        f[O] = lo[0]; f[O + 1] = lo[1]; f[O + 2] = lo[2]; f[O + 3] = lo[3];
        f[O + 4] = hi[0]; f[O + 5] = hi[1]; f[O + 6] = hi[2]; f[O + 7] = hi[3];
    } else {
        float t[8];
        InVec<IN>::loadv(p, e >> 3, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[O + j] = t[j];
    }
}

// eight table entries of dtype dt at element index e (a 16-byte aligned address).  Plain loads: a token's row is read again by every wave of
// that token, so it should stay in the caches - the inputs above are read once and stream past them
FP8MI_DEVICE void load8_table(const void *p, int64_t e, int dt, float (&f)[8])
{
    if (dt == FP8MI_F32) {
        const f32x4 lo = *(const f32x4 *)((const float *)p + e), hi = *(const f32x4 *)((const float *)p + e + 4);
        f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
        f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
        return;
    }
    const u32x4 v = *(const u32x4 *)((const uint16_t *)p + e);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t w = v[q];   // (through a scalar: see InVec<FP8MI_F16>::load)
        if (dt == FP8MI_F16) {
            f[2 * q] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
            f[2 * q + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
        } else {
            f[2 * q] = __uint_as_float(w << 16);
            f[2 * q + 1] = __uint_as_float(w & 0xFFFF0000u);
        }
    }
}

// f[O .. O + 8) rounded to nearest even into dtype OUT at element index e (a 16-byte aligned address)
template <int OUT, int O>
FP8MI_DEVICE void store8(void *p, int64_t e, const float (&f)[16])
{
    if (OUT == FP8MI_F32) {
        const f32x4 lo = {f[O], f[O + 1], f[O + 2], f[O + 3]}, hi = {f[O + 4], f[O + 5], f[O + 6], f[O + 7]};
        *(f32x4 *)((float *)p + e) = lo;
        *(f32x4 *)((float *)p + e + 4) = hi;
    } else {
        const u32x4 w = {pack16<OUT>(f[O], f[O + 1]), pack16<OUT>(f[O + 2], f[O + 3]), pack16<OUT>(f[O + 4], f[O + 5]), pack16<OUT>(f[O + 6], f[O + 7])};
        *(u32x4 *)((uint16_t *)p + e) = w;
    }
}

// the lane's 16 elements of the row that starts at element `base`.  VEC: the quads pair up (qs[1] == qs[0] + 4, qs[3] == qs[2] + 4)
template <int IN, bool VEC>
FP8MI_DEVICE void load_row16(const void *p, int64_t base, const int (&qs)[4], float (&x)[16])
{
    if (VEC) {
        load8<IN, 0>(p, base + qs[0], x);
        load8<IN, 8>(p, base + qs[2], x);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) x[4 * q + r] = InVec<IN>::load1(p, base + qs[q] + r);
    }
}

template <int OUT, bool VEC>
FP8MI_DEVICE void store_row16(void *p, int64_t base, const int (&qs)[4], const float (&x)[16])
{
    if (VEC) {
        store8<OUT, 0>(p, base + qs[0], x);
        store8<OUT, 8>(p, base + qs[2], x);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) store_from_float(p, base + qs[q] + r, x[4 * q + r], OUT);
    }
}

// the lane's eight cosines and sines of table row `row` (element index of its first cosine): pair j uses entry 8 l + j, below `half` only
template <bool VEC>
FP8MI_DEVICE void load_cos_sin(const void *cs, int dt, int64_t row, int l, int half, float (&c)[8], float (&s)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = 1.0f; s[j] = 0.0f; }
    if (VEC) {   // half is a multiple of 8: all eight pairs of a lane are rotary pairs or none is
        if (8 * l < half) {
            load8_table(cs, row + 8 * l, dt, c);
            load8_table(cs, row + half + 8 * l, dt, s);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (8 * l + j < half) {
                c[j] = load_as_float(cs, row + 8 * l + j, dt);
                s[j] = load_as_float(cs, row + half + 8 * l + j, dt);
            }
    }
}

// y_a = fl(fl(x_a c) - fl(x_b s)), y_b = fl(fl(x_b c) + fl(x_a s)); a pair at or beyond `half` passes through untouched
FP8MI_DEVICE void rotate_pair(float &xa, float &xb, float c, float s, bool on)
{
    const float ya = xa * c - xb * s, yb = xb * c + xa * s;   // (not contracted: the pragma above)
    xa = on ? ya : xa;
    xb = on ? yb : xb;
}

template <int STYLE>
FP8MI_DEVICE void rotate16(float (&x)[16], const float (&c)[8], const float (&s)[8], int l, int half)
{
    if (STYLE == FP8MI_ROPE_NEOX) {
#pragma unroll
        for (int j = 0; j < 8; ++j) rotate_pair(x[j], x[j + 8], c[j], s[j], 8 * l + j < half);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) rotate_pair(x[2 * j], x[2 * j + 1], c[j], s[j], 8 * l + j < half);
    }
}

// n_d = fl(fl(x_d rstd) w_d) given the row's sum of squares; w is fp32 [D], 16-byte aligned
FP8MI_DEVICE void rms_apply(float (&x)[16], float sum_sq, float inv_d, float eps, const float *w, const int (&qs)[4])
{
    const float rstd = rsqrtf(sum_sq * inv_d + eps);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 wv = *(const f32x4 *)(w + qs[q]);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[4 * q + r] = (x[4 * q + r] * rstd) * wv[r];
    }
}

FP8MI_DEVICE float sum_sq16(const float (&x)[16])
{
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) ss += x[j] * x[j];
    return ss;
}

// sum over the lpr = 4 or 8 adjacent lanes of a row
FP8MI_DEVICE float row_sum(float v, int lpr)
{
    v = group_sum<4>(v);
    if (lpr == 8) v = dpp_add<0x141>(v);   // row_half_mirror
    return v;
}

// the bytes of x[4 q ..] * prescale, one dword a quad: fp8mi_encode's multiply and encoder
template <int MODE>
FP8MI_DEVICE void encode16(const float (&x)[16], float prescale, uint32_t (&w)[4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
        w[q] = encode4<MODE>(x[4 * q] * prescale, x[4 * q + 1] * prescale, x[4 * q + 2] * prescale, x[4 * q + 3] * prescale);
}

// a row's bytes of this lane to the row that starts at `row` (16-byte aligned): quad q at byte qs[q]
template <bool VEC>
FP8MI_DEVICE void store_bytes16(uint8_t *row, const int (&qs)[4], const uint32_t (&w)[4])
{
    if (VEC) {
        const u32x2 a = {w[0], w[1]}, b = {w[2], w[3]};
        *(u32x2 *)(row + qs[0]) = a;
        *(u32x2 *)(row + qs[2]) = b;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) *(uint32_t *)(row + qs[q]) = w[q];
    }
}

// ---- (T, H, D) queries, keys and values ---------------------------------------------------------------------------------------------------

// One query (r < Hq) or key row of token t: norm, rotation, then q_out or the K bytes (the contiguous copy, and the cache at a valid slot)
template <int IN, int MODE, int STYLE, bool VEC>
FP8MI_DEVICE void qk_row(const RopeArgs &a, int64_t t, int r, int l, int lpr, const int (&qs)[4], const float (&c)[8], const float (&s)[8], int64_t slot,
                         bool slot_ok)
{
    const bool is_q = r < a.Hq;
    const int h = is_q ? r : r - a.Hq;
    float x[16];
    load_row16<IN, VEC>(is_q ? a.q : a.k, t * (is_q ? a.ld_q : a.ld_k) + (int64_t)h * a.D, qs, x);
    const float *w = is_q ? a.qw : a.kw;
    if (w) rms_apply(x, row_sum(sum_sq16(x), lpr), 1.0f / (float)a.D, a.eps, w, qs);   // (every lane of the row is here together)
    rotate16<STYLE>(x, c, s, l, a.rot_dim >> 1);
    if (is_q) {
        store_row16<IN, VEC>(a.q_out, t * a.ld_qo + (int64_t)h * a.D, qs, x);
        return;
    }
    uint32_t wq[4];
    encode16<MODE>(x, __fdiv_rn(1.0f, a.k_scale[a.scale_head ? h : 0]), wq);
    if (a.k8) store_bytes16<VEC>(a.k8 + (t * a.Hkv + h) * a.D, qs, wq);
    if (slot_ok) {
        const int64_t blk = slot >> a.bs_log2;
        const int off = (int)(slot & ((1 << a.bs_log2) - 1));
        store_bytes16<VEC>(a.kc + (((blk * a.Hkv + h) << a.bs_log2) + off) * a.D, qs, wq);
    }
}

// the lane's 16 consecutive channels of value row (t, h) as bytes, and the contiguous copy's 16-byte store
template <int IN, int MODE, bool VEC>
FP8MI_DEVICE u32x4 v_bytes(const RopeArgs &a, int64_t t, int h, int l)
{
    const int qs[4] = {16 * l, 16 * l + 4, 16 * l + 8, 16 * l + 12};
    float x[16];
    load_row16<IN, VEC>(a.v, t * a.ld_v + (int64_t)h * a.D, qs, x);
    uint32_t wq[4];
    encode16<MODE>(x, __fdiv_rn(1.0f, a.v_scale[a.scale_head ? h : 0]), wq);
    const u32x4 w = {wq[0], wq[1], wq[2], wq[3]};
    if (a.v8) *(u32x4 *)(a.v8 + (t * a.Hkv + h) * a.D + 16 * l) = w;
    return w;
}

// those 16 bytes to the V cache, one at a time, block_size apart
FP8MI_DEVICE void v_store_bytes(const RopeArgs &a, int64_t slot, int h, int l, const u32x4 &w)
{
    const int64_t blk = slot >> a.bs_log2;
    const int off = (int)(slot & ((1 << a.bs_log2) - 1));
    uint8_t *p = a.vc + (((blk * a.Hkv + h) * a.D + 16 * l) << a.bs_log2) + off;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t d = w[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[(int64_t)(4 * q + r) << a.bs_log2] = (uint8_t)(d >> (8 * r));
    }
}

// decode sizes: a wave is (token, 64 / lpr consecutive rows of its Hq + 2 Hkv)
template <int IN, int MODE, int STYLE, bool VEC>
__global__ __launch_bounds__(kFlatThreads) void rope_append_flat_kernel(const RopeArgs a)
{
    const int lpr = a.D >> 4, rpw = 64 / lpr, H = a.Hq + 2 * a.Hkv, groups = (H + rpw - 1) / rpw;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kFlatThreads / 64) + (threadIdx.x >> 6);
    if (wave >= a.T * groups) return;
    const int64_t t = wave / groups;
    const int g = (int)(wave - t * groups);
    const int64_t pos = load_index(a.pos, t, a.pos64);
    if (pos < 0 || pos >= a.max_pos) return;   // padding: nothing of the token is written
    const int64_t slot = a.kc ? load_index(a.slot_mapping, t, a.slot64) : -1;
    const bool slot_ok = slot >= 0 && slot < a.slots;
    const int l = lane % lpr, r = g * rpw + lane / lpr;
    if (r >= H) return;
    if (r < a.Hq + a.Hkv) {
        int qs[4];
        float c[8], s[8];
        lane_quads<STYLE>(l, a.rot_dim, qs);
        load_cos_sin<VEC>(a.cs, a.cs_dtype, pos * a.ld_cs, l, a.rot_dim >> 1, c, s);
        qk_row<IN, MODE, STYLE, VEC>(a, t, r, l, lpr, qs, c, s, slot, slot_ok);
    } else {
        const int h = r - a.Hq - a.Hkv;
        const u32x4 w = v_bytes<IN, MODE, VEC>(a, t, h, l);
        if (slot_ok) v_store_bytes(a, slot, h, l, w);
    }
}

// prefill sizes: a workgroup is 16 consecutive tokens; grid.y 1 their query rows, grid.y 0 their key rows and then their value rows
template <int IN, int MODE, int STYLE, bool VEC>
__global__ __launch_bounds__(kTileThreads) void rope_append_tile_kernel(const RopeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t vt[kTileVDwords];   // [head of the slab][quad of channels][token]: a dword is 4 channels of one token
    const int lpr = a.D >> 4, rpw = 64 / lpr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * kRopeTileTokens;
    {   // query or key rows: wave w takes token t0 + w, its cosines and sines in registers across the rows
        const int64_t t = t0 + wave;
        const int64_t pos = t < a.T ? load_index(a.pos, t, a.pos64) : -1;
        if (pos >= 0 && pos < a.max_pos) {
            const int64_t slot = a.kc ? load_index(a.slot_mapping, t, a.slot64) : -1;
            const bool slot_ok = slot >= 0 && slot < a.slots;
            const int l = lane % lpr;
            int qs[4];
            float c[8], s[8];
            lane_quads<STYLE>(l, a.rot_dim, qs);
            load_cos_sin<VEC>(a.cs, a.cs_dtype, pos * a.ld_cs, l, a.rot_dim >> 1, c, s);
            const int begin = blockIdx.y ? 0 : a.Hq, end = blockIdx.y ? a.Hq : a.Hq + a.Hkv;
            for (int r = begin + lane / lpr; r < end; r += rpw) qk_row<IN, MODE, STYLE, VEC>(a, t, r, l, lpr, qs, c, s, slot, slot_ok);
        }
    }
    if (blockIdx.y) return;
    // value rows: thread = (token i, lane l of the row, head of the slab); the slots of the 16 tokens decide the store
    const int i = tid & 15, l = (tid >> 4) % lpr, hl = tid / (16 * lpr);
    const int64_t ti = t0 + i;
    const int64_t pos = ti < a.T ? load_index(a.pos, ti, a.pos64) : -1;
    const bool pos_ok = pos >= 0 && pos < a.max_pos;
    const int64_t slot = a.kc && ti < a.T ? load_index(a.slot_mapping, ti, a.slot64) : -1;
    const int64_t slot0 = a.kc ? load_index(a.slot_mapping, t0, a.slot64) : -1;   // (t0 < T for every workgroup of the grid)
    const bool slot_ok = slot >= 0 && slot < a.slots;
    // one aligned run: every token valid, slot0 a multiple of 16, slot i = slot0 + i, the last one inside the cache - hence inside one block
    const bool in_run = pos_ok && slot0 >= 0 && (slot0 & 15) == 0 && slot == slot0 + i && slot0 + 15 < a.slots;
    const bool run = __ballot(in_run) == ~0ull;   // (each wave holds the 16 tokens four times: the same verdict in every wave)
    const int dq = a.D >> 2;
    for (int hs = 0; hs < a.Hkv; hs += rpw) {
        const int h = hs + hl;
        if (pos_ok && h < a.Hkv) {
            const u32x4 w = v_bytes<IN, MODE, VEC>(a, ti, h, l);
            if (run) {
#pragma unroll
                for (int q = 0; q < 4; ++q) vt[((hl * dq + 4 * l + q) << 4) + i] = w[q];
            } else if (slot_ok) {
                v_store_bytes(a, slot, h, l, w);
            }
        }
        if (run) {   // (uniform over the workgroup)
            __syncthreads();
            const int th = tid / dq, cq = tid - th * dq;   // 64 / lpr heads x D / 4 quads = 256 threads: four channels' 16 positions each
            if (tid < rpw * dq && hs + th < a.Hkv) {
                uint32_t d[16];
                const u32x4 *src = (const u32x4 *)&vt[(th * dq + cq) << 4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const u32x4 v = src[m];
                    d[4 * m] = v[0]; d[4 * m + 1] = v[1]; d[4 * m + 2] = v[2]; d[4 * m + 3] = v[3];
                }
                const int64_t blk = slot0 >> a.bs_log2;
                const int off0 = (int)(slot0 & ((1 << a.bs_log2) - 1));
                uint8_t *dst = a.vc + (((blk * a.Hkv + hs + th) * a.D + 4 * cq) << a.bs_log2) + off0;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    u32x4 o;
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        o[m] = ((d[4 * m] >> (8 * ch)) & 0xFFu) | (((d[4 * m + 1] >> (8 * ch)) & 0xFFu) << 8) | (((d[4 * m + 2] >> (8 * ch)) & 0xFFu) << 16) |
                               (((d[4 * m + 3] >> (8 * ch)) & 0xFFu) << 24);
                    *(u32x4 *)(dst + ((int64_t)ch << a.bs_log2)) = o;
                }
            }
            __syncthreads();
        }
    }
}

// ---- the MLA latent row ---------------------------------------------------------------------------------------------------------------------

constexpr int kMlaLatentLanes = kMlaLatent / kRopeLaneElems;   // 32
constexpr int kMlaRopeLanes = kMlaRope / kRopeLaneElems;       // 4

// A token's lanes: 32 of the latent row, then 4 of the k_pe row, then 4 of each q_pe row; a wave is 64 consecutive ones
template <int IN, int MODE, int STYLE, bool VEC>
__global__ __launch_bounds__(kFlatThreads) void mla_rope_append_kernel(const MlaRopeArgs a)
{
    const int units = kMlaLatentLanes + kMlaRopeLanes * (1 + a.Hq), groups = (units + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kFlatThreads / 64) + (threadIdx.x >> 6);
    if (wave >= a.T * groups) return;
    const int64_t t = wave / groups;
    const int u = (int)(wave - t * groups) * 64 + lane;
    const int64_t pos = load_index(a.pos, t, a.pos64);
    if (pos < 0 || pos >= a.max_pos) return;   // padding
    const int64_t slot = load_index(a.slot_mapping, t, a.slot64);
    const bool slot_ok = slot >= 0 && slot < a.slots;
    if (u >= units) return;
    if (u < kMlaLatentLanes) {   // (lanes 0 .. 31 of the token's first wave, all of them here)
        const int qs[4] = {16 * u, 16 * u + 4, 16 * u + 8, 16 * u + 12};
        float x[16];
        load_row16<IN, VEC>(a.kv_c, t * a.ld_c, qs, x);
        if (a.kvw) {
            float ss = group_sum<16>(sum_sq16(x));
            ss += __shfl_xor(ss, 16, 64);
            rms_apply(x, ss, 1.0f / (float)kMlaLatent, a.eps, a.kvw, qs);
        }
        if (slot_ok) {
            uint32_t wq[4];
            encode16<MODE>(x, __fdiv_rn(1.0f, a.kv_scale[0]), wq);
            const u32x4 w = {wq[0], wq[1], wq[2], wq[3]};
            *(u32x4 *)(a.cache + slot * kMlaRow + 16 * u) = w;
        }
        return;
    }
    const int r = (u - kMlaLatentLanes) / kMlaRopeLanes, l = (u - kMlaLatentLanes) % kMlaRopeLanes;   // row 0: k_pe, row 1 + h: q_pe head h
    int qs[4];
    float c[8], s[8], x[16];
    lane_quads<STYLE>(l, kMlaRope, qs);
    load_cos_sin<VEC>(a.cs, a.cs_dtype, pos * a.ld_cs, l, kMlaRope / 2, c, s);
    if (r == 0) {
        if (!slot_ok) return;
        load_row16<IN, VEC>(a.k_pe, t * a.ld_p, qs, x);
        rotate16<STYLE>(x, c, s, l, kMlaRope / 2);
        uint32_t wq[4];
        encode16<MODE>(x, __fdiv_rn(1.0f, a.kv_scale[0]), wq);
        store_bytes16<VEC>(a.cache + slot * kMlaRow + kMlaLatent, qs, wq);
    } else {
        load_row16<IN, VEC>(a.q_pe, t * a.ld_qp + (int64_t)(r - 1) * kMlaRope, qs, x);
        rotate16<STYLE>(x, c, s, l, kMlaRope / 2);
        store_row16<IN, VEC>(a.q_pe_out, t * a.ld_qpo + (int64_t)(r - 1) * kMlaRope, qs, x);
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
bool stride16(int64_t ld, int esz) { return (ld * esz) % 16 == 0; }

}  // namespace

// host launchers (called from fp8mi_api.hip, which has validated the arguments).  The 16-byte form needs every base and row stride it reads
// or writes by vectors to be a multiple of 16 bytes, and rot_dim of 16.
int fp8mi_launch_rope_kv_cache_append(const RopeArgs &a, int dtype, int mode, hipStream_t s)
{
    const int esz = dtype == FP8MI_F32 ? 4 : 2, csz = a.cs_dtype == FP8MI_F32 ? 4 : 2;
    const bool vec = a.rot_dim % 16 == 0 && aligned16(a.q) && aligned16(a.q_out) && aligned16(a.k) && aligned16(a.v) && aligned16(a.cs) &&
                     stride16(a.ld_q, esz) && stride16(a.ld_qo, esz) && stride16(a.ld_k, esz) && stride16(a.ld_v, esz) && stride16(a.ld_cs, csz);
    const int rpw = 64 / (a.D / kRopeLaneElems), H = a.Hq + 2 * a.Hkv;
    const bool tile = a.T > kRopeFlatMaxT;
    const int64_t flat_waves = a.T * ((H + rpw - 1) / rpw), tiles = (a.T + kRopeTileTokens - 1) / kRopeTileTokens;
    if (tiles > 0x7FFFFFFF) return FP8MI_E_UNSUPPORTED;
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            return dispatch_int<FP8MI_ROPE_NEOX, FP8MI_ROPE_GPTJ>(a.style, [&](auto style_t) {
                constexpr int IN = decltype(in_t)::value, MODE = decltype(mode_t)::value, STYLE = decltype(style_t)::value;
                if (tile) {
                    const dim3 grid((unsigned)tiles, a.Hq > 0 ? 2 : 1);
                    if (vec) return fp8mi_launch(rope_append_tile_kernel<IN, MODE, STYLE, true>, grid, dim3(kTileThreads), s, a);
                    return fp8mi_launch(rope_append_tile_kernel<IN, MODE, STYLE, false>, grid, dim3(kTileThreads), s, a);
                }
                if (vec) return fp8mi_launch_items(rope_append_flat_kernel<IN, MODE, STYLE, true>, flat_waves, kFlatThreads / 64, kFlatThreads, s, a);
                return fp8mi_launch_items(rope_append_flat_kernel<IN, MODE, STYLE, false>, flat_waves, kFlatThreads / 64, kFlatThreads, s, a);
            });
        });
    });
}

int fp8mi_launch_mla_rope_cache_append(const MlaRopeArgs &a, int dtype, int mode, hipStream_t s)
{
    const int esz = dtype == FP8MI_F32 ? 4 : 2, csz = a.cs_dtype == FP8MI_F32 ? 4 : 2;
    const bool vec = aligned16(a.kv_c) && aligned16(a.k_pe) && aligned16(a.q_pe) && aligned16(a.q_pe_out) && aligned16(a.cs) && stride16(a.ld_c, esz) &&
                     stride16(a.ld_p, esz) && stride16(a.ld_qp, esz) && stride16(a.ld_qpo, esz) && stride16(a.ld_cs, csz);
    const int64_t waves = a.T * ((kMlaLatentLanes + kMlaRopeLanes * (1 + a.Hq) + 63) / 64);
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            return dispatch_int<FP8MI_ROPE_NEOX, FP8MI_ROPE_GPTJ>(a.style, [&](auto style_t) {
                constexpr int IN = decltype(in_t)::value, MODE = decltype(mode_t)::value, STYLE = decltype(style_t)::value;
                if (vec) return fp8mi_launch_items(mla_rope_append_kernel<IN, MODE, STYLE, true>, waves, kFlatThreads / 64, kFlatThreads, s, a);
                return fp8mi_launch_items(mla_rope_append_kernel<IN, MODE, STYLE, false>, waves, kFlatThreads / 64, kFlatThreads, s, a);
            });
        });
    });
}
