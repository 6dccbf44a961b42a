// FP8 flash attention over contiguous, token-major K and V for gfx950 (fp8mi_attention_prefill; include/fp8mi.h has the contract, DESIGN.md
// 5.26 the design) and the producer of its operands (fp8mi_attn_kv_quantize).  Prompts: variable lengths by cu_seqlens_q / cu_seqlens_k,
// causal (aligned at the end of the keys) or not, head dimensions 128 / 128 and 192 / 128 - the un-absorbed MLA prefill, whose 64 rotary key
// channels come from a tensor of their own (one key for all heads when its head stride is 0) and are never concatenated in memory.  No block
// table, no cache, no split along K, no workspace: ONE launch.  Few query tokens against long contexts stay with the paged kernels
// (fp8mi_attn_decode.hip, fp8mi_attn_prefill.hip), which split the context.
//
// Work split.  One workgroup of kAttnFlashWaves = 4 waves per (query tile, sequence, KV head); the tile index is the SLOWEST grid dimension and
// runs backwards, so that under the causal mask a sequence's longest tiles are issued first.  A query tile is kAttnFlashCols = 128 MFMA columns:
// eight 16-column tiles of the (token, head-in-group) mapping of fp8mi_attn_prefill.hip - column r of a 16-column tile is token r / G, head r % G
// (G = Hq / Hkv), 16 / G tokens a tile - two per wave (kCT; the reason for two and not four is in DESIGN.md 5.26: registers).  One wave walks
// ALL 128-position steps of its columns in order from position 0: no cross-wave (m, l, O) merge.  The loop ends at the largest limit of the
// workgroup's columns; a wave whose columns all end below a step stages it, meets the barrier and multiplies nothing.
//
// Staging.  K, the rotary K and V are plain strided rows: address = base + (cu_seqlens_k[b] + position) token stride + head stride x head, with
// nothing loaded in front of a load.  Per step the 256 threads fetch 128 x (128 [+ 64] + 128) bytes with 16-byte loads, 8 (10) a thread, into
// registers; the loads of step n + 1 are issued BEFORE the products of step n and written to the other of two LDS stages behind them, one
// barrier per step.  A stage is 32 KiB (40 KiB with the rotary rows); two stages leave room for a second workgroup on the compute unit.  Rows at
// or beyond the workgroup's last limit are zeros in LDS and are never read from memory.
//   LDS layout, swizzled, no padding; every row kind is token-major:
//     K   row p of 128 bytes; 16-byte chunk c lives at chunk c ^ ((p >> 1) & 7).  S tile t reads the 16 CONSECUTIVE rows 16 t + (r ^ 8 (t & 1)),
//         chunks g and 4 + g (one ds_read_b128 each): 16 consecutive rows cover, with bit 0 of p selecting the 128-byte half of a 256-byte bank
//         span, all 16 16-byte units of the span once.
//     Kr  row p of 64 rotary bytes; chunk c lives at chunk c ^ ((p >> 2) & 3): bits 0, 1 of p select the 64-byte quarter of the span, the swizzle
//         the unit inside it.  The second K-step of a score is chunk g of this row and 64 zero bytes, which are register zeros, not LDS.
//     V   row p of 128 bytes, the K swizzle.  The P.V operand wants a channel's 128 positions in one lane: it is read from these rows with
//         ds_read_b64_tr_b8 under the position permutation of fp8mi_attn_mla.hip (slot 64 h + 16 g + 8 u + e is position (e & 3) + 4 (g & 1) +
//         8 ((g >> 1) ^ (e >> 2)) + 16 (e >> 2) + 32 u + 64 h), which makes the packed S registers of tile t dword t of the P operand with no
//         lane movement.  The 16 rows two neighbouring lane groups hand one transpose read are distinct mod 16: the cover above.
//   The staging stores write two rows (K, V) or four (Kr) per 16 lanes, all chunks of each: the same cover.
//
// Numerics are fp8mi_attn_decode.hip's: Q rounded to e4m3 per (token, head) row with ONE amax over its DQK channels (the tiny-Q path included),
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales, online softmax in base 2 in fp32, P = rne(p 2^8) against the running maximum, l from the
// fp32 p, the scales in the epilogue.
//
// Isolation.  No K / V byte of a sequence at or beyond its k_len (bounded by max_k_len) is read, and no row outside [0, Tk).  Rows of out no
// sequence owns, and tokens at or beyond max_q_len, are not written.  A row with no visible position is zero.  Under the causal mask a NaN byte
// of V at a position in [limit_j, last limit of j's 128-column tile) may poison row j (0 x NaN in the shared V operand); without the mask every
// limit is k_len and there is no such position.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

namespace {

constexpr int kScaleOne = 0x7F7F7F7F;
constexpr int kFlashThreads = 64 * kAttnFlashWaves;
constexpr int kCT = kAttnFlashCols / 16 / kAttnFlashWaves;   // column tiles of a wave: 2
constexpr int kDT = kAttnFlashDV / 16;                       // 16-channel tiles of O: 8
constexpr float kNegInf = -__builtin_huge_valf();
static_assert(kAttnStep == 128 && kAttnFlashDV == 128 && kAttnFlashRope == 64 && kCT == 2, "the layouts below");

struct FlashArgs {
    const void *q;
    int64_t ld_q;
    const uint8_t *k, *kr, *v;
    int64_t k_tok, k_head, r_tok, r_head, v_tok, v_head;   // strides in bytes
    int64_t rows_k;                                        // Tk: a K / V row outside [0, Tk) is not read
    const float *k_scale, *v_scale;
    int scale_head;
    float scale_log2;   // softmax_scale log2 e
    int Hq, Hkv, group;
    void *out;
    int64_t ld_out;
    const int32_t *cu_q, *cu_k;   // [B + 1] each
    int64_t B, rows;              // rows: T
    int64_t max_k_len;
    int max_q_len;
    int tq, qtiles;               // query tokens per 16-column tile; 128-column tiles per sequence
};

FP8MI_DEVICE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
FP8MI_DEVICE float xor_lanes(float v, int mask) { return __shfl_xor(v, mask, 64); }
// over the four lanes that hold one query (lane & 15 alike)
FP8MI_DEVICE float query_max(float v) { v = fmaxf(v, xor_lanes(v, 16)); return fmaxf(v, xor_lanes(v, 32)); }
FP8MI_DEVICE float query_sum(float v) { v = v + xor_lanes(v, 16); return v + xor_lanes(v, 32); }

typedef int i32x2 __attribute__((ext_vector_type(2)));
FP8MI_DEVICE i32x2 lds_read_tr8(const uint8_t *p) { return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)p); }

template <int IN, int OUT, int DQK, bool CAUSAL>
__global__ __launch_bounds__(kFlashThreads) void attn_flash_kernel(const FlashArgs a)
{
    constexpr bool ROPE = DQK == kAttnFlashDV + kAttnFlashRope;
    static_assert(ROPE || DQK == kAttnFlashDV, "128 / 128 or 192 / 128");
    constexpr int kStageK = kAttnStep * 128, kStageR = ROPE ? kAttnStep * kAttnFlashRope : 0, kStage = 2 * kStageK + kStageR;   // K, Kr, V
    constexpr int kOffR = kStageK, kOffV = kStageK + kStageR;
    constexpr int kLoads = kAttnStep * 8 / kFlashThreads, kLoadsR = ROPE ? kAttnStep * 4 / kFlashThreads : 0;   // 16-byte loads per thread and step: 4, 2
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    int64_t bh = blockIdx.x;
    const int h = (int)(bh % a.Hkv);
    bh /= a.Hkv;
    const int64_t b = bh % a.B;
    const int tile = a.qtiles - 1 - (int)(bh / a.B);   // longest first

    const int64_t c0 = a.cu_q[b], k0 = a.cu_k[b];
    const int64_t q_len = (int64_t)a.cu_q[b + 1] - c0;
    int64_t seq = (int64_t)a.cu_k[b + 1] - k0;
    seq = seq < 0 ? 0 : seq;
    seq = seq > a.max_k_len ? a.max_k_len : seq;                         // the host bound: nothing at or beyond it is read
    const int64_t q_take = q_len < a.max_q_len ? q_len : a.max_q_len;   // tokens at or beyond max_q_len are not written
    const int tokens = kAttnFlashCols / 16 * a.tq;                       // of a workgroup
    const int64_t j0 = (int64_t)tile * tokens;
    if (j0 >= q_take) return;   // nothing of this tile is owned: before any barrier, every thread alike

    // ---- the columns of this lane: token and head, the query row, the limit ----
    const int tok = r / a.group, col_head = r - tok * a.group;
    const int hq = h * a.group + col_head;
    int64_t row_q[kCT];
    bool live[kCT];
    int hi_col[kCT];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const int64_t j = j0 + (int64_t)(kCT * wave + ct) * a.tq + tok;
        row_q[ct] = c0 + j;
        live[ct] = tok < a.tq && j < q_take && row_q[ct] >= 0 && row_q[ct] < a.rows;
        int64_t limit = CAUSAL ? seq - q_len + j + 1 : seq;
        limit = !live[ct] || limit < 0 ? 0 : limit > seq ? seq : limit;
        hi_col[ct] = (int)limit;   // <= k_len, an int32
    }
    // the limit of the workgroup tile's last token: the loop and the staging run to it
    int64_t hi = seq;
    if (CAUSAL) {
        const int64_t j_last = (j0 + tokens < q_take ? j0 + tokens : q_take) - 1;
        hi = seq - q_len + j_last + 1;
        hi = hi < 0 ? 0 : hi > seq ? seq : hi;
    }
    // the last limit of this wave's columns: a step at or beyond it is skipped by the wave
    int wave_hi = hi_col[0] > hi_col[1] ? hi_col[0] : hi_col[1];
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const int other = __shfl_xor(wave_hi, mask, 64);
        wave_hi = wave_hi > other ? wave_hi : other;
    }
    wave_hi = __builtin_amdgcn_readfirstlane(wave_hi);

    // ---- Q: this lane's bytes of its columns' query rows, quantised per row over all DQK channels ----
    i32x8 qf[kCT];
    u32x4 qr[kCT];   // the rotary K-step: channels 128 + 16 g + [0, 16); its upper 64 bytes are zeros
    float c[kCT];    // an S accumulator times c: the logit, base 2
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        constexpr int kQ = ROPE ? 48 : 32;
        float qv[kQ];   // channels 16 g + [0, 16), 64 + 16 g + [0, 16), then rotary 128 + 16 g + [0, 16)
        float amax = 0.0f;
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int d = (i >> 4) * 64 + g * 16 + (i & 15);
            qv[i] = live[ct] ? InVec<IN>::load1(a.q, row_q[ct] * a.ld_q + (int64_t)hq * DQK + d) : 0.0f;
            amax = fmaxf(amax, fabsf(qv[i]));
        }
        amax = query_max(amax);
        // 448 / amax is +inf for 0 < amax < 448 / FLT_MAX: such a row and its amax are multiplied by 2^64 first - exact, subnormals
        // included - and 2^-64 goes into the logit scale.  No other row changes.
        const bool tiny = amax > 0.0f && amax < kAttnTinyQ;
        if (tiny) {
            amax *= kAttnTinyQUp;
#pragma unroll
            for (int i = 0; i < kQ; ++i) qv[i] *= kAttnTinyQUp;
        }
        const float q_scale = amax > 0.0f ? amax / 448.0f : 1.0f, q_inv = amax > 0.0f ? 448.0f / amax : 1.0f;
        qr[ct] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < kQ / 4; ++w) {
            const uint32_t word = encode4<FP8MI_ENC_RNE>(qv[4 * w] * q_inv, qv[4 * w + 1] * q_inv, qv[4 * w + 2] * q_inv, qv[4 * w + 3] * q_inv);
            if (w < 8) qf[ct][w] = (int)word;
            else qr[ct][w - 8] = word;
        }
        c[ct] = (q_scale * a.k_scale[a.scale_head ? h : 0]) * a.scale_log2;
        if (tiny) c[ct] *= 1.0f / kAttnTinyQUp;
    }

    // ---- staging: global -> registers (fetch), registers -> LDS (commit).  Load i of a thread is chunk idx % 8 (Kr: % 4) of row idx / 8 (/ 4),
    // idx = 256 i + tid; K and V share the row and the chunk ----
    u32x4 st_k[kLoads], st_v[kLoads], st_r[ROPE ? kLoadsR : 1];
    const uint8_t *const k_base = a.k + (int64_t)h * a.k_head, *const v_base = a.v + (int64_t)h * a.v_head;
    const uint8_t *const r_base = ROPE ? a.kr + (int64_t)h * a.r_head : nullptr;
    auto fetch = [&](int64_t p0) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kFlashThreads + tid;
            const int64_t pos = p0 + (idx >> 3), row = k0 + pos;
            const bool ok = pos < hi && row >= 0 && row < a.rows_k;   // at or beyond hi: zeros, nothing read
            st_k[i] = u32x4{0u, 0u, 0u, 0u};
            if (ok) st_k[i] = __builtin_nontemporal_load((const u32x4 *)(k_base + row * a.k_tok + 16 * (idx & 7)));
            st_v[i] = u32x4{0u, 0u, 0u, 0u};
            if (ok) st_v[i] = __builtin_nontemporal_load((const u32x4 *)(v_base + row * a.v_tok + 16 * (idx & 7)));
        }
#pragma unroll
        for (int i = 0; i < kLoadsR; ++i) {
            const int idx = i * kFlashThreads + tid;
            const int64_t pos = p0 + (idx >> 2), row = k0 + pos;
            st_r[i] = u32x4{0u, 0u, 0u, 0u};
            if (pos < hi && row >= 0 && row < a.rows_k) st_r[i] = *(const u32x4 *)(r_base + row * a.r_tok + 16 * (idx & 3));   // shared by the heads: cached
        }
    };
    auto commit = [&](int stage) {
        uint8_t *const base = lds + stage * kStage;
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kFlashThreads + tid, row = idx >> 3, at = row * 128 + (((idx & 7) ^ ((row >> 1) & 7)) << 4);
            *(u32x4 *)(base + at) = st_k[i];
            *(u32x4 *)(base + kOffV + at) = st_v[i];
        }
#pragma unroll
        for (int i = 0; i < kLoadsR; ++i) {
            const int idx = i * kFlashThreads + tid, row = idx >> 2;
            *(u32x4 *)(base + kOffR + row * kAttnFlashRope + (((idx & 3) ^ ((row >> 2) & 3)) << 4)) = st_r[i];
        }
    };
    // this lane's fragment offsets inside a stage.  S tile t: row 16 t + (r ^ 8 (t & 1)) - 16 t leaves both swizzles alone - chunk g; chunk 4 + g
    // is 64 bytes away under the xor.  The transpose read (h, u): this lane as a SOURCE is position e of eight, channel half hh, of its lane
    // group's slots 64 h + 16 g + 8 u + [0, 8); 32 rows a (h, u) step leave the swizzle alone.
    int k_rd[2], r_rd[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int rr = r ^ (8 * par);
        k_rd[par] = rr * 128 + ((g ^ ((rr >> 1) & 7)) << 4);
        r_rd[par] = kOffR + rr * kAttnFlashRope + ((g ^ ((rr >> 2) & 3)) << 4);
    }
    const int e = r >> 1, hh = r & 1;
    const int v_row = (e & 3) + 4 * (g & 1) + 8 * ((g >> 1) ^ (e >> 2)) + 16 * (e >> 2);
    const int v_rd = kOffV + v_row * 128 + 8 * hh, v_swz = ((v_row >> 1) & 7) << 4;

    float m_run[kCT], l_run[kCT];   // l_run: this lane's share of the row sum (its 32 positions of every step)
    f32x4 o[kCT][kDT];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        m_run[ct] = kNegInf;
        l_run[ct] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) o[ct][dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const int steps = (int)((hi + kAttnStep - 1) / kAttnStep);
    if (steps > 0) {
        fetch(0);
        commit(0);
        __syncthreads();
    }
    for (int n = 0; n < steps; ++n) {
        const int64_t p0 = (int64_t)n * kAttnStep;
        const bool more = n + 1 < steps;
        const uint8_t *stage = lds + (n & 1) * kStage;
        if (more) fetch(p0 + kAttnStep);   // in flight under this step's products and softmax
        if (p0 < wave_hi) {   // wave-uniform: a wave whose columns all end below the step stages and waits, no more
            float s[kCT][8][4], mx[kCT];
            int live_to[kCT];   // how many positions of this step lie below the column's limit
#pragma unroll
            for (int ct = 0; ct < kCT; ++ct) {
                const int64_t below = (int64_t)hi_col[ct] - p0;
                live_to[ct] = (int)(below < 0 ? 0 : below > kAttnStep ? kAttnStep : below);
                mx[ct] = kNegInf;
            }
            // ---- S^T tiles: a K fragment is read once and feeds both column tiles ----
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint8_t *row = stage + 16 * t * 128 + k_rd[t & 1];
                const u32x4 x0 = *(const u32x4 *)row, x1 = *(const u32x4 *)(stage + ((16 * t * 128 + k_rd[t & 1]) ^ 64));
                const i32x8 kf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
                i32x8 kf1 = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ROPE) {
                    const u32x4 y = *(const u32x4 *)(stage + 16 * t * kAttnFlashRope + r_rd[t & 1]);
                    kf1[0] = (int)y[0], kf1[1] = (int)y[1], kf1[2] = (int)y[2], kf1[3] = (int)y[3];
                }
#pragma unroll
                for (int ct = 0; ct < kCT; ++ct) {
                    f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[ct], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0, kScaleOne);
                    if (ROPE) {
                        const i32x8 q1 = {(int)qr[ct][0], (int)qr[ct][1], (int)qr[ct][2], (int)qr[ct][3], 0, 0, 0, 0};
                        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf1, q1, acc, 0, 0, 0, kScaleOne, 0, kScaleOne);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int pos = 16 * t + ((4 * g + j) ^ (8 * (t & 1)));   // register j is row 4 g + j of the tile
                        s[ct][t][j] = pos < live_to[ct] ? acc[j] * c[ct] : kNegInf;   // a select: whatever a masked row computed is dropped
                        mx[ct] = fmaxf(mx[ct], s[ct][t][j]);
                    }
                }
            }
            // ---- softmax per column tile: P in fp32 for the row sum, e4m3 of p 2^8 for the product ----
            i32x8 pf[kCT];
            float alpha[kCT];
#pragma unroll
            for (int ct = 0; ct < kCT; ++ct) {
                const float m_new = fmaxf(m_run[ct], query_max(mx[ct]));
                // a column whose limit lies below this step and every step before is still at m = -inf: it keeps (m, l, O) exactly - alpha = 1,
                // p = 0 - where exp2(-inf - -inf) would be NaN.  With m_run finite a masked step does so by itself.
                const bool unborn = m_new == kNegInf;
                alpha[ct] = unborn ? 1.0f : fast_exp2(m_run[ct] - m_new);
                const float m_ref = unborn ? 0.0f : m_new;
                m_run[ct] = m_new;
                float sum = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    float p[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        p[j] = fast_exp2(s[ct][t][j] - m_ref);
                        sum = sum + p[j];
                    }
                    constexpr float kP = (float)(1 << kAttnPScaleLog2);
                    pf[ct][t] = (int)encode4<FP8MI_ENC_RNE>(p[0] * kP, p[1] * kP, p[2] * kP, p[3] * kP);
                }
                l_run[ct] = l_run[ct] * alpha[ct] + sum;
            }
            // ---- O^T += V^T . P^T: a V fragment is read once, through the transpose read, and feeds both column tiles ----
#pragma unroll
            for (int dt = 0; dt < kDT; ++dt) {
                i32x8 vf;
#pragma unroll
                for (int hu = 0; hu < 4; ++hu) {   // hu = 2 h + u: rows 64 h + 32 u further on
                    const i32x2 x = lds_read_tr8(stage + v_rd + 32 * hu * 128 + ((16 * dt) ^ v_swz));
                    vf[2 * hu] = x[0];
                    vf[2 * hu + 1] = x[1];
                }
#pragma unroll
                for (int ct = 0; ct < kCT; ++ct) {
                    o[ct][dt] = o[ct][dt] * alpha[ct];
                    o[ct][dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[ct], o[ct][dt], 0, 0, 0, kScaleOne, 0, kScaleOne);
                }
            }
        }
        if (more) commit((n + 1) & 1);   // the stage step n - 1 read: every wave has passed the barrier behind it
        __syncthreads();
    }

    // ---- the wave owns its columns' whole context: no merge ----
    constexpr float kInvP = 1.0f / (float)(1 << kAttnPScaleLog2);
    const float v_scale = a.v_scale[a.scale_head ? h : 0];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const float L = query_sum(l_run[ct]);
        if (!live[ct]) continue;
        const bool empty = L == 0.0f;   // no visible position (a position's p at the maximum is 1): a zero row
        const float norm = (kInvP / L) * v_scale;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                store_from_float(a.out, row_q[ct] * a.ld_out + (int64_t)hq * kAttnFlashDV + 16 * dt + 4 * g + j, empty ? 0.0f : o[ct][dt][j] * norm, OUT);
        }
    }
}

// ---- the producer: float (T, H, D) with token / head strides -> contiguous e4m3 (T, H, D), the bytes fp8mi_kv_cache_append stores.  One
// thread per 16 channels, one 16-byte store ----
constexpr int kQuantThreads = 256;

struct KvQuantArgs {
    const void *x;
    int64_t T, ld_t, ld_h;   // strides in elements
    int H, D;
    const float *scale;
    int scale_head;
    uint8_t *out;
};

template <int IN, int MODE>
__global__ __launch_bounds__(kQuantThreads) void attn_kv_quantize_kernel(const KvQuantArgs a)
{
    const int d16n = a.D >> 4;
    const int64_t idx = (int64_t)blockIdx.x * kQuantThreads + threadIdx.x;
    const int64_t per_token = (int64_t)a.H * d16n;
    if (idx >= a.T * per_token) return;
    const int64_t t = idx / per_token;
    const int rem = (int)(idx - t * per_token), h = rem / d16n, d = (rem - h * d16n) * 16;
    const float pre = __fdiv_rn(1.0f, a.scale[a.scale_head ? h : 0]);
    const int64_t at = t * a.ld_t + (int64_t)h * a.ld_h + d;
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = InVec<IN>::load1(a.x, at + 4 * i + j) * pre;   // the float32 multiply of fp8mi_encode
        w[i] = encode4<MODE>(f[0], f[1], f[2], f[3]);
    }
    *(u32x4 *)(a.out + idx * 16) = w;
}

}  // namespace

// host launchers (called from fp8mi_api.hip, which has validated the arguments)
int fp8mi_launch_attn_kv_quantize(const void *x, int dtype, int64_t T, int H, int D, int64_t ld_t, int64_t ld_h, const float *scale, int scale_head, int mode,
                                  uint8_t *out, hipStream_t s)
{
    const KvQuantArgs a{x, T, ld_t, ld_h, H, D, scale, scale_head, out};
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            return fp8mi_launch_items(attn_kv_quantize_kernel<decltype(in_t)::value, decltype(mode_t)::value>, T * H * (D / 16), kQuantThreads, kQuantThreads, s, a);
        });
    });
}

int fp8mi_launch_attention_prefill(const void *q, int q_dtype, int64_t rows, int Hq, int DQK, int64_t ld_q, const uint8_t *k, int64_t k_tok, int64_t k_head,
                                   const uint8_t *k_rope, int64_t r_tok, int64_t r_head, const uint8_t *v, int64_t v_tok, int64_t v_head, int64_t rows_k, int Hkv,
                                   const float *k_scale, const float *v_scale, int scale_head, int64_t B, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                                   int64_t max_q_len, int64_t max_k_len, int causal, float softmax_scale, void *out, int out_dtype, int64_t ld_out, hipStream_t s)
{
    FlashArgs a = {};
    a.q = q; a.ld_q = ld_q; a.k = k; a.kr = k_rope; a.v = v;
    a.k_tok = k_tok; a.k_head = k_head; a.r_tok = r_tok; a.r_head = r_head; a.v_tok = v_tok; a.v_head = v_head; a.rows_k = rows_k;
    a.k_scale = k_scale; a.v_scale = v_scale; a.scale_head = scale_head;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.Hkv = Hkv; a.group = Hq / Hkv;
    a.out = out; a.ld_out = ld_out; a.cu_q = cu_seqlens_q; a.cu_k = cu_seqlens_k; a.B = B; a.rows = rows; a.max_k_len = max_k_len;
    const int64_t qtiles = fp8mi_attn_flash_q_tiles(max_q_len, Hq, Hkv);
    if (max_q_len < 1 || max_q_len > 0x7FFFFFFF || max_k_len > 0x7FFFFFFF || B * Hkv > 0x7FFFFFFF / qtiles) return FP8MI_E_UNSUPPORTED;
    a.max_q_len = (int)max_q_len; a.tq = fp8mi_attn_tile_tokens(Hq, Hkv); a.qtiles = (int)qtiles;
    const dim3 grid((unsigned)(B * Hkv * qtiles));
    return dispatch_in(q_dtype, [&](auto in_t) {
        return dispatch_in(out_dtype, [&](auto out_t) {
            return dispatch_int<128, 192>(DQK, [&](auto d_t) {
                constexpr int IN = decltype(in_t)::value, OUT = decltype(out_t)::value, DD = decltype(d_t)::value;
                if (causal) return fp8mi_launch(attn_flash_kernel<IN, OUT, DD, true>, grid, dim3(kFlashThreads), s, a);
                return fp8mi_launch(attn_flash_kernel<IN, OUT, DD, false>, grid, dim3(kFlashThreads), s, a);
            });
        });
    });
}
