// Paged attention for prompt chunks over the FP8 paged KV cache for gfx950 (fp8mi_paged_attention_prefill; include/fp8mi.h has the contract,
// DESIGN.md 5.21 the design): the contract of fp8mi_paged_attention_varlen - paged e4m3 cache, cu_seqlens_q, a causal mask aligned at the
// end of the context - with a work split and a data path of its own.
//
// One workgroup of kAttnPrefillWaves = 4 waves per (sequence, KV head, query tile, split).  A query tile is kAttnPrefillCols = 128 MFMA
// columns: eight 16-column tiles, wave w owns tiles 2 w and 2 w + 1.  Inside a 16-column tile column r is token r / G, head r % G of the
// KV head's group (G = Hq / Hkv), as in the multi-token form of fp8mi_attn_decode.hip: a workgroup takes 8 (16 / G) query tokens.
//
// K and V go through LDS.  Per 128-position step all 256 threads stage the step's 128 K rows (128 x D bytes) and its V runs (D channels x
// 128 positions) with 16-byte loads - a 16-position run of V never crosses a block - through registers into one of two stages (2 x 32 KiB
// at D = 128): the loads of step n + 1 are issued before the products of step n and written to the other stage behind them, one barrier
// per step.  Each wave reads an operand fragment from LDS once and feeds it to the MFMAs of both its column tiles.
//   LDS layout, swizzled, no padding.  A 16-lane group of a ds_read_b128 reads ONE 16-byte chunk index of 16 different rows:
//     K  rows (positions) of D bytes; the S tile t reads rows 64 (t >> 2) + 16 (r >> 2) + 4 (t & 3) + (r & 3), chunks g and 4 + g.  Chunk c
//        of row p lives at chunk c ^ f(p), f(p) = bit 1 of p | bits 4, 5 of p << 1 (D = 128: 8 chunks) or bits 4, 5 of p (D = 64: 4 chunks):
//        the 16 rows of a lane group then cover, with bit 0 (D = 64: bits 0, 1) of p selecting the 128-byte (64-byte) row inside a 256-byte
//        bank span, all 16 16-byte units of the span once.
//     V  rows (channels) of 128 bytes; the O tile dt reads channels 16 dt + r, chunks g and 4 + g.  Chunk c of channel d lives at chunk
//        c ^ ((d >> 1) & 7): 16 consecutive channels cover the 16 units once.
//   The staging stores write 16 consecutive chunks (K: two rows; V: 16 channels of one run) per lane group: the same cover.
//
// Products and softmax are fp8mi_attn_decode.hip's per column tile: v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales, Q quantised to e4m3
// per row in the kernel (the tiny-Q path included), K rows read in the order above so that the packed S registers are the P operand with no
// lane movement, online softmax in base 2, P = rne(p 2^8), l from the fp32 p.  One wave walks ALL steps of its columns' split in order: no
// round-robin, no cross-wave (m, l, O) merge.
//
// Causality and isolation.  The step loop, the staging and the V byte mask run to the limit of the workgroup tile's last live token bounded
// by the split end (hi); zeros are written to LDS for every position at or beyond it, which is not read: no K row, no V run, no table
// entry.  The score select uses each column's own limit; a column a step masks whole keeps (m, l, O) exactly (`unborn`); a wave whose two
// column tiles lie wholly below a step skips its MFMAs and softmax and still stages and meets the barrier.  A NaN byte of V in [limit_j,
// last limit of j's 128-column tile) may poison row j (0 x NaN in the shared V operand); nothing else at or beyond a row's limit moves it.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

int fp8mi_launch_paged_attention_combine(int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, int Hkv, int D, const float *v_scale,
                                         int scale_head, int splits, void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s);

namespace {

constexpr int kScaleOne = 0x7F7F7F7F;
constexpr int kPrefillThreads = 64 * kAttnPrefillWaves;
constexpr int kCT = kAttnPrefillCols / 16 / kAttnPrefillWaves;   // column tiles of a wave: 2
constexpr float kNegInf = -__builtin_huge_valf();

struct PrefillArgs {
    const void *q;
    int64_t ld_q;
    const uint8_t *kc, *vc;
    int64_t num_blocks;
    const int32_t *bt;
    int64_t ld_bt, max_blocks;
    const int32_t *seq_lens;
    const float *k_scale, *v_scale;
    int scale_head;
    float scale_log2;   // softmax_scale log2 e
    int Hq, Hkv, group, bs_log2;
    int splits;
    int64_t chunk;      // positions per split, a multiple of kAttnStep
    float *part_m, *part_l, *part_o;
    void *out;
    int64_t ld_out;
    const int32_t *cu;   // [B + 1]
    int64_t rows;        // T
    int max_q_len;
    int tq, qtiles;      // query tokens per 16-column tile; 128-column tiles per sequence, ceil(max_q_len / (8 tq))
};

FP8MI_DEVICE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
FP8MI_DEVICE float xor_lanes(float v, int mask) { return __shfl_xor(v, mask, 64); }
// over the four lanes that hold one query (lane & 15 alike)
FP8MI_DEVICE float query_max(float v) { v = fmaxf(v, xor_lanes(v, 16)); return fmaxf(v, xor_lanes(v, 32)); }
FP8MI_DEVICE float query_sum(float v) { v = v + xor_lanes(v, 16); return v + xor_lanes(v, 32); }

// the first `keep` (0 .. 16) bytes of a 16-byte run, the others cleared
FP8MI_DEVICE u32x4 keep_bytes(u32x4 v, int keep)
{
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int n = keep - 4 * w;
        const uint32_t mask = n >= 4 ? 0xFFFFFFFFu : n <= 0 ? 0u : ((1u << (8 * n)) - 1u);
        v[w] &= mask;
    }
    return v;
}

// the swizzle of a K row's chunks (the header of this file)
template <int D> FP8MI_DEVICE int k_swizzle(int row) { return D == 128 ? (((row >> 1) & 1) | (((row >> 4) & 3) << 1)) : ((row >> 4) & 3); }

template <int IN, int OUT, int D, bool SPLIT>
__global__ __launch_bounds__(kPrefillThreads) void attn_prefill_kernel(const PrefillArgs a)
{
    constexpr int kDT = D / 16;        // 16-channel tiles of O; also the 16-byte chunks of a K row
    constexpr int kLoads = D / 32;     // 16-byte loads per thread of K, and of V, per step: 128 D / 16 / 256
    constexpr int kStageK = kAttnStep * D, kStage = 2 * kStageK;   // K rows, then V channels
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int split = (int)(blockIdx.x % (unsigned)a.splits);
    int64_t bh = blockIdx.x / (unsigned)a.splits;
    const int tile = (int)(bh % a.qtiles);
    bh /= a.qtiles;
    const int h = (int)(bh % a.Hkv);
    const int64_t b = bh / a.Hkv;
    const int bs = 1 << a.bs_log2;

    int64_t seq = a.seq_lens[b];
    seq = seq < 0 ? 0 : seq;
    seq = seq > (a.max_blocks << a.bs_log2) ? (a.max_blocks << a.bs_log2) : seq;   // the table holds no more
    const int64_t lo = (int64_t)split * a.chunk;
    const int64_t c0 = a.cu[b];
    const int64_t q_len = (int64_t)a.cu[b + 1] - c0;
    const int64_t q_take = q_len < a.max_q_len ? q_len : a.max_q_len;   // tokens at or beyond max_q_len are not written
    const int tokens = kAttnPrefillCols / 16 * a.tq;                   // of a workgroup
    const int64_t j0 = (int64_t)tile * tokens;
    if (j0 >= q_take) return;   // nothing of this tile is owned: before any barrier, every thread alike

    // ---- the columns of this lane: token and head, the query row, the causal limit (what a decode call with seq_len = limit takes of this split) ----
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
        int64_t limit = seq - q_len + j + 1;
        limit = !live[ct] || limit < 0 ? 0 : limit > seq ? seq : limit;
        hi_col[ct] = (int)((split == a.splits - 1 || lo + a.chunk > limit) ? limit : lo + a.chunk);   // <= limit <= seq_len, an int32
    }
    // the limit of the workgroup tile's last live token: the loop, the staging and the V byte mask run to it
    const int64_t j_last = (j0 + tokens < q_take ? j0 + tokens : q_take) - 1;
    int64_t tile_limit = seq - q_len + j_last + 1;
    tile_limit = tile_limit < 0 ? 0 : tile_limit > seq ? seq : tile_limit;
    const int64_t hi = (split == a.splits - 1 || lo + a.chunk > tile_limit) ? tile_limit : lo + a.chunk;
    // the last limit of this wave's columns: a step at or beyond it is skipped by the wave
    int wave_hi = hi_col[0];
#pragma unroll
    for (int ct = 1; ct < kCT; ++ct) wave_hi = wave_hi > hi_col[ct] ? wave_hi : hi_col[ct];
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const int other = __shfl_xor(wave_hi, mask, 64);
        wave_hi = wave_hi > other ? wave_hi : other;
    }
    wave_hi = __builtin_amdgcn_readfirstlane(wave_hi);
    const int32_t *table = a.bt + b * a.ld_bt;

    // ---- Q: this lane's bytes of its columns' query heads, quantised per row ----
    i32x8 qf[kCT];
    float c[kCT];   // an S accumulator times c: the logit, base 2
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        float qv[D / 4];   // channels 16 g + [0, 16), then 64 + 16 g + [0, 16) (D = 128)
        float amax = 0.0f;
#pragma unroll
        for (int i = 0; i < D / 4; ++i) {
            const int d = (i >> 4) * 64 + g * 16 + (i & 15);
            qv[i] = live[ct] ? InVec<IN>::load1(a.q, row_q[ct] * a.ld_q + (int64_t)hq * D + d) : 0.0f;
            amax = fmaxf(amax, fabsf(qv[i]));
        }
        amax = query_max(amax);
        // 448 / amax is +inf for 0 < amax < 448 / FLT_MAX: such a row and its amax are multiplied by 2^64 first - exact, subnormals
        // included - and 2^-64 goes into the logit scale.  No other row changes.
        const bool tiny = amax > 0.0f && amax < kAttnTinyQ;
        if (tiny) {
            amax *= kAttnTinyQUp;
#pragma unroll
            for (int i = 0; i < D / 4; ++i) qv[i] *= kAttnTinyQUp;
        }
        const float q_scale = amax > 0.0f ? amax / 448.0f : 1.0f, q_inv = amax > 0.0f ? 448.0f / amax : 1.0f;
        qf[ct] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < D / 16; ++w)
            qf[ct][w] = (int)encode4<FP8MI_ENC_RNE>(qv[4 * w] * q_inv, qv[4 * w + 1] * q_inv, qv[4 * w + 2] * q_inv, qv[4 * w + 3] * q_inv);
        c[ct] = (q_scale * a.k_scale[a.scale_head ? h : 0]) * a.scale_log2;
        if (tiny) c[ct] *= 1.0f / kAttnTinyQUp;
    }

    // ---- staging: global -> registers (fetch), registers -> LDS (commit) ----
    u32x4 st_k[kLoads], st_v[kLoads];
    // The table entries of a step's loads are read first, all of them, and the 16-byte loads issued behind ONE wait for those: with a table
    // read in front of every load the counter wait for it also waits for the load before, and the step's 16 round trips run one after another.
    auto fetch = [&](int64_t p0) {
        int64_t blk_k[kLoads], blk_v[kLoads];
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kPrefillThreads + tid;
            const int64_t pos = p0 + idx / kDT, ps = p0 + 16 * (idx / D);
            blk_k[i] = pos < hi ? (int64_t)table[pos >> a.bs_log2] : -1;   // at or beyond hi: no table entry is read
            blk_v[i] = ps < hi ? (int64_t)table[ps >> a.bs_log2] : -1;
        }
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kPrefillThreads + tid;
            const int64_t pos = p0 + idx / kDT, ps = p0 + 16 * (idx / D);
            st_k[i] = u32x4{0u, 0u, 0u, 0u};   // chunk idx % kDT of row idx / kDT
            if (blk_k[i] >= 0 && blk_k[i] < a.num_blocks)
                st_k[i] = *(const u32x4 *)(a.kc + (((blk_k[i] * a.Hkv + h) << a.bs_log2) + (pos & (bs - 1))) * D + (idx & (kDT - 1)) * 16);
            st_v[i] = u32x4{0u, 0u, 0u, 0u};   // the 16-position run idx / D of channel idx % D; its bytes at or beyond hi are cleared by commit_v
            if (blk_v[i] >= 0 && blk_v[i] < a.num_blocks)
                st_v[i] = __builtin_nontemporal_load((const u32x4 *)(a.vc + (((blk_v[i] * a.Hkv + h) * D + (idx & (D - 1))) << a.bs_log2) + (ps & (bs - 1))));
        }
    };
    auto commit_k = [&](int stage) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kPrefillThreads + tid, row = idx / kDT;
            *(u32x4 *)(lds + stage * kStage + row * D + (((idx & (kDT - 1)) ^ k_swizzle<D>(row)) << 4)) = st_k[i];
        }
    };
    auto commit_v = [&](int stage, int64_t p0) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * kPrefillThreads + tid, ch = idx & (D - 1);
            const int64_t left = hi - (p0 + 16 * (idx / D));
            *(u32x4 *)(lds + stage * kStage + kStageK + ch * kAttnStep + (((idx / D) ^ ((ch >> 1) & 7)) << 4)) =
                keep_bytes(st_v[i], (int)(left > 16 ? 16 : left < 0 ? 0 : left));
        }
    };
    // this lane's fragment offsets inside a stage: rows 16 (r >> 2) + (r & 3) (+ 64 (t >> 2) + 4 (t & 3), which leaves the swizzle alone) of K,
    // channel r (+ 16 dt, likewise) of V
    const int k_row = 16 * (r >> 2) + (r & 3), k_swz = k_swizzle<D>(k_row), v_swz = (r >> 1) & 7;
    const int k_rd0 = k_row * D + ((g ^ k_swz) << 4), k_rd1 = k_row * D + (((4 + g) ^ k_swz) << 4);
    const int v_rd0 = kStageK + r * kAttnStep + ((g ^ v_swz) << 4), v_rd1 = kStageK + r * kAttnStep + (((4 + g) ^ v_swz) << 4);

    float m_run[kCT], l_run[kCT];   // l_run: this lane's share of the row sum (its 32 positions of every step)
    f32x4 o[kCT][kDT];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        m_run[ct] = kNegInf;
        l_run[ct] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) o[ct][dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const int steps = hi > lo ? (int)((hi - lo + kAttnStep - 1) / kAttnStep) : 0;
    if (steps > 0) {
        fetch(lo);
        commit_k(0);
        commit_v(0, lo);
        __syncthreads();
    }
    for (int n = 0; n < steps; ++n) {
        const int64_t p0 = lo + (int64_t)n * kAttnStep;
        const bool more = n + 1 < steps;
        const uint8_t *stage = lds + (n & 1) * kStage;
        if (more) fetch(p0 + kAttnStep);   // in flight under this step's products and softmax
        if (p0 < wave_hi) {   // wave-uniform: a wave whose columns all lie below the step stages and waits, no more
            float s[kCT][8][4], mx[kCT];
            // ---- S^T tiles: a K fragment is read once and feeds both column tiles ----
            int live_to[kCT];   // how many of this lane's positions p0 + 16 g + [0, 128) lie below the column's limit
#pragma unroll
            for (int ct = 0; ct < kCT; ++ct) {
                const int64_t below = (int64_t)hi_col[ct] - (p0 + 16 * g);
                live_to[ct] = (int)(below < 0 ? 0 : below > kAttnStep ? kAttnStep : below);
                mx[ct] = kNegInf;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int off = (64 * (t >> 2) + 4 * (t & 3)) * D;
                const u32x4 x0 = *(const u32x4 *)(stage + k_rd0 + off);
                u32x4 x1 = {0u, 0u, 0u, 0u};
                if (D == 128) x1 = *(const u32x4 *)(stage + k_rd1 + off);
                const i32x8 kf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
#pragma unroll
                for (int ct = 0; ct < kCT; ++ct) {
                    const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[ct], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0,
                                                                                        kScaleOne);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        s[ct][t][j] = 64 * (t >> 2) + 4 * (t & 3) + j < live_to[ct] ? acc[j] * c[ct] : kNegInf;   // a select: whatever a masked row computed is dropped
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
            // ---- O^T += V^T . P^T: a V fragment is read once and feeds both column tiles ----
#pragma unroll
            for (int dt = 0; dt < kDT; ++dt) {
                const u32x4 x0 = *(const u32x4 *)(stage + v_rd0 + 16 * dt * kAttnStep), x1 = *(const u32x4 *)(stage + v_rd1 + 16 * dt * kAttnStep);
                const i32x8 vf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
#pragma unroll
                for (int ct = 0; ct < kCT; ++ct) {
                    o[ct][dt] = o[ct][dt] * alpha[ct];
                    o[ct][dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[ct], o[ct][dt], 0, 0, 0, kScaleOne, 0, kScaleOne);
                }
            }
        }
        if (more) {   // the stage step n - 1 read: every wave has passed the barrier behind it
            commit_k((n + 1) & 1);
            commit_v((n + 1) & 1, p0 + kAttnStep);
        }
        __syncthreads();
    }

    // ---- the wave owns its columns' whole split: no merge ----
    constexpr float kInvP = 1.0f / (float)(1 << kAttnPScaleLog2);
    const float v_scale = a.v_scale[a.scale_head ? h : 0];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const float L = query_sum(l_run[ct]);
        if (!live[ct]) continue;
        const int64_t row = row_q[ct] * a.Hq + hq;
        if (SPLIT && g == 0) {
            a.part_m[row * a.splits + split] = m_run[ct];   // a split that owns no position of the row: m = -inf, l = 0, O = 0
            a.part_l[row * a.splits + split] = L;
        }
        const bool empty = L == 0.0f;   // no visible position (a position's p at the maximum is 1): a zero row
        const float norm = SPLIT ? kInvP : (kInvP / L) * v_scale;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            const int d = 16 * dt + 4 * g;
            if (SPLIT) {
                *(f32x4 *)(a.part_o + (row * a.splits + split) * D + d) = o[ct][dt] * norm;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    store_from_float(a.out, row_q[ct] * a.ld_out + (int64_t)hq * D + d + j, empty ? 0.0f : o[ct][dt][j] * norm, OUT);
            }
        }
    }
}

}  // namespace

// host launcher (called from fp8mi_api.hip, which has validated the arguments and chosen `splits`): the argument list of
// fp8mi_launch_paged_attention in its multi-token form
int fp8mi_launch_paged_attention_prefill(const void *q, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, int Hkv,
                                         int D, int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size,
                                         const int32_t *block_table, int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len,
                                         const float *k_scale, const float *v_scale, int scale_head, float softmax_scale, int splits, void *workspace, void *out,
                                         int out_dtype, int64_t ld_out, hipStream_t s)
{
    PrefillArgs a = {};
    a.q = q; a.ld_q = ld_q; a.kc = k_cache; a.vc = v_cache; a.num_blocks = num_blocks;
    a.bt = block_table; a.ld_bt = ld_bt; a.max_blocks = max_blocks; a.seq_lens = seq_lens;
    a.k_scale = k_scale; a.v_scale = v_scale; a.scale_head = scale_head;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.Hkv = Hkv; a.group = Hq / Hkv; a.bs_log2 = fp8mi_attn_log2(block_size);
    a.splits = splits; a.chunk = fp8mi_attn_chunk(max_seq_len, splits);
    a.out = out; a.ld_out = ld_out;
    const int64_t qtiles = fp8mi_attn_prefill_q_tiles(max_q_len, Hq, Hkv);
    if (max_q_len < 1 || max_q_len > 0x7FFFFFFF || B * Hkv > 0x7FFFFFFF / qtiles || B * Hkv * qtiles > 0x7FFFFFFF / splits || rows * Hq > 0x7FFFFFFF)
        return FP8MI_E_UNSUPPORTED;
    const int64_t grid = B * Hkv * qtiles * splits;
    a.cu = cu_seqlens_q; a.rows = rows; a.max_q_len = (int)max_q_len;
    a.tq = fp8mi_attn_tile_tokens(Hq, Hkv); a.qtiles = (int)qtiles;
    if (splits > 1) {
        const int64_t parts = rows * Hq * splits;   // fp8mi_attn_decode.hip's layout, which its combine reads
        a.part_o = (float *)workspace;
        a.part_m = a.part_o + parts * D;
        a.part_l = a.part_m + parts;
    }
    return dispatch_in(q_dtype, [&](auto in_t) {
        return dispatch_int<64, 128>(D, [&](auto d_t) {
            constexpr int IN = decltype(in_t)::value, DD = decltype(d_t)::value;
            if (splits > 1) {
                if (int rc = fp8mi_launch(attn_prefill_kernel<IN, FP8MI_F32, DD, true>, dim3((unsigned)grid), dim3(kPrefillThreads), s, a)) return rc;
                return fp8mi_launch_paged_attention_combine(rows, B, cu_seqlens_q, max_q_len, Hq, Hkv, D, v_scale, scale_head, splits, workspace, out, out_dtype,
                                                            ld_out, s);
            }
            return dispatch_in(out_dtype, [&](auto out_t) {
                return fp8mi_launch(attn_prefill_kernel<IN, decltype(out_t)::value, DD, false>, dim3((unsigned)grid), dim3(kPrefillThreads), s, a);
            });
        });
    });
}
