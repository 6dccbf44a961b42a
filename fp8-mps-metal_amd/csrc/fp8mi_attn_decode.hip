// Single-query (decode) attention over the FP8 paged KV cache for gfx950 (fp8mi_paged_attention_decode; include/fp8mi.h has the cache
// layout and the definition): one query token per sequence against e4m3 K and V bytes, the memory-bound vec-mat of attention.
//
// One workgroup of kAttnWaves waves per (sequence, KV head, split).  The Hq / Hkv query heads of the KV head are the 16 columns of an MFMA
// tile (zero beyond the group).  Both products run on v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales, on the cache's own bytes:
//   Q    quantised to e4m3 per (sequence, head) row inside the kernel: q_scale = amax / 448 over D, bytes = rne(q (448 / amax)); a row
//        with amax below kAttnTinyQ goes through a power of two first (448 / amax would be +inf); non-finite q is undefined;
//   S^T  [16 pos][16 q] = K[16 pos][D] . Q^T: K rows are the first source (lane & 15 = the row, 16 (lane >> 4) + [0, 16) and 64 + ... its
//        bytes), Q the second; D = 64 fills the upper half of the K-step with zeros.  A lane then holds, for ITS query (lane & 15), rows
//        4 (lane >> 4) + j of the tile in register j;
//   softmax online in fp32, base 2: logits S q_scale k_scale softmax_scale log2 e, running maximum m, p = exp2(logit - m), the row sum l
//        from the fp32 p;
//   P    packed to e4m3 as rne(p 2^8) (kAttnPScaleLog2: probabilities down to 2^-17 survive next to a dominant key);
//   O^T  [16 d][16 q] += V^T[16 d][128 pos] . P^T[128 pos][16 q]: V rows (one channel, 128 positions) are the first source, P the second.
// Eight S tiles are one lane's 32-byte P operand with no lane movement and no LDS: the fp8 operand holds k-slot 64 h + 16 g + j in byte
// 16 h + j of lane group g (profiles/mxw4a8_operand_map.txt), so row m of S tile t carries position
//   64 (t >> 2) + 16 (m >> 2) + 4 (t & 3) + (m & 3)
// of the 128-position step, and dword t of the P operand is registers 0 .. 3 of tile t (profiles/paged_attn_permutation.txt).  A lane's V
// operand is then two contiguous 16-byte runs of the V cache, never across a block (block_size >= 16).
//
// Nothing outside [0, seq_len) reaches the output: a K row, a V run and a block-table entry beyond the split's last position are not
// read at all (zeros stand in), the bytes of a V run beyond it are cleared (0 x NaN is NaN in the MFMA), and the scores of such positions
// are replaced by -inf with a select.  The waves of a workgroup take the steps of their split round-robin and merge (m, l, O) through LDS.
// Unsplit: O / (2^8 l) v_scale is stored.  Split: (m, l, O / 2^8) go to the workspace in fp32 and attn_combine_kernel merges them; a split
// that owns no position writes m = -inf, l = 0, O = 0, which the combine weighs with 0.
//
// The multi-token form (fp8mi_paged_attention_varlen, template flag MULTI) is the same text: the 16 columns hold (token,
// head) pairs of TQ = 16 / (Hq / Hkv) query tokens of one sequence, one workgroup per (sequence, KV head, tile of TQ tokens, split).  The
// loop, the loads and the V byte mask run to the causal limit of the tile's last live token, the score select to the column's own; a column
// a step masks whole keeps (m, l, O) exactly.  Every row is then, bit for bit, what the decode form gives a sequence of seq_len = its limit.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

namespace {

constexpr int kScaleOne = 0x7F7F7F7F;
constexpr int kAttnThreads = 64 * kAttnWaves;
constexpr float kNegInf = -__builtin_huge_valf();

struct AttnArgs {
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
    // the multi-token form (fp8mi_paged_attention_varlen; nullptr / 0 in the decode form)
    const int32_t *cu;   // [B + 1]: sequence b owns query rows [cu[b], cu[b + 1])
    int64_t rows;        // T: a row at or beyond it is neither read nor written
    int max_q_len;       // host bound of a sequence's query tokens, at most T
    int tq, qtiles;      // query tokens per 16-column tile, 16 / group; tiles per sequence, ceil(max_q_len / tq)
};

// Cache policy of the K loads (compile-time knob for A/B builds; the product value is the default): a K row's 128-byte line is read by two
// load instructions, one per half.  1: non-temporal, like the V loads (whose lines one instruction reads whole); 0: the default policy - 8 to
// 12 % less time wherever the cache is not far beyond the L2s, equal beyond (profiles/paged_attn_k_policy_ab.txt).
#ifndef FP8MI_ATTN_K_NT
#define FP8MI_ATTN_K_NT 0
#endif
FP8MI_DEVICE u32x4 load_k16(const uint8_t *p)
{
#if FP8MI_ATTN_K_NT
    return __builtin_nontemporal_load((const u32x4 *)p);
#else
    return *(const u32x4 *)p;
#endif
}

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

// MULTI: the 16 columns are (token, head) pairs of one sequence's query tokens, each with its own causal limit (the header of
// fp8mi_paged_attention_varlen in include/fp8mi.h); the decode instances compile without a trace of it.
template <int IN, int OUT, int D, bool SPLIT, bool MULTI>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_kernel(const AttnArgs a)
{
    constexpr int kDT = D / 16;   // 16-channel tiles of O
    __shared__ float lds_m[kAttnWaves][64], lds_l[kAttnWaves][64];
    __shared__ f32x4 lds_o[kAttnWaves][kDT][64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int split = (int)(blockIdx.x % (unsigned)a.splits);
    int64_t bh = blockIdx.x / (unsigned)a.splits;
    int tile = 0;
    if (MULTI) {
        tile = (int)(bh % a.qtiles);
        bh /= a.qtiles;
    }
    const int h = (int)(bh % a.Hkv);
    const int64_t b = bh / a.Hkv;
    const int bs = 1 << a.bs_log2;

    int64_t seq = a.seq_lens[b];
    seq = seq < 0 ? 0 : seq;
    seq = seq > (a.max_blocks << a.bs_log2) ? (a.max_blocks << a.bs_log2) : seq;   // the table holds no more
    const int64_t lo = (int64_t)split * a.chunk;
    // MULTI: column r is token j0 + r / group of the sequence's query tokens, head r % group of the KV head's; it attends [0, limit),
    // limit = seq - q_len + token + 1.  The loop, the loads and the V byte mask run to the limit of the tile's LAST live token (hi); the
    // score select uses the column's own (hi_col <= hi): what a decode call with seq_len = limit would take of this split.
    int64_t row_q = b;   // the query row: q and out at row_q ld, partials at row_q Hq + hq
    int col_head = r, hi_col = 0;
    bool col_live = r < a.group;
    if (MULTI) {
        const int64_t c0 = a.cu[b];
        int64_t q_len = (int64_t)a.cu[b + 1] - c0;
        const int64_t q_take = q_len < a.max_q_len ? q_len : a.max_q_len;   // tokens at or beyond max_q_len are not written
        const int64_t j0 = (int64_t)tile * a.tq;
        if (j0 >= q_take) return;   // nothing of this tile is owned: before any barrier, every thread alike
        const int tok = r / a.group;
        col_head = r - tok * a.group;
        row_q = c0 + j0 + tok;
        col_live = tok < a.tq && j0 + tok < q_take && row_q >= 0 && row_q < a.rows;
        int64_t limit = seq - q_len + j0 + tok + 1;
        limit = !col_live || limit < 0 ? 0 : limit > seq ? seq : limit;
        const int64_t j_last = (j0 + a.tq < q_take ? j0 + a.tq : q_take) - 1;
        int64_t tile_limit = seq - q_len + j_last + 1;
        tile_limit = tile_limit < 0 ? 0 : tile_limit > seq ? seq : tile_limit;
        hi_col = (int)((split == a.splits - 1 || lo + a.chunk > limit) ? limit : lo + a.chunk);   // <= limit <= seq_len, an int32
        seq = tile_limit;
    }
    const int64_t hi = (split == a.splits - 1 || lo + a.chunk > seq) ? seq : lo + a.chunk;
    const int32_t *table = a.bt + b * a.ld_bt;

    // ---- Q: this lane's bytes of its query head, quantised per row ----
    const int hq = h * a.group + col_head;
    const bool q_live = col_live;
    float qv[D / 4];   // channels 16 g + [0, 16), then 64 + 16 g + [0, 16) (D = 128)
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < D / 4; ++i) {
        const int d = (i >> 4) * 64 + g * 16 + (i & 15);
        qv[i] = q_live ? InVec<IN>::load1(a.q, row_q * a.ld_q + (int64_t)hq * D + d) : 0.0f;
        amax = fmaxf(amax, fabsf(qv[i]));
    }
    amax = query_max(amax);
    // 448 / amax is +inf for 0 < amax < 448 / FLT_MAX = 1.32e-36 (subnormal rows among them), and q inf is inf or NaN: such a row and its
    // amax are multiplied by 2^64 first - exact, subnormals included - and 2^-64 goes into the logit scale.  No other row changes.
    const bool tiny = amax > 0.0f && amax < kAttnTinyQ;
    if (tiny) {
        amax *= kAttnTinyQUp;
#pragma unroll
        for (int i = 0; i < D / 4; ++i) qv[i] *= kAttnTinyQUp;
    }
    const float q_scale = amax > 0.0f ? amax / 448.0f : 1.0f, q_inv = amax > 0.0f ? 448.0f / amax : 1.0f;
    i32x8 qf = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < D / 16; ++w)
        qf[w] = (int)encode4<FP8MI_ENC_RNE>(qv[4 * w] * q_inv, qv[4 * w + 1] * q_inv, qv[4 * w + 2] * q_inv, qv[4 * w + 3] * q_inv);
    float c = (q_scale * a.k_scale[a.scale_head ? h : 0]) * a.scale_log2;   // an S accumulator times c: the logit, base 2
    if (tiny) c *= 1.0f / kAttnTinyQUp;

    float m_run = kNegInf, l_run = 0.0f;   // l_run: this lane's share of the row sum (its 32 positions of every step)
    f32x4 o[kDT];
#pragma unroll
    for (int dt = 0; dt < kDT; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int64_t p0 = lo + (int64_t)wave * kAttnStep; p0 < hi; p0 += (int64_t)kAttnWaves * kAttnStep) {
        // ---- loads: 8 K rows and the V runs of this lane, zeros in place of everything at or beyond hi ----
        i32x8 kf[8], vf[kDT];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t pos = p0 + 64 * (t >> 2) + 16 * (r >> 2) + 4 * (t & 3) + (r & 3);
            u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
            if (pos < hi) {
                const int64_t blk = table[pos >> a.bs_log2];
                if (blk >= 0 && blk < a.num_blocks) {
                    const uint8_t *row = a.kc + (((blk * a.Hkv + h) << a.bs_log2) + (pos & (bs - 1))) * D + g * 16;
                    x0 = load_k16(row);
                    if (D == 128) x1 = load_k16(row + 64);
                }
            }
            kf[t] = i32x8{(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        }
        {
            const int64_t ps0 = p0 + 16 * g, ps1 = ps0 + 64;
            const uint8_t *run0 = nullptr, *run1 = nullptr;
            if (ps0 < hi) {
                const int64_t blk = table[ps0 >> a.bs_log2];
                if (blk >= 0 && blk < a.num_blocks) run0 = a.vc + (((blk * a.Hkv + h) * D + r) << a.bs_log2) + (ps0 & (bs - 1));
            }
            if (ps1 < hi) {
                const int64_t blk = table[ps1 >> a.bs_log2];
                if (blk >= 0 && blk < a.num_blocks) run1 = a.vc + (((blk * a.Hkv + h) * D + r) << a.bs_log2) + (ps1 & (bs - 1));
            }
            const int keep0 = (int)(hi - ps0 > 16 ? 16 : hi - ps0), keep1 = (int)(hi - ps1 > 16 ? 16 : hi - ps1);
#pragma unroll
            for (int dt = 0; dt < kDT; ++dt) {
                u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
                if (run0) x0 = keep_bytes(__builtin_nontemporal_load((const u32x4 *)(run0 + ((int64_t)(16 * dt) << a.bs_log2))), keep0);
                if (run1) x1 = keep_bytes(__builtin_nontemporal_load((const u32x4 *)(run1 + ((int64_t)(16 * dt) << a.bs_log2))), keep1);
                vf[dt] = i32x8{(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
            }
        }

        // ---- S^T tiles, the logits of this lane's query at its 32 positions ----
        float s[8][4];
        float mx = kNegInf;
        // MULTI: how many of this lane's positions p0 + 16 g + [0, 128) lie below its column's limit, one register for the 32 selects
        int64_t below = MULTI ? (int64_t)hi_col - (p0 + 16 * g) : 0;
        const int live_to = (int)(below < 0 ? 0 : below > kAttnStep ? kAttnStep : below);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf[t], qf, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0,
                                                                                kScaleOne);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t pos = p0 + 64 * (t >> 2) + 16 * g + 4 * (t & 3) + j;
                s[t][j] = (MULTI ? 64 * (t >> 2) + 4 * (t & 3) + j < live_to : pos < hi) ? acc[j] * c : kNegInf;   // a select: whatever a masked row computed is dropped
                mx = fmaxf(mx, s[t][j]);
            }
        }
        mx = query_max(mx);
        const float m_new = fmaxf(m_run, mx);   // finite: the step holds a position below hi
        // MULTI: a column whose limit lies below this step, and below every step this wave took before, is still at m = -inf: it keeps
        // (m, l, O) exactly - alpha = 1, p = 0 - where exp2(-inf - -inf) would be NaN.  With m_run finite a masked step does so by itself.
        const bool unborn = MULTI && m_new == kNegInf;
        const float alpha = unborn ? 1.0f : fast_exp2(m_run - m_new);
        const float m_ref = unborn ? 0.0f : m_new;
        m_run = m_new;

        // ---- P: fp32 for the row sum, e4m3 of p 2^8 for the product ----
        i32x8 pf;
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[j] = fast_exp2(s[t][j] - m_ref);
                sum = sum + p[j];
            }
            constexpr float kP = (float)(1 << kAttnPScaleLog2);
            pf[t] = (int)encode4<FP8MI_ENC_RNE>(p[0] * kP, p[1] * kP, p[2] * kP, p[3] * kP);
        }
        l_run = l_run * alpha + sum;

        // ---- O^T += V^T . P^T ----
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            o[dt] = o[dt] * alpha;
            o[dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf[dt], pf, o[dt], 0, 0, 0, kScaleOne, 0, kScaleOne);
        }
    }

    // ---- the waves' (m, l, O) merged through LDS: wave w finishes the channel tiles w, w + kAttnWaves, ... ----
    lds_m[wave][lane] = m_run;
    lds_l[wave][lane] = l_run;
#pragma unroll
    for (int dt = 0; dt < kDT; ++dt) lds_o[wave][dt][lane] = o[dt];
    __syncthreads();
    float M = kNegInf;
#pragma unroll
    for (int w = 0; w < kAttnWaves; ++w) M = fmaxf(M, lds_m[w][lane]);
    float f[kAttnWaves], L = 0.0f;
#pragma unroll
    for (int w = 0; w < kAttnWaves; ++w) {
        const float mw = lds_m[w][lane];
        f[w] = mw == kNegInf ? 0.0f : fast_exp2(mw - M);   // a wave without a step: weight 0, not exp2(-inf + inf)
        L = L + f[w] * lds_l[w][lane];
    }
    L = query_sum(L);
    constexpr float kInvP = 1.0f / (float)(1 << kAttnPScaleLog2);
    const int64_t row = row_q * a.Hq + hq;
    if (SPLIT && wave == 0 && g == 0 && q_live) {
        a.part_m[row * a.splits + split] = M;
        a.part_l[row * a.splits + split] = L;
    }
    const float v_scale = a.v_scale[a.scale_head ? h : 0];
    const bool empty = L == 0.0f;   // seq_len == 0 (a position's p at the maximum is 1): a zero row
    const float norm = SPLIT ? kInvP : (kInvP / L) * v_scale;
    for (int dt = wave; dt < kDT; dt += kAttnWaves) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < kAttnWaves; ++w) acc += lds_o[w][dt][lane] * f[w];
        if (!q_live) continue;
        const int d = 16 * dt + 4 * g;
        if (SPLIT) {
            *(f32x4 *)(a.part_o + (row * a.splits + split) * D + d) = acc * norm;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) store_from_float(a.out, row_q * a.ld_out + (int64_t)hq * D + d + j, empty ? 0.0f : acc[j] * norm, OUT);
        }
    }
}

// the split partials of one (sequence, query head) merged: one thread per channel
// MULTI: one workgroup per (sequence, token below max_q_len, query head); the tokens a sequence does not own leave, so no unowned row is written
template <int OUT, int D, bool MULTI>
__global__ __launch_bounds__(D) void attn_combine_kernel(const AttnArgs a)
{
    int64_t row = blockIdx.x;   // b Hq + hq
    int64_t b = row / a.Hq;
    const int hq = (int)(row - b * a.Hq), d = threadIdx.x;
    if (MULTI) {
        const int64_t seq_b = b / a.max_q_len, j = b - seq_b * a.max_q_len, c0 = a.cu[seq_b];
        b = c0 + j;   // the query row
        if (j >= (int64_t)a.cu[seq_b + 1] - c0 || b < 0 || b >= a.rows) return;
        row = b * a.Hq + hq;
    }
    const float *pm = a.part_m + row * a.splits, *pl = a.part_l + row * a.splits, *po = a.part_o + row * a.splits * D + d;
    float M = kNegInf;
    for (int s = 0; s < a.splits; ++s) M = fmaxf(M, pm[s]);
    float L = 0.0f, acc = 0.0f;
    for (int s = 0; s < a.splits; ++s) {
        const float ms = pm[s];
        const float w = ms == kNegInf ? 0.0f : fast_exp2(ms - M);   // a split that owns no position contributes zero, not a NaN
        L = L + w * pl[s];
        acc = acc + w * po[(int64_t)s * D];
    }
    const float v_scale = a.v_scale[a.scale_head ? hq / a.group : 0];
    store_from_float(a.out, b * a.ld_out + (int64_t)hq * D + d, L == 0.0f ? 0.0f : (acc / L) * v_scale, OUT);
}

}  // namespace

// host launcher (called from fp8mi_api.hip, which has validated the arguments and chosen `splits`; workspace: fp8mi_attn_workspace_bytes over
// `rows` query rows).  cu_seqlens_q == nullptr: the decode form, rows = B, one row per sequence.  Otherwise the multi-token form: rows = T
// and max_q_len >= 1.
int fp8mi_launch_paged_attention(const void *q, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, int Hkv, int D,
                                 int64_t ld_q, const uint8_t *k_cache, const uint8_t *v_cache, int64_t num_blocks, int block_size, const int32_t *block_table,
                                 int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len, const float *k_scale, const float *v_scale,
                                 int scale_head, float softmax_scale, int splits, void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s)
{
    const bool multi = cu_seqlens_q != nullptr;
    AttnArgs a = {};
    a.q = q; a.ld_q = ld_q; a.kc = k_cache; a.vc = v_cache; a.num_blocks = num_blocks;
    a.bt = block_table; a.ld_bt = ld_bt; a.max_blocks = max_blocks; a.seq_lens = seq_lens;
    a.k_scale = k_scale; a.v_scale = v_scale; a.scale_head = scale_head;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.Hkv = Hkv; a.group = Hq / Hkv; a.bs_log2 = fp8mi_attn_log2(block_size);
    a.splits = splits; a.chunk = fp8mi_attn_chunk(max_seq_len, splits);
    a.out = out; a.ld_out = ld_out;
    // the grids: B Hkv tiles splits workgroups (the API has refused that one with a message) and the combine's B max_q_len Hq, which is the
    // decode form's B Hq; either at or beyond 2^31 is refused
    const int64_t q_max = multi ? max_q_len : 1, qtiles = fp8mi_attn_q_tiles(q_max, Hq, Hkv);
    if (q_max < 1 || q_max > 0x7FFFFFFF || B * Hkv > 0x7FFFFFFF / qtiles || B * Hkv * qtiles > 0x7FFFFFFF / splits || rows * Hq > 0x7FFFFFFF ||
        B > 0x7FFFFFFF / q_max || B * q_max > 0x7FFFFFFF / Hq)
        return FP8MI_E_UNSUPPORTED;
    const int64_t grid = B * Hkv * qtiles * splits, combine_grid = B * q_max * Hq;
    if (multi) {
        a.cu = cu_seqlens_q; a.rows = rows; a.max_q_len = (int)q_max;
        a.tq = fp8mi_attn_tile_tokens(Hq, Hkv); a.qtiles = (int)qtiles;
    }
    if (splits > 1) {
        const int64_t parts = rows * Hq * splits;
        a.part_o = (float *)workspace;   // 16-byte stores: first
        a.part_m = a.part_o + parts * D;
        a.part_l = a.part_m + parts;
    }
    auto launch = [&](auto multi_t) {
        constexpr bool MULTI = decltype(multi_t)::value;
        return dispatch_in(q_dtype, [&](auto in_t) {
            return dispatch_int<64, 128>(D, [&](auto d_t) {
                constexpr int IN = decltype(in_t)::value, DD = decltype(d_t)::value;
                if (splits > 1) {
                    if (int rc = fp8mi_launch(attn_decode_kernel<IN, FP8MI_F32, DD, true, MULTI>, dim3((unsigned)grid), dim3(kAttnThreads), s, a)) return rc;
                    return dispatch_in(out_dtype, [&](auto out_t) {
                        return fp8mi_launch(attn_combine_kernel<decltype(out_t)::value, DD, MULTI>, dim3((unsigned)combine_grid), dim3(DD), s, a);
                    });
                }
                return dispatch_in(out_dtype, [&](auto out_t) {
                    return fp8mi_launch(attn_decode_kernel<IN, decltype(out_t)::value, DD, false, MULTI>, dim3((unsigned)grid), dim3(kAttnThreads), s, a);
                });
            });
        });
    };
    return multi ? launch(std::true_type{}) : launch(std::false_type{});
}
