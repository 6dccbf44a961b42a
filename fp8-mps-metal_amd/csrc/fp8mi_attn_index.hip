// The lightning indexer of the sparse MLA attention for gfx950 (include/fp8mi.h has the contract, DESIGN.md 5.25 the design): the FP8 index-key
// cache's append (fp8mi_mla_index_cache_append), the index logits (fp8mi_mla_index_logits) and the deterministic top-k selection
// (fp8mi_mla_index_topk) whose output is what fp8mi_mla_attention_sparse takes.
//
// The cache is ONE tensor uint8 [num_blocks, block_size 132]: bytes [0, 128 bs) of a block are its bs key rows of 128 e4m3 bytes, bytes
// [128 bs, 132 bs) their bs fp32 scales (a power of two each).  Slot s is row s % bs of block s / bs.
//
// Logits.  logits[t, p] = k_scale[p] sum_h w'[t, h] relu(q8[t, h, :] . k8[p, :]),  w' = weights qs, qs the dequantisation scale of the row's Q.
//   Work split   one workgroup of four waves per (sequence, group of kIdxTokens = 4 query tokens, chunk of positions).  The chunk is chosen
//                on the host for two workgroups per compute unit (fp8mi_mla_index_chunk); a wave takes the chunk's 64-position pieces
//                round-robin.  Positions are independent: no workspace, no combine.
//   Entry        the group's Q rows - (token, head), 128 channels, 16 lanes a row - are rounded to e4m3 with one amax per row (the MLA decode
//                entry's rule, the tiny-Q path included) and written to LDS ONCE, rows of 144 bytes (128 + 16: sixteen consecutive rows start
//                in sixteen different 16-byte bank groups); w' = weights qs goes beside them; the chunk's block-table entries are read once
//                per BLOCK, validated (-1: out of range) and kept in LDS, so no table load sits in the loop.
//   Product      v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales takes the whole 128-deep dot product of 16 heads x 16 positions.  Heads are
//                the ROWS (first operand, two ds_read_b128 from the Q rows), positions the COLUMNS (second operand): lane (r = lane & 15,
//                g = lane >> 4) hands in bytes 32 g + [0, 32) of key row r of the tile - two 16-byte loads straight from the cache, no LDS stage -
//                and receives heads 4 g + [0, 4) of position r.  ReLU and the head weights are then four FMAs in the lane, a running sum over
//                the Hi / 16 head tiles, and ONE add across the four lane groups per tile.  A piece is four tiles held in 32 registers; the next
//                piece's loads are issued ahead of this piece's products.  The group's tokens loop over the held piece - the context is read
//                once per token group - and a token skips pieces at or beyond its limit.  One Q fragment read serves four MFMAs.
//   Store        after the cross-lane add lane (r, g) keeps tile g: position 16 g + r of the piece, 64 consecutive floats a wave, times that
//                position's scale (loaded by the same lane).  A block whose table entry is out of range: 0.0f.
//   NaN          relu is `x < 0 ? 0 : x`: a NaN dot product stays NaN (fmaxf would drop it); a NaN scale times any sum is NaN.
//   Order        the head sum of a position is: per head tile in rising order, fma over heads 4 g + 0 .. 3; then (g ^ 0 + g ^ 1) + (g ^ 2 + g ^ 3)
//                over the lane groups - the same value in all four lanes.  Fixed: a call is bit-reproducible.
//
// Top-k.  One workgroup of 1024 threads per owned token.  A float becomes an order-preserving uint32 key (IEEE totalOrder, every NaN lowest);
// a radix select finds the key of the k-th largest element in up to three sweeps - digits of 11, 11 and 10 bits, histograms in LDS, the bucket
// found by one wave - and leaves early once a bucket fills the remainder exactly.  One ordered sweep then emits, in ascending position, the
// elements above the threshold and the first r ties: per 4096 elements eight wave ballots and one exchange of the waves' counts through LDS.
// Counts alone pass through the LDS atomics, so the output is a pure function of the row.

#include "fp8mi_encode.h"
#include "fp8mi_rowquant.h"
#include "fp8mi_attn.h"

namespace {

constexpr int kScaleOne = 0x7F7F7F7F;
constexpr int kIdxThreads = 64 * kIdxWaves;
constexpr int kIdxQPitch = kMlaIndexDim + 16;   // bytes of a Q row in LDS
constexpr int kIdxTiles = kIdxSuper / 16;       // 16-position MFMA tiles of a piece
static_assert(kIdxTiles == 4 && kMlaIndexDim == 128 && kIdxChunkMax % kIdxChunkUnit == 0, "a lane group keeps one tile of a piece; one MFMA is one dot product");

// ---- append: 32 lanes a token, four channels a lane ------------------------------------------------------------------------------------
constexpr int kIdxAppendThreads = 256;

struct IdxAppendArgs {
    const void *k;
    int64_t T, ld_k;
    int bs_log2;
    int64_t slots;   // num_blocks * block_size
    uint8_t *cache;
    const void *slot_mapping;
};

// the smallest power of two >= d (d >= 0, finite), not below 2^-126.  mx_rceil_biased (fp8mi_mx_exponent.h) is NOT this: it follows torch's
// fp32 log2, which rounds a few mantissa steps above a power of two DOWN to it - a scale below amax / 448.
FP8MI_DEVICE float pow2_at_least(float d)
{
    const uint32_t b = __float_as_uint(d);
    uint32_t e = (b >> 23) + ((b & 0x7FFFFFu) != 0u ? 1u : 0u);
    e = e < 1u ? 1u : e;
    return __uint_as_float(e << 23);
}

template <int IN, int MODE, bool SLOT64>
__global__ __launch_bounds__(kIdxAppendThreads) void mla_index_append_kernel(const IdxAppendArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * kIdxAppendThreads + threadIdx.x;
    int64_t t = idx >> 5;
    const int part = (int)(idx & 31);
    const bool in = t < a.T;   // every lane stays for the reduction
    t = in ? t : 0;
    float f[4];
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[j] = in ? InVec<IN>::load1(a.k, t * a.ld_k + 4 * part + j) : 0.0f;
        m = max(m, abs_bits(f[j]));   // bit patterns: a NaN is the largest
    }
    m = row16_umax(m);
    m = max(m, (uint32_t)__shfl_xor((int)m, 16, 64));
    if (!in) return;
    const int64_t slot = SLOT64 ? ((const int64_t *)a.slot_mapping)[t] : (int64_t)((const int32_t *)a.slot_mapping)[t];
    if (slot < 0 || slot >= a.slots) return;   // padding
    const float scale = m >= 0x7F800000u ? __uint_as_float(0x7FC00000u) : (m == 0u ? 1.0f : pow2_at_least(__uint_as_float(m) / 448.0f));
    const float prescale = __fdiv_rn(1.0f, scale);
    const int bs = 1 << a.bs_log2;
    uint8_t *block = a.cache + (slot >> a.bs_log2) * ((int64_t)kMlaIndexRow << a.bs_log2);
    const int row = (int)(slot & (bs - 1));
    *(uint32_t *)(block + row * kMlaIndexDim + 4 * part) = encode4<MODE>(f[0] * prescale, f[1] * prescale, f[2] * prescale, f[3] * prescale);
    if (part == 0) *(float *)(block + bs * kMlaIndexDim + 4 * row) = scale;
}

// ---- logits ----------------------------------------------------------------------------------------------------------------------------
struct IdxArgs {
    const void *q;
    const float *w;
    int64_t ld_q, ld_w;
    const uint8_t *cache;
    int64_t num_blocks;
    const int32_t *bt;
    int64_t ld_bt;
    const int32_t *seq_lens;
    const int32_t *cu;   // nullptr: one token per sequence, row b
    int64_t rows;        // T
    int max_q_len, Hi, bs_log2;
    int64_t cap;         // min(max_blocks block_size, max_seq_len): no limit is larger
    int chunk, chunks, groups;
    float *logits;
    int64_t ld_logits;
};

FP8MI_DEVICE float row16_max(float v)
{
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    return dpp_max<0x140>(v);
}

template <int IN>
__global__ __launch_bounds__(kIdxThreads) void mla_index_logits_kernel(const IdxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t q_lds[kIdxTokens * kIdxMaxHeads * kIdxQPitch];
    __shared__ __attribute__((aligned(16))) float w_lds[kIdxTokens * kIdxMaxHeads];
    __shared__ int32_t tab[kIdxChunkMax / 16];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int ck = (int)(blockIdx.x % (unsigned)a.chunks);
    const int64_t bg = blockIdx.x / (unsigned)a.chunks;
    const int grp = (int)(bg % a.groups);
    const int64_t b = bg / a.groups;
    const int bs = 1 << a.bs_log2;

    // ---- the group's tokens: j0 + [0, ntok) of sequence b, rows row0 + i, limits clamp(past + j0 + i) ----
    const int64_t seq = a.seq_lens[b];
    int64_t c0 = b, q_len = 1;
    if (a.cu) {
        c0 = a.cu[b];
        q_len = (int64_t)a.cu[b + 1] - c0;
        q_len = q_len < 0 ? 0 : q_len;
    }
    const int64_t owned = q_len < a.max_q_len ? q_len : a.max_q_len;   // tokens at or beyond max_q_len are not written
    const int64_t j0 = (int64_t)kIdxTokens * grp;
    if (j0 >= owned) return;   // before any barrier, every thread alike
    const int ntok = (int)(owned - j0 < kIdxTokens ? owned - j0 : kIdxTokens);
    const int64_t row0 = c0 + j0, past = seq - q_len + 1 + j0;
    auto limit_of = [&](int i) {   // 0 for a row outside [0, T)
        int64_t l = past + i;
        l = l < 0 ? 0 : (l > a.cap ? a.cap : l);
        return row0 + i >= 0 && row0 + i < a.rows ? l : 0;
    };
    int64_t hi = 0;
    for (int i = 0; i < ntok; ++i) hi = limit_of(i) > hi ? limit_of(i) : hi;
    const int64_t lo = (int64_t)ck * a.chunk;
    hi = hi < lo + a.chunk ? hi : lo + a.chunk;
    if (lo >= hi) return;   // the chunk lies beyond every limit of the group

    // ---- entry: Q rows to e4m3 in LDS, w' beside them, the chunk's table entries ----
    {
        const int l16 = tid & 15, nrows = ntok * a.Hi;
        for (int R = tid >> 4; R < ((nrows + 15) & ~15); R += kIdxThreads / 16) {   // whole rows of 16 lanes: the DPP reduction's lanes are all there
            const int i = R / a.Hi, head = R - i * a.Hi;
            const bool own = R < nrows && limit_of(i) > 0;
            const int64_t at = (row0 + i) * a.ld_q + (int64_t)head * kMlaIndexDim + 8 * l16;
            float v[8], amax = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[k] = own ? InVec<IN>::load1(a.q, at + k) : 0.0f;
                amax = fmaxf(amax, fabsf(v[k]));
            }
            amax = row16_max(amax);
            // the MLA decode entry's Q rule: 448 / amax overflows for a tiny row, which is multiplied by 2^64 first and 2^-64 goes into its scale
            const bool tiny = amax > 0.0f && amax < kAttnTinyQ;
            const float up = tiny ? kAttnTinyQUp : 1.0f;
            amax *= up;
            const float q_scale = amax > 0.0f ? amax / 448.0f : 1.0f, q_inv = amax > 0.0f ? 448.0f / amax : 1.0f;
            if (R < nrows) {
                const u32x2 bytes = {encode4<FP8MI_ENC_RNE>((v[0] * up) * q_inv, (v[1] * up) * q_inv, (v[2] * up) * q_inv, (v[3] * up) * q_inv),
                                     encode4<FP8MI_ENC_RNE>((v[4] * up) * q_inv, (v[5] * up) * q_inv, (v[6] * up) * q_inv, (v[7] * up) * q_inv)};
                *(u32x2 *)(q_lds + R * kIdxQPitch + 8 * l16) = bytes;
                if (l16 == 0) w_lds[R] = own ? a.w[(row0 + i) * a.ld_w + head] * (tiny ? q_scale * (1.0f / kAttnTinyQUp) : q_scale) : 0.0f;
            }
        }
        const int nblk = (int)((hi - lo + bs - 1) >> a.bs_log2);
        const int32_t *table = a.bt + b * a.ld_bt + (lo >> a.bs_log2);
        for (int k = tid; k < nblk; k += kIdxThreads) {
            const int32_t e = table[k];
            tab[k] = e >= 0 && e < a.num_blocks ? e : -1;   // a needed entry out of range: zero logits
        }
    }
    __syncthreads();

    // ---- a piece: the lane's 32 bytes of four tiles' rows, and the scale of the position it stores ----
    const int64_t block_bytes = (int64_t)kMlaIndexRow << a.bs_log2;
    auto fetch = [&](int64_t p0, u32x4 (&kf)[kIdxTiles][2], float &sc, bool &ok) {
#pragma unroll
        for (int t = 0; t < kIdxTiles; ++t) {
            const int64_t tp = p0 + 16 * t;   // a tile lies inside one block
            kf[t][0] = kf[t][1] = u32x4{0u, 0u, 0u, 0u};
            if (tp < hi) {   // wave-uniform: a tile at or beyond the group's last limit reads nothing
                const int32_t e = __builtin_amdgcn_readfirstlane(tab[(tp - lo) >> a.bs_log2]);
                if (e >= 0) {
                    const u32x4 *src = (const u32x4 *)(a.cache + e * block_bytes + (((int)tp & (bs - 1)) + r) * kMlaIndexDim + 32 * g);
                    kf[t][0] = __builtin_nontemporal_load(src);
                    kf[t][1] = __builtin_nontemporal_load(src + 1);
                }
            }
        }
        const int64_t ps = p0 + 16 * g + r;
        sc = 0.0f;
        ok = false;
        if (ps < hi) {
            const int32_t e = tab[(ps - lo) >> a.bs_log2];
            ok = e >= 0;
            if (ok) sc = *(const float *)(a.cache + e * block_bytes + bs * kMlaIndexDim + 4 * ((int)ps & (bs - 1)));
        }
    };
    const int nht = a.Hi >> 4;
    auto products = [&](int64_t p0, const u32x4 (&kf)[kIdxTiles][2], float sc, bool ok) {
        i32x8 kb[kIdxTiles];
#pragma unroll
        for (int t = 0; t < kIdxTiles; ++t)
            kb[t] = i32x8{(int)kf[t][0][0], (int)kf[t][0][1], (int)kf[t][0][2], (int)kf[t][0][3], (int)kf[t][1][0], (int)kf[t][1][1], (int)kf[t][1][2], (int)kf[t][1][3]};
        const int64_t ps = p0 + 16 * g + r;
        for (int i = 0; i < ntok; ++i) {
            const int64_t lim = limit_of(i);
            if (p0 >= lim) continue;   // wave-uniform: this token has no position in the piece
            float sum[kIdxTiles] = {0.0f, 0.0f, 0.0f, 0.0f};
            const uint8_t *qrow = q_lds + (i * a.Hi + r) * kIdxQPitch + 32 * g;
            const float *wrow = w_lds + i * a.Hi + 4 * g;
            for (int ht = 0; ht < nht; ++ht) {
                const u32x4 x0 = *(const u32x4 *)(qrow + 16 * ht * kIdxQPitch), x1 = *(const u32x4 *)(qrow + 16 * ht * kIdxQPitch + 16);
                const f32x4 w = *(const f32x4 *)(wrow + 16 * ht);
                const i32x8 qa = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
#pragma unroll
                for (int t = 0; t < kIdxTiles; ++t) {
                    const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qa, kb[t], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kScaleOne, 0, kScaleOne);
#pragma unroll
                    for (int j = 0; j < 4; ++j) sum[t] = __builtin_fmaf(w[j], acc[j] < 0.0f ? 0.0f : acc[j], sum[t]);   // a NaN stays
                }
            }
            float v = 0.0f;
#pragma unroll
            for (int t = 0; t < kIdxTiles; ++t) {
                float s = sum[t] + __shfl_xor(sum[t], 16, 64);
                s = s + __shfl_xor(s, 32, 64);
                v = g == t ? s : v;
            }
            if (ps < lim) a.logits[(row0 + i) * a.ld_logits + ps] = ok ? v * sc : 0.0f;
        }
    };

    u32x4 cur[kIdxTiles][2], nxt[kIdxTiles][2];
    float sc_cur, sc_nxt = 0.0f;
    bool ok_cur, ok_nxt = false;
    int64_t p0 = lo + (int64_t)kIdxSuper * wave;
    if (p0 >= hi) return;   // no barrier below
    fetch(p0, cur, sc_cur, ok_cur);
    for (; p0 < hi; p0 += kIdxChunkUnit) {
        const bool more = p0 + kIdxChunkUnit < hi;
        if (more) fetch(p0 + kIdxChunkUnit, nxt, sc_nxt, ok_nxt);   // in flight under this piece's products
        products(p0, cur, sc_cur, ok_cur);
#pragma unroll
        for (int t = 0; t < kIdxTiles; ++t) cur[t][0] = nxt[t][0], cur[t][1] = nxt[t][1];
        sc_cur = sc_nxt;
        ok_cur = ok_nxt;
    }
}

// ---- top-k -----------------------------------------------------------------------------------------------------------------------------
struct TopkArgs {
    const float *logits;
    int64_t ld_logits, n_cols;
    int64_t rows;
    const int32_t *cu;
    int max_q_len;
    const int32_t *seq_lens;
    int topk;
    int32_t *indices;
    int64_t ld_idx;
};

constexpr int kTopkWaves = kIdxTopkThreads / 64;
constexpr int kTopkBins = 2048;
constexpr int kTopkPer = 8;    // elements a thread takes per step of a histogram sweep
constexpr int kTopkEmit = 4;   // consecutive elements a thread takes per step of the emit sweep

// IEEE totalOrder on the bits as an unsigned order, every NaN below -inf (-inf is 0x007FFFFF)
FP8MI_DEVICE uint32_t order_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kIdxTopkThreads) void mla_index_topk_kernel(const TopkArgs a)
{
    __shared__ uint32_t hist[kTopkBins];
    __shared__ uint32_t found[3];                 // the bucket's digit, the elements in buckets above it, the bucket's count
    __shared__ uint32_t counts[2][kTopkWaves][2];   // per sweep parity and wave: elements above the threshold, ties

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t b = blockIdx.x, row = blockIdx.x, limit;
    if (a.cu) {
        b = blockIdx.x / (unsigned)a.max_q_len;
        const int64_t j = blockIdx.x - b * a.max_q_len, c0 = a.cu[b], q_len = (int64_t)a.cu[b + 1] - c0;
        row = c0 + j;
        if (j >= q_len || row < 0 || row >= a.rows) return;   // nobody's row: before any barrier, every thread alike
        limit = (int64_t)a.seq_lens[b] - q_len + j + 1;
    } else {
        limit = a.seq_lens[b];
    }
    limit = limit < 0 ? 0 : (limit > a.n_cols ? a.n_cols : limit);
    const int n = (int)limit, k = a.topk;
    const float *x = a.logits + row * a.ld_logits;
    int32_t *out = a.indices + row * a.ld_idx;
    if (n <= k) {   // everything is selected
        for (int i = tid; i < k; i += kIdxTopkThreads) out[i] = i < n ? i : -1;
        return;
    }

    // ---- radix select: the k-th largest key is `prefix` in the bits above `shift`; kk of the elements that share the prefix are selected ----
    uint32_t prefix = 0u, kk = (uint32_t)k;
    int shift = 32;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = pass < 2 ? 11 : 10, bins = 1 << bits, above_shift = shift;
        shift -= bits;
        for (int i = tid; i < bins; i += kIdxTopkThreads) hist[i] = 0u;
        __syncthreads();
        for (int base = 0; base < n; base += kTopkPer * kIdxTopkThreads) {   // kTopkPer loads in flight ahead of the LDS atomics, which would order them
            float v[kTopkPer];
#pragma unroll
            for (int u = 0; u < kTopkPer; ++u) {
                const int i = base + u * kIdxTopkThreads + tid;
                v[u] = i < n ? x[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kTopkPer; ++u) {
                const uint32_t key = order_key(v[u]);
                if (base + u * kIdxTopkThreads + tid < n && (pass == 0 || (key >> above_shift) == prefix)) atomicAdd(&hist[(key >> shift) & (uint32_t)(bins - 1)], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {   // lane l owns the bins [bins - per (l + 1), bins - per l): lane 0 the highest
            const int per = bins >> 6, top = bins - per * lane;
            uint32_t mine = 0u;
            for (int i = 1; i <= per; ++i) mine += hist[top - i];
            uint32_t incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                incl += lane >= d ? up : 0u;
            }
            uint32_t above = incl - mine;   // elements in the bins above this lane's
            if (above < kk && kk <= incl) {   // one lane: the bucket is among its bins
                for (int i = 1; i <= per; ++i) {
                    const uint32_t c = hist[top - i];
                    if (above + c >= kk) {
                        found[0] = (uint32_t)(top - i), found[1] = above, found[2] = c;
                        break;
                    }
                    above += c;
                }
            }
        }
        __syncthreads();
        prefix = (prefix << bits) | found[0];
        kk -= found[1];
        if (found[2] == kk) break;   // the bucket fills the remainder exactly: all of it is selected, no deeper digit is needed
    }
    // here: selected = the elements with (key >> shift) > prefix, and the first kk by position of those with (key >> shift) == prefix

    // ---- the ordered emit ----
    uint32_t done = 0u, ties = 0u;   // emitted so far, ties seen so far: the same in every thread
    const uint64_t below = ((uint64_t)1 << lane) - 1u;
    for (int base = 0, sweep = 0; base < n && done < (uint32_t)k; base += kTopkEmit * kIdxTopkThreads, ++sweep) {
        const int i0 = base + kTopkEmit * tid;   // position order is wave, lane, element
        bool is_above[kTopkEmit], is_tie[kTopkEmit];
        uint32_t wave_above = 0u, wave_ties = 0u, my_above = 0u, my_ties = 0u;   // of the wave; of the lanes below this one
#pragma unroll
        for (int e = 0; e < kTopkEmit; ++e) {
            const uint32_t hk = i0 + e < n ? order_key(x[i0 + e]) >> shift : 0u;
            is_above[e] = i0 + e < n && hk > prefix;
            is_tie[e] = i0 + e < n && hk == prefix;
            const uint64_t va = __ballot(is_above[e]), vt = __ballot(is_tie[e]);
            wave_above += (uint32_t)__popcll(va), wave_ties += (uint32_t)__popcll(vt);
            my_above += (uint32_t)__popcll(va & below), my_ties += (uint32_t)__popcll(vt & below);
        }
        if (lane == 0) counts[sweep & 1][wave][0] = wave_above, counts[sweep & 1][wave][1] = wave_ties;
        __syncthreads();   // one barrier a sweep: the other parity is not written before every wave has read this one's predecessor
        uint32_t before = 0u, ties_before = 0u, all = 0u, all_ties = 0u;   // of the earlier waves of this sweep; of the whole sweep
#pragma unroll
        for (int w = 0; w < kTopkWaves; ++w) {
            const uint32_t ca = counts[sweep & 1][w][0], ct = counts[sweep & 1][w][1];
            const uint32_t room = kk > ties + all_ties ? kk - (ties + all_ties) : 0u;   // ties still to take when wave w starts
            if (w == wave) before = all, ties_before = all_ties;
            all += ca + (ct < room ? ct : room);
            all_ties += ct;
        }
        const uint32_t room = kk > ties + ties_before ? kk - (ties + ties_before) : 0u;
#pragma unroll
        for (int e = 0; e < kTopkEmit; ++e) {
            if (is_above[e] || (is_tie[e] && my_ties < room)) out[done + before + my_above + (my_ties < room ? my_ties : room)] = i0 + e;
            my_above += is_above[e] ? 1u : 0u;
            my_ties += is_tie[e] ? 1u : 0u;
        }
        done += all;
        ties += all_ties;
    }
}

}  // namespace

// host launchers (called from fp8mi_api.hip, which has validated the arguments)
int fp8mi_launch_mla_index_cache_append(const void *k, int dtype, int64_t T, int64_t ld_k, uint8_t *cache, int64_t num_blocks, int block_size, const void *slot_mapping,
                                        int slot_bytes, int mode, hipStream_t s)
{
    const IdxAppendArgs a{k, T, ld_k, fp8mi_attn_log2(block_size), num_blocks * block_size, cache, slot_mapping};
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            constexpr int IN = decltype(in_t)::value, MODE = decltype(mode_t)::value;
            if (slot_bytes == 8) return fp8mi_launch_items(mla_index_append_kernel<IN, MODE, true>, T * 32, kIdxAppendThreads, kIdxAppendThreads, s, a);
            return fp8mi_launch_items(mla_index_append_kernel<IN, MODE, false>, T * 32, kIdxAppendThreads, kIdxAppendThreads, s, a);
        });
    });
}

// rows = T query rows; cu_seqlens_q == nullptr: one token per sequence (rows = B, max_q_len = 1).  B ceil(max_q_len / 4) chunks workgroups
int fp8mi_launch_mla_index_logits(const void *q, int q_dtype, const float *weights, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hi,
                                  int64_t ld_q, int64_t ld_w, const uint8_t *cache, int64_t num_blocks, int block_size, const int32_t *block_table, int64_t ld_bt,
                                  int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len, float *logits, int64_t ld_logits, hipStream_t s)
{
    const int64_t cap = max_blocks * block_size < max_seq_len ? max_blocks * block_size : max_seq_len;
    if (cap <= 0) return 0;   // every limit is zero: nothing is written
    const int64_t groups = fp8mi_mla_index_token_groups(max_q_len);
    if (max_q_len < 1 || max_q_len > 0x7FFFFFFF || B > 0x7FFFFFFF / groups) return FP8MI_E_UNSUPPORTED;
    const int64_t chunk = fp8mi_mla_index_chunk(B * groups, cap, fp8mi_cu_count()), chunks = (cap + chunk - 1) / chunk;
    if (B * groups > 0x7FFFFFFF / chunks) return FP8MI_E_UNSUPPORTED;
    const IdxArgs a{q, weights, ld_q, ld_w, cache, num_blocks, block_table, ld_bt, seq_lens, cu_seqlens_q, rows, (int)max_q_len, Hi, fp8mi_attn_log2(block_size),
                    cap, (int)chunk, (int)chunks, (int)groups, logits, ld_logits};
    return dispatch_in(q_dtype, [&](auto in_t) {
        return fp8mi_launch(mla_index_logits_kernel<decltype(in_t)::value>, dim3((unsigned)(B * groups * chunks)), dim3(kIdxThreads), s, a);
    });
}

int fp8mi_launch_mla_index_topk(const float *logits, int64_t ld_logits, int64_t n_cols, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len,
                                const int32_t *seq_lens, int64_t topk, int32_t *indices, int64_t ld_idx, hipStream_t s)
{
    if (max_q_len < 1 || max_q_len > 0x7FFFFFFF || B > 0x7FFFFFFF / max_q_len) return FP8MI_E_UNSUPPORTED;
    const TopkArgs a{logits, ld_logits, n_cols, rows, cu_seqlens_q, (int)max_q_len, seq_lens, (int)topk, indices, ld_idx};
    return fp8mi_launch(mla_index_topk_kernel, dim3((unsigned)(B * max_q_len)), dim3(kIdxTopkThreads), s, a);
}
