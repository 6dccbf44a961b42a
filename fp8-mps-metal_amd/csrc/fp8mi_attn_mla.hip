// Multi-head latent attention (MLA) over an FP8 latent KV cache for gfx950: the cache's append (fp8mi_mla_cache_append) and weight-absorbed
// decode attention, one query token per sequence (fp8mi_mla_attention_decode; include/fp8mi.h has the contract, DESIGN.md 5.22 the design).
//
// The cache is ONE tensor [num_blocks, block_size, 576] of e4m3 bytes: bytes [0, 512) of a row are the compressed latent c_kv, bytes
// [512, 576) the rotary key k_pe.  A row is the "K" of the scores (all 576 channels) and its first 512 bytes are the "V" of the output: there
// is no second, transposed copy.
//
// Work split.  One workgroup of four waves per (sequence, tile of kMlaHeadTile = 64 heads, split).  Wave w owns the 16 MFMA columns of heads
// 64 tile + 16 w + [0, 16); columns at or beyond Hq are zero and never stored; a wave with no live column stages and meets the barrier, no
// more.  One wave walks ALL 128-position steps of its split in order: no cross-wave (m, l, O) merge.
//
// Staging.  A step's 128 rows of 576 bytes (72 KiB) are read from memory once per workgroup: 4608 16-byte loads, 18 a thread, the step's
// block-table entries all read first and the loads issued behind one wait for them, through registers into one of two LDS stages.  The loads
// of step n + 1 are issued ahead of the products of step n and written to the other stage behind them, one barrier per step.  Rows at or
// beyond the split's last position are written as zeros and never read from memory - neither the row nor its table entry.
//   LDS: rows of kMlaPitch = 592 bytes (576 + 16: 148 dwords, 20 mod 64 banks), 2 x 128 x 592 = 148 KiB of gfx950's 160.  Sixteen consecutive
//   rows then start in sixteen different 16-byte bank groups, which is what both kinds of read below touch at a time.
//
// Products, per wave and step (softmax arithmetic as in fp8mi_attn_decode.hip, as written there):
//   Q    [q_lat | q_pe] quantised to e4m3 per (sequence, head) row with ONE amax over the 576 channels, the tiny-Q path included; five
//        K-steps of the scaled MFMA, the fifth the 64 rope bytes and 64 zero bytes;
//   S^T  [16 pos][16 heads] = rows . Q^T, eight tiles of 5 v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales; a row's fragment is two
//        ds_read_b128 per K-step (bytes 128 ks + 16 g + [0, 16) and 64 more), one for the fifth.  Tile t takes the LDS rows
//        16 t + (m ^ 8 (t & 1)), m = lane & 15 (below);
//   softmax online in fp32, base 2, P = rne(p 2^8) packed to e4m3, l from the fp32 p;
//   O^T  [16 ch][16 heads] += V^T . P^T for 32 channel tiles (128 accumulator registers).  The first operand wants a channel's 128 positions
//        contiguous in a lane while the rows keep channels contiguous: it is read from the SAME rows with gfx950's LDS transpose read
//        ds_read_b64_tr_b8.  Within 16 lanes, source lane 2 e + hh hands in the 8 bytes of (position e of eight, channel half hh) and
//        destination lane c receives channel c of the 16 at the eight positions, position e in byte e (profiles/mla_transpose_map.txt).
//        Four such reads are a lane's 32-byte operand: slots 64 h + 16 g + 8 u + [0, 8) for (h, u) in 2 x 2.
// The row order of the S tiles is free (it is only an LDS address), so slot 64 h + 16 g + 8 u + e is position
//   pi = (e & 3) + 4 (g & 1) + 8 ((g >> 1) ^ (e >> 2)) + 16 (e >> 2) + 32 u + 64 h
// of the step: the packed S registers of tile t (rows 16 t + (m ^ 8 (t & 1))) then ARE dword t of the P operand with no lane movement, the
// 16 rows of an S read are consecutive, and the 16 rows two neighbouring lane groups hand a transpose read are distinct mod 16.
//
// Isolation.  V is taken from the staged rows, and rows at or beyond the split's end are zeros there: zero V, and p = 0 from the score
// select (-inf), so no V byte mask is needed.  Nothing at or beyond seq_len is read; a needed table entry out of range contributes zero
// rows; NaN bytes inside [0, seq_len) poison their sequence.
// Unsplit: O / (2^8 l) kv_scale is stored.  Split: (m, l, O / 2^8) go to the workspace in fp8mi_attn_decode.hip's layout and its
// attn_combine_kernel (D = 512 instance) merges them.
//
// The multi-token form (fp8mi_mla_attention_varlen, template flag MULTI on the same body): the 64 columns are (token, head)
// pairs of one sequence, each with its own causal limit, and every output row equals the decode kernel on a sequence cut at that limit, bit
// for bit.  What differs is said at mla_attention_body.
//
// The sparse form (fp8mi_mla_attention_sparse, template flag SPARSE on the same body): every query token attends the rows its
// own index list names - indices[t, 0 .. topk) are logical positions of the token's sequence, valid iff 0 <= index < the token's limit - so
// one workgroup serves ONE token (and 64 of its heads, and one split of its LIST), a step is 128 list entries, and each of the 128 staged
// rows has an address of its own.  Everything behind the stage is the decode text; what is new is in front of it:
//   resolve   thread e < 128 (waves 0 and 1) turns entry e of a step into the physical cache row number
//             block_table[b, index >> log2 bs] block_size + (index & (bs - 1)), or -1 (an invalid entry, whose table entry is not read, or a
//             table entry out of range: a zero row), and the two waves' ballots of "valid" into the step's 128-bit mask.  Both go to a ring of
//             three entries (128 int32 + 16 bytes each, 1584 bytes behind the two stages).  The two dependent round trips - index, then table
//             entry - are taken in DIFFERENT iterations of the step loop, each under work that hides it: in iteration n the index of step
//             n + 3 is loaded ahead of the products of step n and turned into (valid, offset in block, table load) behind them; the table
//             value is awaited in iteration n + 1 BEHIND the issue of that iteration's row loads, and entry n + 3 of the ring is written
//             there.  fetch(n + 3) runs in iteration n + 2 and finds plain row numbers in LDS: no memory round trip sits between a barrier
//             and the row loads.  Through the products one value lives (the index), across the barrier two and the ballot (scalar).
//   hazards   entry k of the ring is WRITTEN in iteration k - 2, its rows are READ by fetch(k) in iteration k - 1 and its mask by the
//             products of step k in iteration k; every iteration ends in the one barrier.  The write is behind barrier k - 3 and ahead of
//             barrier k - 2, every read of it behind barrier k - 2: written before read.  The slot's previous occupant is entry k - 3, last
//             read (its mask) in iteration k - 3, that is ahead of barrier k - 3, which the writer has passed: no wave can still be reading
//             what is overwritten.  Three entries are the fewest: k - 2, k - 1 and k are occupied at once.  No barrier is added to the loop.
//   mask      a lane reads the step's 128 bits once (one broadcast ds_read_b128), packs the 32 of ITS S registers - tile t, register j is
//             row 16 t + ((4 g + j) ^ 8 (t & 1)): the nibble at bit 16 (t & 1) + (4 g ^ 8 (t & 1)) of word t >> 1 - into one register, and the
//             score select takes bit 4 t + j in place of `pos < live_to`.  Invalid rows are committed as zeros: no V mask.  A step without a
//             valid entry is staged and not multiplied (the mask is the workgroup's: wave-uniform).
// For a list valid up to n and invalid from there on, a token's row is the decode kernel's on the compacted cache, bit for bit.

#include "fp8mi_encode.h"
#include "fp8mi_attn.h"

int fp8mi_launch_mla_combine(int64_t B, int Hq, const float *kv_scale, int splits, void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s);
int fp8mi_launch_mla_combine_varlen(int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq, const float *kv_scale, int splits, void *workspace,
                                    void *out, int out_dtype, int64_t ld_out, hipStream_t s);

namespace {

constexpr int kScaleOne = 0x7F7F7F7F;
constexpr int kMlaThreads = 64 * kMlaWaves;
constexpr int kMlaPitch = kMlaRow + 16;                   // bytes of an LDS row
constexpr int kMlaStage = kAttnStep * kMlaPitch;          // bytes of a stage
constexpr int kMlaChunks = kMlaRow / 16;                  // 16-byte chunks of a row: 36
constexpr int kMlaLoads = kAttnStep * kMlaChunks / kMlaThreads;   // per thread and step: 18
constexpr int kMlaDT = kMlaLatent / 16;                   // 16-channel tiles of O: 32
constexpr int kMlaKS = kMlaLatent / 128;                  // full K-steps of a score: 4, and the rope step
constexpr float kNegInf = -__builtin_huge_valf();
// the sparse form's ring of resolved steps, behind the two stages: per entry the 128 physical row numbers and the 128-bit validity mask
constexpr int kMlaRing = 3;
constexpr int kMlaRingEntry = kAttnStep * 4 + 16;
static_assert(2 * kMlaStage + kMlaRing * kMlaRingEntry <= 160 * 1024 && (2 * kMlaStage) % 16 == 0 && kMlaRingEntry % 16 == 0 && kAttnStep == 128, "the ring beside the stages");
static_assert(kAttnStep * kMlaChunks % kMlaThreads == 0 && 2 * kMlaStage <= 160 * 1024 && kMlaRope == 64, "the staging split and the two stages");

struct MlaArgs {
    const void *q_lat, *q_pe;
    int64_t ld_ql, ld_qp;
    const uint8_t *cache;
    int64_t num_blocks;
    const int32_t *bt;
    int64_t ld_bt, max_blocks;
    const int32_t *seq_lens;
    const float *kv_scale;
    float scale_log2;   // softmax_scale log2 e
    int Hq, tiles, bs_log2;
    int splits;
    int64_t chunk;      // positions per split, a multiple of kAttnStep
    float *part_m, *part_l, *part_o;
    void *out;
    int64_t ld_out;
    // the multi-token form (fp8mi_mla_attention_varlen; nullptr / 0 in the decode form)
    const int32_t *cu;   // [B + 1]: sequence b owns query rows [cu[b], cu[b + 1])
    int64_t rows;        // T: a row at or beyond it is neither read nor written
    int max_q_len;       // host bound of a sequence's query tokens, at most T
    // the sparse form (fp8mi_mla_attention_sparse): cu may be nullptr there (one token per sequence, rows = B); chunk counts list entries
    const int32_t *indices;   // (T, topk), row stride ld_idx
    int64_t ld_idx;
    int topk;
};

FP8MI_DEVICE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
FP8MI_DEVICE float xor_lanes(float v, int mask) { return __shfl_xor(v, mask, 64); }
// over the four lanes that hold one query (lane & 15 alike)
FP8MI_DEVICE float query_max(float v) { v = fmaxf(v, xor_lanes(v, 16)); return fmaxf(v, xor_lanes(v, 32)); }
FP8MI_DEVICE float query_sum(float v) { v = v + xor_lanes(v, 16); return v + xor_lanes(v, 32); }

typedef int i32x2 __attribute__((ext_vector_type(2)));
FP8MI_DEVICE i32x2 lds_read_tr8(const uint8_t *p) { return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)p); }

// The body of both kernels below.  MULTI (fp8mi_mla_attention_varlen): the workgroup's 64 columns are the (token, head)
// pairs col = 64 tile + 16 wave + r = j Hq + h of ONE sequence's query tokens, each with its own causal limit; a.tiles is
// ceil(max_q_len Hq / 64).  The workgroup stages up to the largest limit of its columns, a wave multiplies up to the largest of its own, a
// lane masks by its column's.  The decode instances compile without a trace of it.
// SPARSE (fp8mi_mla_attention_sparse; never with MULTI): the workgroup is one (sequence, token, head tile, split of the token's
// index list); lo, hi and the steps count LIST entries; the header comment has the resolve-ahead staging.  Without a trace in the others.
template <int IN, int OUT, bool SPLIT, bool MULTI, bool SPARSE = false>
FP8MI_DEVICE void mla_attention_body(const MlaArgs &a)
{
    static_assert(!(MULTI && SPARSE), "a sparse workgroup holds one token");
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kMlaStage + (SPARSE ? kMlaRing * kMlaRingEntry : 0)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int split = (int)(blockIdx.x % (unsigned)a.splits);
    const int64_t bt_ = blockIdx.x / (unsigned)a.splits;
    const int tile = (int)(bt_ % a.tiles);
    const int64_t b = SPARSE ? bt_ / a.tiles / a.max_q_len : bt_ / a.tiles;   // SPARSE: (sequence, token j below max_q_len)
    const int bs = 1 << a.bs_log2;

    int64_t seq = a.seq_lens[b];
    const int64_t cap = a.max_blocks << a.bs_log2;   // the table holds no more
    const int64_t lo = (int64_t)split * a.chunk;
    // what a decode call with seq_len = `limit` takes of this split: its end
    auto split_end = [&](int64_t limit) {
        limit = limit < 0 ? 0 : limit;
        limit = limit > cap ? cap : limit;
        return (split == a.splits - 1 || lo + a.chunk > limit) ? limit : lo + a.chunk;
    };
    int hq = kMlaHeadTile * tile + 16 * wave + r;   // MULTI: the column, then its head
    bool live = hq < a.Hq;
    bool wave_live = kMlaHeadTile * tile + 16 * wave < a.Hq;   // wave-uniform
    int64_t row_q = b;        // the query row: q and out at row_q ld, partials at row_q Hq + hq
    int64_t hi_tile;          // the workgroup stages [lo, hi_tile)
    int64_t hi_wave = 0;      // MULTI: the largest split end among this wave's columns (wave-uniform)
    int rem_col = 0;          // MULTI: this column's split end less lo, 0 if it ends at or below lo (an int32: seq_lens is)
    // MULTI: (token, head) and the query row of column col0 + c of this workgroup; false: a column nobody owns.  Derived here for Q and the
    // limit and AGAIN for the stores (from an opaque copy of the thread index), so that none of it lives through the loop.
    int64_t c0 = 0, cols = 0;
    const int64_t col0 = (int64_t)kMlaHeadTile * tile;
    auto column = [&](int c, int &j, int &head, int64_t &row) {
        const int64_t col = col0 + c;
        j = (int)(col / a.Hq);
        head = (int)(col - (int64_t)j * a.Hq);
        row = c0 + j;
        const bool own = col < cols && row >= 0 && row < a.rows;
        if (!own) row = 0, head = 0;
        return own;
    };
    if constexpr (MULTI) {
        c0 = a.cu[b];
        int64_t q_len = (int64_t)a.cu[b + 1] - c0;
        q_len = q_len < 0 ? 0 : q_len;
        cols = (q_len < a.max_q_len ? q_len : a.max_q_len) * a.Hq;   // tokens at or beyond max_q_len are not written
        if (col0 >= cols) return;   // nothing of this tile is owned: before any barrier, every thread alike
        const int64_t past = seq - q_len + 1;   // token j attends [0, past + j)
        const int64_t last = (col0 + kMlaHeadTile <= cols ? col0 + kMlaHeadTile : cols) - 1;
        hi_tile = split_end(past + last / a.Hq);
        const int64_t wcol0 = col0 + 16 * __builtin_amdgcn_readfirstlane(wave);
        wave_live = wcol0 < cols;
        if (wave_live) hi_wave = split_end(past + ((wcol0 + 16 <= cols ? wcol0 + 16 : cols) - 1) / a.Hq);
        int j;
        live = column(16 * wave + r, j, hq, row_q);
        const int64_t end = live ? split_end(past + j) : 0;
        rem_col = end > lo ? (int)(end - lo) : 0;
    } else if constexpr (SPARSE) {
        if (a.cu) {   // token j of sequence b: a token the sequence does not own leaves before any barrier, every thread alike
            const int64_t j = bt_ / a.tiles - b * a.max_q_len;
            c0 = a.cu[b];
            const int64_t q_len = (int64_t)a.cu[b + 1] - c0;
            row_q = c0 + j;
            if (j >= q_len || row_q < 0 || row_q >= a.rows) return;
            seq = seq - q_len + j + 1;
        }
        seq = seq < 0 ? 0 : seq;
        seq = seq > cap ? cap : seq;   // the token's limit: an int32, seq_lens is
        hi_tile = lo + a.chunk < a.topk ? lo + a.chunk : a.topk;
    } else {
        seq = seq < 0 ? 0 : seq;
        seq = seq > cap ? cap : seq;
        hi_tile = (split == a.splits - 1 || lo + a.chunk > seq) ? seq : lo + a.chunk;
    }
    const int64_t hi = hi_tile;
    const int32_t *table = a.bt + b * a.ld_bt;

    // ---- Q: this lane's bytes of its column's head, [q_lat | q_pe] quantised as one row ----
    i32x8 qf[kMlaKS + 1];
    float c;   // an S accumulator times c: the logit, base 2
    {
        // element i of this lane, K-step ks = i >> 5: channel 128 ks + 64 ((i >> 4) & 1) + 16 g + (i & 15); the last step: rope channel
        // 16 g + (i & 15).  Read twice - for the amax, then K-step by K-step for the bytes - so that 144 values are never live at once.
        const int64_t row_l = row_q * a.ld_ql + (int64_t)(live ? hq : 0) * kMlaLatent + 16 * g, row_p = row_q * a.ld_qp + (int64_t)(live ? hq : 0) * kMlaRope + 16 * g;
        auto q_at = [&](int i) {
            const float v = i < 32 * kMlaKS ? InVec<IN>::load1(a.q_lat, row_l + 128 * (i >> 5) + 64 * ((i >> 4) & 1) + (i & 15))
                                            : InVec<IN>::load1(a.q_pe, row_p + (i & 15));
            return live ? v : 0.0f;
        };
        float amax = 0.0f;
#pragma unroll 16
        for (int i = 0; i < 32 * kMlaKS + 16; ++i) amax = fmaxf(amax, fabsf(q_at(i)));
        amax = query_max(amax);
        // 448 / amax is +inf for 0 < amax < 448 / FLT_MAX: such a row and its amax are multiplied by 2^64 first - exact, subnormals
        // included - and 2^-64 goes into the logit scale.  No other row changes.
        const bool tiny = amax > 0.0f && amax < kAttnTinyQ;
        const float up = tiny ? kAttnTinyQUp : 1.0f;   // q times 1.0f is q
        amax *= up;
        const float q_scale = amax > 0.0f ? amax / 448.0f : 1.0f, q_inv = amax > 0.0f ? 448.0f / amax : 1.0f;
#pragma unroll
        for (int ks = 0; ks <= kMlaKS; ++ks) {
            qf[ks] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < (ks < kMlaKS ? 8 : 4); ++w) {
                const int i = 32 * ks + 4 * w;
                qf[ks][w] = (int)encode4<FP8MI_ENC_RNE>((q_at(i) * up) * q_inv, (q_at(i + 1) * up) * q_inv, (q_at(i + 2) * up) * q_inv, (q_at(i + 3) * up) * q_inv);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        c = (q_scale * a.kv_scale[0]) * a.scale_log2;
        if (tiny) c *= 1.0f / kAttnTinyQUp;
    }

    // ---- staging: global -> registers (fetch), registers -> LDS (commit) ----
    // The table entries of a step's 18 loads are read first, all of them, and the 16-byte loads issued back to back behind ONE wait for those.
    u32x4 st[kMlaLoads];
    // (row, chunk) of a load are derived from the thread index behind an opaque copy of it, inside the loop: hoisted out of it they are
    // loop-invariant registers, 36 of them, that spill
    auto opaque = [](int t) {
        asm volatile("" : "+v"(t));
        return t;
    };
    auto fetch = [&](int64_t p0) {
        const int tid = opaque((int)threadIdx.x);
        int32_t blk[kMlaLoads];
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int64_t pos = p0 + (i * kMlaThreads + tid) / kMlaChunks;
            blk[i] = pos < hi ? table[pos >> a.bs_log2] : -1;   // at or beyond hi: no table entry is read
        }
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int idx = i * kMlaThreads + tid, row = idx / kMlaChunks, ch = idx - row * kMlaChunks;
            const int64_t pos = p0 + row;
            st[i] = u32x4{0u, 0u, 0u, 0u};
            if (blk[i] >= 0 && blk[i] < a.num_blocks)
                st[i] = __builtin_nontemporal_load((const u32x4 *)(a.cache + (((int64_t)blk[i] << a.bs_log2) + (pos & (bs - 1))) * kMlaRow + 16 * ch));
        }
    };
    // ---- SPARSE: resolve (thread e < 128: entry e of a step), the ring, and the fetch that reads row numbers where the one above reads the table ----
    uint8_t *const ring = lds + 2 * kMlaStage;
    const int32_t *const list = SPARSE ? a.indices + row_q * a.ld_idx : nullptr;
    auto load_index = [&](int k) {   // entry e of step k; at or beyond the split's end (and a thread that resolves nothing): not read, -1
        const int e = opaque((int)threadIdx.x);
        const int64_t at = lo + (int64_t)k * kAttnStep + e;
        return e < kAttnStep && at < hi ? list[at] : -1;
    };
    // -> the table entry of a valid index (an invalid one reads none: -1); off: its offset in the block, -1 if invalid; vote: the wave's ballot
    auto look_up = [&](int32_t index, int32_t &off, uint64_t &vote) {
        const bool valid = (uint32_t)index < (uint32_t)(int32_t)seq;   // 0 <= index < limit
        vote = __ballot(valid);
        off = valid ? index & (bs - 1) : -1;
        return valid ? table[index >> a.bs_log2] : -1;
    };
    auto publish = [&](int k, int32_t off, int32_t entry, uint64_t vote) {
        const int tid = opaque((int)threadIdx.x);
        uint8_t *slot = ring + (k % kMlaRing) * kMlaRingEntry;
        if (tid < kAttnStep) {
            // a valid entry whose table entry is out of range: a zero row that is still scored (its mask bit is set)
            ((int32_t *)slot)[tid] = off >= 0 && entry >= 0 && entry < a.num_blocks ? (entry << a.bs_log2) + off : -1;
            if ((tid & 63) == 0) ((uint64_t *)(slot + 4 * kAttnStep))[tid >> 6] = vote;
        }
    };
    auto fetch_rows = [&](int k) {
        const int tid = opaque((int)threadIdx.x);
        const int32_t *rows = (const int32_t *)(ring + (k % kMlaRing) * kMlaRingEntry);
        int32_t rn[kMlaLoads];
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) rn[i] = rows[(i * kMlaThreads + tid) / kMlaChunks];
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int idx = i * kMlaThreads + tid, ch = idx - idx / kMlaChunks * kMlaChunks;
            st[i] = u32x4{0u, 0u, 0u, 0u};
            if (rn[i] >= 0) st[i] = __builtin_nontemporal_load((const u32x4 *)(a.cache + (int64_t)rn[i] * kMlaRow + 16 * ch));
        }
    };
    auto commit = [&](int stage) {
        const int tid = opaque((int)threadIdx.x);
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int idx = i * kMlaThreads + tid, row = idx / kMlaChunks, ch = idx - row * kMlaChunks;
            *(u32x4 *)(lds + stage * kMlaStage + row * kMlaPitch + 16 * ch) = st[i];
        }
    };
    // this lane's fragment offsets inside a stage.  S tile t: row 16 t + (r ^ 8 (t & 1)), bytes 16 g + [0, 16) of each 64.  The transpose read
    // (h, u): this lane as a SOURCE is position e of eight, channel half hh, of its lane group's slots 64 h + 16 g + 8 u + [0, 8).
    const int s_rd[2] = {r * kMlaPitch + 16 * g, (r ^ 8) * kMlaPitch + 16 * g};
    const int e = r >> 1, hh = r & 1;
    const int v_rd = ((e & 3) + 4 * (g & 1) + 8 * ((g >> 1) ^ (e >> 2)) + 16 * (e >> 2)) * kMlaPitch + 8 * hh;

    // MULTI: a column without a position in a step its wave walks - its limit ended a step earlier than a neighbour's, or lies at or below the
    // split's start - must keep its (m, l, O) exactly: alpha = 1, p = 0.  With m_run finite the text below does that by itself; at -inf it
    // would make exp2(-inf - -inf) = NaN of both.  So m_run starts at the lowest finite float there: alpha = exp2(0) and p = exp2(-inf) for such
    // a column, and alpha = exp2(-FLT_MAX - m) = 0 = exp2(-inf - m) at the column's first position, whose O and l are zeros anyway.
    // SPARSE: a list may be valid only behind a step of holes, and the text is shared: the same start
    float m_run = MULTI || SPARSE ? -__FLT_MAX__ : kNegInf, l_run = 0.0f;   // l_run: this lane's share of the row sum (its 32 positions of every step)
    f32x4 o[kMlaDT];
#pragma unroll
    for (int dt = 0; dt < kMlaDT; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int steps = hi > lo ? (int)((hi - lo + kAttnStep - 1) / kAttnStep) : 0;
    // SPARSE: what iteration n + 1 publishes as entry n + 3 of the ring, and the index loaded ahead of the products
    int32_t r_index = -1, r_off = -1, r_entry = -1;
    uint64_t r_vote = 0;
    if (steps > 0) {
        if constexpr (SPARSE) {
            // entries 0 and 1 whole and the table load of entry 2, the three steps' loads side by side: two round trips, once
            int32_t index[kMlaRing], off[kMlaRing], entry[kMlaRing];
            uint64_t vote[kMlaRing];
#pragma unroll
            for (int k = 0; k < kMlaRing; ++k) index[k] = load_index(k);
#pragma unroll
            for (int k = 0; k < kMlaRing; ++k) entry[k] = look_up(index[k], off[k], vote[k]);
            publish(0, off[0], entry[0], vote[0]);
            publish(1, off[1], entry[1], vote[1]);
            r_off = off[2], r_entry = entry[2], r_vote = vote[2];
            __syncthreads();
            fetch_rows(0);
        } else {
            fetch(lo);
        }
        commit(0);
        __syncthreads();
    }
    for (int n = 0; n < steps; ++n) {
        const int64_t p0 = lo + (int64_t)n * kAttnStep;
        const bool more = n + 1 < steps;
        const uint8_t *stage = lds + (n & 1) * kMlaStage;
        uint32_t bits = 0;   // SPARSE: bit 4 t + j: the row of S tile t, register j, is a valid entry
        bool any = true;     // SPARSE: the step holds one (workgroup-uniform)
        if constexpr (SPARSE) {
            if (more) fetch_rows(n + 1);                  // row numbers from LDS, resolved two iterations ago
            publish(n + 2, r_off, r_entry, r_vote);       // the table value was loaded an iteration ago, awaited behind the row loads' issue
            r_index = load_index(n + 3);                  // under the products
            const u32x4 w = *(const u32x4 *)(ring + (n % kMlaRing) * kMlaRingEntry + 4 * kAttnStep);
            any = __builtin_amdgcn_readfirstlane((int)(w[0] | w[1] | w[2] | w[3])) != 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) bits |= ((w[t >> 1] >> (16 * (t & 1) + ((4 * g) ^ (8 * (t & 1))))) & 0xFu) << (4 * t);
        } else {
            if (more) fetch(p0 + kAttnStep);   // in flight under this step's products and softmax
        }
        // MULTI: a step at or beyond every limit of this wave's columns is staged, not multiplied; SPARSE: nor is a step of holes
        if (wave_live && (!MULTI || p0 < hi_wave) && (!SPARSE || any)) {
            const int64_t below = hi - p0;
            int live_to = (int)(below > kAttnStep ? kAttnStep : below);   // positions of this step below the split's end
            if constexpr (MULTI) {   // below this COLUMN's end; zero or less: it has no position in a step its wave still walks
                live_to = rem_col - n * kAttnStep;
                live_to = live_to > kAttnStep ? kAttnStep : live_to;
            }
            float s[8][4], mx = kNegInf;
            // ---- S^T tiles ----
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint8_t *row = stage + s_rd[t & 1] + 16 * t * kMlaPitch;
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks <= kMlaKS; ++ks) {
                    const u32x4 x0 = *(const u32x4 *)(row + 128 * ks);
                    u32x4 x1 = {0u, 0u, 0u, 0u};
                    if (ks < kMlaKS) x1 = *(const u32x4 *)(row + 128 * ks + 64);
                    const i32x8 kf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
                    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[ks], acc, 0, 0, 0, kScaleOne, 0, kScaleOne);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int pos = 16 * t + ((4 * g + j) ^ (8 * (t & 1)));   // register j is row 4 g + j of the tile
                    const bool keep = SPARSE ? (bits >> (4 * t + j) & 1u) != 0 : pos < live_to;
                    s[t][j] = keep ? acc[j] * c : kNegInf;                   // a select: whatever a masked row computed is dropped
                    mx = fmaxf(mx, s[t][j]);
                }
                __builtin_amdgcn_sched_barrier(0);   // a tile's reads stay with its MFMAs: hoisted, the fragments of all eight spill
            }
            // ---- softmax: P in fp32 for the row sum, e4m3 of p 2^8 for the product ----
            const float m_new = fmaxf(m_run, query_max(mx));   // finite: a step holds at least one live position, unless NaN
            const float alpha = fast_exp2(m_run - m_new);
            m_run = m_new;
            i32x8 pf;
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                float p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p[j] = fast_exp2(s[t][j] - m_new);
                    sum = sum + p[j];
                }
                constexpr float kP = (float)(1 << kAttnPScaleLog2);
                pf[t] = (int)encode4<FP8MI_ENC_RNE>(p[0] * kP, p[1] * kP, p[2] * kP, p[3] * kP);
            }
            l_run = l_run * alpha + sum;
            // ---- O^T += V^T . P^T: the first operand through the transpose read of the same rows ----
#pragma unroll
            for (int dt = 0; dt < kMlaDT; ++dt) {
                i32x8 vf;
#pragma unroll
                for (int hu = 0; hu < 4; ++hu) {   // hu = 2 h + u: rows 64 h + 32 u further on
                    const i32x2 x = lds_read_tr8(stage + v_rd + 32 * hu * kMlaPitch + 16 * dt);
                    vf[2 * hu] = x[0];
                    vf[2 * hu + 1] = x[1];
                }
                o[dt] = o[dt] * alpha;
                o[dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf, o[dt], 0, 0, 0, kScaleOne, 0, kScaleOne);
                if ((dt & 1) == 1) __builtin_amdgcn_sched_barrier(0);   // two tiles' reads in flight, not thirty-two
            }
        }
        if constexpr (SPARSE) r_entry = look_up(r_index, r_off, r_vote);   // entry n + 3: its table load flies over the barrier
        if (more) commit((n + 1) & 1);   // the stage step n - 1 read: every wave has passed the barrier behind it
        __syncthreads();
    }

    // ---- the wave owns its columns' whole split: no merge ----
    constexpr float kInvP = 1.0f / (float)(1 << kAttnPScaleLog2);
    const float L = query_sum(l_run);
    if constexpr (MULTI) {
        int j;
        live = column(opaque((int)threadIdx.x) >> 6 << 4 | r, j, hq, row_q);
    }
    if (!live) return;
    const int64_t row = row_q * a.Hq + hq;
    if (SPLIT && g == 0) {
        a.part_m[row * a.splits + split] = (MULTI || SPARSE) && L == 0.0f ? kNegInf : m_run;   // a split that owns no position: m = -inf, l = 0, O = 0
        a.part_l[row * a.splits + split] = L;
    }
    const bool empty = L == 0.0f;   // no position (a position's p at the maximum is 1): a zero row
    const float norm = SPLIT ? kInvP : (kInvP / L) * a.kv_scale[0];
#pragma unroll
    for (int dt = 0; dt < kMlaDT; ++dt) {
        const int d = 16 * dt + 4 * g;
        if (SPLIT) {
            *(f32x4 *)(a.part_o + (row * a.splits + split) * kMlaLatent + d) = o[dt] * norm;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) store_from_float(a.out, row_q * a.ld_out + (int64_t)hq * kMlaLatent + d + j, empty ? 0.0f : o[dt][j] * norm, OUT);
        }
    }
}

template <int IN, int OUT, bool SPLIT>
__global__ __launch_bounds__(kMlaThreads) void mla_decode_kernel(const MlaArgs a)
{
    mla_attention_body<IN, OUT, SPLIT, false>(a);
}

template <int IN, int OUT, bool SPLIT>
__global__ __launch_bounds__(kMlaThreads) void mla_varlen_kernel(const MlaArgs a)
{
    mla_attention_body<IN, OUT, SPLIT, true>(a);
}

template <int IN, int OUT, bool SPLIT>
__global__ __launch_bounds__(kMlaThreads) void mla_sparse_kernel(const MlaArgs a)
{
    mla_attention_body<IN, OUT, SPLIT, false, true>(a);
}

// ---- append: one thread per (token, 16 channels of the 576-byte row), one 16-byte store ----
constexpr int kMlaAppendThreads = 256;

struct MlaAppendArgs {
    const void *kv_c, *k_pe;
    int64_t T, ld_c, ld_p;
    int bs_log2;
    int64_t slots;   // num_blocks * block_size
    uint8_t *cache;
    const void *slot_mapping;
    const float *kv_scale;
};

template <int IN, int MODE, bool SLOT64>
__global__ __launch_bounds__(kMlaAppendThreads) void mla_append_kernel(const MlaAppendArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * kMlaAppendThreads + threadIdx.x;
    if (idx >= a.T * kMlaChunks) return;
    const int64_t t = idx / kMlaChunks;
    const int ch = (int)(idx - t * kMlaChunks);
    const int64_t slot = SLOT64 ? ((const int64_t *)a.slot_mapping)[t] : (int64_t)((const int32_t *)a.slot_mapping)[t];
    if (slot < 0 || slot >= a.slots) return;   // padding
    const float prescale = __fdiv_rn(1.0f, a.kv_scale[0]);
    const bool rope = ch >= kMlaLatent / 16;
    const void *src = rope ? a.k_pe : a.kv_c;
    const int64_t i0 = rope ? t * a.ld_p + 16 * (ch - kMlaLatent / 16) : t * a.ld_c + 16 * ch;
    u32x4 w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = InVec<IN>::load1(src, i0 + 4 * k + j) * prescale;   // the float32 multiply of fp8mi_encode
        w[k] = encode4<MODE>(f[0], f[1], f[2], f[3]);
    }
    *(u32x4 *)(a.cache + slot * kMlaRow + 16 * ch) = w;   // slot s is row s % block_size of block s / block_size: row s of the tensor
}

}  // namespace

// host launchers (called from fp8mi_api.hip, which has validated the arguments and chosen `splits`)
int fp8mi_launch_mla_cache_append(const void *kv_c, const void *k_pe, int dtype, int64_t T, int64_t ld_c, int64_t ld_p, uint8_t *cache, int64_t num_blocks,
                                  int block_size, const void *slot_mapping, int slot_bytes, const float *kv_scale, int mode, hipStream_t s)
{
    const MlaAppendArgs a{kv_c, k_pe, T, ld_c, ld_p, fp8mi_attn_log2(block_size), num_blocks * block_size, cache, slot_mapping, kv_scale};
    const int64_t n = T * kMlaChunks;
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(mode, [&](auto mode_t) {
            constexpr int IN = decltype(in_t)::value, MODE = decltype(mode_t)::value;
            if (slot_bytes == 8) return fp8mi_launch_items(mla_append_kernel<IN, MODE, true>, n, kMlaAppendThreads, kMlaAppendThreads, s, a);
            return fp8mi_launch_items(mla_append_kernel<IN, MODE, false>, n, kMlaAppendThreads, kMlaAppendThreads, s, a);
        });
    });
}

int fp8mi_launch_mla_attention_decode(const void *q_lat, const void *q_pe, int q_dtype, int64_t B, int Hq, int64_t ld_ql, int64_t ld_qp, const uint8_t *cache,
                                      int64_t num_blocks, int block_size, const int32_t *block_table, int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens,
                                      int64_t max_seq_len, const float *kv_scale, float softmax_scale, int splits, void *workspace, void *out, int out_dtype,
                                      int64_t ld_out, hipStream_t s)
{
    MlaArgs a = {};
    a.q_lat = q_lat; a.q_pe = q_pe; a.ld_ql = ld_ql; a.ld_qp = ld_qp; a.cache = cache; a.num_blocks = num_blocks;
    a.bt = block_table; a.ld_bt = ld_bt; a.max_blocks = max_blocks; a.seq_lens = seq_lens; a.kv_scale = kv_scale;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.tiles = fp8mi_mla_head_tiles(Hq); a.bs_log2 = fp8mi_attn_log2(block_size);
    a.splits = splits; a.chunk = fp8mi_attn_chunk(max_seq_len, splits);
    a.out = out; a.ld_out = ld_out;
    if (B * a.tiles > 0x7FFFFFFF / splits || B * Hq > 0x7FFFFFFF) return FP8MI_E_UNSUPPORTED;
    const int64_t grid = B * a.tiles * splits;
    if (splits > 1) {
        const int64_t parts = B * Hq * splits;   // fp8mi_attn_decode.hip's layout, which its combine reads
        a.part_o = (float *)workspace;
        a.part_m = a.part_o + parts * kMlaLatent;
        a.part_l = a.part_m + parts;
    }
    return dispatch_in(q_dtype, [&](auto in_t) {
        constexpr int IN = decltype(in_t)::value;
        if (splits > 1) {
            if (int rc = fp8mi_launch(mla_decode_kernel<IN, FP8MI_F32, true>, dim3((unsigned)grid), dim3(kMlaThreads), s, a)) return rc;
            return fp8mi_launch_mla_combine(B, Hq, kv_scale, splits, workspace, out, out_dtype, ld_out, s);
        }
        return dispatch_in(out_dtype, [&](auto out_t) {
            return fp8mi_launch(mla_decode_kernel<IN, decltype(out_t)::value, false>, dim3((unsigned)grid), dim3(kMlaThreads), s, a);
        });
    });
}

// the multi-token form: rows = T query rows dealt to B sequences by cu_seqlens_q, 1 <= max_q_len <= T; B ceil(max_q_len Hq / 64) splits
// workgroups, partials per query row, the combine's grid B max_q_len Hq.  Any of the three at or beyond 2^31 is refused.
int fp8mi_launch_mla_attention_varlen(const void *q_lat, const void *q_pe, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq,
                                      int64_t ld_ql, int64_t ld_qp, const uint8_t *cache, int64_t num_blocks, int block_size, const int32_t *block_table, int64_t ld_bt,
                                      int64_t max_blocks, const int32_t *seq_lens, int64_t max_seq_len, const float *kv_scale, float softmax_scale, int splits,
                                      void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s)
{
    if (max_q_len < 1 || max_q_len > 0x7FFFFFFF / Hq) return FP8MI_E_UNSUPPORTED;
    const int64_t tiles = fp8mi_mla_col_tiles(max_q_len, Hq);
    if (B > 0x7FFFFFFF / tiles || B * tiles > 0x7FFFFFFF / splits || rows * Hq > 0x7FFFFFFF) return FP8MI_E_UNSUPPORTED;
    MlaArgs a = {};
    a.q_lat = q_lat; a.q_pe = q_pe; a.ld_ql = ld_ql; a.ld_qp = ld_qp; a.cache = cache; a.num_blocks = num_blocks;
    a.bt = block_table; a.ld_bt = ld_bt; a.max_blocks = max_blocks; a.seq_lens = seq_lens; a.kv_scale = kv_scale;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.tiles = (int)tiles; a.bs_log2 = fp8mi_attn_log2(block_size);
    a.splits = splits; a.chunk = fp8mi_attn_chunk(max_seq_len, splits);
    a.out = out; a.ld_out = ld_out;
    a.cu = cu_seqlens_q; a.rows = rows; a.max_q_len = (int)max_q_len;
    const int64_t grid = B * tiles * splits;
    if (splits > 1) {
        const int64_t parts = rows * Hq * splits;
        a.part_o = (float *)workspace;
        a.part_m = a.part_o + parts * kMlaLatent;
        a.part_l = a.part_m + parts;
    }
    return dispatch_in(q_dtype, [&](auto in_t) {
        constexpr int IN = decltype(in_t)::value;
        if (splits > 1) {
            if (int rc = fp8mi_launch(mla_varlen_kernel<IN, FP8MI_F32, true>, dim3((unsigned)grid), dim3(kMlaThreads), s, a)) return rc;
            return fp8mi_launch_mla_combine_varlen(rows, B, cu_seqlens_q, max_q_len, Hq, kv_scale, splits, workspace, out, out_dtype, ld_out, s);
        }
        return dispatch_in(out_dtype, [&](auto out_t) {
            return fp8mi_launch(mla_varlen_kernel<IN, decltype(out_t)::value, false>, dim3((unsigned)grid), dim3(kMlaThreads), s, a);
        });
    });
}

// the sparse form: rows = T query rows, each with its list of topk logical positions; cu_seqlens_q == nullptr: one token per sequence, rows = B,
// max_q_len = 1.  B max_q_len ceil(Hq / 64) splits workgroups; splits divide the LIST (chunk = fp8mi_attn_chunk(topk, splits)); partials per
// query row, merged by the combines above.  The ring holds physical row numbers as int32: num_blocks block_size stays below 2^31.
int fp8mi_launch_mla_attention_sparse(const void *q_lat, const void *q_pe, int q_dtype, int64_t rows, int64_t B, const int32_t *cu_seqlens_q, int64_t max_q_len, int Hq,
                                      int64_t ld_ql, int64_t ld_qp, const int32_t *indices, int64_t topk, int64_t ld_idx, const uint8_t *cache, int64_t num_blocks,
                                      int block_size, const int32_t *block_table, int64_t ld_bt, int64_t max_blocks, const int32_t *seq_lens, const float *kv_scale,
                                      float softmax_scale, int splits, void *workspace, void *out, int out_dtype, int64_t ld_out, hipStream_t s)
{
    const int64_t tiles = fp8mi_mla_head_tiles(Hq);
    if (max_q_len < 1 || topk < 1 || topk > 0x7FFFFFFF || num_blocks > 0x7FFFFFFF / block_size || B > 0x7FFFFFFF / max_q_len ||
        B * max_q_len > 0x7FFFFFFF / tiles || B * max_q_len * tiles > 0x7FFFFFFF / splits || rows * Hq > 0x7FFFFFFF)
        return FP8MI_E_UNSUPPORTED;
    MlaArgs a = {};
    a.q_lat = q_lat; a.q_pe = q_pe; a.ld_ql = ld_ql; a.ld_qp = ld_qp; a.cache = cache; a.num_blocks = num_blocks;
    a.bt = block_table; a.ld_bt = ld_bt; a.max_blocks = max_blocks; a.seq_lens = seq_lens; a.kv_scale = kv_scale;
    a.scale_log2 = softmax_scale * 1.44269504088896340736f;
    a.Hq = Hq; a.tiles = (int)tiles; a.bs_log2 = fp8mi_attn_log2(block_size);
    a.splits = splits; a.chunk = fp8mi_attn_chunk(topk, splits);
    a.out = out; a.ld_out = ld_out;
    a.cu = cu_seqlens_q; a.rows = rows; a.max_q_len = (int)max_q_len;
    a.indices = indices; a.ld_idx = ld_idx; a.topk = (int)topk;
    const int64_t grid = B * max_q_len * tiles * splits;
    if (splits > 1) {
        const int64_t parts = rows * Hq * splits;
        a.part_o = (float *)workspace;
        a.part_m = a.part_o + parts * kMlaLatent;
        a.part_l = a.part_m + parts;
    }
    return dispatch_in(q_dtype, [&](auto in_t) {
        constexpr int IN = decltype(in_t)::value;
        if (splits > 1) {
            if (int rc = fp8mi_launch(mla_sparse_kernel<IN, FP8MI_F32, true>, dim3((unsigned)grid), dim3(kMlaThreads), s, a)) return rc;
            if (!cu_seqlens_q) return fp8mi_launch_mla_combine(B, Hq, kv_scale, splits, workspace, out, out_dtype, ld_out, s);   // rows = B: every row is owned
            return fp8mi_launch_mla_combine_varlen(rows, B, cu_seqlens_q, max_q_len, Hq, kv_scale, splits, workspace, out, out_dtype, ld_out, s);
        }
        return dispatch_in(out_dtype, [&](auto out_t) {
            return fp8mi_launch(mla_sparse_kernel<IN, decltype(out_t)::value, false>, dim3((unsigned)grid), dim3(kMlaThreads), s, a);
        });
    });
}
