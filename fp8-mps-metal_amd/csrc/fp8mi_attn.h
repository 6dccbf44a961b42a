// What the paged KV cache (fp8mi_kvcache.hip), the decode attention and its multi-token form (fp8mi_attn_decode.hip) and their argument checks
// (fp8mi_api.hip) share: the geometry of the cache, the split choice and the workspace layout.  Host and device, header-only.
#pragma once

#include <stdint.h>

constexpr int kAttnStep = 128;        // positions of one K-step of the P.V product: what one wave takes at a time
constexpr int kAttnWaves = 4;         // waves of a decode workgroup; they take the steps of their split round-robin
constexpr int kAttnMaxGroup = 16;     // query heads per KV head: the 16 columns of an MFMA tile
constexpr int kAttnMaxSplits = 256;   // the largest num_splits a caller may force
constexpr int kAttnAutoSplits = 64;   // the largest num_splits the library chooses (fp8mi_paged_attention_workspace_bytes(.., 0) sizes for it)
constexpr int kAttnPScaleLog2 = 8;    // P is packed to e4m3 as p 2^8: [2^-17, 1] lands on [2^-9, 256], subnormals included
constexpr float kAttnTinyQ = 0x1p-64f;    // a query row with 0 < amax < this is quantised as the row times kAttnTinyQUp: 448 / amax stays finite
constexpr float kAttnTinyQUp = 0x1p64f;   // (the smallest amax, 2^-149, becomes 2^-85; 448 / amax overflows below 448 / FLT_MAX = 2^-119.2)

inline bool fp8mi_attn_block_size_ok(int bs) { return bs == 16 || bs == 32 || bs == 64 || bs == 128; }
inline bool fp8mi_attn_head_dim_ok(int D) { return D == 64 || D == 128; }
inline int fp8mi_attn_log2(int bs) { return bs == 16 ? 4 : bs == 32 ? 5 : bs == 64 ? 6 : 7; }

// bytes of the split partials: m and l (one float per sequence, query head and split), then O (D floats each)
inline int64_t fp8mi_attn_workspace_bytes(int64_t B, int Hq, int D, int splits)
{
    return splits <= 1 ? 0 : B * Hq * (int64_t)splits * (D + 2) * (int64_t)sizeof(float);
}

// positions per split: the 128-position steps of max_seq_len dealt out evenly (the last split runs to the sequence's end whatever it is)
inline int64_t fp8mi_attn_chunk(int64_t max_seq_len, int splits)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep;
    return ((steps + splits - 1) / splits) * kAttnStep;
}

// num_splits == 0: enough workgroups for two per compute unit, no split shorter than one step per wave, no more than the workspace holds
inline int fp8mi_attn_auto_splits(int64_t B, int Hq, int Hkv, int D, int64_t max_seq_len, int64_t workspace_bytes, int cus)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep, wgs = B * Hkv;
    if (wgs <= 0 || steps <= kAttnWaves) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnWaves - 1) / kAttnWaves;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(B, Hq, D, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// The multi-token form (fp8mi_paged_attention_varlen): the 16 columns of a tile hold (token, head) pairs of one KV head's group, so a
// tile takes 16 / (Hq / Hkv) query tokens (integer division: Hq / Hkv = 5 gives 3 and a dead column) and a sequence ceil(max_q_len / that)
// tiles.
inline int fp8mi_attn_tile_tokens(int Hq, int Hkv) { return kAttnMaxGroup / (Hq / Hkv); }
inline int64_t fp8mi_attn_q_tiles(int64_t max_q_len, int Hq, int Hkv)
{
    const int tq = fp8mi_attn_tile_tokens(Hq, Hkv);
    return (max_q_len + tq - 1) / tq;
}

// num_splits == 0 of the multi-token form: fp8mi_attn_auto_splits with B Hkv ceil(max_q_len / TQ) workgroups - every sequence counted at
// max_q_len tokens, so a mixed batch over-counts them and splits less than it could - and partials for T query rows.  All sequences at
// one token (T = B, max_q_len = 1) give the decode choice.
inline int fp8mi_attn_auto_splits_varlen(int64_t T, int64_t B, int64_t max_q_len, int Hq, int Hkv, int D, int64_t max_seq_len, int64_t workspace_bytes,
                                         int cus)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep, wgs = B * Hkv * fp8mi_attn_q_tiles(max_q_len, Hq, Hkv);
    if (wgs <= 0 || steps <= kAttnWaves) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnWaves - 1) / kAttnWaves;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(T, Hq, D, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// The LDS-tiled form for prompt chunks (fp8mi_paged_attention_prefill, fp8mi_attn_prefill.hip): a workgroup of kAttnPrefillWaves waves owns
// kAttnPrefillCols MFMA columns - eight 16-column tiles of the multi-token form's mapping, two per wave - which is 8 (16 / (Hq / Hkv)) query
// tokens, and a sequence ceil(max_q_len / that) workgroup tiles.
constexpr int kAttnPrefillWaves = 4;
constexpr int kAttnPrefillCols = 128;
inline int fp8mi_attn_prefill_tokens(int Hq, int Hkv) { return kAttnPrefillCols / kAttnMaxGroup * fp8mi_attn_tile_tokens(Hq, Hkv); }
inline int64_t fp8mi_attn_prefill_q_tiles(int64_t max_q_len, int Hq, int Hkv)
{
    const int tokens = fp8mi_attn_prefill_tokens(Hq, Hkv);
    return (max_q_len + tokens - 1) / tokens;
}

// num_splits == 0 of that form: the rule above with its workgroup count, B Hkv ceil(max_q_len / tokens per workgroup).  One wave walks a
// split alone there, so the floor is no split shorter than four steps.
constexpr int kAttnPrefillMinSteps = 4;
inline int fp8mi_attn_auto_splits_prefill(int64_t T, int64_t B, int64_t max_q_len, int Hq, int Hkv, int D, int64_t max_seq_len, int64_t workspace_bytes,
                                          int cus)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep, wgs = B * Hkv * fp8mi_attn_prefill_q_tiles(max_q_len, Hq, Hkv);
    if (wgs <= 0 || steps <= kAttnPrefillMinSteps) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnPrefillMinSteps - 1) / kAttnPrefillMinSteps;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(T, Hq, D, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// Multi-head latent attention (fp8mi_mla_cache_append, fp8mi_mla_attention_decode; fp8mi_attn_mla.hip): one cache row per position, the
// compressed latent's kMlaLatent bytes and then the rotary key's kMlaRope.  No other geometry is accepted.  A workgroup of kMlaWaves waves
// owns kMlaHeadTile query heads, 16 MFMA columns a wave, and a sequence ceil(Hq / kMlaHeadTile) workgroup tiles.
constexpr int kMlaLatent = 512;
constexpr int kMlaRope = 64;
constexpr int kMlaRow = kMlaLatent + kMlaRope;
constexpr int kMlaWaves = 4;
constexpr int kMlaHeadTile = 16 * kMlaWaves;
constexpr int kMlaMaxHeads = 128;
inline int fp8mi_mla_head_tiles(int Hq) { return (Hq + kMlaHeadTile - 1) / kMlaHeadTile; }

// num_splits == 0 of the MLA decode: the rule above with B ceil(Hq / 64) workgroups; one wave walks a split alone, so the floor is
// kAttnPrefillMinSteps steps a split.  Partials are fp8mi_attn_workspace_bytes(B, Hq, kMlaLatent, splits).
inline int fp8mi_attn_auto_splits_mla(int64_t B, int Hq, int64_t max_seq_len, int64_t workspace_bytes, int cus)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep, wgs = B * fp8mi_mla_head_tiles(Hq);
    if (wgs <= 0 || steps <= kAttnPrefillMinSteps) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnPrefillMinSteps - 1) / kAttnPrefillMinSteps;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(B, Hq, kMlaLatent, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// The multi-token form (fp8mi_mla_attention_varlen): a sequence's (token, head) pairs are numbered col = token Hq + head and a workgroup owns
// kMlaHeadTile consecutive columns, 16 a wave, so a sequence has ceil(max_q_len Hq / 64) workgroup tiles for any Hq - no dead column but at
// the sequence's end.
inline int64_t fp8mi_mla_col_tiles(int64_t max_q_len, int Hq) { return (max_q_len * Hq + kMlaHeadTile - 1) / kMlaHeadTile; }

// num_splits == 0 of that form: fp8mi_attn_auto_splits_mla with B ceil(max_q_len Hq / 64) workgroups - every sequence counted at max_q_len
// tokens - and partials for T query rows.  All sequences at one token (T = B, max_q_len = 1) give the decode choice.
inline int fp8mi_attn_auto_splits_mla_varlen(int64_t T, int64_t B, int64_t max_q_len, int Hq, int64_t max_seq_len, int64_t workspace_bytes, int cus)
{
    const int64_t steps = (max_seq_len + kAttnStep - 1) / kAttnStep, wgs = B * fp8mi_mla_col_tiles(max_q_len, Hq);
    if (wgs <= 0 || steps <= kAttnPrefillMinSteps) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnPrefillMinSteps - 1) / kAttnPrefillMinSteps;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(T, Hq, kMlaLatent, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// num_splits == 0 of the sparse form (fp8mi_mla_attention_sparse): a workgroup is one (sequence, token, tile of 64 heads) and walks the token's
// LIST, so the rule above with B max_q_len ceil(Hq / 64) workgroups and ceil(topk / 128) steps - the four-step floor and the cap kept - and
// partials for T query rows.
inline int fp8mi_attn_auto_splits_mla_sparse(int64_t T, int64_t B, int64_t max_q_len, int Hq, int64_t topk, int64_t workspace_bytes, int cus)
{
    const int64_t steps = (topk + kAttnStep - 1) / kAttnStep, wgs = B * max_q_len * fp8mi_mla_head_tiles(Hq);
    if (wgs <= 0 || steps <= kAttnPrefillMinSteps) return 1;
    int64_t s = (2 * (int64_t)cus + wgs - 1) / wgs;
    const int64_t by_steps = (steps + kAttnPrefillMinSteps - 1) / kAttnPrefillMinSteps;
    s = s < by_steps ? s : by_steps;
    s = s < kAttnAutoSplits ? s : kAttnAutoSplits;
    while (s > 1 && fp8mi_attn_workspace_bytes(T, Hq, kMlaLatent, (int)s) > workspace_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// The lightning indexer over an FP8 index-key cache (fp8mi_mla_index_cache_append, fp8mi_mla_index_logits, fp8mi_mla_index_topk;
// fp8mi_attn_index.hip).  The cache is uint8 [num_blocks, block_size kMlaIndexRow]: a block holds its block_size key rows of
// kMlaIndexDim e4m3 bytes and then their block_size fp32 scales.  A logits workgroup of kIdxWaves waves is (sequence, group of kIdxTokens
// query tokens, chunk of positions); a wave takes kIdxSuper positions at a time, so a chunk is a multiple of kIdxWaves kIdxSuper positions, and
// at most kIdxChunkMax of them: its resolved block-table entries (one per 16 positions at the smallest block) are held in LDS.
constexpr int kMlaIndexDim = 128;
constexpr int kMlaIndexRow = kMlaIndexDim + 4;
constexpr int kIdxWaves = 4;
constexpr int kIdxTokens = 4;
constexpr int kIdxSuper = 64;
constexpr int kIdxChunkUnit = kIdxWaves * kIdxSuper;
constexpr int kIdxChunkMax = 16384;
constexpr int kIdxMaxHeads = 64;
constexpr int kIdxTopkThreads = 1024;   // one workgroup per query token selects its row

inline bool fp8mi_mla_index_heads_ok(int Hi) { return Hi == 16 || Hi == 32 || Hi == 64; }
inline int64_t fp8mi_mla_index_token_groups(int64_t max_q_len) { return (max_q_len + kIdxTokens - 1) / kIdxTokens; }

// positions per chunk: two workgroups per compute unit from seq_groups = B ceil(max_q_len / kIdxTokens) (sequence, token group) pairs, no chunk
// shorter than one pass of the waves and none longer than the table in LDS holds
inline int64_t fp8mi_mla_index_chunk(int64_t seq_groups, int64_t max_seq_len, int cus)
{
    const int64_t want = seq_groups > 0 ? (2 * (int64_t)cus + seq_groups - 1) / seq_groups : 1;
    int64_t chunk = (max_seq_len + want - 1) / want;
    chunk = (chunk + kIdxChunkUnit - 1) / kIdxChunkUnit * kIdxChunkUnit;
    return chunk < kIdxChunkUnit ? kIdxChunkUnit : (chunk > kIdxChunkMax ? kIdxChunkMax : chunk);
}

// Flash attention over contiguous K / V (fp8mi_attention_prefill; fp8mi_attn_flash.hip): head dimensions (DQK, DV) = (128, 128) or
// (192, 128) - the second is 128 channels of k and kAttnFlashRope of k_rope.  A workgroup of kAttnFlashWaves waves owns kAttnFlashCols MFMA
// columns of the multi-token mapping: 8 (16 / (Hq / Hkv)) query tokens, and a sequence ceil(max_q_len / that) workgroup tiles.  One launch of
// B Hkv tiles workgroups; nothing is split along K.
constexpr int kAttnFlashWaves = 4;
constexpr int kAttnFlashCols = 128;
constexpr int kAttnFlashDV = 128;
constexpr int kAttnFlashRope = 64;
inline bool fp8mi_attn_flash_dims_ok(int DQK, int DV) { return DV == kAttnFlashDV && (DQK == kAttnFlashDV || DQK == kAttnFlashDV + kAttnFlashRope); }
inline int fp8mi_attn_flash_tokens(int Hq, int Hkv) { return kAttnFlashCols / kAttnMaxGroup * fp8mi_attn_tile_tokens(Hq, Hkv); }
inline int64_t fp8mi_attn_flash_q_tiles(int64_t max_q_len, int Hq, int Hkv)
{
    const int tokens = fp8mi_attn_flash_tokens(Hq, Hkv);
    return (max_q_len + tokens - 1) / tokens;
}

// The fused rotary embedding (+ per-head RMSNorm) in front of the cache appends (fp8mi_rope_kv_cache_append, fp8mi_mla_rope_cache_append;
// fp8mi_rope.hip).  A (token, head) row is owned by D / kRopeLaneElems adjacent lanes, 16 elements each, chosen so that both
// partners of a rotation sit in one lane.  Up to kRopeFlatMaxT tokens a wave is (token, 64 / lanes-per-row rows); beyond that a workgroup of
// kRopeTileWaves waves owns kRopeTileTokens consecutive tokens, one wave a token, and transposes their V bytes through LDS when their slots
// are one aligned run.  The kernarg structs, validated by the entry points in fp8mi_api.hip.
constexpr int kRopeLaneElems = 16;
constexpr int kRopeFlatMaxT = 64;
constexpr int kRopeTileTokens = 16;
constexpr int kRopeTileWaves = 16;

struct RopeArgs {
    const void *q, *k, *v;
    void *q_out;
    int64_t T, ld_q, ld_k, ld_v, ld_qo;
    int Hq, Hkv, D, rot_dim, style;
    const void *pos;
    int pos64;
    const void *cs;
    int cs_dtype;
    int64_t max_pos, ld_cs;
    const float *qw, *kw;   // nullptr: no norm
    float eps;
    uint8_t *kc, *vc;       // both nullptr: nothing is appended
    int bs_log2;
    int64_t slots;          // num_blocks * block_size
    const void *slot_mapping;
    int slot64;
    const float *k_scale, *v_scale;
    int scale_head;
    uint8_t *k8, *v8;       // nullptr or contiguous (T, Hkv, D)
};

struct MlaRopeArgs {
    const void *kv_c, *k_pe, *q_pe;
    void *q_pe_out;
    int64_t T, ld_c, ld_p, ld_qp, ld_qpo;
    int Hq, style;
    const void *pos;
    int pos64;
    const void *cs;
    int cs_dtype;
    int64_t max_pos, ld_cs;
    const float *kvw;       // nullptr: no norm
    float eps;
    uint8_t *cache;
    int64_t slots;
    const void *slot_mapping;
    int slot64;
    const float *kv_scale;
};
