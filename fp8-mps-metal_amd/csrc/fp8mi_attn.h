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
