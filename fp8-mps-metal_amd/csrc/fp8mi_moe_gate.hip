// The MoE gate for gfx950 (fp8mi_moe_gate): router logits (T, G) -> the k expert ids and weights of every token, in one launch - softmax or
// sigmoid scores, a selection-only bias, group-limited routing, renormalisation and scale (include/fp8mi.h has the definition).  No host
// sync, no global atomics, no workspace: capturable into a HIP graph, replays on new logits.
//
// One wave per token, kMoeGateTokensPerBlock tokens per workgroup.  Lane l holds the E = fp8mi_gate_slots(G) experts [l E, (l + 1) E) in
// registers (unrolled selects only, no run-time-indexed register array): a lane's experts are contiguous, so a row is read with loads of
// min(16, E * element size) bytes where base, ld and G allow and one element at a time otherwise, and an expert's group comes from one
// division per lane.  Every key becomes the 64-bit sort word of fp8mi_moe_gate.h; the selection is k rounds of (lane-local unsigned
// maximum over E words, wave maximum with DPP inside rows of 16 lanes and readlane across them, the owner clears its slot), lane j keeps
// result j, lanes < k store.  Three forms:
//   plain    key = logit.  A winner's logit is read back out of its word; the sigmoid needs k exponentials, the softmax G for its sum.
//   scored   key = score + bias: all G scores first; a winner's score is handed out by its owner lane with readlane.
//   grouped  scored, plus the group stage: the words go to LDS once, L = 64 / n_group (rounded down to a power of two) lanes reduce one
//            group's largest (and, excluding it, second largest) word, the same selection runs over the group scores, one per team,
//            and every lane clears the slots whose group lost.
// A wave past the last token repeats the last token and stores nothing, so that every wave reaches the group stage's barrier.

#include "fp8mi_rowquant.h"
#include "fp8mi_moe_gate.h"

#pragma clang fp contract(off)   // the definition is individually rounded fp32 operations

static_assert(kMoeGateMaxK == FP8MI_MOE_GATE_MAX_K, "include/fp8mi.h exports this");
static_assert(kMoeGateMaxK <= 64 && kMoeGateMaxGroups <= 64, "result j and group g live in one lane each");

namespace {

enum { kGatePlain = 0, kGateScored = 1, kGateGrouped = 2 };
constexpr int kGateThreads = 64 * kMoeGateTokensPerBlock;

struct GateArgs {
    const void *logits;
    int64_t T, ld;
    int G, k;
    const float *bias;
    int scoring, renormalize;
    float scale;
    int n_group, topk_group, group_score, team_log2;
    int32_t *ids;
    float *weights;
};

template <int CTRL>
FP8MI_DEVICE uint64_t dpp_umax64(uint64_t x)   // every lane of the wave is active wherever this is called
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, false);
    const uint64_t y = ((uint64_t)hi << 32) | lo;
    return x > y ? x : y;
}

FP8MI_DEVICE uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

FP8MI_DEVICE uint64_t read_row64(uint64_t v, int lane)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

FP8MI_DEVICE uint64_t wave_umax64(uint64_t v)   // wave-uniform: the structure of wave_umax
{
    v = dpp_umax64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v = dpp_umax64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v = dpp_umax64<0x141>(v);   // row_half_mirror
    v = dpp_umax64<0x140>(v);   // row_mirror
    return umax64(umax64(read_row64(v, 0), read_row64(v, 16)), umax64(read_row64(v, 32), read_row64(v, 48)));
}

FP8MI_DEVICE float lane_value(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }

template <int IN>
FP8MI_DEVICE void unpack_word(uint32_t w, float *f)   // one 32-bit word of a row: one fp32 element or two 16-bit ones
{
    if (IN == FP8MI_F32) {
        f[0] = __uint_as_float(w);
    } else if (IN == FP8MI_F16) {
        f[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
        f[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    } else {
        f[0] = __uint_as_float(w << 16);
        f[1] = __uint_as_float(w & 0xFFFF0000u);
    }
}

// the lane's E logits as floats; a slot at or beyond G gets 0 (its word is the pad word whatever it holds)
template <int IN, int E, bool VEC>
FP8MI_DEVICE void load_logits(const uint8_t *row, int e0, int G, float (&x)[E])
{
    constexpr int kEsz = IN == FP8MI_F32 ? 4 : 2, kBytes = E * kEsz, kW = kBytes >= 16 ? 16 : kBytes;
    if constexpr (VEC && kW >= 4) {
        constexpr int kPer = kW / kEsz, kWords = kW / 4, kPerWord = 4 / kEsz;
#pragma unroll
        for (int p = 0; p < E / kPer; ++p) {
            const int ep = e0 + p * kPer;   // G is a multiple of kPer here: a piece lies inside the row or outside it
            uint32_t raw[kWords];
#pragma unroll
            for (int q = 0; q < kWords; ++q) raw[q] = 0u;
            if (ep < G) {
                const uint8_t *src = row + (int64_t)ep * kEsz;
                if constexpr (kW == 16) {
                    const u32x4 v = *(const u32x4 *)src;
                    raw[0] = v[0]; raw[1] = v[1]; raw[2] = v[2]; raw[3] = v[3];
                } else if constexpr (kW == 8) {
                    const u32x2 v = *(const u32x2 *)src;
                    raw[0] = v[0]; raw[1] = v[1];
                } else {
                    raw[0] = *(const uint32_t *)src;
                }
            }
#pragma unroll
            for (int q = 0; q < kWords; ++q) {
                float f[2] = {0.0f, 0.0f};
                unpack_word<IN>(raw[q], f);
#pragma unroll
                for (int h = 0; h < kPerWord; ++h) x[p * kPer + q * kPerWord + h] = f[h];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) x[i] = e0 + i < G ? InVec<IN>::load1(row, e0 + i) : 0.0f;
    }
}

template <int IN, int E, bool VEC, int MODE>
__global__ __launch_bounds__(kGateThreads) void moe_gate_kernel(const GateArgs a)
{
    constexpr int kEsz = IN == FP8MI_F32 ? 4 : 2;
    constexpr int kLog2E = E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : E == 8 ? 3 : 4;
    __shared__ uint64_t lds_w[MODE == kGateGrouped ? kGateThreads * E : 1];   // [wave][expert]: the sort words, for the group stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t_raw = (int64_t)blockIdx.x * kMoeGateTokensPerBlock + wave;
    const bool live = t_raw < a.T;
    const int64_t t = live ? t_raw : a.T - 1;
    const int G = a.G, e0 = lane * E;
    const bool softmax = a.scoring == FP8MI_GATE_SOFTMAX;

    float x[E];
    load_logits<IN, E, VEC>((const uint8_t *)a.logits + t * a.ld * kEsz, e0, G, x);

    // ---- scores: the softmax's maximum and sum over all G experts; in the scored forms every expert's score ----
    float m = 0.0f, den = 1.0f;
    float s[E];
#pragma unroll
    for (int i = 0; i < E; ++i) s[i] = 0.0f;
    if (softmax) {
        uint32_t mo = 0u;
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (e0 + i < G) mo = max(mo, fp8mi_gate_ordered32(__float_as_uint(x[i])));
        m = __uint_as_float(fp8mi_gate_unordered32(wave_umax(mo)));
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const float ex = e0 + i < G ? __expf(x[i] - m) : 0.0f;
            s[i] = ex;
            part = part + ex;
        }
        den = wave_sum(part);
        if (MODE != kGatePlain) {
#pragma unroll
            for (int i = 0; i < E; ++i) s[i] = s[i] / den;
        }
    } else if (MODE != kGatePlain) {
#pragma unroll
        for (int i = 0; i < E; ++i) s[i] = 1.0f / (1.0f + __expf(-x[i]));
    }

    // ---- sort words ----
    uint64_t w[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = e0 + i;
        float key = x[i];
        if (MODE != kGatePlain) key = s[i] + ((a.bias && e < G) ? a.bias[e] : 0.0f);
        w[i] = e < G ? fp8mi_gate_word(__float_as_uint(key), (uint32_t)e) : kMoeGatePadWord;
    }

    // ---- groups: the groups that stay, then the pad word for every expert of the others ----
    if (MODE == kGateGrouped) {
        uint64_t *lw = lds_w + wave * 64 * E;
#pragma unroll
        for (int i = 0; i < E; ++i) lw[e0 + i] = w[i];
        __syncthreads();
        const int gs = G / a.n_group, L = 1 << a.team_log2, g = lane >> a.team_log2, sub = lane & (L - 1);
        const bool has = g < a.n_group;   // lanes [g L, (g + 1) L) reduce group g
        uint64_t m1 = 0u;
        if (has)
            for (int i = sub; i < gs; i += L) m1 = umax64(m1, lw[g * gs + i]);
        for (int d = 1; d < L; d <<= 1) m1 = umax64(m1, (uint64_t)__shfl_xor((unsigned long long)m1, d, 64));
        uint32_t score = (uint32_t)(m1 >> 32);   // FP8MI_GATE_GROUP_MAX: the group's first key, ordered already
        if (a.group_score == FP8MI_GATE_GROUP_TOP2) {
            uint64_t m2 = 0u;   // the largest word that is not m1: words are distinct
            if (has)
                for (int i = sub; i < gs; i += L) {
                    const uint64_t v = lw[g * gs + i];
                    m2 = umax64(m2, v == m1 ? 0u : v);
                }
            for (int d = 1; d < L; d <<= 1) m2 = umax64(m2, (uint64_t)__shfl_xor((unsigned long long)m2, d, 64));
            const float sum = __uint_as_float(fp8mi_gate_word_key(m1)) + __uint_as_float(fp8mi_gate_word_key(m2));
            score = fp8mi_gate_ordered32(__float_as_uint(sum));
        }
        uint64_t gw = has && sub == 0 ? (((uint64_t)score << 32) | (0xFFFFFFFFu - (uint32_t)g)) : kMoeGatePadWord;
        uint64_t keep = 0u;
        for (int r = 0; r < a.topk_group; ++r) {
            const uint64_t win = wave_umax64(gw);
            keep |= 1ull << (fp8mi_gate_word_index(win) & 63u);
            if (gw == win) gw = kMoeGatePadWord;
        }
        // the group of the lane's first expert, one division; its experts are contiguous.  A pad slot's group is at or beyond n_group: its
        // word is the pad word already, whichever bit of `keep` it reads.  Selects only.
        uint32_t ge = (uint32_t)e0 / (uint32_t)gs, r = (uint32_t)e0 - ge * (uint32_t)gs;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const uint64_t bit = (keep >> (ge & 63u)) & 1ull;
            w[i] = bit ? w[i] : kMoeGatePadWord;
            const bool wrap = r + 1u == (uint32_t)gs;
            r = wrap ? 0u : r + 1u;
            ge += wrap ? 1u : 0u;
        }
    }

    // ---- selection: k rounds; lane j keeps result j ----
    uint32_t my_id = 0u;
    float my_val = 0.0f;   // plain: the winner's logit; scored: its score
    for (int j = 0; j < a.k; ++j) {
        uint64_t lm = w[0];
#pragma unroll
        for (int i = 1; i < E; ++i) lm = umax64(lm, w[i]);
        const uint64_t win = wave_umax64(lm);
        const uint32_t e = fp8mi_gate_word_index(win);
        float val;
        if (MODE == kGatePlain) {
            val = __uint_as_float(fp8mi_gate_word_key(win));
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (w[i] == win) w[i] = kMoeGatePadWord;
        } else {
            float sv = 0.0f;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const bool hit = w[i] == win;
                sv = hit ? s[i] : sv;
                w[i] = hit ? kMoeGatePadWord : w[i];
            }
            val = lane_value(sv, (int)((e >> kLog2E) & 63u));
        }
        if (lane == j) {
            my_id = e;
            my_val = val;
        }
    }

    // ---- weights: the score, renormalised over the k in order, scaled ----
    float wgt = my_val;
    if (MODE == kGatePlain) wgt = softmax ? __expf(my_val - m) / den : 1.0f / (1.0f + __expf(-my_val));
    if (a.renormalize) {
        float d = lane_value(wgt, 0);
        for (int j = 1; j < a.k; ++j) d = d + lane_value(wgt, j);
        wgt = wgt / (d + 1e-20f);
    }
    wgt = wgt * a.scale;
    if (live && lane < a.k) {
        const int64_t at = t * a.k + lane;
        a.ids[at] = (int32_t)my_id;
        a.weights[at] = wgt;
    }
}

template <int IN, int E, bool VEC, int MODE>
int launch_gate(const GateArgs &a, hipStream_t s)
{
    const int64_t blocks = (a.T + kMoeGateTokensPerBlock - 1) / kMoeGateTokensPerBlock;
    return fp8mi_launch(moe_gate_kernel<IN, E, VEC, MODE>, dim3((unsigned)blocks), dim3(kGateThreads), s, a);
}

}  // namespace

// host launcher (called from fp8mi_api.hip, which has validated the arguments)
int fp8mi_launch_moe_gate(const void *logits, int dtype, int64_t T, int G, int64_t ld, const float *bias, int k, int scoring, int renormalize, float scale,
                          int n_group, int topk_group, int group_score, int32_t *ids, float *weights, hipStream_t s)
{
    const GateArgs a{logits, T, ld, G, k, bias, scoring, renormalize, scale, n_group, topk_group, group_score, fp8mi_gate_team_log2(n_group), ids, weights};
    const int E = fp8mi_gate_slots(G), esz = dtype == FP8MI_F32 ? 4 : 2;
    const int width = E * esz >= 16 ? 16 : E * esz;   // bytes of one load of the vector form
    const bool vec = width >= 4 && aligned_to(logits, (uintptr_t)width) && (T <= 1 || (ld * esz) % width == 0) && G % (width / esz) == 0;
    const int mode = n_group > 1 ? kGateGrouped : bias ? kGateScored : kGatePlain;
    return dispatch_in(dtype, [&](auto in_t) {
        return dispatch_int<1, 2, 4, 8, 16>(E, [&](auto e_t) {
            return dispatch_int<kGatePlain, kGateScored, kGateGrouped>(mode, [&](auto mode_t) {
                constexpr int IN = decltype(in_t)::value, EE = decltype(e_t)::value, MODE = decltype(mode_t)::value;
                if (vec) return launch_gate<IN, EE, true, MODE>(a, s);
                return launch_gate<IN, EE, false, MODE>(a, s);
            });
        });
    });
}
