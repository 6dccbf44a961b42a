// MoE routing on the device, for gfx950: from the gate's (T, k) expert ids to the sorted-row plan the grouped GEMM reads
// (fp8mi_moe_route), the activations quantised once per token and stored to each of its k rows (fp8mi_moe_scatter_quantize), and the
// weighted sum of a token's k result rows (fp8mi_moe_combine).  No host sync, no global atomics, nothing whose result depends on the
// order in which workgroups run: every call is capturable into a HIP graph and replays on new ids.
//
// Route: a STABLE counting sort by expert.  A wave holds 64 consecutive assignments, one per lane, and loops over the distinct ids among
// them - a leader's id broadcast, a ballot of the lanes that match, the popcount below the lane - so that an assignment's rank inside its
// wave and the wave's count per id come from ballots alone; the first lane of every id stores the count to the wave's LDS row (distinct
// ids, distinct addresses: no atomics anywhere).  Waves own consecutive 64s and workgroups consecutive chunks (fp8mi_moe_route.h), so
// "earlier waves of the workgroup" + "earlier workgroups" + "earlier experts" complete the row.  n <= kMoeRouteSingleMax: one workgroup
// does all of it in one launch.  Otherwise: count (per workgroup and expert, into the workspace), scan (one workgroup per expert, over
// the workgroups' counts), rank (which scans the experts' totals itself; its first workgroup writes offs).
// Scatter-quantise: the register-resident forms of the row quantisers (fp8mi_rowquant.h) with an output side of k destinations.
// Combine: a gather - one lane per 16-byte piece of an output row, the k products added in order, each rounded on its own.

#include "fp8mi_rowquant.h"
#include "fp8mi_moe_route.h"

#pragma clang fp contract(off)   // the combine is k individually rounded products and k individually rounded sums

static_assert(kMoeRouteChunk == FP8MI_MOE_ROUTE_CHUNK && kMoeRouteSingleMax == FP8MI_MOE_ROUTE_SINGLE_MAX, "include/fp8mi.h exports these");
static_assert(kMoeRouteMaxExperts == kMoeRouteThreads, "the expert scan holds one expert per thread");

namespace {

// ---- route ----------------------------------------------------------------------------------------------------------------------------
enum { kRouteSingle = 0, kRouteCount = 1, kRouteRank = 2 };

// Exclusive scan of `a` over the workgroup's threads, in thread order; `total`: the sum over all of them.  Every thread calls it (two
// barriers); `wsum` holds kMoeRouteWaves ints that nothing else uses meanwhile.
FP8MI_DEVICE int block_scan(int a, int *wsum, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = a;   // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = x - a;
    total = 0;
#pragma unroll
    for (int w = 0; w < kMoeRouteWaves; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    return before;
}

// The experts' first rows from their counts: thread g owns expert g (count `a`, 0 for g >= G); start[0 .. G) (LDS) = the exclusive scan,
// start[G] = the rows in use; offs[g] = start[g] + a where `offs` is given.  Ends behind a barrier.
FP8MI_DEVICE void scan_experts(int a, int *start, int *wsum, int G, int32_t *__restrict__ offs)
{
    const int g = threadIdx.x;
    int total;
    const int before = block_scan(a, wsum, total);
    if (g < G) {
        start[g] = before;
        if (offs) offs[g] = before + a;
    }
    if (g == 0) start[G] = total;
    __syncthreads();
}

// ID: int32_t or int64_t.  MODE kRouteSingle: the whole call (grid 1).  kRouteCount: base[g][b] = this workgroup's count.  kRouteRank:
// the rows, from the scanned workspace; every workgroup scans the experts' totals for itself (G <= 1024 values), workgroup 0 writes offs.
template <typename ID, int MODE>
__global__ __launch_bounds__(kMoeRouteThreads) void moe_route_kernel(const ID *__restrict__ ids, int64_t n, int G, int32_t *__restrict__ offs,
                                                                      int32_t *__restrict__ row_of, int32_t *__restrict__ src_of_row,
                                                                      int32_t *__restrict__ ws)
{
    __shared__ uint16_t wcnt[kMoeRouteWaves * kMoeRouteMaxExperts];   // [wave][expert]: the wave's count, at most 64
    __shared__ int start[kMoeRouteMaxExperts + 1];
    __shared__ int wsum[kMoeRouteWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    for (int j = threadIdx.x; j < kMoeRouteWaves * G; j += kMoeRouteThreads) wcnt[j] = 0;
    __syncthreads();

    const int64_t i = fp8mi_moe_route_index(b, wave, lane);
    const int64_t v = i < n ? (int64_t)ids[i] : -1;
    const bool ok = v >= 0 && v < G;
    const int id = ok ? (int)v : -1;
    int rank = 0, cnt = 0;   // the matching lanes below this one; all matching lanes of the wave
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t todo = __ballot(ok);
    while (todo) {   // wave-uniform: once per distinct id of the wave
        const int lid = __builtin_amdgcn_readlane(id, __builtin_ctzll(todo));
        const uint64_t m = __ballot(id == lid);
        if (id == lid) {
            rank = __popcll(m & below);
            cnt = __popcll(m);
        }
        todo &= ~m;
    }
    if (ok && rank == 0) wcnt[wave * G + id] = (uint16_t)cnt;
    __syncthreads();

    {
        const int g = threadIdx.x;   // this thread's expert
        int c = 0;
        if (MODE == kRouteRank) {
            c = g < G ? ws[fp8mi_moe_route_ws_total(n, G, g)] : 0;
        } else if (g < G) {   // the workgroup's count
#pragma unroll
            for (int w = 0; w < kMoeRouteWaves; ++w) c += wcnt[w * G + g];
        }
        if (MODE == kRouteCount) {
            if (g < G) ws[fp8mi_moe_route_ws_base(n, b, g)] = c;
            return;
        }
        scan_experts(c, start, wsum, G, b == 0 ? offs : nullptr);
    }
    if (i >= n) return;
    if (src_of_row && i >= start[G]) src_of_row[i] = -1;   // the tail: rows offs[G - 1] .. n - 1 (a row below that has exactly one owner)
    int row = -1;
    if (ok) {
        row = rank + start[id] + (MODE == kRouteRank ? ws[fp8mi_moe_route_ws_base(n, b, id)] : 0);
        for (int w = 0; w < wave; ++w) row += wcnt[w * G + id];
        if (src_of_row) src_of_row[row] = (int32_t)i;
    }
    row_of[i] = row;
}

// One workgroup per expert: its row base[g][0 .. blocks) -> the counts of the workgroups before each, total[g] = the sum.  Thread t sums
// its segment of the row (fp8mi_moe_route_scan_first), the segments' sums are scanned over the workgroup, a second pass writes.
__global__ __launch_bounds__(kMoeRouteThreads) void moe_route_scan_kernel(int64_t n, int G, int32_t *__restrict__ ws)
{
    __shared__ int wsum[kMoeRouteWaves];
    const int g = blockIdx.x;
    const int64_t blocks = fp8mi_moe_route_blocks(n);
    int32_t *row = ws + fp8mi_moe_route_ws_base(n, 0, g);
    const int64_t b0 = fp8mi_moe_route_scan_first(blocks, threadIdx.x), b1 = fp8mi_moe_route_scan_first(blocks, threadIdx.x + 1);
    int sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += row[b];
    int total;
    int run = block_scan(sum, wsum, total);
    for (int64_t b = b0; b < b1; ++b) {
        const int c = row[b];
        row[b] = run;
        run += c;
    }
    if (threadIdx.x == 0) ws[fp8mi_moe_route_ws_total(n, G, g)] = total;
}

template <typename ID>
int launch_route(const void *ids, int64_t n, int G, int32_t *offs, int32_t *row_of, int32_t *src_of_row, int32_t *ws, hipStream_t s)
{
    const ID *p = (const ID *)ids;
    if (fp8mi_moe_route_single(n))
        return fp8mi_launch(moe_route_kernel<ID, kRouteSingle>, dim3(1), dim3(kMoeRouteThreads), s, p, n, G, offs, row_of, src_of_row, ws);
    const dim3 grid((unsigned)fp8mi_moe_route_blocks(n));
    int rc = fp8mi_launch(moe_route_kernel<ID, kRouteCount>, grid, dim3(kMoeRouteThreads), s, p, n, G, offs, row_of, src_of_row, ws);
    if (rc == 0) rc = fp8mi_launch(moe_route_scan_kernel, dim3((unsigned)G), dim3(kMoeRouteThreads), s, n, G, ws);
    if (rc == 0) rc = fp8mi_launch(moe_route_kernel<ID, kRouteRank>, grid, dim3(kMoeRouteThreads), s, p, n, G, offs, row_of, src_of_row, ws);
    return rc;
}

// ---- scatter-quantise -------------------------------------------------------------------------------------------------------------------
// The register-resident form of quantize_rowwise_reg_kernel / act_quant_reg_kernel (FP8MI_ACT_NONE): W waves share token r, wave w owns
// the pieces 64 (w + W j) + lane, j < NV.  The encoded words (and the groups' scales) are held; the output side then walks the token's k
// destinations, read 64 at a time by the lanes and handed out with readlane: a destination is wave-uniform.  QS: an e4m3 ENC value (one
// scale per row), kQGroup, or kQMx8 / kQMx4.  cols is a multiple of 16 (MX: of 32): whole pieces only.
// MX (mx_piece's recipe, fp8mi_rowquant.h): a block is 32 / kPer adjacent lanes of one piece; its exponent and the piece's encoded words
// are made once, and the scale bytes of the 16 lanes of a DPP row - four blocks (fp32 input: two) - are gathered into one word that every
// lane of the row holds (sx).  A piece past the row carries 0x7F there: the pad bytes of the row's last four blocks.
template <int IN, int QS, int W>
__global__ __launch_bounds__(W >= 4 ? 64 * W : 256) void moe_scatter_quant_kernel(const void *__restrict__ in, int64_t T, int64_t cols, int64_t ld_in,
                                                                                   const int32_t *__restrict__ row_of, int k, int64_t rows_out,
                                                                                   const QuantOut q)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2, NV = 8, kGpp = 128 / kPer;
    __shared__ float lds_m[W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = W == 1 ? 0 : wave;
    const int64_t r = W == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
    if (r >= T) return;   // wave-uniform, and only where a wave is a row (W == 1: no barrier below)
    const u32x4 *in4 = (const u32x4 *)((const uint8_t *)in + r * ld_in * kEsz);
    const int64_t nv = cols / kPer;
    const u32x4 zero{0u, 0u, 0u, 0u};

    u32x4 raw[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * (wr + W * j);
        raw[j] = v < nv ? __builtin_nontemporal_load(in4 + v) : zero;
    }

    constexpr bool MX = QS == kQMx8 || QS == kQMx4;
    constexpr int kBl = 32 / kPer;   // MX: lanes per block
    uint32_t w0[NV], w1[NV];
    float gs[NV];    // kQGroup: the scale of the piece's group
    uint32_t sx[NV];    // MX: the scale bytes of the lane's DPP row
    float inv = 1.0f;   // one scale per row: the inverse scale, in the lane that publishes it
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        w0[j] = w1[j] = 0u;
        gs[j] = 0.0f;
        sx[j] = 0u;
    }
    if constexpr (MX) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (64 * (int64_t)(wr + W * j) >= nv) continue;   // wave-uniform: none of this wave's lanes has a piece here
            float y[8];
            unpack<IN>(raw[j], y);   // a piece past the row is zeros
            uint32_t m = 0u;
#pragma unroll
            for (int e = 0; e < kPer; ++e) m = max(m, abs_bits(y[e]));
            m = dpp_umax<0xB1>(m);                     // quad_perm [1, 0, 3, 2]
            m = dpp_umax<0x4E>(m);                     // quad_perm [2, 3, 0, 1]
            if (kBl == 8) m = dpp_umax<0x141>(m);      // row_half_mirror
            const uint32_t ex = mx_block_exponent<QS>(m);
            piece_words_mx<QS, kPer>(y, ex, w0[j], w1[j]);
            const uint32_t byte = lane + 64 * (int64_t)(wr + W * j) < nv ? ex : 0x7Fu;
            uint32_t w = byte << (kPer == 8 ? 8 * ((lane >> 2) & 3) : 8 * ((lane >> 3) & 1));
            if (kPer == 8) w = dpp_or<0x141>(w);   // quads 0 | 1 and 2 | 3 ...
            sx[j] = dpp_or<0x140>(w);              // ... and all of the row (row_mirror)
        }
    } else if constexpr (QS == kQGroup) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (64 * (int64_t)(wr + W * j) >= nv) continue;   // wave-uniform: none of this wave's lanes has a piece here
            float y[8];
            unpack<IN>(raw[j], y);   // a piece past the row is zeros
            gs[j] = piece_group_scale<kPer>(y, lane, false, 0, nullptr, 0);
            piece_words<QS, kPer>(y, gs[j], w0[j], w1[j]);
        }
    } else {
        float m = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) m = piece_amax<IN>(raw[j], m);
        m = row_max<W>(m, lds_m, wave, lane);
        const float scale = row_scale<QS>(m, lane, false, nullptr, 0, nullptr, r);
        if (wr == 0 && lane == 0) {
            float unused;
            scale_of_amax<QS>(m, unused, inv);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (64 * (int64_t)(wr + W * j) >= nv) continue;
            float y[8];
            unpack<IN>(raw[j], y);
            piece_words<QS, kPer>(y, scale, w0[j], w1[j]);
        }
    }

    const int32_t *dst = row_of + r * k;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int held = j0 + lane < k ? dst[j0 + lane] : -1;
        const int cnt = k - j0 < 64 ? k - j0 : 64;
        for (int jj = 0; jj < cnt; ++jj) {
            const int64_t d = __builtin_amdgcn_readlane(held, jj);
            if (d < 0 || d >= rows_out) continue;   // -1 and anything else outside the output: skipped
            uint8_t *orow = q.out + d * q.ld_out;
            if constexpr (MX) {
                uint8_t *mrow = (uint8_t *)q.scales + d * q.s_sr;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int64_t v = lane + 64 * (wr + W * j);
                    if (v < nv) store_words_mx<QS, kPer>(w0[j], w1[j], orow, v);
                    const bool live = (v & ~(int64_t)(4 * kBl - 1)) < nv;   // this lane's four blocks hold a block of the row
                    const int64_t b = v / kBl;
                    if (q.mx_flags & kMxWord) {
                        if (live && (lane & 15) == 0) {
                            if (kPer == 8) *(uint32_t *)(mrow + b) = sx[j];
                            else *(uint16_t *)(mrow + b) = (uint16_t)sx[j];
                        }
                    } else if ((lane & (kBl - 1)) == 0 && (v < nv || ((q.mx_flags & kMxPad) && live))) {
                        mrow[b] = (uint8_t)(sx[j] >> (kPer == 8 ? 8 * ((lane >> 2) & 3) : 8 * ((lane >> 3) & 1)));
                    }
                }
                continue;
            }
            float *srow = (float *)q.scales + d * q.s_sr;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int64_t v = lane + 64 * (wr + W * j);
                if (v < nv) {
                    store_words<kPer>(w0[j], w1[j], orow, v);
                    if (QS == kQGroup && (lane & (kGpp - 1)) == 0) srow[(v / kGpp) * q.s_sk] = gs[j];
                }
            }
            if (QS != kQGroup && wr == 0 && lane == 0) srow[0] = inv;
        }
    }
}

template <int IN, int QS>
int launch_scatter_quant(const void *in, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, int64_t rows_out, const QuantOut &q,
                         hipStream_t s)
{
    constexpr int kPer = InVec<IN>::kPer;
    if (T > kRowMaxRows) return FP8MI_E_UNSUPPORTED;
    const int w = row_rung(cols, kPer, IN == FP8MI_F32).w;   // (every instance, the MX ones included, holds NV = 8 pieces without scratch: profiles/grouped_mx_isa.txt)
#define FP8MI_SQ_REG(W) launch_row_reg<W>(moe_scatter_quant_kernel<IN, QS, W>, T, s, in, T, cols, ld_in, row_of, k, rows_out, q)
    if (w == 1) return FP8MI_SQ_REG(1);
    if (w == 4) return FP8MI_SQ_REG(4);
    if constexpr (IN == FP8MI_F32)
        if (w == 8) return FP8MI_SQ_REG(8);
#undef FP8MI_SQ_REG
    return FP8MI_E_UNSUPPORTED;
}

// ---- combine ------------------------------------------------------------------------------------------------------------------------------
// fl32(acc + fl32(w * y)): the asm statements keep the product and the sum from meeting a neighbour in one instruction (a multiply-add,
// or a sum rounded straight to f16 - e5m2_scaled, fp8mi_rowquant.h)
FP8MI_DEVICE float combine_step(float acc, float w, float y)
{
    float p = w * y;
    asm("" : "+v"(p));
    float a = acc + p;
    asm("" : "+v"(a));
    return a;
}

constexpr int kCombineThreads = 256, kCombineBatch = 4;

// grid (T, column blocks).  VEC: a lane owns one 16-byte piece of the y rows (4 fp32 / 8 16-bit columns) and stores it as one vector;
// otherwise one column, any alignment.  The token's destinations and weights are read 64 at a time by the lanes of every wave and handed
// out with readlane; the loads of kCombineBatch rows are issued before the first of them is added.
template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(kCombineThreads) void moe_combine_kernel(const void *__restrict__ y, int64_t rows, int64_t N, int64_t ld_y,
                                                                       const int32_t *__restrict__ row_of, const float *__restrict__ weights, int k,
                                                                       void *__restrict__ out, int64_t ld_out)
{
    constexpr int kPer = VEC ? InVec<IN>::kPer : 1, kEsz = IN == FP8MI_F32 ? 4 : 2;
    const int lane = threadIdx.x & 63;
    const int64_t t = blockIdx.x;
    const int64_t p = (int64_t)blockIdx.y * kCombineThreads + threadIdx.x;   // this lane's piece (VEC) or column
    const bool live = p * kPer < N;
    const int32_t *dst = row_of + t * k;
    const float *wt = weights ? weights + t * k : nullptr;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;

    for (int j0 = 0; j0 < k; j0 += 64) {
        const int held = j0 + lane < k ? dst[j0 + lane] : -1;
        const float held_w = wt && j0 + lane < k ? wt[j0 + lane] : 1.0f;
        const int cnt = k - j0 < 64 ? k - j0 : 64;
        for (int jb = 0; jb < cnt; jb += kCombineBatch) {
            u32x4 raw[kCombineBatch];
            float one[kCombineBatch], w[kCombineBatch];
            bool ok[kCombineBatch];
#pragma unroll
            for (int u = 0; u < kCombineBatch; ++u) {
                const int jj = jb + u < cnt ? jb + u : cnt - 1;
                const int64_t d = __builtin_amdgcn_readlane(held, jj);
                w[u] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, held_w), jj));
                ok[u] = jb + u < cnt && d >= 0 && d < rows;   // wave-uniform
                raw[u] = u32x4{0u, 0u, 0u, 0u};
                one[u] = 0.0f;
                if (ok[u] && live) {
                    const uint8_t *yrow = (const uint8_t *)y + d * ld_y * kEsz;
                    if (VEC)
                        raw[u] = *((const u32x4 *)yrow + p);
                    else
                        one[u] = load_as_float(yrow, p, IN);
                }
            }
#pragma unroll
            for (int u = 0; u < kCombineBatch; ++u) {
                if (!ok[u]) continue;
                if (VEC) {
                    float f[8];
                    unpack<IN>(raw[u], f);
#pragma unroll
                    for (int e = 0; e < kPer; ++e) acc[e] = combine_step(acc[e], w[u], f[e]);
                } else {
                    acc[0] = combine_step(acc[0], w[u], one[u]);
                }
            }
        }
    }
    if (!live) return;
    if (!VEC) {
        store_from_float((uint8_t *)out + t * ld_out * (OUT == FP8MI_F32 ? 4 : 2), p, acc[0], OUT);
    } else if (OUT == FP8MI_F32) {
        f32x4 *o = (f32x4 *)((float *)out + t * ld_out + p * kPer);
        o[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
        if (kPer == 8) o[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
    } else {
        uint16_t *o = (uint16_t *)out + t * ld_out + p * kPer;
        const uint32_t h0 = pack16<OUT>(acc[0], acc[1]), h1 = pack16<OUT>(acc[2], acc[3]);
        if (kPer == 8)
            *(u32x4 *)o = u32x4{h0, h1, pack16<OUT>(acc[4], acc[5]), pack16<OUT>(acc[6], acc[7])};
        else
            *(u32x2 *)o = u32x2{h0, h1};
    }
}

template <int IN, int OUT>
int launch_combine(const void *y, int64_t rows, int64_t N, int64_t ld_y, const int32_t *row_of, const float *weights, int64_t T, int k, void *out,
                   int64_t ld_out, hipStream_t s)
{
    constexpr int kPer = InVec<IN>::kPer, kEsz = IN == FP8MI_F32 ? 4 : 2, kOsz = OUT == FP8MI_F32 ? 4 : 2;
    const bool vec = N % kPer == 0 && aligned_to(y, 16) && (rows <= 1 || (ld_y * kEsz) % 16 == 0) && aligned_to(out, kPer * kOsz) &&
                     (T == 1 || ld_out % kPer == 0);
    const int64_t gy = ((vec ? N / kPer : N) + kCombineThreads - 1) / kCombineThreads;
    if (T > 0x7FFFFFFF || gy > 65535) return FP8MI_E_UNSUPPORTED;
    const dim3 grid((unsigned)T, (unsigned)gy);
    if (vec) return fp8mi_launch(moe_combine_kernel<IN, OUT, true>, grid, dim3(kCombineThreads), s, y, rows, N, ld_y, row_of, weights, k, out, ld_out);
    return fp8mi_launch(moe_combine_kernel<IN, OUT, false>, grid, dim3(kCombineThreads), s, y, rows, N, ld_y, row_of, weights, k, out, ld_out);
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers (called from fp8mi_api.hip, which has validated the arguments)
// ---------------------------------------------------------------------------
int fp8mi_launch_moe_route(const void *ids, int id_bytes, int64_t n, int G, int32_t *offs, int32_t *row_of, int32_t *src_of_row, void *workspace,
                           hipStream_t s)
{
    if (id_bytes == 8) return launch_route<int64_t>(ids, n, G, offs, row_of, src_of_row, (int32_t *)workspace, s);
    return launch_route<int32_t>(ids, n, G, offs, row_of, src_of_row, (int32_t *)workspace, s);
}

int fp8mi_launch_moe_scatter_quantize(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                      int64_t rows_out, int64_t ld_out, float *scales, int64_t s_stride_row, int64_t s_stride_k, int scale_mode,
                                      int mode, hipStream_t s)
{
    const int qs = scale_mode == FP8MI_QSCALE_GROUP128 ? kQGroup : mode;
    const QuantOut q{out, ld_out, scales, s_stride_row, s_stride_k, 0, nullptr};
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<kQGroup, FP8MI_ENC_REFERENCE, FP8MI_ENC_RNE>(qs, [&](auto qs_t) {
            return launch_scatter_quant<decltype(in_t)::value, decltype(qs_t)::value>(in, T, cols, ld_in, row_of, k, rows_out, q, s);
        });
    });
}

int fp8mi_launch_moe_scatter_quantize_mx(const void *in, int in_dtype, int64_t T, int64_t cols, int64_t ld_in, const int32_t *row_of, int k, uint8_t *out,
                                         int64_t rows_out, int64_t ld_out, uint8_t *scales, int64_t ld_s, int mx_format, hipStream_t s)
{
    const QuantOut q{out, ld_out, scales, ld_s, 0, mx_scale_flags(scales, rows_out, cols, ld_s), nullptr};
    return dispatch_in(in_dtype, [&](auto in_t) {
        return dispatch_int<kQMx8, kQMx4>(kQMx8 + mx_format, [&](auto qs_t) {
            return launch_scatter_quant<decltype(in_t)::value, decltype(qs_t)::value>(in, T, cols, ld_in, row_of, k, rows_out, q, s);
        });
    });
}

int fp8mi_launch_moe_combine(const void *y, int y_dtype, int64_t rows, int64_t N, int64_t ld_y, const int32_t *row_of, const float *weights, int64_t T,
                             int k, void *out, int out_dtype, int64_t ld_out, hipStream_t s)
{
    return dispatch_in(y_dtype, [&](auto in_t) {
        return dispatch_in(out_dtype, [&](auto out_t) {
            return launch_combine<decltype(in_t)::value, decltype(out_t)::value>(y, rows, N, ld_y, row_of, weights, T, k, out, ld_out, s);
        });
    });
}
