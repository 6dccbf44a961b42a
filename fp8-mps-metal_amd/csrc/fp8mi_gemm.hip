// LDS-tiled FP8 e4m3fn GEMM for gfx950 on the CDNA4 scaled-MFMA path:
//
//     C[m,n] = cast(((sum_k dec(A[m,k]) dec(B[n,k])) * sa[m] * sb[n] + bias[n]) * sr)
//
// Replaces fp8_scaled_matmul_kernel (fp8_matmul.metal:99-147: one thread per
// output, 2K scalar byte loads and 2K software decodes per output, no reuse)
// and the dequant -> fp16 matmul detour fp8_scaled_mm_fast
// (fp8_mps_native.py:213-267).  Design, MI355X-first:
//
//   * math: v_mfma_scale_f32_16x16x128_f8f6f4 with both block scales = 2^0.
//     It consumes OCP e4m3fn bytes directly (no decode instructions at all) at
//     twice the rate of the non-scaled fp8 MFMA; fp32 accumulators.
//   * both operands are "K-contiguous rows" (A is (M,K), B is (N,K)), so one
//     staging routine and one fragment reader serve both.  The MFMA pairs the
//     j-th byte of lane-group g of its two operands, so any assignment of the
//     128 k-bytes of a step to (g, j) is correct as long as A and B use the
//     same one; we use chunk g and chunk 4+g (16-byte chunks) for lane group
//     g, which with the XOR swizzle below makes every ds_read_b128 of a
//     fragment bank-conflict free.
//   * staging: buffer_load_dwordx4 ... lds (HBM/L2 -> LDS without touching
//     VGPRs).  One wave-instruction moves 8 rows x 128 B = whole cache lines.
//     The LDS image is lane-linear (hardware rule), so the swizzle
//     chunk' = chunk ^ ((row >> 1) & 7) is applied to the per-lane SOURCE
//     address and again on the fragment read.  Rows >= M / N and the K tail
//     are masked by pointing the lane outside the buffer (hardware returns 0,
//     and a zero byte is +0.0 in e4m3).
//   * pipeline: an NSTAGE-deep LDS ring.  NSTAGE-1 K-steps of LDS-DMA stay in
//     flight ACROSS the per-step barrier: the wait is a counted
//     `s_waitcnt vmcnt(n)` (n = loads of the newer stages), the barrier a raw
//     s_barrier - a __syncthreads() would drain the DMA queue (vmcnt(0)) and
//     expose a full memory round trip per K-step (measured on the 2-stage
//     version of this kernel: 49-66 % of wave time parked in waits,
//     profiles/r01_v1_*).  One barrier per K-step.  (Ping-pong wave groups, an
//     in-wave software pipeline and interleaved DMA issue were built and
//     measured too - none beat this loop, see DESIGN.md 6 - and were removed.)
//   * output orientation: the W fragment is the MFMA "A" operand and the X
//     fragment the "B" operand, so each lane ends up with 4 CONSECUTIVE n of
//     one row m in an accumulator register quad -> one 16-byte store.
//   * the epilogue (scales, bias, result scale, cast) is fused.
//   * block -> tile mapping is XCD-aware: the 8 XCDs get contiguous runs of
//     tiles in a grouped order (4 m-tiles x all n-tiles per group), so the
//     tiles an XCD runs at one time share a few A and B panels in its L2.
//   * split-K (fp8mi_scaled_mm_ws): when the tile grid leaves most CUs idle,
//     K is cut into slices, one workgroup per (tile, slice); fp32 partial
//     tiles meet in a caller-owned workspace and the last workgroup of a tile
//     to arrive adds them in slice order and runs the epilogue.
//
// NaN bytes: the hardware treats 0x7F/0xFF as NaN; the reference decodes them
// to 0.0 (fp8_matmul.metal:21).  The K loop runs unscrubbed; because finite
// e4m3 products cannot overflow fp32, a NaN accumulator proves a NaN byte was
// involved, and only then the workgroup redoes its tile with a SWAR scrub of
// every fragment.  Clean inputs (everything the reference's encoder can emit)
// never pay for it.  The block-scaled (MXFP8) instances run the same check and redo, but there a NaN accumulator
// proves less: finite products times scales up to 2^254 CAN overflow fp32, and inf - inf is NaN.  Such a redo only costs
// time - the scrubbed pass overflows the same way and gives the same result.  The MXFP4 instances have neither: e2m1 has
// no NaN encoding, and a scrub would zero finite bytes.

#include "fp8mi_gemm_epi.h"
#include "fp8mi_dispatch.h"
#include "fp8mi_group_slot.h"

namespace {

template <int BM, int BN, int WM, int WN, int NSTAGE_, int MODE_ = 0, int ABL_ = 0, int KS_ = 1, int LD_ = 0, int MXS_ = 0, int FMT_ = 0>
struct Cfg {
    // Operand formats of the tensorwise instances (FMT_ = a_format + 2 * b_format, FP8MI_FMT_*): the MFMA's format codes, 0 = e4m3, 1 = e5m2.
    // The W fragment (rows of B_nk) is the MFMA "A" operand, so cbsz carries B's format and blgp A's.  FMT_ != 0: OCP semantics only -
    // no NaN verdict, no scrubbed redo (an e5m2 inf is a legal value, and inf - inf a legal NaN).
    static constexpr int FW = (FMT_ >> 1) & 1, FX = FMT_ & 1;
    static constexpr bool OCP = FMT_ != 0;
    static_assert(FMT_ >= 0 && FMT_ <= 3 && (FMT_ == 0 || MXS_ == 0), "the block-scaled and blockwise forms are e4m3 / e2m1 only");
    // MXS_ = 4 (MXW4A8): e2m1 W rows against e4m3 X rows.  A 128-byte K-step of W is 256 k and meets TWO 128-byte K-steps
    // of X ("X sub-steps"), staged as kXS images of the X rows ahead of the W rows; K, the K tail and the split-K slices count W bytes
    static constexpr bool W4A8 = MXS_ == 4;
    static constexpr int kXS = W4A8 ? 2 : 1;
    static_assert(MXS_ != 4 || (KS_ == 1 && MODE_ == 0 && ABL_ == 0), "the mixed form: one 256-k K-step per ring stage, the plain loop order, no L2 prefetch");

    static constexpr int KS = KS_;      // K-steps (of 128 bytes) per ring stage: KS = 2 halves the barriers per byte
    static constexpr int PFD = ABL_ & 7;  // L2 prefetch distance in ring stages beyond the stage being staged (0 = none): see prefetch_stage
    static constexpr int PFA = (ABL_ >> 3) & 1;  // diagnostic variants: one more wave warms this tile's share of its A panel's lines too
    // Timing-only FLOOR forms of a tile kernel (wrong results; instantiated ONLY by tools/floor_probe.hip, which compiles this file with
    // FP8MI_FLOOR_PROBE for bench.py's `roofline.floor`): 1 = the K loop's LDS-DMA stream, waits and barriers without fragment reads and MFMAs;
    // 2 = no K loop at all (launch, arguments, tile map, the C store of the fused epilogue, kernel end); 3 = return behind the argument loads
    // (the launch itself with this kernel's grid, block and LDS allocation).  What each leaves out is hidden under the others in the real
    // kernel, so the floors bound the kernel from below; they do not add up to it.
    static constexpr int FLOOR = (ABL_ >> 4) & 3;
    // Timing-only, diagnostic library (ids 137, 138): the B operand's stage loads go into a register sink as plain `buffer_load_dwordx4` instead of
    // through the LDS-DMA (the B half of the ring stays zero: wrong results).  An upper bound on what a register-staged W loader could gain on the
    // weight-streaming shapes, where plain loads were probed 10-15 % faster than the DMA path (profiles/r04_wstream_probe.txt).
    static constexpr bool BREG = ((ABL_ >> 6) & 1) != 0;
    // Timing experiment, diagnostic library (id 144): the K slices of a tile on ONE XCD (consecutive entries of the XCD's run of the work list) and the
    // split-K exchange at GROUP scope - stores that stop at the XCD's L2, loads that start there, the arrival counter in it.  Right only as long as
    // workgroup b really runs on XCD b mod 8, which the product never relies on for correctness (fp8mi_gemm_epi.h): it measures what that reliance would buy.
    static constexpr bool XLOCAL = ((ABL_ >> 7) & 1) != 0;
    static constexpr int MODE = MODE_;  // 0: stage DMA issued first, then fragment reads + MFMAs; 1: fragment reads first (see run_tile)
    static constexpr int NSTAGE = NSTAGE_;
    static constexpr int PF = NSTAGE_ - 1;  // K-steps of loads in flight
    static constexpr int kWavesM = BM / WM;
    static constexpr int kWavesN = BN / WN;
    static constexpr int kWaves = kWavesM * kWavesN;
    static constexpr int kThreads = kWaves * 64;
    static constexpr int kCThreads = kThreads;  // every wave holds accumulators
    static constexpr int TM = WM / 16;
    static constexpr int TN = WN / 16;
    static constexpr int kGroupsA = BM / 8;  // 8-row staging groups
    static constexpr int kGroupsB = BN / 8;
    static constexpr int kGroups = kXS * kGroupsA + kGroupsB;   // per K-step
    static constexpr int kStepBytes = (kXS * BM + BN) * BK;
    // Waves that issue the LDS-DMA (0 = all).  Every 1-KiB DMA instruction takes ~16 cycles in the CU's
    // one address path and blocks its wave until accepted; with all waves loading, both waves of a SIMD
    // sit in that queue at the head of each K-step and the matrix pipe idles (measured with in-kernel
    // stamps).  With kLoaders = kWaves / 2 only waves 0..kLoaders-1 (one per SIMD) load, and their SIMD
    // partners start the step's fragment reads and MFMAs at once.
    static constexpr int kLoaders = LD_ == 0 ? kWaves : LD_;
    static constexpr int kGroupsPerWave = KS_ * kGroups / kLoaders;  // per stage, per loading wave
    // Block-scaled (MXFP8) instances: every ring stage also carries the stage's E8M0 scales, staged by the same loading waves
    // with 4-byte LDS-DMA pieces (64 rows x one K-step's 4 blocks each: X rows first, then W rows), behind the operand bytes
    static constexpr bool MXS = MXS_ != 0;
    // MXS_ = 2 (MXFP4): e2m1 operands, two per byte - a 128-byte K-step is 256 k, 8 blocks, two MFMAs of 4 blocks each; its
    // scales are two 4-byte pieces per row ("halves": blocks 0-3, then 4-7), so a row's scale stride needs only 4-byte alignment
    static constexpr bool FP4 = MXS_ == 2;
    // MXS_ = 3 (blockwise, "1x128 / 128x128"): one fp32 scale per row and K-step, staged in the same 4-byte pieces; the MFMAs run
    // with unit block scales and every K-step's product is folded into the accumulators with its scale product (mfma_fold_bw)
    static constexpr bool BW = MXS_ == 3;
    static constexpr int kScaleHalves = FP4 || W4A8 ? 2 : 1;   // (W4A8: the MXFP4 scale layout, both sides)
    static constexpr int kScalePiecesA = (BM + 63) / 64, kScalePieces = kScalePiecesA + (BN + 63) / 64;   // per K-step (per half)
    static constexpr int kScaleLoadsPerWave = MXS ? (KS_ * kScaleHalves * kScalePieces + kLoaders - 1) / kLoaders : 0;   // per stage, per loading wave
    static constexpr int kScaleBytes = MXS ? (kScaleLoadsPerWave * kLoaders * 256 + 1023) / 1024 * 1024 : 0;
    static constexpr int kLoadsPerWave = kGroupsPerWave + kScaleLoadsPerWave;   // LDS-DMA instructions per stage, per loading wave
    static constexpr int kStageBytes = KS_ * kStepBytes + kScaleBytes;
    static_assert(kGroupsA % kLoaders == 0 && kGroupsB % kLoaders == 0 && kLoaders % 2 == 0 && kLoaders <= kWaves,
                  "each loading wave stages whole groups of both operands; the shared swizzle needs an even count");
    static constexpr int kRingBytes = NSTAGE_ * kStageBytes;
    static_assert(NSTAGE_ >= 2 && NSTAGE_ <= 6 && (NSTAGE_ - 1) * kLoadsPerWave <= 63, "vmcnt is a 6-bit counter");
    static_assert(kRingBytes + 16 <= 160 * 1024, "LDS is 160 KiB per CU");
    static_assert(MODE_ >= 0 && MODE_ <= 2 && (MODE_ != 2 || KS_ == 1), "three orders of the loop body are built (the staggered one for KS = 1)");
};

// one K-step's fragments: LDS -> registers
template <typename C, bool SCRUB>
FP8MI_DEVICE void load_frags(const uint8_t *a_rows, const uint8_t *b_rows, int a_row0 /* m */, int b_row0 /* n */,
                             uint32_t off1, uint32_t off2, i32x8 (&xf)[C::TM], i32x8 (&wf)[C::TN])
{
    const uint8_t *sa = a_rows + a_row0 * BK;   // X rows (m)
    const uint8_t *sB = b_rows + b_row0 * BK;   // W rows (n)
#pragma unroll
    for (int t = 0; t < C::TM; ++t) {
        i32x4 lo = *(const i32x4 *)(sa + t * 16 * BK + off1);
        i32x4 hi = *(const i32x4 *)(sa + t * 16 * BK + off2);
        xf[t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int t = 0; t < C::TN; ++t) {
        i32x4 lo = *(const i32x4 *)(sB + t * 16 * BK + off1);
        i32x4 hi = *(const i32x4 *)(sB + t * 16 * BK + off2);
        wf[t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    if (SCRUB) {
#pragma unroll
        for (int t = 0; t < C::TM; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[t][j] = (int)scrub_nan4((uint32_t)xf[t][j]);
#pragma unroll
        for (int t = 0; t < C::TN; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) wf[t][j] = (int)scrub_nan4((uint32_t)wf[t][j]);
    }
}

// registers -> MFMAs (W fragment is the MFMA "A" operand, X fragment the "B" operand)
template <typename C>
FP8MI_DEVICE void mfma_all(const i32x8 (&xf)[C::TM], const i32x8 (&wf)[C::TN], f32x4 (&acc)[C::TN][C::TM])
{
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[tn], xf[tm], acc[tn][tm], C::FW, C::FX, 0,
                                                                            kScaleOne, 0, kScaleOne);
}

template <typename C, bool SCRUB>
FP8MI_DEVICE void compute_step(const uint8_t *stage, int a_row0, int b_row0, uint32_t off1, uint32_t off2,
                               f32x4 (&acc)[C::TN][C::TM])
{
    i32x8 xf[C::TM], wf[C::TN];
    load_frags<C, SCRUB>(stage, stage + C::kGroupsA * 1024, a_row0, b_row0, off1, off2, xf, wf);  // per K-step: A's rows, then B's
    mfma_all<C>(xf, wf, acc);
}

// ---- block-scaled (MXFP8) instances ------------------------------------------------------------------------------
// The scale operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands, measured with exact data
// (tools/probes/mxfp8_scale_probe.hip, profiles/mxfp8_scale_map.txt): lane group g, register half h (bytes 16h .. 16h + 15 of
// the lane's 32) holds hardware K = 64h + 16g + j, i.e. 32-K block 2h + g / 2; the scale of (row r, block b) is the byte op_sel
// picks from lane 16b + r's scale operand - both operands alike.  The ring kernels' staging (chunks g and 4 + g of a K-step
// for lane group g) is therefore already the hardware's own K order: the block-scaled instances stage the operands exactly as
// the tensorwise ones, and lane (r, g) supplies the scale of its row r, block g of the K-step.

// lane constants of the scale reads (empty for the tensorwise instances)
template <typename C, bool = C::MXS> struct MxLane { };
template <typename C> struct MxLane<C, true> {
    uint32_t xo, wo;        // LDS offset of this lane's X / W scale byte in a K-step's scale area (fragment 0)
    uint32_t rows_ok;       // bit tm: X row of fragment tm is inside the tensor; bit 16 + tn: W row of fragment tn
    int64_t kend;           // K - 32 x (this lane's block in the step): the block is real while kstep x 128 < kend (C::FP4: bytes, K / 2 - 16 x block)
};

// four fragments' scale bytes per register (op_sel picks the byte): the 256x256 tile keeps a K-step's scales across its barrier
template <typename C> struct StepScales { uint32_t x[(C::TM + 3) / 4], w[(C::TN + 3) / 4]; };

// one K-step's scale bytes: LDS -> registers.  Rows past the tensor and blocks past K carry 2^0 (0x7F) - their operand
// bytes are zero, and a zero times the NaN scale 0xFF would be NaN.
// koff: the bytes of the K-step before this scale half (C::FP4: 64 for blocks 4-7)
template <typename C>
FP8MI_DEVICE void load_scales(const uint8_t *sc, const MxLane<C, true> &ml, int64_t kstep, StepScales<C> &s, int koff = 0)
{
    const bool kin = kstep * BK + koff < ml.kend;
#pragma unroll
    for (int t = 0; t < (C::TM + 3) / 4; ++t) s.x[t] = 0u;
#pragma unroll
    for (int t = 0; t < (C::TN + 3) / 4; ++t) s.w[t] = 0u;
#pragma unroll
    for (int t = 0; t < C::TM; ++t) {
        const uint32_t b = sc[ml.xo + t * 64];
        s.x[t >> 2] |= ((kin && ((ml.rows_ok >> t) & 1u)) ? b : 0x7Fu) << (8 * (t & 3));
    }
#pragma unroll
    for (int t = 0; t < C::TN; ++t) {
        const uint32_t b = sc[ml.wo + t * 64];
        s.w[t >> 2] |= ((kin && ((ml.rows_ok >> (16 + t)) & 1u)) ? b : 0x7Fu) << (8 * (t & 3));
    }
}

// one scaled MFMA with the scale bytes ow / ox of sw / sx (constants once the callers' loops are unrolled).  FW / FX: the format codes of
// the W ("A" operand) and X fields - (0, 0) e4m3 x e4m3, (4, 4) e2m1 x e2m1, (4, 0) e2m1 W x e4m3 X; an e2m1 operand's low 4 registers are read
template <int FW, int FX>
FP8MI_DEVICE f32x4 mfma_mx(i32x8 w, i32x8 x, f32x4 c, uint32_t sw, int ow, uint32_t sx, int ox)
{
#define FP8MI_MX_CASE(a, b) \
    case a * 4 + b: return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, FW, FX, a, (int)sw, b, (int)sx);
    switch (ow * 4 + ox) {
        FP8MI_MX_CASE(0, 0) FP8MI_MX_CASE(0, 1) FP8MI_MX_CASE(0, 2) FP8MI_MX_CASE(0, 3)
        FP8MI_MX_CASE(1, 0) FP8MI_MX_CASE(1, 1) FP8MI_MX_CASE(1, 2) FP8MI_MX_CASE(1, 3)
        FP8MI_MX_CASE(2, 0) FP8MI_MX_CASE(2, 1) FP8MI_MX_CASE(2, 2) FP8MI_MX_CASE(2, 3)
        FP8MI_MX_CASE(3, 0) FP8MI_MX_CASE(3, 1) FP8MI_MX_CASE(3, 2) FP8MI_MX_CASE(3, 3)
    default: return c;
    }
#undef FP8MI_MX_CASE
}

// the W fragment is the MFMA "A" operand: its scale goes in the scale_a slot
template <typename C>
FP8MI_DEVICE void mfma_all(const i32x8 (&xf)[C::TM], const i32x8 (&wf)[C::TN], f32x4 (&acc)[C::TN][C::TM], const StepScales<C> &s)
{
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = mfma_mx<0, 0>(wf[tn], xf[tm], acc[tn][tm], s.w[tn >> 2], tn & 3, s.x[tm >> 2], tm & 3);
}

// ---- MXFP4 (C::FP4) ----------------------------------------------------------------------------------------------
// The e2m1 operand map, measured with exact data (tools/probes/mxfp4_map_probe.hip, profiles/mxfp4_operand_map.txt): the
// instruction reads only the low 4 of the 8 operand registers, and lane group g's 16 bytes there are ONE 32-k block, block g
// (k = 32g + 2t + n for nibble n of byte t, the low nibble first); the scale of (row r, block b) comes from lane 16b + r.  A
// lane's two staged chunks are therefore two whole blocks: chunk g (fragment registers 0-3) is block g of the K-step's first
// 128 k, chunk 4 + g (registers 4-7) block g of its last 128 k.  Staging and fragment reads stay as they are; each fragment
// feeds two MFMAs, one per half, each with its own scale byte.

// registers 4-7 of a fragment as an operand's low 4 (a subregister: no copies)
FP8MI_DEVICE i32x8 frag_hi(i32x8 f) { return __builtin_shufflevector(f, f, 4, 5, 6, 7, 4, 5, 6, 7); }

// one K-step: every fragment pair's first half (blocks 0-3), then its second half (blocks 4-7).  `sc` is the K-step's scale area
template <typename C>
FP8MI_DEVICE void mfma_step_fp4(const i32x8 (&xf)[C::TM], const i32x8 (&wf)[C::TN], f32x4 (&acc)[C::TN][C::TM], const uint8_t *sc,
                                const MxLane<C> &ml, int64_t kstep)
{
    StepScales<C> s0, s1;
    load_scales<C>(sc, ml, kstep, s0);
    load_scales<C>(sc + C::kScalePieces * 256, ml, kstep, s1, 64);
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = mfma_mx<4, 4>(wf[tn], xf[tm], acc[tn][tm], s0.w[tn >> 2], tn & 3, s0.x[tm >> 2], tm & 3);
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = mfma_mx<4, 4>(frag_hi(wf[tn]), frag_hi(xf[tm]), acc[tn][tm], s1.w[tn >> 2], tn & 3, s1.x[tm >> 2], tm & 3);
}

// ---- MXW4A8 (C::W4A8) --------------------------------------------------------------------------------------------
// e2m1 W against e4m3 X in one instruction: format code 4 in the W ("A" operand) field, 0 in the X field.  Measured with exact data
// (tools/probes/mxw4a8_map_probe.hip, profiles/mxw4a8_operand_map.txt): each operand keeps the map of its own format - the W lane
// group g's low four registers are block g (k = 32g + 2t + n), the X lane group g's register half h holds k = 64h + 16g + j - and the
// scale of (row r, block b) comes from lane 16b + r on both sides.  So the staged images are the two recipes' own: a W fragment's low
// four registers (chunk g) are block g of the K-step's first 128 k and meet the X fragment of sub-step 0; its high four (chunk 4 + g)
// are block g of the last 128 k and meet sub-step 1.  Two MFMAs per fragment pair, each with its own scale byte on each side.

// one K-step (256 k) of the mixed form: `st` the stage's operand bytes (X sub-step 0, X sub-step 1, W), `sc` its scale area.
// SCRUB touches the X fragments only: e2m1 has no NaN encoding, and a scrub of W would zero the finite codes 0x7F / 0xFF.
template <typename C, bool SCRUB>
FP8MI_DEVICE void step_w4a8(const uint8_t *st, const uint8_t *sc, int a_row0, int b_row0, uint32_t off1, uint32_t off2, const MxLane<C> &ml,
                            int64_t kstep, f32x4 (&acc)[C::TN][C::TM])
{
    i32x8 x0[C::TM], x1[C::TM], wf[C::TN];
    const uint8_t *sx0 = st + a_row0 * BK, *sx1 = sx0 + C::kGroupsA * 1024, *sw = st + 2 * C::kGroupsA * 1024 + b_row0 * BK;
#pragma unroll
    for (int t = 0; t < C::TM; ++t) {
        const i32x4 lo0 = *(const i32x4 *)(sx0 + t * 16 * BK + off1), hi0 = *(const i32x4 *)(sx0 + t * 16 * BK + off2);
        const i32x4 lo1 = *(const i32x4 *)(sx1 + t * 16 * BK + off1), hi1 = *(const i32x4 *)(sx1 + t * 16 * BK + off2);
        x0[t] = i32x8{lo0[0], lo0[1], lo0[2], lo0[3], hi0[0], hi0[1], hi0[2], hi0[3]};
        x1[t] = i32x8{lo1[0], lo1[1], lo1[2], lo1[3], hi1[0], hi1[1], hi1[2], hi1[3]};
    }
#pragma unroll
    for (int t = 0; t < C::TN; ++t) {
        const i32x4 lo = *(const i32x4 *)(sw + t * 16 * BK + off1), hi = *(const i32x4 *)(sw + t * 16 * BK + off2);
        wf[t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    if (SCRUB) {
#pragma unroll
        for (int t = 0; t < C::TM; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x0[t][j] = (int)scrub_nan4((uint32_t)x0[t][j]);
                x1[t][j] = (int)scrub_nan4((uint32_t)x1[t][j]);
            }
    }
    StepScales<C> s0, s1;
    load_scales<C>(sc, ml, kstep, s0);
    load_scales<C>(sc + C::kScalePieces * 256, ml, kstep, s1, 64);
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = mfma_mx<4, 0>(wf[tn], x0[tm], acc[tn][tm], s0.w[tn >> 2], tn & 3, s0.x[tm >> 2], tm & 3);
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm)
            acc[tn][tm] = mfma_mx<4, 0>(frag_hi(wf[tn]), x1[tm], acc[tn][tm], s1.w[tn >> 2], tn & 3, s1.x[tm >> 2], tm & 3);
}

// ---- blockwise (C::BW) -------------------------------------------------------------------------------------------
// A K-step of 128 bytes is one 128-k scale block.  Its scale area holds one fp32 per X row (m), then one per W row (n); lane
// (fr, fg) of fragment (tn, tm) holds the 4 consecutive n = wn0 + 16 tn + 4 fg + j of row m = wm0 + 16 tm + fr, so it reads one
// X scale per tm (ml.xo) and four W scales per tn (ml.wo, one 16-byte read).  Each MFMA starts from zero with unit block scales
// (P_b exactly as the tensorwise instances sum a K-step) and is folded as acc = fma(P_b, sa * sb, acc), sa * sb rounded to
// fp32; the fold of one product is written next to the issue of the next MFMA, which does not depend on it.
// (the scale products and the results each pass an empty asm on their own: four adjacent multiplies and fmas building the
// accumulator quad are otherwise SLP-packed into v_pk_mul_f32 / v_pk_fma_f32, which cost more than the scalar forms next to
// MFMAs - MI355X_MICROARCH.md)
template <typename C>
FP8MI_DEVICE void fold_bw(f32x4 &acc, const f32x4 &pb, float sa, const f32x4 &sb)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = sa * sb[j];
        asm("" : "+v"(s));
        float r = __builtin_fmaf(pb[j], s, acc[j]);
        asm("" : "+v"(r));
        acc[j] = r;
    }
}

template <typename C>
FP8MI_DEVICE void mfma_fold_bw(const i32x8 (&xf)[C::TM], const i32x8 (&wf)[C::TN], f32x4 (&acc)[C::TN][C::TM], const uint8_t *sc,
                               const MxLane<C> &ml)
{
    float sa[C::TM];
    f32x4 sb[C::TN];
#pragma unroll
    for (int t = 0; t < C::TM; ++t) sa[t] = *(const float *)(sc + ml.xo + t * 64);
#pragma unroll
    for (int t = 0; t < C::TN; ++t) sb[t] = *(const f32x4 *)(sc + ml.wo + t * 64);
    f32x4 prev = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < C::TN * C::TM; ++i) {
        const int tn = i / C::TM, tm = i % C::TM;
        const f32x4 cur = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[tn], xf[tm], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0,
                                                                          kScaleOne, 0, kScaleOne);
        if (i > 0) fold_bw<C>(acc[(i - 1) / C::TM][(i - 1) % C::TM], prev, sa[(i - 1) % C::TM], sb[(i - 1) / C::TM]);
        prev = cur;
    }
    constexpr int kLast = C::TN * C::TM - 1;
    fold_bw<C>(acc[kLast / C::TM][kLast % C::TM], prev, sa[kLast % C::TM], sb[kLast / C::TM]);
}

template <typename C, bool SCRUB>
FP8MI_DEVICE void compute_step(const uint8_t *stage, int q, int a_row0, int b_row0, uint32_t off1, uint32_t off2,
                               const MxLane<C> &ml, int64_t kstep, f32x4 (&acc)[C::TN][C::TM])
{
    if constexpr (C::W4A8) {
        step_w4a8<C, SCRUB>(stage + q * C::kStepBytes, stage + C::KS * C::kStepBytes + q * 2 * C::kScalePieces * 256, a_row0, b_row0, off1, off2, ml, kstep, acc);
    } else if constexpr (C::BW) {
        i32x8 xf[C::TM], wf[C::TN];
        const uint8_t *st = stage + q * C::kStepBytes;
        load_frags<C, SCRUB>(st, st + C::kGroupsA * 1024, a_row0, b_row0, off1, off2, xf, wf);
        mfma_fold_bw<C>(xf, wf, acc, stage + C::KS * C::kStepBytes + q * C::kScalePieces * 256, ml);
    } else if constexpr (C::FP4) {
        i32x8 xf[C::TM], wf[C::TN];
        const uint8_t *st = stage + q * C::kStepBytes;
        load_frags<C, false>(st, st + C::kGroupsA * 1024, a_row0, b_row0, off1, off2, xf, wf);
        mfma_step_fp4<C>(xf, wf, acc, stage + C::KS * C::kStepBytes + q * 2 * C::kScalePieces * 256, ml, kstep);
    } else if constexpr (C::MXS) {
        i32x8 xf[C::TM], wf[C::TN];
        StepScales<C> sc;
        const uint8_t *st = stage + q * C::kStepBytes;
        load_frags<C, SCRUB>(st, st + C::kGroupsA * 1024, a_row0, b_row0, off1, off2, xf, wf);
        load_scales<C>(stage + C::KS * C::kStepBytes + q * C::kScalePieces * 256, ml, kstep, sc);
        mfma_all<C>(xf, wf, acc, sc);
    } else {
        compute_step<C, SCRUB>(stage + q * C::kStepBytes, a_row0, b_row0, off1, off2, acc);
    }
}

// Per-lane staging plan.  A wave stages kGroupsPerWave 1-KiB groups per stage
// (8 rows x 128 B each).  Its groups of one operand are kWaves * 8 rows apart and
// - because kWaves is even - share one swizzled chunk, so the whole plan is two
// base offsets, a row and a K position; rows are only bounds-checked in ragged
// (edge) tiles.
// the block-scaled instances' scale staging: per scale piece this wave issues, its descriptor (X or W scales) and lane offset
template <typename C, bool = C::MXS> struct ScaleStage { };
template <typename C> struct ScaleStage<C, true> {
    __amdgpu_buffer_rsrc_t rx, rw;             // this tile's rows of the X / W scales
    uint32_t voff[C::kScaleLoadsPerWave];      // row x ld_s + 4 x (K-step in the stage), or kOOB
    bool is_x[C::kScaleLoadsPerWave];          // wave-uniform
    // C::BW: bytes between the X / W scales of consecutive K-steps, the K-steps that exist, and each piece's K-step in the stage
    uint32_t kx, kw;
    int nkb;
    int q[C::kScaleLoadsPerWave];              // wave-uniform
};

template <typename C>
struct StagePlan {
    uint32_t va0, vb0;  // byte offset of this lane's 16 bytes in the wave's first A / B group
    uint32_t row0;      // its row there (the same for A and B)
    uint32_t kpos;      // chunk * 16: position inside the 128-byte K-step
    uint32_t sa, sb;    // uniform byte stride between the wave's consecutive A / B groups
    int rows_a, rows_b; // valid rows of this tile
    bool full;          // interior tile: no row masking
    uint32_t pf_off;    // C::PFD: this lane's line of the B panel's share to prefetch (kOOB: none)
    u32x4 pf_rsrc;      // ... and the B panel's descriptor as plain words (an asm operand)
    int pf_waves;       // how many waves prefetch (1 when the panel has 4 readers on the XCD, 2 with 2, 0 when this tile is its only reader)
    mutable u32x4 bsink;  // C::BREG (timing-only): landing registers of the B operand's plain loads (never read)
    ScaleStage<C> sc;     // C::MXS: the stage's scale pieces
};

template <typename C, bool TAIL>
FP8MI_DEVICE void issue_stage(const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb,
                              uint8_t *stage, int wave, int k0, int64_t K)
{
    constexpr int JA = C::kGroupsA / C::kLoaders, JB = C::kGroupsB / C::kLoaders, JS = JA + JB;
    if (C::kLoaders < C::kWaves && wave >= C::kLoaders) return;  // wave-uniform: this wave does not load
    if constexpr (C::W4A8) {
        // the stage (one K-step, k0 = its first W byte): X sub-steps 0 and 1 - the 256 X bytes from 2 x k0 - then the W rows; K counts W bytes
#pragma unroll
        for (int j = 0; j < C::kGroupsPerWave; ++j) {
            const bool is_a = j < 2 * JA;
            const int sub = j / JA, jo = is_a ? j % JA : j - 2 * JA;   // (sub: 0, 1 = the X sub-step; 2 = W)
            const int gs = (is_a ? sub * C::kGroupsA : 2 * C::kGroupsA) + wave + jo * C::kLoaders;  // LDS group slot (wave-uniform)
            uint32_t vo = is_a ? pl.va0 + jo * pl.sa + sub * BK : pl.vb0 + jo * pl.sb;
            if (!pl.full && (int)(pl.row0 + jo * C::kLoaders * 8) >= (is_a ? pl.rows_a : pl.rows_b)) vo = kOOB;
            if (TAIL && (is_a ? 2 * (int64_t)k0 + sub * BK + pl.kpos >= 2 * K : (int64_t)k0 + pl.kpos >= K)) vo = kOOB;
            lds_void *dst = (lds_void *)(stage + gs * 1024);
            if (is_a) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, dst, 16, (int)vo, 2 * k0, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, dst, 16, (int)vo, k0, 0, 0);
        }
    } else {
#pragma unroll
    for (int j = 0; j < C::kGroupsPerWave; ++j) {
        const int q = j / JS, jj = j % JS;            // K-step inside the stage, group inside the K-step
        const bool is_a = jj < JA;
        const int jo = is_a ? jj : jj - JA;
        const int gs = q * C::kGroups + (is_a ? 0 : C::kGroupsA) + wave + jo * C::kLoaders;  // LDS group slot (wave-uniform)
        uint32_t vo = (is_a ? pl.va0 + jo * pl.sa : pl.vb0 + jo * pl.sb) + q * BK;
        if (!pl.full && (int)(pl.row0 + jo * C::kLoaders * 8) >= (is_a ? pl.rows_a : pl.rows_b)) vo = kOOB;
        if (TAIL && (int64_t)k0 + q * BK + pl.kpos >= K) vo = kOOB;  // K tail: only in the peeled last step
        // the LDS image is consecutive 1-KiB groups (8 rows x 128 B), per K-step A's rows first, then B's
        lds_void *dst = (lds_void *)(stage + gs * 1024);
        if (is_a) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, dst, 16, (int)vo, k0, 0, 0);
        else if constexpr (C::BREG) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(pl.bsink) : "v"(vo), "s"(pl.pf_rsrc), "s"((uint32_t)k0) : "memory");
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, dst, 16, (int)vo, k0, 0, 0);
    }
    }
    if constexpr (C::BW) {
        // the stage's fp32 scales, piece wave + j x kLoaders: the K-step's offset goes into the lane offset (not the scalar one), so
        // that the descriptor's range check covers it; a K-step past the last block (the second of a KS = 2 stage) loads nothing
        const int kb = k0 / BK;
#pragma unroll
        for (int j = 0; j < C::kScaleLoadsPerWave; ++j) {
            lds_void *dst = (lds_void *)(stage + C::KS * C::kStepBytes + (wave + j * C::kLoaders) * 256);
            const uint32_t vo = kb + pl.sc.q[j] < pl.sc.nkb ? pl.sc.voff[j] + (uint32_t)kb * (pl.sc.is_x[j] ? pl.sc.kx : pl.sc.kw) : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pl.sc.is_x[j] ? pl.sc.rx : pl.sc.rw, dst, 4, (int)vo, 0, 0, 0);
        }
    } else if constexpr (C::MXS) {
        // the stage's scale bytes (one per 32-K block: byte k0 / 32 of a row is the stage's first block): piece wave + j x kLoaders
        // of the stage's scale area.  Rows are masked like the operands'; the K tail is not (the readers give its blocks 2^0).
        // C::FP4, C::W4A8: byte k0 / 16 (a byte of the stage holds two k)
#pragma unroll
        for (int j = 0; j < C::kScaleLoadsPerWave; ++j) {
            lds_void *dst = (lds_void *)(stage + C::KS * C::kStepBytes + (wave + j * C::kLoaders) * 256);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pl.sc.is_x[j] ? pl.sc.rx : pl.sc.rw, dst, 4, (int)pl.sc.voff[j], C::FP4 || C::W4A8 ? k0 / 16 : k0 / 32, 0, 0);
        }
    }
}

// Diagnostic build only (-DFP8MI_STAMP, never shipped): per-phase cycle sums of
// wave 0 of every workgroup, written over the first bytes of each C tile row 0.
#ifdef FP8MI_STAMP
#define STAMP(var)                                                                 \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        unsigned long long t_;                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                         \
        var = t_;                                                                  \
    } while (0)
__device__ unsigned long long g_stamp[256 * 32];  // per block: [wave 0 | wave kWaves/2] x 8 sums, then their 5 absolute stamps of step 5
#else
#define STAMP(var) do { } while (0)
#endif

template <int N>
FP8MI_DEVICE void wait_loads_and_lds()
{
    // this wave's LDS-DMA except the N youngest have landed; its ds_reads are done
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// wait until at most `newer_stages` stages' worth of this wave's LDS-DMA is outstanding
// (loads retire in issue order, so the older stage has landed), and its ds_reads are done
template <typename C>
FP8MI_DEVICE void wait_stage(int newer_stages)
{
    constexpr int G = C::kLoadsPerWave;
    if (5 * G <= 63 && newer_stages >= 5) wait_loads_and_lds<(5 * G <= 63 ? 5 * G : 0)>();
    else if (4 * G <= 63 && newer_stages == 4) wait_loads_and_lds<(4 * G <= 63 ? 4 * G : 0)>();
    else if (3 * G <= 63 && newer_stages == 3) wait_loads_and_lds<(3 * G <= 63 ? 3 * G : 0)>();
    else if (2 * G <= 63 && newer_stages == 2) wait_loads_and_lds<(2 * G <= 63 ? 2 * G : 0)>();
    else if (newer_stages == 1) wait_loads_and_lds<G>();
    else wait_loads_and_lds<0>();
}

template <typename C>
FP8MI_DEVICE void issue_any(const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb,
                            uint8_t *stage, int wave, int step, int nk, bool ktail, int64_t K)
{
    if (ktail && step == nk - 1) issue_stage<C, true>(pl, ra, rb, stage, wave, step * (BK * C::KS), K);
    else issue_stage<C, false>(pl, ra, rb, stage, wave, step * (BK * C::KS), K);
}

// The prologue of the K loop: the first PF stages of this workgroup's range (stage s -> ring slot s), walked from `rot` as the loop
// walks it.  The kernels issue it at ENTRY, as soon as the tile map, the two descriptors and the lane's staging offsets exist - the
// rest of the set-up (L2 prefetch plan, fragment offsets, scale lanes, epilogue scalars, NaN verdict word) is computed while these
// loads are in flight - and then run the loop with STAGED = true; the scrubbed redo pass (STAGED = false) issues its own.
template <typename C>
FP8MI_DEVICE void issue_prologue(const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, uint8_t *smem, int wave,
                                 int ks0, int nk, int rot, int64_t K)
{
    const int nk_all = (int)((K + BK * C::KS - 1) / (BK * C::KS));
    const bool ktail = (K % (BK * C::KS)) != 0;
    int ks = rot;
#pragma unroll
    for (int s = 0; s < C::PF; ++s)
        if (s < nk) {
            issue_any<C>(pl, ra, rb, smem + s * C::kStageBytes, wave, ks0 + ks, nk_all, ktail, K);
            ks = (ks + 1 == nk) ? 0 : ks + 1;
        }
}

// L2 prefetch (C::PFD > 0).  The tiles an XCD runs at one time are 4 m-tiles x 8 n-tiles (tile_of_block): a B panel - the
// weights, streamed from HBM - has 4 readers that ask for the same lines at the same time, and every one of them waits out
// the HBM latency inside the ring's prefetch window.  Wave 0 of each tile touches one dword per 128-byte line of ITS quarter of
// the panel for a stage PFD stages beyond the one being staged; the others then hit the L2.  The load's result is never used;
// the register it lands in (`sink`) is carried through the loop so that hipcc does not hand it to anything else.
FP8MI_DEVICE void prefetch_stage(uint32_t &sink, uint32_t voff, u32x4 rsrc, uint32_t koff)
{
    asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "+v"(sink) : "v"(voff), "s"(rsrc), "s"(koff) : "memory");
}

template <typename C, bool SCRUB, bool STAGED>
FP8MI_DEVICE void run_tile(const MMParams &p, uint8_t *smem, const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra,
                           __amdgpu_buffer_rsrc_t rb, int wave, int wm0, int wn0, uint32_t off1, uint32_t off2,
                           int ks0, int nk, int rot, const MxLane<C> &ml, f32x4 (&acc)[C::TN][C::TM])
{
    // ks0, nk: this workgroup's range of ring stages (all of K, or one split-K slice); rot in [0, nk)
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm) acc[tn][tm] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int64_t K = p.K;
    const int nk_all = (int)((K + BK * C::KS - 1) / (BK * C::KS));
    const bool ktail = (K % (BK * C::KS)) != 0;  // then the tile's last stage is staged with per-lane K masking
    if (nk == 0) return;
    unsigned long long p0_ = 0, p1_ = 0, p2_ = 0; (void)p0_; (void)p1_; (void)p2_;
    STAMP(p0_);

    // The K loop is walked circularly from `rot` (a per-m-tile offset): the tiles
    // that share a B panel run at the same time on one XCD, and if they all
    // started at k = 0 each of them would wait out HBM latency on the same lines;
    // staggered, each one fetches a different K range from HBM and finds the
    // rest already in the XCD's L2.  (Only the summation order changes.)
    int ks = rot;  // stage (relative to ks0) the next issue loads
    auto next_ks = [&]() { const int r = ks; ks = (ks + 1 == nk) ? 0 : ks + 1; return ks0 + r; };
    uint32_t sink = 0;  // C::PFD: landing register of the L2 prefetch loads (never read)
    auto prefetch = [&](int stage) {  // stage relative to ks0, clamped to this workgroup's last one
        if (C::PFD > 0 && wave < pl.pf_waves + C::PFA) prefetch_stage(sink, pl.pf_off, pl.pf_rsrc, (uint32_t)((ks0 + min(stage, nk - 1)) * (BK * C::KS)));
    };

    // prologue: PF stages in flight (stage s -> ring slot s); STAGED: the caller issued them at kernel entry (issue_prologue)
#pragma unroll
    for (int s = 0; s < C::PF; ++s)
        if (s < nk) {
            const int first = next_ks();
            if constexpr (!STAGED) issue_any<C>(pl, ra, rb, smem + s * C::kStageBytes, wave, first, nk_all, ktail, K);
        }
#pragma unroll
    for (int s = 0; s < C::PFD; ++s) prefetch(C::PF + s);

    STAMP(p1_);
    int slot = 0;             // ring slot of step t
    int fill = C::PF % C::NSTAGE;  // ring slot the next issue goes to (= slot of step t-1)
    unsigned long long c_wait = 0, c_bar = 0, c_issue = 0, c_comp = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    (void)c_wait; (void)c_bar; (void)c_issue; (void)c_comp; (void)s0; (void)s1; (void)s2; (void)s3; (void)s4;
    for (int t = 0; t < nk; ++t) {
        const int64_t kst = (int64_t)(ks0 + (rot + t < nk ? rot + t : rot + t - nk)) * C::KS;  // C::MXS: absolute K-step of the stage
        STAMP(s0);
        // stage t has landed for this wave once at most the newer stages' loads are outstanding
        wait_stage<C>(min(C::PF - 1, nk - 1 - t));
        STAMP(s1);
        __builtin_amdgcn_s_barrier();  // ... for every wave; and every wave is done reading slot of step t-1
        STAMP(s2);
        if constexpr (C::MODE == 1) {
            // reads first: this K-step's fragment reads are issued BEFORE the stage DMA, so that they land while the
            // loading waves sit in the DMA issue (a `buffer_load ... lds` holds its wave ~64 cycles: 1,085 cycles per
            // K-step on the 256x256 tile, in-kernel stamps) and the MFMAs start the moment the issue is through
            i32x8 xf[C::TM], wf[C::TN];
            const uint8_t *st = smem + slot * C::kStageBytes;
            if constexpr (C::FLOOR == 0) load_frags<C, SCRUB>(st, st + C::kGroupsA * 1024, wm0, wn0, off1, off2, xf, wf);
            __builtin_amdgcn_sched_barrier(0);
            if (t + C::PF < nk) {
                issue_any<C>(pl, ra, rb, smem + fill * C::kStageBytes, wave, next_ks(), nk_all, ktail, K);
                prefetch(t + C::PF + C::PFD);
            }
            STAMP(s3);
            if constexpr (C::FLOOR == 0 && C::BW) {
                mfma_fold_bw<C>(xf, wf, acc, st + C::KS * C::kStepBytes, ml);
#pragma unroll
                for (int q = 1; q < C::KS; ++q) compute_step<C, SCRUB>(st, q, wm0, wn0, off1, off2, ml, kst + q, acc);
            } else if constexpr (C::FLOOR == 0 && C::FP4) {
                mfma_step_fp4<C>(xf, wf, acc, st + C::KS * C::kStepBytes, ml, kst);
#pragma unroll
                for (int q = 1; q < C::KS; ++q) compute_step<C, SCRUB>(st, q, wm0, wn0, off1, off2, ml, kst + q, acc);
            } else if constexpr (C::FLOOR == 0 && C::MXS) {
                StepScales<C> sc;
                load_scales<C>(st + C::KS * C::kStepBytes, ml, kst, sc);
                mfma_all<C>(xf, wf, acc, sc);
#pragma unroll
                for (int q = 1; q < C::KS; ++q) compute_step<C, SCRUB>(st, q, wm0, wn0, off1, off2, ml, kst + q, acc);
            } else if constexpr (C::FLOOR == 0) {
                mfma_all<C>(xf, wf, acc);
#pragma unroll
                for (int q = 1; q < C::KS; ++q)
                    compute_step<C, SCRUB>(st + q * C::kStepBytes, wm0, wn0, off1, off2, acc);
            }
        } else {
            if (t + C::PF < nk) {
                issue_any<C>(pl, ra, rb, smem + fill * C::kStageBytes, wave, next_ks(), nk_all, ktail, K);
                prefetch(t + C::PF + C::PFD);
            }
            STAMP(s3);
            if constexpr (C::FLOOR == 0 && C::MXS) {
#pragma unroll
                for (int q = 0; q < C::KS; ++q) compute_step<C, SCRUB>(smem + slot * C::kStageBytes, q, wm0, wn0, off1, off2, ml, kst + q, acc);
            } else if constexpr (C::FLOOR == 0) {
#pragma unroll
                for (int q = 0; q < C::KS; ++q)
                    compute_step<C, SCRUB>(smem + slot * C::kStageBytes + q * C::kStepBytes, wm0, wn0, off1, off2, acc);
            }
        }
        STAMP(s4);
        c_wait += s1 - s0; c_bar += s2 - s1; c_issue += s3 - s2; c_comp += s4 - s3;
#ifdef FP8MI_STAMP
        if (t == 5 && (threadIdx.x & 63) == 0 && blockIdx.x < 256 && (wave == 0 || wave == C::kWaves / 2)) {
            unsigned long long *o = g_stamp + blockIdx.x * 32 + 16 + (wave ? 5 : 0);
            o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3; o[4] = s4;
        }
#endif
        slot = (slot + 1 == C::NSTAGE) ? 0 : slot + 1;
        fill = (fill + 1 == C::NSTAGE) ? 0 : fill + 1;
    }
#ifdef FP8MI_STAMP
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && (wave == 0 || wave == C::kWaves / 2)) {
        unsigned long long *o = g_stamp + blockIdx.x * 32 + (wave ? 8 : 0);
        o[0] = c_wait; o[1] = c_bar; o[2] = c_issue; o[3] = c_comp; o[4] = nk;
    }
#endif
    // all loads were waited for in the last iteration (newer_stages == 0); the caller's barrier makes the ring reusable
    if (C::PFD > 0) asm volatile("" ::"v"(sink));  // the prefetch loads' landing register stays reserved up to here
#ifdef FP8MI_STAMP
    STAMP(p2_);
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && wave == 0) {
        unsigned long long *o = g_stamp + blockIdx.x * 32 + 26;
        if (!STAGED) o[0] = p0_;   // (STAGED: the kernel stamps its own first DMA issue)
        o[1] = p1_; o[2] = p2_;
    }
    if (!STAGED && (threadIdx.x & 63) == 0 && blockIdx.x < 256 && wave == 1) g_stamp[blockIdx.x * 32 + 14] = p0_;   // wave 1: its first DMA issue
#endif
}

// STAGGERED wave groups (MODE 2).  Left alone all 8 waves run in lockstep: first everybody reads fragments (the LDS is
// the bottleneck and the matrix pipes idle: 192 KiB per K-step of a 256x256 tile = 768 cycles at 256 B/clk), then everybody
// multiplies (the LDS idles).  Here waves kWaves/2.. ("late") run half a step behind their SIMD partners: they multiply
// K-step t - 1, whose fragments they kept in registers across the barrier, while waves 0..kWaves/2-1 read K-step t; then
// they read K-step t while the partners multiply it.  Same instructions per wave, same registers, same number of
// barriers, bit-identical results; two separate loops so that each keeps one clean register assignment.
template <typename C, bool SCRUB, bool STAGED>
FP8MI_DEVICE void run_tile_staggered(const MMParams &p, uint8_t *smem, const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra,
                                     __amdgpu_buffer_rsrc_t rb, int wave, int wm0, int wn0, uint32_t off1, uint32_t off2,
                                     int ks0, int nk, int rot, const MxLane<C> &ml, f32x4 (&acc)[C::TN][C::TM])
{
    static_assert(C::KS == 1, "one K-step per ring stage");
    static_assert(!C::FP4 && !C::BW && !C::W4A8, "the MXFP4, MXW4A8 and blockwise instances are built on the MODE 0 / 1 loops");
#pragma unroll
    for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < C::TM; ++tm) acc[tn][tm] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t K = p.K;
    const int nk_all = (int)((K + BK - 1) / BK);
    const bool ktail = (K % BK) != 0;
    if (nk == 0) return;
    int ks = rot;
    auto next_ks = [&]() { const int r = ks; ks = (ks + 1 == nk) ? 0 : ks + 1; return ks0 + r; };
#pragma unroll
    for (int s = 0; s < C::PF; ++s)   // (STAGED: issued at kernel entry, issue_prologue)
        if (s < nk) {
            const int first = next_ks();
            if constexpr (!STAGED) issue_any<C>(pl, ra, rb, smem + s * C::kStageBytes, wave, first, nk_all, ktail, K);
        }
    int slot = 0, fill = C::PF % C::NSTAGE;
    auto advance = [&]() {
        slot = (slot + 1 == C::NSTAGE) ? 0 : slot + 1;
        fill = (fill + 1 == C::NSTAGE) ? 0 : fill + 1;
    };
    i32x8 xf[C::TM], wf[C::TN];
    StepScales<C> sc;   // C::MXS: kept with the fragments
// C::MXS: fragments and scales of step t together (the absolute K-step of step t is ks0 + (rot + t) mod nk)
#define FP8MI_READ_STEP(st, t)                                                                                                   \
    do {                                                                                                                         \
        load_frags<C, SCRUB>(st, st + C::kGroupsA * 1024, wm0, wn0, off1, off2, xf, wf);                                          \
        if constexpr (C::MXS) load_scales<C>(st + C::kStepBytes, ml, (int64_t)(ks0 + (rot + t < nk ? rot + t : rot + t - nk)), sc); \
    } while (0)
#define FP8MI_MULTIPLY()                                        \
    do {                                                        \
        if constexpr (C::MXS) mfma_all<C>(xf, wf, acc, sc);     \
        else mfma_all<C>(xf, wf, acc);                          \
    } while (0)
    if (wave < C::kWaves / 2) {  // early group: read, (load,) multiply
        for (int t = 0; t < nk; ++t) {
            wait_stage<C>(min(C::PF - 1, nk - 1 - t));
            __builtin_amdgcn_s_barrier();
            const uint8_t *st = smem + slot * C::kStageBytes;
            FP8MI_READ_STEP(st, t);
            __builtin_amdgcn_sched_barrier(0);
            if (t + C::PF < nk) issue_any<C>(pl, ra, rb, smem + fill * C::kStageBytes, wave, next_ks(), nk_all, ktail, K);
            FP8MI_MULTIPLY();
            advance();
        }
    } else {                     // late group: multiply the previous K-step, (load,) read this one
        for (int t = 0; t < nk; ++t) {
            wait_stage<C>(min(C::PF - 1, nk - 1 - t));
            __builtin_amdgcn_s_barrier();
            if (t > 0) {
                FP8MI_MULTIPLY();
#pragma unroll
                for (int tn = 0; tn < C::TN; ++tn)
#pragma unroll
                    for (int tm = 0; tm < C::TM; ++tm) asm volatile("" : "+v"(acc[tn][tm]));  // the MFMAs stay above the reads
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (t + C::PF < nk) issue_any<C>(pl, ra, rb, smem + fill * C::kStageBytes, wave, next_ks(), nk_all, ktail, K);
            const uint8_t *st = smem + slot * C::kStageBytes;
            FP8MI_READ_STEP(st, t);
            advance();
        }
        FP8MI_MULTIPLY();  // the last K-step
    }
#undef FP8MI_READ_STEP
#undef FP8MI_MULTIPLY
}

template <typename C, bool SCRUB, bool STAGED>
FP8MI_DEVICE void run_tile_any(const MMParams &p, uint8_t *smem, const StagePlan<C> &pl, __amdgpu_buffer_rsrc_t ra,
                               __amdgpu_buffer_rsrc_t rb, int wave, int wm0, int wn0, uint32_t off1, uint32_t off2,
                               int ks0, int nk, int rot, const MxLane<C> &ml, f32x4 (&acc)[C::TN][C::TM])
{
    if constexpr (C::MODE == 2) run_tile_staggered<C, SCRUB, STAGED>(p, smem, pl, ra, rb, wave, wm0, wn0, off1, off2, ks0, nk, rot, ml, acc);
    else run_tile<C, SCRUB, STAGED>(p, smem, pl, ra, rb, wave, wm0, wn0, off1, off2, ks0, nk, rot, ml, acc);
}

using MxArgs = MxScales;   // (fp8mi_common.h)
// The block-scaled instances' kernel argument (MMParams, the kernarg of every tensorwise kernel, stays as it is; mm.scale_a / scale_b are unused)
struct MxParams {
    MMParams mm;
    MxArgs s;
};

// One tile (or one K slice of it) of a ring kernel, from the staging plan to the fused epilogue.  ONE source text, fp8mi_gemm_tile_body.inc,
// expanded at TWO sites: in gemm_tile below, which every scaled, e5m2 and grouped kernel calls, and directly in gemm_kernel, the tensorwise
// e4m3 kernel.  The rule: edit the one text; never give a site lines of its own.  Two sites because the tensorwise instances' machine code
// is kept exactly as measured and a call does not keep it: gemm_kernel calling gemm_tile<C>(p, NoScales{}, ...) changed all 8 of its
// instances (the 256x256 one from 0 to 20 bytes of scratch), while the same text expanded in place changes none of the 95 kernels
// (profiles/gemm_tile_body_isa.txt).  Every difference between the families is an `if constexpr (C::...)` of the text.
// S: MxArgs (C::MXS = 1, 2, 4), BwScales (C::BW) or NoScales
// Map: where this workgroup's tile comes from.  GridTileMap (every kernel of one problem): tile_of_block over the launch grid.  GivenTile (the
// grouped kernels): a tile the kernel resolved itself; tiles_m is then the m-tiles of the tile's own group (the L2 prefetch plan counts a B
// panel's readers with it), and nwg is unused.
struct GridTileMap {
    FP8MI_DEVICE void operator()(int nwg, int tiles_m, int tiles_n, int &tile_m, int &tile_n, int &kslice, int &wg) const
    {
        tile_of_block(blockIdx.x, nwg, tiles_m, tiles_n, tile_m, tile_n, kslice, wg);  // XCD-aware, grouped order (fp8mi_gemm_epi.h)
    }
};
struct GivenTile {
    int tile_m, tile_n;
    FP8MI_DEVICE void operator()(int, int, int, int &tm, int &tn, int &kslice, int &wg) const { tm = tile_m; tn = tile_n; kslice = 0; wg = 0; }
};
struct NoScales { };   // the scale carrier of the instances that stage no scales (C::MXS = 0)

// a buffer descriptor as plain words (an asm operand; wave-uniform): 48-bit base, byte extent clamped to 2^31 - 1, raw dwords
FP8MI_DEVICE u32x4 rsrc_words(const uint8_t *base, int64_t bytes)
{
    const uint64_t b = (uint64_t)base;
    return u32x4{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(b >> 32) & 0xFFFFu)),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)min(bytes, (int64_t)0x7FFFFFFF)), 0x00020000u};
}

template <typename C, typename S, typename Map = GridTileMap>
FP8MI_DEVICE void gemm_tile(const MMParams &p, const S &mx, uint8_t *smem, int tiles_m, int tiles_n, int vec_store, int nwg, const Map &map = Map{})
{
    constexpr int BM = C::kWavesM * (C::TM * 16), BN = C::kWavesN * (C::TN * 16), WM = C::TM * 16, WN = C::TN * 16;
#include "fp8mi_gemm_tile_body.inc"
}

template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>::kThreads)) void gemm_kernel(MMParams p_in, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>;
    unsigned long long e0_ = 0; (void)e0_;
    STAMP(e0_);   // kernel entry, ahead of the argument loads
    const MMParams p = pin_params(p_in);  // every kernel argument in one scalar-load clause (fp8mi_common.h)
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    if constexpr (C::FLOOR == 3) {   // timing-only (tools/floor_probe.hip): the launch alone - arguments fetched and used, nothing else
        if (p.M < 0) *(volatile int *)p.C = tiles_m + tiles_n + vec_store + nwg;   // (never true: keeps the argument loads alive)
        return;
    }
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];

    // the tile body, expanded here and not called (see gemm_tile): the launch grid's tile map and no scales - `mx` of a type that depends on C,
    // so that the body's discarded scale branches are not checked against it
    const GridTileMap map{};
    const std::conditional_t<C::MXS, MxArgs, NoScales> mx{}; (void)mx;
#define FP8MI_TILE_ENTRY_STAMP e0_   // the hook of this site: the FP8MI_STAMP build writes it out behind the wave's coordinates
#include "fp8mi_gemm_tile_body.inc"
#undef FP8MI_TILE_ENTRY_STAMP
}

// The block-scaled (MXFP8) form of the same kernel: Cfg<..., MXS = 1>.  The epilogue's per-tensor factors are 1 (the scales
// were applied inside the MFMAs: load_epi_scalars<true> in gemm_tile); bias and scale_result as in the tensorwise form.
template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 1>::kThreads)) void gemm_mxfp8_kernel(MxParams px, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 1>;
    static_assert(C::FLOOR == 0 && !C::BREG && !C::XLOCAL, "the block-scaled form is built from product configurations only");
    const MMParams p = pin_params(px.mm);
    MxArgs mx = px.s;
    FP8MI_PIN_S(mx.sx); FP8MI_PIN_S(mx.sw); FP8MI_PIN_S(mx.ld_sx); FP8MI_PIN_S(mx.ld_sw);
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];
    gemm_tile<C>(p, mx, smem, tiles_m, tiles_n, vec_store, nwg);
}

// The MXFP4 form: Cfg<..., MXS = 2>.  px.mm counts K, lda and ldb in BYTES (K / 2 of the e2m1 k), so that staging, K tail and
// split-K run on the bytes exactly as in the other forms; nan_zero is ignored (no NaN redo is compiled in).
template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 2>::kThreads)) void gemm_mxfp4_kernel(MxParams px, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 2>;
    static_assert(C::FLOOR == 0 && !C::BREG && !C::XLOCAL, "the block-scaled form is built from product configurations only");
    const MMParams p = pin_params(px.mm);
    MxArgs mx = px.s;
    FP8MI_PIN_S(mx.sx); FP8MI_PIN_S(mx.sw); FP8MI_PIN_S(mx.ld_sx); FP8MI_PIN_S(mx.ld_sw);
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];
    gemm_tile<C>(p, mx, smem, tiles_m, tiles_n, vec_store, nwg);
}

// The MXW4A8 form: Cfg<..., MXS = 4> on the mixed recipe's own stage shape (W4A8Tile below).  px.mm counts K and ldb in W BYTES (K / 2 of the
// k), lda in X bytes; an X row holds 2 x px.mm.K bytes.  Both nan modes: the verdict and the scrubbed redo of the MXFP8 form, on the X side only.
template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 4>::kThreads)) void gemm_mxw4a8_kernel(MxParams px, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 4>;
    const MMParams p = pin_params(px.mm);
    MxArgs mx = px.s;
    FP8MI_PIN_S(mx.sx); FP8MI_PIN_S(mx.sw); FP8MI_PIN_S(mx.ld_sx); FP8MI_PIN_S(mx.ld_sw);
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];
    gemm_tile<C>(p, mx, smem, tiles_m, tiles_n, vec_store, nwg);
}

// The blockwise form: Cfg<..., MXS = 3>.  The epilogue's per-tensor factors are 1 (the scales were folded in per K-step).
struct BwParams {
    MMParams mm;
    BwScales s;
};

template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 3>::kThreads)) void gemm_blockwise_kernel(BwParams px, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 3>;
    static_assert(C::FLOOR == 0 && !C::BREG && !C::XLOCAL, "the blockwise form is built from product configurations only");
    static_assert(128 % BM == 0 && 128 % BN == 0, "a tile lies inside one 128-row scale block");
    const MMParams p = pin_params(px.mm);
    BwScales bs = px.s;
    FP8MI_PIN_S(bs.sa); FP8MI_PIN_S(bs.sb); FP8MI_PIN_S(bs.sa_sr); FP8MI_PIN_S(bs.sa_sk); FP8MI_PIN_S(bs.sb_sr); FP8MI_PIN_S(bs.sb_sk);
    FP8MI_PIN_S(bs.nkb); FP8MI_PIN_S(bs.sh_a); FP8MI_PIN_S(bs.sh_b);
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];
    gemm_tile<C>(p, bs, smem, tiles_m, tiles_n, vec_store, nwg);
}

#ifndef FP8MI_FLOOR_PROBE   // (the timing-only floor build of this file has no e5m2 instances)
// The tensorwise form with an e5m2 operand: Cfg<..., MXS = 0, FMT> (FMT = a_format + 2 * b_format, 1..3).  Same staging, same
// fragment -> operand map (profiles/mfma_numerics_e5m2.txt: the e5m2 K-map is the e4m3 one), same epilogue; only the MFMA's format
// codes differ.  Built on gemm_tile, so the e4m3 x e4m3 kernel above keeps its machine code.  OCP semantics: no NaN redo.
template <int FMT, int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 0, FMT>::kThreads)) void gemm_fmt_kernel(MMParams p_in, int tiles_m, int tiles_n, int vec_store, int nwg)
{
    using C = Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, 0, FMT>;
    static_assert(C::OCP && C::FLOOR == 0 && !C::BREG && !C::XLOCAL, "the e5m2 forms are built from product configurations only");
    const MMParams p = pin_params(p_in);
    FP8MI_PIN_S(tiles_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];
    gemm_tile<C>(p, NoScales{}, smem, tiles_m, tiles_n, vec_store, nwg);
}

// ---- grouped (MoE) forms: one launch over rows sorted by expert, each run of rows against its own expert's B ----
// ONE kernel for the four scale modes, MXS as in Cfg: 0 tensorwise, 1 MXFP8, 2 MXFP4 (K, lda, ldb and stride_b in BYTES, as gemm_mxfp4_kernel
// counts them), 3 blockwise.
// mm describes the whole problem: A (M_total, K), C (M_total, N), scale_a [1] or [M_total]; B, scale_b ([G] or [G, N]) and bias ([G, N]) at
// expert 0.  The grid is slots_m x tiles_n workgroups, slots_m = M_total / BM + G (the host does not know offs); each workgroup counts the real
// m-tiles (fp8mi_group_tiles), takes its place in tile_of_block's order over them, resolves that m-tile slot to (group, m-tile of the group) with
// fp8mi_group_slot, rebases the parameters to the group - its first row, its expert - and runs gemm_tile's body at that tile: an unsplit tile's
// bits do not depend on where it sits, so a group's rows equal the single-problem call on them.
// s, the scale carrier: BwScales for MXS 3 (activation scales 1 x 128 over M_total rows, weight scales of expert 0, stride_sb FLOATS between the
// experts') and, unused, for MXS 0 (the tensorwise instances keep the kernel-argument layout they were measured with); MxScales for MXS 1 / 2
// (s.sx (M_total, K/32) E8M0 bytes at row stride s.ld_sx, s.sw the (N, K/32) scales of expert 0 at row stride s.ld_sw, stride_sb BYTES between
// the experts' scales).  gemm_tile sizes the two MX scale descriptors from the rebased bases and the tile's own rows (rows_a x ld_sx with M = the
// group's rows, rows_b x ld_sw inside one expert): a group's scale DMA cannot reach another group's rows or another expert's scales, and rows
// past the group read 2^0 as rows past the tensor do in the single-problem kernels.  ld_sx, ld_sw and stride_sb are multiples of 4, so every
// rebased scale base stays 4-byte aligned.
template <class S>
struct GroupedParams {
    MMParams mm;
    S s;
    const int32_t *offs;   // int32[G] in device memory: cumulative row ends
    int G;
    int64_t stride_b;      // bytes between the experts' B
    int64_t stride_sb;     // between the experts' weight scales: floats (BwScales) or bytes (MxScales)
};
template <int MXS>
using GroupedParamsOf = GroupedParams<std::conditional_t<MXS == 1 || MXS == 2 || MXS == 4, MxScales, BwScales>>;

// The grouped kernels' configuration: the single-problem one as a type of its own.  Every template of the tile body is then instantiated
// apart from the single-problem kernels' (same source, same constants); sharing the instances changed the register assignment of the
// tensorwise and blockwise kernels, whose machine code is kept exactly as measured (profiles/grouped_gemm_isa.txt, profiles/grouped_mx_isa.txt).
// The same rule as for the tile body's two expansion sites (gemm_tile): one source text, as many instantiations as the measured machine code asks for.
template <int MXS, int... R>
struct GroupedCfg : Cfg<R..., MXS> { };

template <int MXS, int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
__global__ __launch_bounds__((Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD, MXS>::kThreads)) void gemm_grouped_kernel(GroupedParamsOf<MXS> px, int slots_m, int tiles_n, int vec_store, int nwg)
{
    using C = GroupedCfg<MXS, BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>;
    static_assert(MXS >= 0 && MXS <= 4, "tensorwise, MXFP8, MXFP4, blockwise or MXW4A8 (mm.K, ldb and stride_b in W bytes, lda in X bytes)");
    static_assert(C::FLOOR == 0 && !C::BREG && !C::XLOCAL, "the grouped forms are built from product configurations only");
    static_assert(MXS != 3 || (128 % BM == 0 && 128 % BN == 0), "a tile lies inside one 128-row scale block");
    MMParams p = pin_params(px.mm);
    auto sc = px.s;
    if constexpr (MXS == 3) {
        FP8MI_PIN_S(sc.sa); FP8MI_PIN_S(sc.sb); FP8MI_PIN_S(sc.sa_sr); FP8MI_PIN_S(sc.sa_sk); FP8MI_PIN_S(sc.sb_sr); FP8MI_PIN_S(sc.sb_sk);
        FP8MI_PIN_S(sc.nkb); FP8MI_PIN_S(sc.sh_a); FP8MI_PIN_S(sc.sh_b);
    } else if constexpr (MXS != 0) {
        FP8MI_PIN_S(sc.sx); FP8MI_PIN_S(sc.sw); FP8MI_PIN_S(sc.ld_sx); FP8MI_PIN_S(sc.ld_sw);
    }
    const int32_t *offs = px.offs;
    int G = px.G;
    int64_t stride_b = px.stride_b, stride_sb = px.stride_sb;
    FP8MI_PIN_S(offs); FP8MI_PIN_S(G); FP8MI_PIN_S(stride_b); FP8MI_PIN_S(stride_sb);
    FP8MI_PIN_S(slots_m); FP8MI_PIN_S(tiles_n); FP8MI_PIN_S(vec_store); FP8MI_PIN_S(nwg);
    __shared__ __attribute__((aligned(16))) uint8_t smem[C::kRingBytes + kFlagBytes];

    // The work list is the REAL m-tiles x n-tiles in the XCD-aware order of the single-problem kernels (tile_of_block with the real count, not
    // the launched one): every XCD gets an equal run of real tiles, and its blocks behind that run are the surplus.  Mapping the launched slots
    // instead left the surplus at the end of the list, i.e. on the last XCDs alone: 4096 tokens in 8 even groups on the 128x64 tile ran on 6.4
    // of 8 XCDs, 1.27x the time of the per-group loop (profiles/grouped_timing.txt).
    const int real_m = __builtin_amdgcn_readfirstlane((int)fp8mi_group_tiles(offs, G, p.M, BM));   // <= slots_m
    const int real = real_m * tiles_n, xcd = blockIdx.x & 7;
    if ((int)(blockIdx.x >> 3) >= (real >> 3) + (xcd < (real & 7) ? 1 : 0)) return;   // a surplus workgroup (uniform): before any barrier or LDS access
    int slot, tile_n, kslice, wg;
    tile_of_block(blockIdx.x, real, real_m, tiles_n, slot, tile_n, kslice, wg);
    const Fp8miGroupSlot gs = fp8mi_group_slot(offs, G, p.M, BM, slot);
    if (gs.group < 0) return;   // (cannot happen: slot < real_m; kept so that no content of offs reaches the rebasing below unresolved)

    // the group's problem: its rows of A, C and the row scales, its expert's B, scales and bias.  Every value is wave-uniform by
    // construction (kernel arguments, blockIdx, scalar loads); readfirstlane says so to the compiler, the pins keep them in SGPRs
    const int g = __builtin_amdgcn_readfirstlane(gs.group), tile_m = __builtin_amdgcn_readfirstlane(gs.tile);
    const int rows = __builtin_amdgcn_readfirstlane(gs.rows);
    const int64_t start = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(gs.start >> 32)) << 32) |
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)gs.start));
    p.A += start * p.lda;
    p.C = (uint8_t *)p.C + start * p.ldc * (p.out_dtype == FP8MI_F32 ? 4 : 2);
    p.M = rows;
    p.B += g * stride_b;
    if (p.bias) p.bias = (const uint8_t *)p.bias + (int64_t)g * p.N * (p.bias_dtype == FP8MI_F32 ? 4 : 2);
    if constexpr (MXS == 3) {
        sc.sa += start * sc.sa_sr;
        sc.sb += g * stride_sb;
        FP8MI_PIN_S(sc.sa); FP8MI_PIN_S(sc.sb);
    } else if constexpr (MXS == 0) {
        if (p.sa_row) p.scale_a += start;
        p.scale_b += p.sb_row ? (int64_t)g * p.N : (int64_t)g;
        FP8MI_PIN_S(p.scale_a); FP8MI_PIN_S(p.scale_b);
    } else {
        sc.sx += start * sc.ld_sx;
        sc.sw += g * stride_sb;
        FP8MI_PIN_S(sc.sx); FP8MI_PIN_S(sc.sw);
    }
    FP8MI_PIN_S(p.A); FP8MI_PIN_S(p.B); FP8MI_PIN_S(p.C); FP8MI_PIN_S(p.M); FP8MI_PIN_S(p.bias);
    const int tiles_m = (rows + BM - 1) / BM;
    if constexpr (MXS == 0) gemm_tile<C>(p, NoScales{}, smem, tiles_m, tiles_n, vec_store, nwg, GivenTile{tile_m, tile_n});
    else gemm_tile<C>(p, sc, smem, tiles_m, tiles_n, vec_store, nwg, GivenTile{tile_m, tile_n});
}

#endif

// ---- host side: one launch body and one table of product tiles for every family (tensorwise, e5m2 operands, MXFP8, MXFP4, blockwise) ----
inline MMParams &mm_of(MMParams &p) { return p; }
template <class P> MMParams &mm_of(P &px) { return px.mm; }   // MxParams / BwParams

// The launch of one ring-tile kernel (an instance on Cfg C): tile grid, split-K resolution, vector-store flag.  `px` is the kernel's first
// argument - MMParams itself, or MxParams / BwParams around it; the resolved split lands in the MMParams the kernel receives.
template <class C, int BM, int BN, class Params>
int launch_ring(void (*kernel)(Params, int, int, int, int), Params px, hipStream_t s)
{
    MMParams &p = mm_of(px);
    const int64_t tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
    if (tm * tn > 0x7FFFFFFF) return FP8MI_E_UNSUPPORTED;
    // slices on ring-stage (128 x KS) boundaries: whole 128-k blocks of the blockwise scales; an MX scale index is the absolute K-step
    const int rc = resolve_split(p, tm, tn, BM, BN, BK * C::KS);
    if (rc) return rc;
    const int esz = p.out_dtype == FP8MI_F32 ? 4 : 2;
    // 16-byte aligned rows and 4-element groups: enables the vector stores of both epilogues
    const int vec = (((p.ldc * esz) % 16) == 0 && (((uintptr_t)p.C) % 16) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)(tm * tn * p.split);
    return fp8mi_launch(kernel, dim3(grid), dim3(C::kThreads), s, px, (int)tm, (int)tn, vec, (int)grid);
}

// A tile's template parameters as a type: <BM, BN, WM, WN, ring stages, loop order, ABL, K-steps per stage, loading waves>
template <int BM, int BN, int... R>
struct Tile { };

template <int BM, int BN, int WM, int WN, int NSTAGE, int PP = 0, int ABL = 0, int KS = 1, int LD = 0>
int launch(const MMParams &p, hipStream_t s)
{
    return launch_ring<Cfg<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>, BM, BN>(gemm_kernel<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>, p, s);
}

template <int BM, int BN, int... R>
int launch(Tile<BM, BN, R...>, const MMParams &p, hipStream_t s)
{
    return launch<BM, BN, R...>(p, s);
}

#ifndef FP8MI_FLOOR_PROBE
template <int FMT, int BM, int BN, int... R>
int launch_fmt(Tile<BM, BN, R...>, const MMParams &p, hipStream_t s)
{
    return launch_ring<Cfg<BM, BN, R..., 0, FMT>, BM, BN>(gemm_fmt_kernel<FMT, BM, BN, R...>, p, s);
}
#endif

// MXS = 1: gemm_mxfp8_kernel; MXS = 2: gemm_mxfp4_kernel (p in bytes)
template <int MXS, int BM, int BN, int... R>
int launch_mx(Tile<BM, BN, R...>, const MMParams &p, const MxScales &sc, hipStream_t s)
{
    MxParams px;
    px.mm = p;
    px.s = sc;
    if constexpr (MXS == 4) return launch_ring<Cfg<BM, BN, R..., 4>, BM, BN>(gemm_mxw4a8_kernel<BM, BN, R...>, px, s);
    else if constexpr (MXS == 2) return launch_ring<Cfg<BM, BN, R..., 2>, BM, BN>(gemm_mxfp4_kernel<BM, BN, R...>, px, s);
    else return launch_ring<Cfg<BM, BN, R..., 1>, BM, BN>(gemm_mxfp8_kernel<BM, BN, R...>, px, s);
}

template <int BM, int BN, int... R>
int launch_bw(Tile<BM, BN, R...>, const MMParams &p, const BwScales &sc, hipStream_t s)
{
    BwParams px;
    px.mm = p;
    px.s = sc;
    return launch_ring<Cfg<BM, BN, R..., 3>, BM, BN>(gemm_blockwise_kernel<BM, BN, R...>, px, s);
}

#ifndef FP8MI_FLOOR_PROBE
// The slot grid of a ring tile's grouped form: M_total / BM + G m-tile slots (>= the tiles of any split of M_total rows into G groups:
// fp8mi_group_slot.h) x the n-tiles -> the workgroups, INT64_MAX beyond 2^31 - 1.  (slots and n-tiles are each checked against 2^31 before they
// are multiplied: the API layer bounds neither M_total nor N)
template <int BM, int BN, int... R>
int64_t grouped_workgroups(Tile<BM, BN, R...>, const MMParams &p, int G, int64_t &slots, int64_t &tn)
{
    slots = p.M / BM + G;
    tn = (p.N + BN - 1) / BN;
    return (slots > 0x7FFFFFFF || tn > 0x7FFFFFFF || slots * tn > 0x7FFFFFFF) ? INT64_MAX : slots * tn;
}

// The grouped launch of one ring tile on its slot grid: no split-K, no workspace
template <int MXS, int BM, int BN, int... R>
int launch_grouped(Tile<BM, BN, R...> t, GroupedParamsOf<MXS> px, hipStream_t s)
{
    using C = Cfg<BM, BN, R..., MXS>;
    MMParams &p = px.mm;
    int64_t slots, tn;
    const int64_t grid = grouped_workgroups(t, p, px.G, slots, tn);
    if (grid == INT64_MAX) return FP8MI_E_UNSUPPORTED;
    p.split = 1;
    p.ws = nullptr;
    p.ws_bytes = 0;
    const int esz = p.out_dtype == FP8MI_F32 ? 4 : 2;
    const int vec = (((p.ldc * esz) % 16) == 0 && (((uintptr_t)p.C) % 16) == 0) ? 1 : 0;   // every group's first row is then 16-byte aligned too
    return fp8mi_launch(gemm_grouped_kernel<MXS, BM, BN, R...>, dim3((unsigned)grid), dim3(C::kThreads), s, px, (int)slots, (int)tn, vec, (int)grid);
}
#endif

// THE table of product tiles: kernel id -> tile, for all five launchers below (f is a generic lambda that takes the Tile; `otherwise` is
// returned for any other id).  8 waves, waves 0-3 (one per SIMD) issue the stage DMA.  Loop orders (run_tile / run_tile_staggered): the small
// tiles issue their fragment reads ahead of the stage DMA (C3 15.9 -> 15.3 us); the 256x256 tile runs its two wave groups half a K-step apart
// (FLUX 130 -> 124 us, 8192^3 509 -> 479 us); for the 128x128 tile neither order is a consistent gain (shard +1.6 %, 8192^3 -4.5 %): it keeps
// the plain one.
template <class F>
int with_product_tile(int id, int otherwise, F &&f)
{
    switch (id) {
    case FP8MI_KERNEL_GEMM_128: return f(Tile<128, 128, 64, 32, 2, 0, 0, 1, 4>{});     // 2 x 32 KiB ring: 2 workgroups / CU
    case FP8MI_KERNEL_GEMM_128x64: return f(Tile<128, 64, 32, 32, 3, 1, 1, 2, 4>{});   // 3 x 48 KiB ring, 2 K-steps per stage, L2 prefetch one stage beyond the ring (C3 16.0 -> 15.3 us)
    case FP8MI_KERNEL_GEMM_64x128: return f(Tile<64, 128, 32, 32, 3, 1, 0, 2, 4>{});   // 3 x 48 KiB ring, for M <= 64
    // small-batch tiles (round 3, tools/sweep_decode.py, profiles/r03_decode_tiles.txt): against a deep K a 64x128 tile x 8 K slices leaves 32 KiB
    // partials and a last arriver that re-reads 256 KiB; 64x64 x 4 slices (16 KiB partials) and, for M <= 32, 32x64 tiles (half the x traffic)
    // took 13-30 % less time on every shape of the sweep (K=14336 N=4096: M=32 17.2 -> 13.2 us, M=64 17.2 -> 14.9 us)
    case FP8MI_KERNEL_GEMM_64x64: return f(Tile<64, 64, 16, 32, 4, 1, 0, 2, 4>{});     // 8 waves of 16x32, 4 x 32 KiB ring, waves 0-3 load
    case FP8MI_KERNEL_GEMM_32x64: return f(Tile<32, 64, 16, 32, 4, 1, 0, 2, 4>{});     // 4 waves of 16x32, 4 x 24 KiB ring
    case FP8MI_KERNEL_GEMM_32x32: return f(Tile<32, 32, 16, 32, 4, 1, 0, 2, 2>{});     // 2 waves of 16x32, 4 x 16 KiB ring: N / 32 tiles need half the K slices (K = N = 8192, M = 32: 14.7 against 18.0 us)
    // One 128x128 tile per CU at most (end of round 3): the 2 x 32 KiB ring above is built for TWO co-resident workgroups, whose other half hides each one's
    // single stage in flight; alone on its CU a workgroup waits out a memory round trip per K-step (0.8 us per step).  The same tile on 4 x 32 KiB (three
    // stages in flight, fragment reads ahead of the stage DMA): M=1024 K=N=4096 21.8 us against 28.1 (128x64, two rounds) / 29.2 (256x128W on half the CUs) /
    // 31.1 (this tile, shallow ring); M=512 K=N=8192 39.5 against 52.0; M=256 K=4096 N=14336 23.1 against 31.7 (profiles/r03_deep_ring.txt)
    case FP8MI_KERNEL_GEMM_128D: return f(Tile<128, 128, 64, 32, 4, 1, 0, 1, 4>{});
    default: return otherwise;
    }
}

// A product tile's MXW4A8 form: the same workgroup, waves and loading waves on the mixed recipe's own stage - ONE 256-k K-step (X rows at 256
// bytes, W rows at 128), the plain loop order, no L2 prefetch - and the deepest ring up to the tile's own depth that 160 KiB of LDS holds
// (2 KiB allowed for a stage's scale area): 128x128 2, 128x128-deep 3, 128x64 3, 64x128 3, 64x64 / 32x64 / 32x32 4.
constexpr int w4a8_depth(int BM, int BN, int NSTAGE)
{
    const int fit = (160 * 1024 - 16) / ((2 * BM + BN) * BK + 2048);
    return NSTAGE < fit ? NSTAGE : fit;
}
template <int BM, int BN, int WM, int WN, int NSTAGE, int PP, int ABL, int KS, int LD>
constexpr auto w4a8_tile(Tile<BM, BN, WM, WN, NSTAGE, PP, ABL, KS, LD>) { return Tile<BM, BN, WM, WN, w4a8_depth(BM, BN, NSTAGE), 0, 0, 1, LD>{}; }

// The 256x256 tile (2 x 64 KiB ring, staggered wave groups) is tensorwise / e5m2 only: its tensorwise form already fills the 256-register file
// (128 accumulators + 96 fragment registers), and the scale staging pushed either loop order of it into scratch (tools/check_spills.py).
// A block-scaled form needs fragments read in halves first: a follow-up.
using Tile256 = Tile<256, 256, 128, 64, 2, 2, 0, 1, 4>;

#ifndef FP8MI_FLOOR_PROBE
// one operand-format pair (FMT = 1..3) on the tensorwise launcher's tiles
template <int FMT>
int launch_gemm_fmt(const MMParams &p, int variant, hipStream_t s)
{
    switch (variant) {
    case FP8MI_KERNEL_GEMM_256: return launch_fmt<FMT>(Tile256{}, p, s);
    case FP8MI_KERNEL_GEMM_256W: return fp8mi_launch_gemm256_fmt(p, 0, s, FMT);
    case FP8MI_KERNEL_GEMM_256x128W: return fp8mi_launch_gemm256_fmt(p, 1000, s, FMT);
    default: return with_product_tile(variant, FP8MI_E_ENUM, [&](auto t) { return launch_fmt<FMT>(t, p, s); });
    }
}
#endif


}  // namespace

#ifdef FP8MI_STAMP
extern "C" int fp8mi_debug_read_stamps(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(unsigned long long) * n);
}
#endif

bool fp8mi_gemm_supported(const MMParams &p)
{
    return p.M >= 1 && p.N >= 1 && p.K >= 0 && (p.K % 16) == 0 && (p.lda % 16) == 0 && (p.ldb % 16) == 0 &&
           (((uintptr_t)p.A) & 15u) == 0 && (((uintptr_t)p.B) & 15u) == 0 && p.lda < (1 << 22) && p.ldb < (1 << 22);
}

// AUTO of every family: the cheapest tile kernel by the cost model (fp8mi_dispatch.h) for the shape `q` to price, among the kernels `takes`
// admits (in kTileCosts' order; the first of equals wins); the 128x64 tile when the model prices none
template <class Filter>
static int cheapest_tile(const MMParams &q, Filter &&takes)
{
    const double cus = (double)fp8mi_cu_count();
    int best = FP8MI_KERNEL_GEMM_128x64;
    double best_us = 1e300;
    for (const fp8mi_dispatch::TileCost &t : fp8mi_dispatch::kTileCosts) {
        if (!takes(t.id)) continue;
        const double us = fp8mi_dispatch::predict_us(q, t.id, cus);
        if (us >= 0.0 && us < best_us) { best_us = us; best = t.id; }
    }
    return best;
}

// The tile kernel the automatic dispatch uses for a shape the tile kernels support
int fp8mi_choose_gemm_variant(const MMParams &p)
{
    return cheapest_tile(p, [](int) { return true; });
}

int fp8mi_launch_gemm(const MMParams &p, int variant, hipStream_t s, int fmt)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_variant(p);
    // an e5m2 operand (fmt = a_format + 2 * b_format != 0): the same tile, chosen by the same model, with the MFMA's format codes set
#ifndef FP8MI_FLOOR_PROBE
    if (fmt == 1) return launch_gemm_fmt<1>(p, variant, s);
    if (fmt == 2) return launch_gemm_fmt<2>(p, variant, s);
    if (fmt == 3) return launch_gemm_fmt<3>(p, variant, s);
#endif
    if (fmt != 0) return FP8MI_E_UNSUPPORTED;
    switch (variant) {
    case FP8MI_KERNEL_GEMM_256: return launch(Tile256{}, p, s);
    case FP8MI_KERNEL_GEMM_256W: return fp8mi_launch_gemm256(p, 0, s);                   // (only chosen above when fp8mi_gemm256_supported)
    case FP8MI_KERNEL_GEMM_256x128W: return fp8mi_launch_gemm256(p, 1000, s);
#ifdef FP8MI_FLOOR_PROBE  // tools/floor_probe.hip only (never in libfp8mi.so): timing-only floors of the kernels bench.py's headline workloads run on
    case 901: return launch<128, 64, 32, 32, 3, 1, 1 | (1 << 4), 2, 4>(p, s);   // FP8MI_KERNEL_GEMM_128x64 (config C3): DMA stream only
    case 902: return launch<128, 64, 32, 32, 3, 1, 1 | (2 << 4), 2, 4>(p, s);   //   ... launch + C store only
    case 903: return launch<128, 64, 32, 32, 3, 1, 1 | (3 << 4), 2, 4>(p, s);   //   ... launch only
    case 911: return launch<128, 128, 64, 32, 4, 1, 0 | (1 << 4), 1, 4>(p, s);  // FP8MI_KERNEL_GEMM_128D (the `wide` class): the same three
    case 912: return launch<128, 128, 64, 32, 4, 1, 0 | (2 << 4), 1, 4>(p, s);
    case 913: return launch<128, 128, 64, 32, 4, 1, 0 | (3 << 4), 1, 4>(p, s);
#endif
#ifdef FP8MI_DIAG  // schedule variants kept for A/B timing (diagnostic library only; same results): tools/ab_kernels.py
    case 30: return launch<256, 256, 128, 64, 2, 1, 0, 1, 4>(p, s);            // 256x256, fragment reads before the stage DMA
    case 31: return launch<128, 128, 64, 32, 2, 1, 0, 1, 4>(p, s);             // 128x128, same
    case 32: return launch<128, 64, 32, 32, 3, 0, 0, 2, 4>(p, s);              // 128x64, stage DMA first (the round-1 order)
    case 33: return launch<256, 256, 128, 64, 2, 1>(p, s);                     // 256x256 reads first, all 8 waves load
    case 34: return launch<256, 256, 128, 64, 2, 0, 0, 1, 4>(p, s);            // 256x256, lockstep (the round-1 order)
    case 35: return launch<256, 256, 128, 64, 2, 2>(p, s);                     // 256x256, staggered, all waves load
    case 36: return launch<128, 128, 64, 32, 2, 2, 0, 1, 4>(p, s);             // 128x128, staggered, waves 0-3 load
    case 37: return launch<128, 128, 64, 32, 2, 2>(p, s);                      // 128x128, staggered, all waves load
    case 38: return launch<128, 64, 32, 32, 3, 1, 0, 2, 4>(p, s);              // 128x64 without the L2 prefetch
    case 39: return launch<128, 64, 32, 32, 3, 1, 2, 2, 4>(p, s);              //   ... two stages
    case 120: return launch<128, 128, 64, 32, 2, 0, 1, 1, 4>(p, s);            // 128x128 + L2 prefetch one stage further
    case 121: return launch<128, 128, 64, 32, 2, 0, 2, 1, 4>(p, s);            //   ... two stages
    case 122: return launch<128, 128, 64, 32, 2, 0, 4, 1, 4>(p, s);            //   ... four stages
    case 130: return launch<128, 128, 64, 32, 2, 0, 0, 1, 4>(p, s);            // 128x128 ring depths for the paired-split bound (with SPLIT=2, FP8MI_DEBUG=1): 2 x 32 KiB (the shipped 128x128)
    case 131: return launch<128, 128, 64, 32, 4, 1, 0, 1, 4>(p, s);            //   4 x 32 KiB
    case 132: return launch<128, 128, 64, 32, 2, 1, 0, 2, 4>(p, s);            //   2 x 64 KiB (two K-steps per stage)
    case 133: return launch<128, 128, 64, 32, 3, 1, 0, 1, 4>(p, s);            //   3 x 32 KiB
    case 134: return launch<128, 128, 64, 32, 4, 1, 1, 1, 4>(p, s);            //   4 x 32 KiB + L2 prefetch
    case 135: return launch<128, 128, 64, 32, 3, 1, 1, 1, 4>(p, s);            //   3 x 32 KiB + L2 prefetch
    case 136: return launch<128, 128, 64, 32, 4, 0, 0, 1, 4>(p, s);            //   4 x 32 KiB, stage DMA first
    case 140: return launch<128, 64, 32, 32, 3, 1, 9, 2, 4>(p, s);             // 128x64 as shipped + A-panel prefetch by one more wave
    case 141: return launch<128, 64, 32, 32, 3, 1, 10, 2, 4>(p, s);            //   ... both two stages ahead
    case 150: return launch<64, 64, 32, 32, 3, 1, 0, 2, 4>(p, s);              // 64x64 tiles, 4 waves, 3 x 32 KiB ring (decode regime: M <= 64 with a 4-way K split instead of 64x128 x 8)
    case 151: return launch<64, 64, 32, 32, 4, 1, 0, 2, 4>(p, s);              //   4 x 32 KiB
    case 152: return launch<64, 64, 16, 32, 4, 1, 0, 2, 4>(p, s);              //   8 waves
    case 153: return launch<32, 128, 16, 32, 3, 1, 0, 2, 4>(p, s);             // 32x128, 8 waves of 16x32, 3 x 40 KiB (M <= 32)
    case 154: return launch<32, 64, 16, 32, 4, 1, 0, 2, 4>(p, s);              // 32x64, 4 waves, 4 x 24 KiB
    case 155: return launch<16, 128, 16, 32, 4, 1, 0, 2, 2>(p, s);             // 16x128, 4 waves (2 loading), 4 x 36 KiB (M <= 16)
    case 137: return launch<64, 64, 16, 32, 4, 1, 64, 2, 4>(p, s);             // 64x64 as shipped, B operand through plain loads into a register sink: TIMING ONLY (wrong results)
    case 138: return launch<32, 64, 16, 32, 4, 1, 64, 2, 4>(p, s);             //   ... 32x64
    case 144: return launch<64, 64, 16, 32, 4, 1, 128, 2, 4>(p, s);            // 64x64 as shipped, a tile's K slices on one XCD and the exchange at group scope (Cfg::XLOCAL): what relying on the placement would buy
    case 139: return launch<64, 64, 16, 32, 4, 1, 16, 2, 4>(p, s);             // 64x64 as shipped, timing-only floors (Cfg::FLOOR, with the split-K exchange the launch resolves): the DMA stream only
    case 142: return launch<64, 64, 16, 32, 4, 1, 32, 2, 4>(p, s);             //   ... no K loop: launch + split-K exchange + epilogue
    case 143: return launch<64, 64, 16, 32, 4, 1, 48, 2, 4>(p, s);             //   ... the launch alone
    case 156: return launch<64, 64, 16, 32, 3, 1, 0, 2, 4>(p, s);              // 64x64, 8 waves, 3 x 32 KiB
    case 157: return launch<64, 64, 16, 32, 2, 1, 0, 2, 4>(p, s);              // 64x64, 8 waves, 2 x 32 KiB (two workgroups per CU)
    case 126: return launch<64, 16, 16, 16, 4, 1, 0, 2, 2>(p, s);              // 64x16, 4 waves (2 loading), 4 x 20 KiB: N / 16 tiles fill the chip at N = 4096 with NO K split (fp32 out only: timing experiment)
    case 127: return launch<64, 16, 16, 16, 6, 1, 0, 2, 2>(p, s);              //   6 x 20 KiB
    case 128: return launch<32, 16, 16, 16, 6, 1, 0, 2, 2>(p, s);              // 32x16, 2 waves
    case 158: return launch<64, 32, 16, 32, 4, 1, 0, 2, 4>(p, s);              // 64x32, 4 waves, 4 x 24 KiB (more tiles -> fewer K slices, smaller partials)
    case 159: return launch<32, 32, 16, 32, 4, 1, 0, 2, 2>(p, s);              // 32x32, 2 waves, 4 x 16 KiB
    case 7: return launch<128, 64, 64, 32, 6>(p, s);                           // 128x64, 4 waves
    case 8: return launch<128, 128, 64, 64, 4>(p, s);                          // 128x128, 4 waves, 4-stage ring
    case 9: return launch<256, 128, 64, 64, 3, 0, 0, 1, 4>(p, s);              // 256x128, 8 waves (0-3 load), 3 x 48 KiB
    case 10: return launch<128, 64, 32, 32, 6>(p, s);                          // 128x64, 8 waves, one K-step per stage (6 x 24 KiB)
    case 11: return launch<256, 256, 128, 64, 2>(p, s);                        // 256x256, all 8 waves load
    case 12: return launch<128, 64, 32, 32, 3, 0, 0, 2>(p, s);                 // 128x64 KS=2, all 8 waves load
    case 13: return launch<128, 128, 64, 32, 2>(p, s);                         // 128x128, all 8 waves load
#endif
    default: return with_product_tile(variant, FP8MI_E_ENUM, [&](auto t) { return launch(t, p, s); });
    }
}

// ---- block-scaled (MXFP8) forms of the product's ring tiles ---------------------------------------------------------
bool fp8mi_gemm_mxfp8_supported(const MMParams &p, const MxScales &sc)
{
    return fp8mi_gemm_supported(p) && p.K > 0 && (p.K % 32) == 0 && (sc.ld_sx % 4) == 0 && (sc.ld_sw % 4) == 0 &&
           (((uintptr_t)sc.sx) & 3u) == 0 && (((uintptr_t)sc.sw) & 3u) == 0;
}

// AUTO: the cheapest block-scaled ring tile by the tensorwise cost model (fp8mi_dispatch.h)
int fp8mi_choose_gemm_mxfp8_variant(const MMParams &p)
{
    MMParams q = p;
    if (q.M == 1) q.M = 2;   // (the model prices the tile kernels from M = 2: one row costs what two do)
    return cheapest_tile(q, [](int id) { return id != FP8MI_KERNEL_GEMM_256W && id != FP8MI_KERNEL_GEMM_256x128W; });   // (no block-scaled form)
}

int fp8mi_launch_gemm_mxfp8(const MMParams &p, const MxScales &sc, int variant, hipStream_t s)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_mxfp8_variant(p);
    return with_product_tile(variant, FP8MI_E_UNSUPPORTED, [&](auto t) { return launch_mx<1>(t, p, sc, s); });
}

// ---- MXFP4 (e2m1) forms: p counts K, lda and ldb in bytes (K / 2 of the e2m1 k) -----------------------------------------
bool fp8mi_gemm_mxfp4_supported(const MMParams &p, const MxScales &sc)
{
    // p.K % 16 == 0 (whole 16-byte chunks, one 32-k block each) is fp8mi_gemm_supported's own condition
    return fp8mi_gemm_supported(p) && p.K > 0 && (sc.ld_sx % 4) == 0 && (sc.ld_sw % 4) == 0 && (((uintptr_t)sc.sx) & 3u) == 0 &&
           (((uintptr_t)sc.sw) & 3u) == 0;
}

// AUTO is the MXFP8 choice priced at the operands' byte depth K / 2 - the tensorwise cost model, not fitted to fp4 timings
// (tools/check_spills.py: no fp4 instance touches scratch)
int fp8mi_launch_gemm_mxfp4(const MMParams &p, const MxScales &sc, int variant, hipStream_t s)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_mxfp8_variant(p);
    return with_product_tile(variant, FP8MI_E_UNSUPPORTED, [&](auto t) { return launch_mx<2>(t, p, sc, s); });
}

// ---- MXW4A8 (e4m3 A x e2m1 B_nk) forms: p counts K and ldb in W bytes (K / 2 of the k), lda in X bytes (an X row holds 2 x p.K) ----------
bool fp8mi_gemm_mxw4a8_supported(const MMParams &p, const MxScales &sc)
{
    return fp8mi_gemm_mxfp4_supported(p, sc);   // the same conditions on what it is given: whole 16-byte W chunks (32 X bytes), aligned rows and scales
}

// AUTO is the MXFP8 choice priced at the W operand's byte depth K / 2 - the weight stream these shapes are bound by; the tensorwise cost
// model, not fitted to this recipe (X streams four times W's bytes per k, which the model does not see)
int fp8mi_launch_gemm_mxw4a8(const MMParams &p, const MxScales &sc, int variant, hipStream_t s)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_mxfp8_variant(p);
    return with_product_tile(variant, FP8MI_E_UNSUPPORTED, [&](auto t) { return launch_mx<4>(w4a8_tile(t), p, sc, s); });
}

// ---- blockwise (fp32 scale per 128 k of a row or of a 128-row block) forms -------------------------------------------------
// The ring tiles take the tensorwise alignment, 4-byte aligned scale pointers, and scale extents a 32-bit lane offset can address.
static int64_t bw_extent_bytes(int64_t rows, int sh, int64_t sr, int64_t sk, int64_t nkb)
{
    return ((((rows - 1) >> sh)) * sr + (nkb - 1) * sk + 1) * 4;
}

bool fp8mi_gemm_blockwise_supported(const MMParams &p, const BwScales &sc)
{
    if (!fp8mi_gemm_supported(p) || p.K <= 0 || (((uintptr_t)sc.sa) & 3u) != 0 || (((uintptr_t)sc.sb) & 3u) != 0) return false;
    constexpr int64_t kMaxStride = 0x1FFFFFFF;   // (bounds the products below)
    if (sc.sa_sr > kMaxStride || sc.sa_sk > kMaxStride || sc.sb_sr > kMaxStride || sc.sb_sk > kMaxStride) return false;
    return bw_extent_bytes(p.M, sc.sh_a, sc.sa_sr, sc.sa_sk, sc.nkb) < 0x7FFFFFFF && bw_extent_bytes(p.N, sc.sh_b, sc.sb_sr, sc.sb_sk, sc.nkb) < 0x7FFFFFFF;
}

int fp8mi_launch_gemm_blockwise(const MMParams &p, const BwScales &sc, int variant, hipStream_t s)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_mxfp8_variant(p);   // the MXFP8 choice: the tensorwise cost model, no refit
    return with_product_tile(variant, FP8MI_E_UNSUPPORTED, [&](auto t) { return launch_bw(t, p, sc, s); });
}


// ---- grouped (MoE) forms of the product's ring tiles ------------------------------------------------------------------------
#ifndef FP8MI_FLOOR_PROBE
// AUTO of the grouped forms: the cost model above priced at ONE group of the average size, ceil(M_total / G) rows, restricted to the seven
// ring tiles.  Not fitted to grouped timings.
int fp8mi_choose_gemm_grouped_variant(const MMParams &p, int G)
{
    MMParams q = p;
    q.M = (p.M + G - 1) / G;
    if (q.M < 2) q.M = 2;   // (the model prices the tile kernels from M = 2)
    q.split = 1;
    q.ws = nullptr;
    q.ws_bytes = 0;
    return cheapest_tile(q, [](int id) { return with_product_tile(id, 0, [](auto) { return 1; }) != 0; });
}

int64_t fp8mi_gemm_grouped_workgroups(const MMParams &p, int G, int variant)
{
    int64_t n = -1, slots, tn;
    with_product_tile(variant, 0, [&](auto t) { n = grouped_workgroups(t, p, G, slots, tn); return 0; });
    return n;
}

// The host entry of the grouped forms.  p: the whole problem (MXS = 2: K, lda, ldb and stride_b in bytes); sc: the scale carrier of
// GroupedParamsOf<MXS>; AUTO is fp8mi_choose_gemm_grouped_variant.  MXS = 4 runs on the tile's MXW4A8 form (w4a8_tile).
template <int MXS, class S>
static int launch_gemm_grouped(const MMParams &p, const S &sc, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb, int variant, hipStream_t s)
{
    if (variant == FP8MI_KERNEL_AUTO) variant = fp8mi_choose_gemm_grouped_variant(p, G);
    GroupedParamsOf<MXS> px = {};
    px.mm = p;
    px.s = sc;
    px.offs = offs;
    px.G = G;
    px.stride_b = stride_b;
    px.stride_sb = stride_sb;
    return with_product_tile(variant, FP8MI_E_UNSUPPORTED, [&](auto t) {
        if constexpr (MXS == 4) return launch_grouped<4>(w4a8_tile(t), px, s);
        else return launch_grouped<MXS>(t, px, s);
    });
}

int fp8mi_launch_gemm_grouped(const MMParams &p, const BwScales *sc, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb, int variant,
                              hipStream_t s)
{
    return sc ? launch_gemm_grouped<3>(p, *sc, offs, G, stride_b, stride_sb, variant, s)
              : launch_gemm_grouped<0>(p, BwScales{}, offs, G, stride_b, stride_sb, variant, s);
}

// MXW4A8: p.K, ldb and stride_b in W bytes (K / 2), lda in X bytes
int fp8mi_launch_gemm_grouped_mxw4a8(const MMParams &p, const MxScales &sc, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb, int variant,
                                     hipStream_t s)
{
    return launch_gemm_grouped<4>(p, sc, offs, G, stride_b, stride_sb, variant, s);
}

int fp8mi_launch_gemm_grouped_mx(const MMParams &p, const MxScales &sc, bool fp4, const int32_t *offs, int G, int64_t stride_b, int64_t stride_sb,
                                 int variant, hipStream_t s)
{
    return fp4 ? launch_gemm_grouped<2>(p, sc, offs, G, stride_b, stride_sb, variant, s)
               : launch_gemm_grouped<1>(p, sc, offs, G, stride_b, stride_sb, variant, s);
}
#endif
