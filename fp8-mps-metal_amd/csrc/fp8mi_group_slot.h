// Grouped (MoE) GEMM: which rows an m-tile slot of the launch grid computes.  One function for the kernels (fp8mi_gemm.hip) and for the
// host program that checks it against a brute-force enumeration without a GPU (tests/c/group_slot.cpp).
//
// `offs` is int32[G], cumulative row ENDS (torch._scaled_grouped_mm's convention).  Group g owns rows [start_g, end_g):
//     start_0 = 0,  start_g = end_{g-1},  end_g = clamp(offs[g], start_g, M_total)
// For every non-decreasing offs inside [0, M_total] that is start_g = offs[g-1], end_g = offs[g].  The clamps are part of the
// definition: whatever offs holds (decreasing, negative, beyond M_total) the groups are disjoint, in order, inside [0, M_total), and
//     sum_g ceil(M_g / BM)  <=  floor(sum_g M_g / BM) + G  <=  M_total / BM + G  =  T,
// the m-tile slots the host launches without knowing offs.  (Basing start_g on offs[g-1] alone would let a group that follows a
// decrease overlap an earlier one: offs = [M, 0, M, 0, ...] then needs G / 2 x ceil(M / BM) tiles, more than T.)
// Slots are handed out in group order, a group's tiles in row order: the slot -> group map is monotone.  The first
// fp8mi_group_tiles() slots are the real tiles; every slot behind them resolves to "none".
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FP8MI_SLOT_FN __host__ __device__ inline
#else
#define FP8MI_SLOT_FN inline
#endif
#if defined(__clang__)
#define FP8MI_SLOT_UNROLL _Pragma("unroll")
#else
#define FP8MI_SLOT_UNROLL
#endif

// offs[i] at a wave-uniform address: on the device one scalar load through the constant address space (load_uniform_f32,
// fp8mi_common.h: the scalar cache is invalidated at kernel start, so the previous kernel's offs are seen)
#if defined(__HIP_DEVICE_COMPILE__)
#define FP8MI_SLOT_LOAD(p, i) (*(const __attribute__((address_space(4))) int32_t *)((p) + (i)))
#else
#define FP8MI_SLOT_LOAD(p, i) ((p)[i])
#endif

struct Fp8miGroupSlot {
    int group;       // -1: the slot lies beyond the real tiles (nothing to do)
    int tile;        // the slot's m-tile inside its group
    int64_t start;   // the group's first row
    int rows;        // the group's rows, M_g >= 1
};

// The walk is serial in g: one scalar load per group ahead of the slot's own, eight in flight at a time (the loads of a batch do not
// depend on one another).  Its cost at kernel entry has NOT been measured; a lane-parallel scan is the follow-up if large G shows it.
FP8MI_SLOT_FN Fp8miGroupSlot fp8mi_group_slot(const int32_t *offs, int G, int64_t M_total, int BM, int64_t slot)
{
    Fp8miGroupSlot r = {-1, 0, 0, 0};
    int64_t start = 0, first = 0;   // first row / first slot of group g
    for (int g0 = 0; g0 < G; g0 += 8) {
        int32_t e8[8];
FP8MI_SLOT_UNROLL
        for (int j = 0; j < 8; ++j) e8[j] = FP8MI_SLOT_LOAD(offs, g0 + j < G ? g0 + j : G - 1);
FP8MI_SLOT_UNROLL
        for (int j = 0; j < 8; ++j) {
            if (g0 + j >= G) break;
            int64_t end = e8[j];
            end = end < start ? start : (end > M_total ? M_total : end);
            const int64_t tiles = (uint32_t)(end - start + BM - 1) / (uint32_t)BM;   // (M_g < 2^31: offs is int32; BM a constant where inlined)
            if (slot < first + tiles) {
                r.group = g0 + j;
                r.tile = (int)(slot - first);
                r.start = start;
                r.rows = (int)(end - start);
                return r;
            }
            first += tiles;
            start = end;
        }
    }
    return r;
}

// The real m-tiles of all groups, sum_g ceil(M_g / BM) <= M_total / BM + G: a walk over all of offs (G / 8 batches of scalar loads).
// The kernels map their workgroups onto this many m-tiles (not onto the slots the host launched), so that the surplus workgroups are
// the LAST of every XCD instead of whole XCDs at the end of the list.
FP8MI_SLOT_FN int64_t fp8mi_group_tiles(const int32_t *offs, int G, int64_t M_total, int BM)
{
    int64_t start = 0, tiles = 0;
    for (int g0 = 0; g0 < G; g0 += 8) {
        int32_t e8[8];
FP8MI_SLOT_UNROLL
        for (int j = 0; j < 8; ++j) e8[j] = FP8MI_SLOT_LOAD(offs, g0 + j < G ? g0 + j : G - 1);
FP8MI_SLOT_UNROLL
        for (int j = 0; j < 8; ++j) {
            if (g0 + j >= G) break;
            int64_t end = e8[j];
            end = end < start ? start : (end > M_total ? M_total : end);
            tiles += (uint32_t)(end - start + BM - 1) / (uint32_t)BM;
            start = end;
        }
    }
    return tiles;
}
