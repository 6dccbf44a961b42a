#!/usr/bin/env python3
"""Times the grouped (MoE) GEMM launch (fp8mi_scaled_mm_grouped / _grouped_blockwise) against what a caller could do without it: a loop of
per-group fp8mi_scaled_mm_ex / fp8mi_scaled_mm_blockwise calls on the SAME ring tile, unsplit, with the group sizes already on the host
(the loop is spared the device-to-host copy of offs and the sync it needs in real use; empty groups cost it nothing).

Shapes: the expert set of one DeepSeek-V3 rank - G = 8 experts, K = 7168, N = 4096, bf16 out - at 64 .. 4096 total tokens, split evenly
and skewed (half of the tokens to expert 0, a quarter to expert 1, ...; the last expert empty).  Two recipes: per-token x per-channel scales
(the tensorwise form with both scale modes ROW) and blockwise 1x128 x 128x128.  The tile is what FP8MI_KERNEL_AUTO of the grouped entry point
picks (fp8mi_choose_kernel_grouped), or --kernel.

Both candidates are called through ctypes on raw pointers (no op-layer work in either), ALTERNATING call by call in one process after warm-up;
median of --iters (>= 20).  Two clocks, printed side by side:
  kernels   the sum of the launches' own durations (fp8mi_profile_begin / _end: the dispatch packets' timestamps) - the loop's launches run
            back to back on one stream, so this leaves out the gaps between them;
  stream    two events around the candidate's calls: what the stream is busy for, launch gaps included, less the interval the same bracket
            measures around nothing (printed as `empty bracket`).
The experts' weights rotate over enough copies to exceed the 256 MiB last-level cache, so a call does not find them where the previous
call left them.  Before a shape is timed the two candidates' outputs are compared bit for bit on the rows the groups own.
    python tools/time_grouped.py [--iters 30] [--kernel ID]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

G, K, NN = 8, 7168, 4096
TOKENS = (64, 256, 1024, 4096)
CACHE_BYTES = 256 << 20
NKB = (K + 127) // 128
TILE_NAMES = {L.KERNEL_GEMM_128: "128x128", L.KERNEL_GEMM_128x64: "128x64", L.KERNEL_GEMM_64x128: "64x128", L.KERNEL_GEMM_64x64: "64x64",
              L.KERNEL_GEMM_32x64: "32x64", L.KERNEL_GEMM_32x32: "32x32", L.KERNEL_GEMM_128D: "128x128D"}


def splits(m):
    even = [m // G] * G
    skew, left = [], m
    for g in range(G - 1):
        take = left if g == G - 2 else max(left // 2, 1 if left else 0)
        skew.append(take)
        left -= take
    skew.append(0)
    assert sum(even) == m and sum(skew) == m
    return (("even", even), ("skewed", skew))


def med(v):
    return statistics.median(v)


def bracket(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kernel", type=int, default=L.KERNEL_AUTO)
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    lib = L.load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    nbuf = max(2, -(-2 * CACHE_BYTES // (G * NN * K)))
    Bs = [torch.randint(0, 0x7F, (G, NN, K), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nbuf)]
    sb_row = torch.rand((G, NN), device=dev, generator=gen) + 0.5
    sb_blk = torch.rand((G, (NN + 127) // 128, NKB), device=dev, generator=gen) + 0.5
    empty = []
    for _ in range(50):
        empty.append(bracket(lambda: None))
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    print(f"{torch.cuda.get_device_name(0)}; G = {G} experts, K = {K}, N = {NN}, bf16 out; times in us, median of {a.iters} alternating calls; "
          f"{nbuf} rotating weight sets; empty bracket {ovh:.2f} us (subtracted from the stream columns)")
    print(f"{'tokens':>6s} {'split':>7s} {'recipe':>9s} {'tile':>8s} | {'grouped kernels':>15s} {'loop kernels':>13s} {'ratio':>6s} | {'grouped stream':>14s} "
          f"{'loop stream':>12s} {'ratio':>6s} | {'loop launches':>13s}")
    for m in TOKENS:
        A = torch.randint(0, 0x7F, (m, K), device=dev, generator=gen, dtype=torch.uint8)
        sa_row = torch.rand((m,), device=dev, generator=gen) + 0.5
        sa_blk = torch.rand((m, NKB), device=dev, generator=gen) + 0.5
        Cg = torch.empty((m, NN), device=dev, dtype=torch.bfloat16)
        Cl = torch.empty((m, NN), device=dev, dtype=torch.bfloat16)
        for split_name, sizes in splits(m):
            ends, run = [], 0
            for s in sizes:
                run += s
                ends.append(run)
            offs = torch.tensor(ends, dtype=torch.int32, device=dev)
            tile = a.kernel if a.kernel != L.KERNEL_AUTO else lib.fp8mi_choose_kernel_grouped(G, m, NN, K, K, K, NN, L.BF16)
            assert tile in TILE_NAMES, tile
            for recipe in ("rowwise", "blockwise"):
                def grouped(i, C=Cg):
                    B = Bs[i % nbuf]
                    if recipe == "rowwise":
                        rc = lib.fp8mi_scaled_mm_grouped(A.data_ptr(), B.data_ptr(), C.data_ptr(), sa_row.data_ptr(), sb_row.data_ptr(), None, None,
                                                         offs.data_ptr(), G, m, NN, K, K, K, NN * K, NN, L.SCALE_ROW, L.SCALE_ROW, L.BF16, L.F32, L.NAN_ZERO,
                                                         tile, stream)
                    else:
                        rc = lib.fp8mi_scaled_mm_grouped_blockwise(A.data_ptr(), B.data_ptr(), C.data_ptr(), sa_blk.data_ptr(), NKB, 1, 1, sb_blk.data_ptr(),
                                                                   NKB, 1, sb_blk.stride(0), 128, None, None, offs.data_ptr(), G, m, NN, K, K, K, NN * K, NN,
                                                                   L.BF16, L.F32, L.NAN_ZERO, tile, stream)
                    L.check(rc, "grouped")

                def loop(i, C=Cl):
                    B = Bs[i % nbuf]
                    start = 0
                    for g, rows in enumerate(sizes):
                        if rows:
                            pa, pb, pc = A.data_ptr() + start * K, B.data_ptr() + g * NN * K, C.data_ptr() + start * NN * 2
                            if recipe == "rowwise":
                                rc = lib.fp8mi_scaled_mm_ex(pa, pb, pc, sa_row.data_ptr() + start * 4, sb_row.data_ptr() + g * NN * 4, None, None, rows, NN, K,
                                                            K, K, NN, L.SCALE_ROW, L.SCALE_ROW, L.BF16, L.F32, L.NAN_ZERO, tile, stream)
                            else:
                                rc = lib.fp8mi_scaled_mm_blockwise(pa, pb, pc, sa_blk.data_ptr() + start * NKB * 4, NKB, 1, 1,
                                                                   sb_blk.data_ptr() + g * sb_blk.stride(0) * 4, NKB, 1, 128, None, None, rows, NN, K, K, K, NN,
                                                                   L.BF16, L.F32, L.NAN_ZERO, tile, 1, None, 0, stream)
                            L.check(rc, "loop")
                        start += rows

                for i in range(3):
                    grouped(i)
                    loop(i)
                Cg.fill_(-1.0)
                Cl.fill_(-1.0)
                grouped(0)
                loop(0)
                torch.cuda.synchronize()
                assert torch.equal(Cg, Cl), "the grouped launch and the loop differ"
                kg, kl, sg, sl, launches = [], [], [], [], 0
                for i in range(a.iters):
                    with L.kernel_timer(4) as p:
                        grouped(i)
                    assert len(p.ms) == 1, "one launch"
                    kg.append(p.ms[0] * 1e3)
                    with L.kernel_timer(2 * G) as p:
                        loop(i)
                    launches = len(p.ms)
                    kl.append(sum(p.ms) * 1e3)
                torch.cuda.synchronize()
                for i in range(a.iters):
                    eg = bracket(lambda: grouped(i))
                    el = bracket(lambda: loop(i))
                    torch.cuda.synchronize()
                    sg.append(max(0.0, eg[0].elapsed_time(eg[1]) * 1e3 - ovh))
                    sl.append(max(0.0, el[0].elapsed_time(el[1]) * 1e3 - ovh))
                print(f"{m:6d} {split_name:>7s} {recipe:>9s} {TILE_NAMES[tile]:>8s} | {med(kg):15.2f} {med(kl):13.2f} {med(kg) / med(kl):6.3f} | {med(sg):14.2f} "
                      f"{med(sl):12.2f} {med(sg) / med(sl):6.3f} | {launches:13d}", flush=True)


if __name__ == "__main__":
    main()
