#!/usr/bin/env python3
"""tools/time_grouped.py for the grouped MXFP8 / MXFP4 GEMM (fp8mi_scaled_mm_grouped_mxfp8 / _mxfp4): the one launch against a loop of
per-group fp8mi_scaled_mm_mxfp8 / _mxfp4 calls on the SAME ring tile, unsplit, group sizes already on the host - and, from the same run
and on the same tile, the tensorwise grouped launch against its own loop (the rows of profiles/grouped_timing.txt), so that the MX ratios
stand next to the yardstick they are read against.

Same shapes (G = 8, K = 7168, N = 4096, bf16 out; 64 .. 4096 tokens, even and skewed), same two clocks, same rotation of the experts' weights
beyond the last-level cache, same alternation and median as that tool; its docstring has the details.  The tile is what
fp8mi_choose_kernel_grouped_mx picks for the MX format (MXFP4 is priced at its byte depth K / 2, so its tile can differ from MXFP8's), or
--kernel; the tensorwise rows run on fp8mi_choose_kernel_grouped's.  Before a shape is timed the two candidates' outputs are compared bit
for bit.
    python tools/time_grouped_mx.py [--iters 30] [--kernel ID]"""
import argparse

import torch

from time_grouped import CACHE_BYTES, G, K, NN, TILE_NAMES, TOKENS, L, bracket, med, splits

NB = K // 32   # scale bytes per row (a multiple of 4)


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
    nbuf4 = max(2, -(-2 * CACHE_BYTES // (G * NN * K // 2)))
    Bs = [torch.randint(0, 0x7F, (G, NN, K), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nbuf)]
    Bs4 = [torch.randint(0, 256, (G, NN, K // 2), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nbuf4)]
    sb_row = torch.rand((G, NN), device=dev, generator=gen) + 0.5
    sb_mx = torch.randint(120, 135, (G, NN, NB), device=dev, generator=gen, dtype=torch.uint8)
    empty = []
    for _ in range(50):
        empty.append(bracket(lambda: None))
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    print(f"{torch.cuda.get_device_name(0)}; G = {G} experts, K = {K}, N = {NN}, bf16 out; times in us, median of {a.iters} alternating calls; "
          f"{nbuf} rotating weight sets ({nbuf4} for MXFP4); empty bracket {ovh:.2f} us (subtracted from the stream columns)")
    print(f"{'tokens':>6s} {'split':>7s} {'recipe':>9s} {'tile':>8s} | {'grouped kernels':>15s} {'loop kernels':>13s} {'ratio':>6s} | {'grouped stream':>14s} "
          f"{'loop stream':>12s} {'ratio':>6s} | {'loop launches':>13s}")
    for m in TOKENS:
        A = torch.randint(0, 0x7F, (m, K), device=dev, generator=gen, dtype=torch.uint8)
        A4 = torch.randint(0, 256, (m, K // 2), device=dev, generator=gen, dtype=torch.uint8)
        sa_row = torch.rand((m,), device=dev, generator=gen) + 0.5
        sa_mx = torch.randint(120, 135, (m, NB), device=dev, generator=gen, dtype=torch.uint8)
        Cg = torch.empty((m, NN), device=dev, dtype=torch.bfloat16)
        Cl = torch.empty((m, NN), device=dev, dtype=torch.bfloat16)
        for split_name, sizes in splits(m):
            ends, run = [], 0
            for s in sizes:
                run += s
                ends.append(run)
            offs = torch.tensor(ends, dtype=torch.int32, device=dev)
            for recipe in ("rowwise", "mxfp8", "mxfp4"):
                fp4 = recipe == "mxfp4"
                kb = K // 2 if fp4 else K
                if a.kernel != L.KERNEL_AUTO:
                    tile = a.kernel
                elif recipe == "rowwise":
                    tile = lib.fp8mi_choose_kernel_grouped(G, m, NN, K, K, K, NN, L.BF16)
                else:
                    tile = lib.fp8mi_choose_kernel_grouped_mx(L.MX_FP4 if fp4 else L.MX_FP8, G, m, NN, K, kb, kb, NN, L.BF16)
                assert tile in TILE_NAMES, tile
                Aq, Bq = (A4, Bs4) if fp4 else (A, Bs)

                def grouped(i, C=Cg):
                    B = Bq[i % len(Bq)]
                    if recipe == "rowwise":
                        rc = lib.fp8mi_scaled_mm_grouped(Aq.data_ptr(), B.data_ptr(), C.data_ptr(), sa_row.data_ptr(), sb_row.data_ptr(), None, None,
                                                         offs.data_ptr(), G, m, NN, K, K, K, NN * K, NN, L.SCALE_ROW, L.SCALE_ROW, L.BF16, L.F32, L.NAN_ZERO,
                                                         tile, stream)
                    elif fp4:
                        rc = lib.fp8mi_scaled_mm_grouped_mxfp4(Aq.data_ptr(), B.data_ptr(), C.data_ptr(), sa_mx.data_ptr(), NB, sb_mx.data_ptr(), NB, NN * NB,
                                                               None, None, offs.data_ptr(), G, m, NN, K, kb, kb, NN * kb, NN, L.BF16, L.F32, tile, stream)
                    else:
                        rc = lib.fp8mi_scaled_mm_grouped_mxfp8(Aq.data_ptr(), B.data_ptr(), C.data_ptr(), sa_mx.data_ptr(), NB, sb_mx.data_ptr(), NB, NN * NB,
                                                               None, None, offs.data_ptr(), G, m, NN, K, kb, kb, NN * kb, NN, L.BF16, L.F32, L.NAN_ZERO, tile,
                                                               stream)
                    L.check(rc, "grouped")

                def loop(i, C=Cl):
                    B = Bq[i % len(Bq)]
                    start = 0
                    for g, rows in enumerate(sizes):
                        if rows:
                            pa, pb, pc = Aq.data_ptr() + start * kb, B.data_ptr() + g * NN * kb, C.data_ptr() + start * NN * 2
                            if recipe == "rowwise":
                                rc = lib.fp8mi_scaled_mm_ex(pa, pb, pc, sa_row.data_ptr() + start * 4, sb_row.data_ptr() + g * NN * 4, None, None, rows, NN, K,
                                                            K, K, NN, L.SCALE_ROW, L.SCALE_ROW, L.BF16, L.F32, L.NAN_ZERO, tile, stream)
                            elif fp4:
                                rc = lib.fp8mi_scaled_mm_mxfp4(pa, pb, pc, sa_mx.data_ptr() + start * NB, NB, sb_mx.data_ptr() + g * NN * NB, NB, None, None,
                                                               rows, NN, K, kb, kb, NN, L.BF16, L.F32, tile, 1, None, 0, stream)
                            else:
                                rc = lib.fp8mi_scaled_mm_mxfp8(pa, pb, pc, sa_mx.data_ptr() + start * NB, NB, sb_mx.data_ptr() + g * NN * NB, NB, None, None,
                                                               rows, NN, K, kb, kb, NN, L.BF16, L.F32, L.NAN_ZERO, tile, 1, None, 0, stream)
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
