#!/usr/bin/env python3
"""Times the MXFP4 (e2m1 x e2m1) GEMM against the MXFP8 and the tensorwise GEMM on the same forced kernel, and the MXFP4 AUTO
choice, for the four shapes of profiles/mxfp8_timing.txt: C3 (512x4096x4096, GEMM_128x64), FLUX (4096x3072x12288, GEMM_128),
decode M=64 (K=14336, N=4096, GEMM_64x64, split-K) and M=1 (GEMM_32x32).  K counts elements: the fp4 operands are K/2 bytes a row.
Per-dispatch kernel times (fp8mi_profile_begin / _end, the dispatch packet's timestamps), median of --iters.
    python tools/time_mxfp4.py [--iters 50] [--out profiles/mxfp4_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

NAMES = {v: k for k, v in vars(L).items() if k.startswith("KERNEL_") and isinstance(v, int)}


def med_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    with L.kernel_timer(iters + 8) as prof:
        for _ in range(iters):
            fn()
    ms = prof.ms[-iters:]
    return statistics.median(ms) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [("C3", 512, 4096, 4096, L.KERNEL_GEMM_128x64, 1), ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_128, 1),
              ("decode M=64", 64, 4096, 14336, L.KERNEL_GEMM_64x64, 0), ("M=1", 1, 4096, 4096, L.KERNEL_GEMM_32x32, 0)]
    lines = [f"# tools/time_mxfp4.py --iters {a.iters} on MI355X (per-dispatch kernel times, median; bf16 out). ratio = mxfp4 / mxfp8 on the same forced kernel.",
             f"{'shape':12s} {'M':>5s} {'N':>5s} {'K':>6s} {'kernel':20s} {'tensorwise us':>14s} {'mxfp8 us':>9s} {'mxfp4 us':>9s} {'ratio':>6s}   "
             f"{'AUTO mx4 us':>11s} {'AUTO mx4 kernel':s}"]
    print(lines[0])
    print(lines[1], flush=True)
    for name, M, Nn, K, kern, split in shapes:
        A = torch.randint(0, 126, (M, K), dtype=torch.uint8, device=dev, generator=g)
        B = torch.randint(0, 126, (Nn, K), dtype=torch.uint8, device=dev, generator=g)
        A4 = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=g)
        B4 = torch.randint(0, 256, (Nn, K // 2), dtype=torch.uint8, device=dev, generator=g)
        sa = torch.ones(1, device=dev)
        sb = torch.ones(1, device=dev)
        xa = torch.full((M, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        xb = torch.full((Nn, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        o = torch.bfloat16
        tw = med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        mx8 = med_us(lambda: N.fp8_scaled_mm_mxfp8(A, B, xa, xb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        mx4 = med_us(lambda: N.fp8_scaled_mm_mxfp4(A4, B4, xa, xb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        mx4_auto = med_us(lambda: N.fp8_scaled_mm_mxfp4(A4, B4, xa, xb, out_dtype=o), a.iters)
        auto_k = L.load().fp8mi_choose_kernel_mxfp4(M, Nn, K, K // 2, K // 2, Nn, L.BF16, 1, 0)
        line = (f"{name:12s} {M:5d} {Nn:5d} {K:6d} {NAMES.get(kern, kern):20s} {tw:14.2f} {mx8:9.2f} {mx4:9.2f} {mx4 / mx8:6.3f}   "
                f"{mx4_auto:11.2f} {NAMES.get(auto_k, auto_k)}")
        lines.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
