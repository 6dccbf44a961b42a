#!/usr/bin/env python3
"""Times the MXFP8 (block-scaled) GEMM against the tensorwise GEMM on the same forced kernel, and both AUTO choices:
C3 (512x4096x4096, GEMM_128x64), FLUX (4096x3072x12288, GEMM_128: the 256x256 tile has no block-scaled form yet), decode M=64 (K=14336, N=4096, split-K) and M=1.
Per-dispatch kernel times (fp8mi_profile_begin / _end, the dispatch packet's timestamps), median of --iters.
    python tools/time_mxfp8.py [--iters 50]"""
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
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [("C3", 512, 4096, 4096, L.KERNEL_GEMM_128x64, 1), ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_128, 1),
              ("decode M=64", 64, 4096, 14336, L.KERNEL_GEMM_64x64, 0), ("M=1", 1, 4096, 4096, L.KERNEL_GEMM_32x32, 0)]
    print(f"{'shape':12s} {'M':>5s} {'N':>5s} {'K':>6s} {'kernel':20s} {'tensorwise us':>14s} {'mxfp8 us':>9s} {'ratio':>6s}   "
          f"{'AUTO tw us':>10s} {'AUTO mx us':>10s} {'AUTO mx kernel':s}")
    for name, M, Nn, K, kern, split in shapes:
        A = torch.randint(0, 126, (M, K), dtype=torch.uint8, device=dev, generator=g)
        B = torch.randint(0, 126, (Nn, K), dtype=torch.uint8, device=dev, generator=g)
        sa = torch.ones(1, device=dev)
        sb = torch.ones(1, device=dev)
        xa = torch.full((M, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        xb = torch.full((Nn, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        o = torch.bfloat16
        tw = med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        mx = med_us(lambda: N.fp8_scaled_mm_mxfp8(A, B, xa, xb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        tw_auto = med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o), a.iters)
        mx_auto = med_us(lambda: N.fp8_scaled_mm_mxfp8(A, B, xa, xb, out_dtype=o), a.iters)
        auto_k = L.load().fp8mi_choose_kernel_mxfp8(M, Nn, K, K, K, Nn, L.BF16, 1, 0)
        print(f"{name:12s} {M:5d} {Nn:5d} {K:6d} {NAMES.get(kern, kern):20s} {tw:14.2f} {mx:9.2f} {mx / tw:6.3f}   {tw_auto:10.2f} {mx_auto:10.2f} "
              f"{NAMES.get(auto_k, auto_k)}", flush=True)


if __name__ == "__main__":
    main()
