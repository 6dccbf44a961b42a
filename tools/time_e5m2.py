#!/usr/bin/env python3
"""Times the tensorwise GEMM with e5m2 operands against e4m3 x e4m3 on the same forced kernel, for the four operand-format pairs
(A x B: e4m3 x e4m3, e5m2 x e4m3, e4m3 x e5m2, e5m2 x e5m2), and what AUTO picks (the cost model does not see the format):
C3 (512x4096x4096: GEMM_128x64), FLUX (4096x3072x12288: GEMM_256W and GEMM_128), decode M=64 (K=14336, N=4096: GEMM_64x64 with
split-K, and SKINNY) and M=1 (K=N=4096: the vec-mat's fp32-FMA form; K=14336: its matrix-core form).  Per-dispatch kernel times
(fp8mi_profile_begin / _end, the dispatch packet's timestamps), median of --iters.  Report only: nothing is asserted.
    python tools/time_e5m2.py [--iters 50]"""
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
SHAPES = [("C3", 512, 4096, 4096, L.KERNEL_GEMM_128x64, 1), ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_256W, 1),
          ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_128, 1), ("decode M=64", 64, 4096, 14336, L.KERNEL_GEMM_64x64, 0),
          ("decode M=64", 64, 4096, 14336, L.KERNEL_SKINNY, 1), ("M=1", 1, 4096, 4096, L.KERNEL_GEMV, 1),
          ("M=1 deep K", 1, 4096, 14336, L.KERNEL_GEMV, 1)]
PAIRS = [(L.FMT_E4M3, L.FMT_E4M3), (L.FMT_E5M2, L.FMT_E4M3), (L.FMT_E4M3, L.FMT_E5M2), (L.FMT_E5M2, L.FMT_E5M2)]


def med_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    with L.kernel_timer(iters + 8) as prof:
        for _ in range(iters):
            fn()
    return statistics.median(prof.ms[-iters:]) * 1e3


def finite_bytes(shape, fmt, dev, g):
    """Random finite bytes of either format: e4m3 magnitudes below the NaN pattern, e5m2 exponents below 31."""
    b = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
    if fmt == L.FMT_E5M2:
        return torch.where((b & 0x7C) == 0x7C, b & 0xBF, b)
    return torch.where((b & 0x7F) == 0x7F, b & 0xFE, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.bfloat16
    print(f"{'shape':12s} {'M':>5s} {'N':>5s} {'K':>6s} {'kernel':22s} {'e4m3xe4m3 us':>13s} {'e5m2xe4m3':>10s} {'e4m3xe5m2':>10s} {'e5m2xe5m2':>10s} "
          f"{'ratios to e4m3xe4m3':>22s}   {'AUTO e5m2xe5m2 us':>17s} {'AUTO kernel':s}")
    for name, M, Nn, K, kern, split in SHAPES:
        sa = torch.full((1,), 2.0 ** -8, device=dev)
        sb = torch.full((1,), 2.0 ** -8, device=dev)
        us = []
        for fa, fb in PAIRS:
            A = finite_bytes((M, K), fa, dev, g)
            B = finite_bytes((Nn, K), fb, dev, g)
            us.append(med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o, kernel=kern, split_k=split, nan_mode=L.NAN_PROPAGATE,
                                                     a_format=fa, b_format=fb), a.iters))
        A = finite_bytes((M, K), L.FMT_E5M2, dev, g)
        B = finite_bytes((Nn, K), L.FMT_E5M2, dev, g)
        auto = med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o, a_format=L.FMT_E5M2, b_format=L.FMT_E5M2), a.iters)
        auto_k = L.load().fp8mi_choose_kernel(M, Nn, K, K, K, Nn, L.BF16, 1 if (M > 1 and K >= 1024) else 0, 0)
        ratios = " ".join(f"{u / us[0]:6.3f}" for u in us[1:])
        print(f"{name:12s} {M:5d} {Nn:5d} {K:6d} {NAMES.get(kern, kern):22s} {us[0]:13.2f} {us[1]:10.2f} {us[2]:10.2f} {us[3]:10.2f} {ratios:>22s}   "
              f"{auto:17.2f} {NAMES.get(auto_k, auto_k)}", flush=True)


if __name__ == "__main__":
    main()
