#!/usr/bin/env python3
"""Times the blockwise GEMM (1x128 activation x 128x128 weight fp32 scales) against the tensorwise and MXFP8 GEMMs on the same forced
kernel, and its AUTO choice: C3 (512x4096x4096, GEMM_128x64), FLUX (4096x3072x12288, GEMM_128: the 256x256 tile has no blockwise
form), decode M=64 (K=14336, N=4096, GEMM_64x64, split-K) and M=1 (K=N=4096, GEMM_32x32).  Per-dispatch kernel times
(fp8mi_profile_begin / _end, the dispatch packet's timestamps), median of --iters.

Then the linear y = x W^T on the same shapes, two routes per call, both timed with the same CUDA events (median of --iters calls):
  fp8:      fp8_linear_blockwise (1x128 quantisation of x, then the AUTO blockwise GEMM)
  dequant:  what a torch-ROCm user runs on a blockwise checkpoint today - the weight dequantized to bf16 (here with the library's own
            dequant kernel, the fastest such pass available), then torch.matmul in bf16
    python tools/time_blockwise.py [--iters 50]"""
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
SHAPES = [("C3", 512, 4096, 4096, L.KERNEL_GEMM_128x64, 1), ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_128, 1),
          ("decode M=64", 64, 4096, 14336, L.KERNEL_GEMM_64x64, 0), ("M=1", 1, 4096, 4096, L.KERNEL_GEMM_32x32, 0)]


def med_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    with L.kernel_timer(iters + 8) as prof:
        for _ in range(iters):
            fn()
    ms = prof.ms[-iters:]
    return statistics.median(ms) * 1e3


def event_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.bfloat16
    print(f"{'shape':12s} {'M':>5s} {'N':>5s} {'K':>6s} {'kernel':20s} {'tensorwise us':>14s} {'mxfp8 us':>9s} {'blockwise us':>13s} "
          f"{'bw/tw':>6s} {'bw/mx':>6s}   {'AUTO bw us':>10s} {'AUTO bw kernel':s}")
    for name, M, Nn, K, kern, split in SHAPES:
        A = torch.randint(0, 126, (M, K), dtype=torch.uint8, device=dev, generator=g)
        B = torch.randint(0, 126, (Nn, K), dtype=torch.uint8, device=dev, generator=g)
        sa = torch.ones(1, device=dev)
        sb = torch.ones(1, device=dev)
        xa = torch.full((M, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        xb = torch.full((Nn, (K // 32 + 3) // 4 * 4), 127, dtype=torch.uint8, device=dev)
        ba = torch.rand((M, K // 128), device=dev, generator=g) + 0.5
        bb = torch.rand(((Nn + 127) // 128, K // 128), device=dev, generator=g) + 0.5
        tw = med_us(lambda: N.fp8_scaled_mm(A, B, sa, sb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        mx = med_us(lambda: N.fp8_scaled_mm_mxfp8(A, B, xa, xb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        bw = med_us(lambda: N.fp8_scaled_mm_blockwise(A, B, ba, bb, out_dtype=o, kernel=kern, split_k=split), a.iters)
        bw_auto = med_us(lambda: N.fp8_scaled_mm_blockwise(A, B, ba, bb, out_dtype=o), a.iters)
        auto_k = L.load().fp8mi_choose_kernel_blockwise(M, Nn, K, K, K, Nn, L.BF16, 1, 128, 1, 0)
        print(f"{name:12s} {M:5d} {Nn:5d} {K:6d} {NAMES.get(kern, kern):20s} {tw:14.2f} {mx:9.2f} {bw:13.2f} {bw / tw:6.3f} {bw / mx:6.3f}   "
              f"{bw_auto:10.2f} {NAMES.get(auto_k, auto_k)}", flush=True)
    print()
    print(f"{'linear':12s} {'M':>5s} {'N':>5s} {'K':>6s} {'fp8_linear_blockwise us':>24s} {'dequant bf16 + matmul us':>25s} {'speed-up':>9s}")
    for name, M, Nn, K, _, _ in SHAPES:
        x = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn((Nn, K), device=dev, generator=g) * 0.02).to(torch.bfloat16)
        wq, ws = N.fp8_quantize_blockwise(w, 128)
        fp8 = event_us(lambda: N.fp8_linear_blockwise(x, wq, ws), a.iters)
        deq = event_us(lambda: torch.matmul(x, N.fp8_dequantize_blockwise(wq, ws, 128, torch.bfloat16).t()), a.iters)
        print(f"{name:12s} {M:5d} {Nn:5d} {K:6d} {fp8:24.2f} {deq:25.2f} {deq / fp8:8.2f}x", flush=True)


if __name__ == "__main__":
    main()
