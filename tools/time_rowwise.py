#!/usr/bin/env python3
"""Times the per-row quantiser (fp8mi_quantize_rowwise, one launch) against the unchanged per-tensor quantiser (fp8mi_quantize: an amax
launch and an encode launch) on the same tensor, and fp8_linear_rowwise against fp8_linear.  Per-dispatch kernel times
(fp8mi_profile_begin / _end: the dispatch packet's timestamps), after warm-up, the candidates ALTERNATING call by call in one process,
median of --iters (>= 20).  The per-tensor figure is the SUM of its two kernels (the gap between them and its memset node are not in it).
Achieved bytes/s are over (esz + 1) rows cols for both - the bytes the recipe has to move once; fp8mi_quantize itself moves 2 esz + 1.

The tensors rotate over --buffers copies (default: enough to exceed the 256 MiB of last-level cache, at most 64), so a call does not find its
input where the previous call left it.
    python tools/time_rowwise.py [--iters 30] [--buffers N]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

TENSORS = [(torch.bfloat16, 4096, 3072), (torch.bfloat16, 4096, 12288), (torch.bfloat16, 64, 14336), (torch.bfloat16, 1, 14336),
           (torch.float32, 8192, 8192), (torch.bfloat16, 4096, 20000)]
LINEARS = [("FLUX", 4096, 3072, 12288), ("decode M=64", 64, 14336, 4096)]
NAME = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float16: "f16"}
CACHE_BYTES = 256 << 20


def kernel_us(fn):
    """-> the kernel times (us) of the launches one call of fn makes"""
    with L.kernel_timer(16) as prof:
        fn()
    return [t * 1e3 for t in prof.ms]


def alternate(fns, iters, warmup=5):
    """fns: callables taking the iteration number; -> per candidate, the list over iterations of its per-launch kernel times"""
    for i in range(warmup):
        for fn in fns:
            fn(i)
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            out[k].append(kernel_us(lambda: fn(i)))
    return out


def med(rows, sel=sum):
    return statistics.median(sel(r) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=0)
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}; kernel times in us, median of {a.iters} alternating calls")
    print(f"{'tensor':22s} {'rowwise us':>11s} {'TB/s':>6s} | {'per-tensor us':>14s} {'(amax':>8s} {'+ encode)':>10s} {'TB/s':>6s} | {'rowwise / per-tensor':>21s}")
    for dt, rows, cols in TENSORS:
        esz = torch.empty(0, dtype=dt).element_size()
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (rows * cols * (esz + 1)))))
        xs = [torch.randn((rows, cols), device=dev, generator=g, dtype=torch.float32).to(dt) for _ in range(nbuf)]
        rw, pt = alternate([lambda i: N.fp8_quantize_rowwise(xs[i % nbuf], encode_mode=L.ENC_REFERENCE),
                            lambda i: N.fp8_quantize(xs[i % nbuf], encode_mode=L.ENC_REFERENCE)], a.iters)
        assert all(len(r) == 1 for r in rw) and all(len(r) == 2 for r in pt), "one launch against two"
        t_rw, t_pt = med(rw), med(pt)
        need = (esz + 1) * rows * cols
        print(f"{NAME[dt]:5s}{rows:6d} x {cols:<8d} {t_rw:11.2f} {need / t_rw * 1e-6:6.2f} | {t_pt:14.2f} {med(pt, lambda r: r[0]):8.2f} {med(pt, lambda r: r[1]):10.2f} "
              f"{need / t_pt * 1e-6:6.2f} | {t_rw / t_pt:21.3f}", flush=True)
        del xs
    print()
    print(f"{'linear':12s} {'M':>5s} {'K':>6s} {'N':>6s} | {'fp8_linear_rowwise us':>22s} {'(quantise':>10s} {'+ GEMM)':>9s} | {'fp8_linear us':>14s} {'(quantise':>10s} {'+ GEMM)':>9s} | "
          f"{'rowwise / per-tensor':>21s}")
    for name, M, K, Nn in LINEARS:
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (M * K * 3))))
        xs = [torch.randn((M, K), device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16) for _ in range(nbuf)]
        w = torch.randn((Nn, K), device=dev, generator=g) * 0.02
        wq, ws = N.fp8_quantize_rowwise(w)
        wq1, ws1 = N.fp8_quantize(w)
        rw, pt = alternate([lambda i: N.fp8_linear_rowwise(xs[i % nbuf], wq, ws), lambda i: N.fp8_linear(xs[i % nbuf], wq1, ws1)], a.iters)
        t_rw, t_pt = med(rw), med(pt)
        print(f"{name:12s} {M:5d} {K:6d} {Nn:6d} | {t_rw:22.2f} {med(rw, lambda r: r[0]):10.2f} {med(rw, lambda r: sum(r[1:])):9.2f} | "
              f"{t_pt:14.2f} {med(pt, lambda r: r[0] + r[1]):10.2f} {med(pt, lambda r: sum(r[2:])):9.2f} | {t_rw / t_pt:21.3f}", flush=True)


if __name__ == "__main__":
    main()
