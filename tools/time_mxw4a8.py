#!/usr/bin/env python3
"""Times the MXW4A8 GEMM (e4m3 activations x e2m1 weights) against the MXFP8 and the MXFP4 GEMM - the two recipes it sits between - in ONE
run: the same forced ring tile for the three, alternating calls (mxfp8, mxfp4, mxw4a8, mxfp8, ...), the median of --iters per-dispatch
kernel times (fp8mi_profile_begin / _end: the dispatch packets' timestamps, summed over a call's dispatches), weights rotated through
enough sets to exceed the 256 MiB last-level cache, so that every call streams its weights from HBM.  bf16 out, unit-free random data.

Single problems: M = 512, K = N = 4096 (128x64, unsplit); 4096 x 3072 x 12288 (128x128, unsplit); M = 64 and M = 1 against K = 14336,
N = 4096 (64x64 / 32x32, the library's own split-K).  Grouped form: 64 and 1024 tokens in G = 8 even groups, K = 7168, N = 4096, the
three grouped MX launches on the tile fp8mi_choose_kernel_grouped_mxw4a8 names.  Before a row is timed the mixed result is checked against
the MXFP8 kernel on the weights re-encoded as e4m3 (2e-3 of the magnitude sum: two matrix-core kernels on the same values).
    python tools/time_mxw4a8.py [--iters 30] [--out profiles/mxw4a8_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

CACHE_BYTES = 256 << 20
TILE_NAMES = {L.KERNEL_GEMM_128: "128x128", L.KERNEL_GEMM_128x64: "128x64", L.KERNEL_GEMM_64x128: "64x128", L.KERNEL_GEMM_64x64: "64x64",
              L.KERNEL_GEMM_32x64: "32x64", L.KERNEL_GEMM_32x32: "32x32", L.KERNEL_GEMM_128D: "128x128D"}
E4M3_OF_E2M1 = [0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C, 0x80, 0xB0, 0xB8, 0xBC, 0xC0, 0xC4, 0xC8, 0xCC]


def sets(bytes_per_set):
    return max(2, -(-2 * CACHE_BYTES // bytes_per_set))


def alternate(fns, iters):
    """-> per function the median over `iters` rounds of one call's summed kernel time in us; the functions take the round number"""
    for i in range(3):
        for fn in fns:
            fn(i)
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for i in range(iters):
        for j, fn in enumerate(fns):
            with L.kernel_timer(8) as p:
                fn(i)
            times[j].append(sum(p.ms) * 1e3)
    return [statistics.median(v) for v in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lut = torch.tensor(E4M3_OF_E2M1, dtype=torch.uint8, device=dev)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# tools/time_mxw4a8.py --iters {a.iters} on {torch.cuda.get_device_name(0)}: kernel times in us, median of {a.iters} alternating calls, "
         "weights rotated beyond the last-level cache, bf16 out, one forced tile per row for the three recipes")
    emit(f"{'shape':14s} {'M':>5s} {'N':>5s} {'K':>6s} {'tile':>8s} {'sets':>4s} | {'mxfp8 us':>9s} {'mxfp4 us':>9s} {'mxw4a8 us':>10s} | {'w4a8/mxfp8':>10s} {'w4a8/mxfp4':>10s}")
    o = torch.bfloat16
    shapes = [("C3", 512, 4096, 4096, L.KERNEL_GEMM_128x64, 1), ("FLUX", 4096, 3072, 12288, L.KERNEL_GEMM_128, 1),
              ("decode M=64", 64, 4096, 14336, L.KERNEL_GEMM_64x64, 0), ("decode M=1", 1, 4096, 14336, L.KERNEL_GEMM_32x32, 0)]
    for name, M, Nn, K, tile, split in shapes:
        n4 = sets(Nn * K // 2)   # the same number of sets for both weight widths: the fp8 sets are then twice the cache bound
        A8 = torch.randint(0, 0x7F, (M, K), dtype=torch.uint8, device=dev, generator=gen)
        A4 = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        B4 = [torch.randint(0, 256, (Nn, K // 2), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n4)]
        B8 = [torch.randint(0, 0x7F, (Nn, K), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n4)]
        xa = torch.randint(120, 135, (M, (K // 32 + 3) // 4 * 4), dtype=torch.uint8, device=dev, generator=gen)
        xb = torch.randint(120, 135, (Nn, (K // 32 + 3) // 4 * 4), dtype=torch.uint8, device=dev, generator=gen)
        sa, sb = xa[:, :K // 32], xb[:, :K // 32]
        # the mixed kernel against the MXFP8 kernel on the same values
        b8 = lut[torch.stack((B4[0] & 15, B4[0] >> 4), dim=2).reshape(Nn, K).long()]
        got = N.fp8_scaled_mm_mxw4a8(A8, B4[0], sa, sb, kernel=tile, split_k=1).double()
        ref = N.fp8_scaled_mm_mxfp8(A8, b8, sa, sb, kernel=tile, split_k=1).double()
        assert bool(((got - ref).abs() <= 2e-3 * ref.abs().max()).all()), "the mixed kernel disagrees with MXFP8 on the same values"
        fns = [lambda i: N.fp8_scaled_mm_mxfp8(A8, B8[i % n4], sa, sb, out_dtype=o, kernel=tile, split_k=split),
               lambda i: N.fp8_scaled_mm_mxfp4(A4, B4[i % n4], sa, sb, out_dtype=o, kernel=tile, split_k=split),
               lambda i: N.fp8_scaled_mm_mxw4a8(A8, B4[i % n4], sa, sb, out_dtype=o, kernel=tile, split_k=split)]
        t8, t4, tm = alternate(fns, a.iters)
        emit(f"{name:14s} {M:5d} {Nn:5d} {K:6d} {TILE_NAMES[tile]:>8s} {n4:4d} | {t8:9.2f} {t4:9.2f} {tm:10.2f} | {tm / t8:10.3f} {tm / t4:10.3f}")
        del B4, B8

    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    G, K, NN = 8, 7168, 4096
    NB = K // 32
    n4 = sets(G * NN * K // 2)
    B4 = [torch.randint(0, 256, (G, NN, K // 2), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n4)]
    B8 = [torch.randint(0, 0x7F, (G, NN, K), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n4)]
    sb = torch.randint(120, 135, (G, NN, NB), device=dev, generator=gen, dtype=torch.uint8)
    emit(f"grouped: G = {G} even groups, K = {K}, N = {NN}, {n4} rotating weight sets; the tile of fp8mi_choose_kernel_grouped_mxw4a8 for the three")
    emit(f"{'tokens':>14s} {'':>5s} {'':>5s} {'':>6s} {'tile':>8s} {'sets':>4s} | {'mxfp8 us':>9s} {'mxfp4 us':>9s} {'mxw4a8 us':>10s} | {'w4a8/mxfp8':>10s} {'w4a8/mxfp4':>10s}")
    for m in (64, 1024):
        A8 = torch.randint(0, 0x7F, (m, K), dtype=torch.uint8, device=dev, generator=gen)
        A4 = torch.randint(0, 256, (m, K // 2), dtype=torch.uint8, device=dev, generator=gen)
        sa = torch.randint(120, 135, (m, NB), device=dev, generator=gen, dtype=torch.uint8)
        offs = torch.arange(1, G + 1, dtype=torch.int32, device=dev) * (m // G)
        C = torch.empty((m, NN), device=dev, dtype=o)
        tile = lib.fp8mi_choose_kernel_grouped_mxw4a8(G, m, NN, K, K, K // 2, NN, L.BF16)
        assert tile in TILE_NAMES, tile

        def call(entry, A, B, lda, ldb, nan):
            rc = getattr(lib, entry)(A.data_ptr(), B.data_ptr(), C.data_ptr(), sa.data_ptr(), NB, sb.data_ptr(), NB, NN * NB, None, None, offs.data_ptr(),
                                     G, m, NN, K, lda, ldb, NN * ldb, NN, L.BF16, L.F32, *nan, tile, stream)
            L.check(rc, entry)

        fns = [lambda i: call("fp8mi_scaled_mm_grouped_mxfp8", A8, B8[i % n4], K, K, (L.NAN_ZERO,)),
               lambda i: call("fp8mi_scaled_mm_grouped_mxfp4", A4, B4[i % n4], K // 2, K // 2, ()),
               lambda i: call("fp8mi_scaled_mm_grouped_mxw4a8", A8, B4[i % n4], K, K // 2, (L.NAN_ZERO,))]
        t8, t4, tm = alternate(fns, a.iters)
        emit(f"{m:14d} {'':>5s} {'':>5s} {'':>6s} {TILE_NAMES[tile]:>8s} {n4:4d} | {t8:9.2f} {t4:9.2f} {tm:10.2f} | {tm / t8:10.3f} {tm / t4:10.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
