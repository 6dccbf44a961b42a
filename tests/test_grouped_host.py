"""Grouped (MoE) FP8 GEMM on the host (no GPU): the slot -> (group, m-tile) resolution against a brute-force enumeration (tests/c/group_slot.cpp,
a program of its own), every argument error of fp8mi_scaled_mm_grouped / _grouped_blockwise through the built library (each check runs before
any HIP call), fp8mi_choose_kernel_grouped, and the torch._scaled_grouped_mm route of the monkey-patch."""
import os
import re
import subprocess

import pytest
import torch

import fp8_mi355x_lib as L

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = (L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_32x32,
        L.KERNEL_GEMM_128D)
NOT_RING = (L.KERNEL_GEMV, L.KERNEL_GENERIC, L.KERNEL_GEMM_256, L.KERNEL_SKINNY, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_GEMM_256W,
            L.KERNEL_GEMM_256x128W)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_slot_resolution_equals_the_brute_force_enumeration(tmp_path):
    """fp8mi_group_slot (csrc/fp8mi_group_slot.h) as a host program: BM in {32, 64, 128} x sizes [0, 1, 130, 64, 33, 0] in 240 rows, all-empty
    groups, one group, 1024 groups of one row, decreasing / over-range / negative offs, offs alternating between M_total and 0, INT32 extremes.
    The slots that resolve tile exactly the clamped groups, once each; no resolved row outside [0, M_total); real tiles <= M_total / BM + G."""
    exe = str(tmp_path / "group_slot")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fp8-mps-metal_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "group_slot.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok 39", out.stdout + out.stderr


def grouped(lib, A=P, B=P, C=P, sa=P, sb=P, bias=None, sr=None, offs=P, G=4, M=64, N=32, K=128, lda=None, ldb=None, stride_b=None, ldc=None,
            sa_mode=L.SCALE_ROW, sb_mode=L.SCALE_ROW, out=L.BF16, bias_dtype=L.F32, nan=L.NAN_ZERO, kernel=L.KERNEL_AUTO):
    lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
    return lib.fp8mi_scaled_mm_grouped(A, B, C, sa, sb, bias, sr, offs, G, M, N, K, lda, ldb, N * ldb if stride_b is None else stride_b, ldc,
                                       sa_mode, sb_mode, out, bias_dtype, nan, kernel, None)


def grouped_bw(lib, A=P, B=P, C=P, sa=P, sa_sr=1, sa_sk=64, block_a=1, sb=P, sb_sr=1, sb_sk=1, sb_se=1, block_b=128, bias=None, sr=None, offs=P,
               G=4, M=64, N=32, K=128, lda=None, ldb=None, stride_b=None, ldc=None, out=L.BF16, bias_dtype=L.F32, nan=L.NAN_ZERO,
               kernel=L.KERNEL_AUTO):
    lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
    return lib.fp8mi_scaled_mm_grouped_blockwise(A, B, C, sa, sa_sr, sa_sk, block_a, sb, sb_sr, sb_sk, sb_se, block_b, bias, sr, offs, G, M, N, K, lda, ldb,
                                                 N * ldb if stride_b is None else stride_b, ldc, out, bias_dtype, nan, kernel, None)


@pytest.mark.parametrize("call", [grouped, grouped_bw], ids=["tensorwise", "blockwise"])
def test_grouped_argument_errors_without_gpu(lib, call):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    # FP8MI_E_NULL: a missing pointer, offs among them
    for name in ("A", "B", "C", "sa", "sb"):
        assert call(lib, **{name: None}) == E_NULL, name
        assert b"NULL" in err()
    assert call(lib, offs=None) == E_NULL and b"offs" in err()
    # FP8MI_E_SHAPE: negative sizes, leading dimensions or strides too small, G < 1
    assert call(lib, M=-1) == E_SHAPE and b"negative" in err()
    assert call(lib, N=-1, ldc=0) == E_SHAPE and call(lib, K=-16, lda=0, ldb=0) == E_SHAPE
    assert call(lib, lda=127) == E_SHAPE and b"leading dimension" in err()
    assert call(lib, ldb=127) == E_SHAPE and call(lib, ldc=31) == E_SHAPE
    assert call(lib, stride_b=31 * 128 + 127) == E_SHAPE and b"stride_b" in err()
    assert call(lib, stride_b=-16) == E_SHAPE and b"stride_b" in err()
    assert call(lib, G=0) == E_SHAPE and b"G=0" in err()
    assert call(lib, G=-3) == E_SHAPE
    # FP8MI_E_ENUM: unknown dtypes, modes, kernel ids
    assert call(lib, out=3) == E_ENUM and b"out_dtype" in err()
    assert call(lib, bias=P, bias_dtype=7) == E_ENUM
    assert call(lib, nan=2) == E_ENUM and b"nan mode" in err()
    assert call(lib, kernel=999) == E_ENUM and b"kernel id 999" in err()
    assert call(lib, kernel=-1) == E_ENUM
    # FP8MI_E_UNSUPPORTED
    assert call(lib, G=1025) == E_UNSUPPORTED and b"G=1025" in err()
    assert call(lib, K=0, lda=16, ldb=16) == E_UNSUPPORTED and b"K = 0" in err()
    for k in NOT_RING:
        assert call(lib, kernel=k) == E_UNSUPPORTED, k
        assert b"no grouped form" in err()
    assert call(lib, bias=P, bias_dtype=L.F32 | L.EPILOGUE_TRANSPOSED) == E_UNSUPPORTED and b"TRANSPOSED" in err()
    # operands the ring tiles cannot read: K, lda, ldb, stride_b not multiples of 16, misaligned A / B, a row stride of 2^22
    assert call(lib, K=120) == E_UNSUPPORTED and b"multiples of 16" in err()
    assert call(lib, lda=136) == E_UNSUPPORTED and call(lib, ldb=136, stride_b=32 * 136) == E_UNSUPPORTED
    assert call(lib, stride_b=32 * 128 + 8) == E_UNSUPPORTED and b"stride_b" in err()
    assert call(lib, A=P + 4) == E_UNSUPPORTED and call(lib, B=P + 8) == E_UNSUPPORTED
    assert call(lib, lda=1 << 22) == E_UNSUPPORTED
    # a slot grid beyond 2^31 - 1 workgroups: (M_total / BM + G) x n-tiles, on AUTO and on a forced tile
    big = dict(M=1 << 31, N=1 << 31, ldc=1 << 31, G=1)
    assert call(lib, **big) == E_UNSUPPORTED and b"slot grid" in err() and b"M_total=2147483648" in err()
    assert call(lib, kernel=L.KERNEL_GEMM_128, **big) == E_UNSUPPORTED and b"slot grid" in err()
    # M_total = 0 or N = 0 is a no-op that needs no pointers - but not with bad sizes
    none = dict(A=None, B=None, C=None, sa=None, sb=None, offs=None)
    assert call(lib, M=0, **none) == 0 and call(lib, N=0, ldc=0, **none) == 0
    assert call(lib, M=0, G=0, **none) == E_SHAPE and call(lib, M=0, K=-1, **none) == E_SHAPE


def test_grouped_tensorwise_and_blockwise_own_errors(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    assert grouped(lib, sa_mode=2) == E_ENUM and b"scale mode" in err()
    assert grouped(lib, sb_mode=-1) == E_ENUM
    assert grouped(lib, sa_mode=2, A=None) == E_NULL   # (the pointer checks come first, as in fp8mi_scaled_mm)
    assert grouped(lib, sa_mode=2, M=0) == 0           # (... and so does the no-op)
    assert grouped_bw(lib, block_a=3) == E_ENUM and b"block_a" in err()
    assert grouped_bw(lib, block_b=64) == E_ENUM
    assert grouped_bw(lib, block_a=L.BLOCK_128) == E_UNSUPPORTED and b"FP8MI_BLOCK_1" in err()
    for name in ("sa_sr", "sa_sk", "sb_sr", "sb_sk", "sb_se"):
        assert grouped_bw(lib, **{name: -1}) == E_SHAPE, name
        assert b"negative scale stride" in err()
    assert grouped_bw(lib, sa=P + 2) == E_UNSUPPORTED and b"4-byte aligned" in err()
    assert grouped_bw(lib, sa_sr=1 << 30) == E_UNSUPPORTED


def test_choose_kernel_grouped_returns_a_ring_tile(lib):
    for (G, M, N, K) in ((8, 64, 4096, 7168), (8, 4096, 4096, 7168), (8, 512, 7168, 2048), (1, 240, 200, 400), (256, 8192, 2048, 7168),
                         (1024, 1024, 512, 128)):
        assert lib.fp8mi_choose_kernel_grouped(G, M, N, K, K, K, N, L.BF16) in RING, (G, M, N, K)
    # priced at ceil(M_total / G) rows: what the single-problem model's ring tiles give for that many rows, whatever G is
    assert lib.fp8mi_choose_kernel_grouped(8, 8 * 512, 4096, 7168, 7168, 7168, 4096, L.BF16) == \
        lib.fp8mi_choose_kernel_grouped(2, 2 * 512, 4096, 7168, 7168, 7168, 4096, L.BF16)
    assert lib.fp8mi_choose_kernel_grouped(0, 64, 64, 128, 128, 128, 64, L.BF16) == E_ENUM
    assert lib.fp8mi_choose_kernel_grouped(4, -1, 64, 128, 128, 128, 64, L.BF16) == E_ENUM
    assert lib.fp8mi_choose_kernel_grouped(4, 64, 64, 128, 128, 128, 64, 9) == E_ENUM
    assert lib.fp8mi_choose_kernel_grouped(4, 64, 64, 120, 120, 120, 64, L.BF16) == E_UNSUPPORTED
    assert lib.fp8mi_choose_kernel_grouped(2000, 64, 64, 128, 128, 128, 64, L.BF16) == E_UNSUPPORTED
    assert lib.fp8mi_choose_kernel_grouped(4, 64, 64, 0, 16, 16, 64, L.BF16) == E_UNSUPPORTED


def test_grouped_symbols_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_scaled_mm_grouped", 23), ("fp8mi_scaled_mm_grouped_blockwise", 28), ("fp8mi_choose_kernel_grouped", 8)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_op_layer_exposes_the_grouped_ops():
    import fp8_mi355x_native as N
    for name in ("fp8_scaled_mm_grouped", "fp8_scaled_mm_grouped_blockwise", "fp8_moe_linear_rowwise", "fp8_moe_linear_blockwise",
                 "fp8_moe_mlp_rowwise", "fp8_moe_mlp_blockwise", "scaled_grouped_mm_colmajor"):
        assert callable(getattr(N, name)), name
    assert set(N.GROUPED_KERNELS) == set(RING)


# ---- the torch._scaled_grouped_mm route of the monkey-patch ----------------------------------------------------------------------------


def test_install_swaps_and_uninstall_restores_scaled_grouped_mm():
    import fp8_mps_patch as patch
    assert not patch.is_installed()
    original = torch._scaled_grouped_mm
    patch.install()
    try:
        assert torch._scaled_grouped_mm is patch._metal_scaled_grouped_mm
        assert patch._original_scaled_grouped_mm is original
        patch.install()   # idempotent
        assert patch._original_scaled_grouped_mm is original
    finally:
        patch.uninstall()
    assert torch._scaled_grouped_mm is original and patch._original_scaled_grouped_mm is None


def test_non_routed_grouped_calls_reach_the_original(monkeypatch):
    """A recording stub stands in for torch's op before install(): 2D x 2D, 3D x 3D, float8_e8m0fnu scales, other dtypes and CPU tensors all
    arrive there with the caller's own objects; nothing touches the native library (CPU tensors never could)."""
    import fp8_mps_patch as patch
    calls = []

    def stub(*args, **kwargs):
        calls.append((args, kwargs))
        return "original"

    monkeypatch.setattr(torch, "_scaled_grouped_mm", stub)
    monkeypatch.setattr(patch, "_native", lambda: pytest.fail("a non-routed call reached the native library"))
    e4 = torch.float8_e4m3fn
    M, K, N, G = 16, 32, 16, 2
    a2 = torch.zeros(M, K).to(e4)
    b3 = torch.zeros(G, N, K).to(e4).transpose(1, 2)
    b2 = torch.zeros(N, K).to(e4).t()
    a3 = torch.zeros(G, M, K).to(e4)
    sa, sb = torch.ones(M), torch.ones(G, N)
    offs = torch.tensor([8, 16], dtype=torch.int32)
    cases = {
        "cpu 2d x 3d": (a2, b3, sa, sb, offs),
        "2d x 2d": (a2, b2, torch.ones(G * M), torch.ones(G * N), offs),
        "3d x 3d": (a3, b3, torch.ones(G, M), sb, None),
        "bf16 operands": (a2.to(torch.bfloat16), b3.to(torch.bfloat16), sa, sb, offs),
        "int64 offs": (a2, b3, sa, sb, offs.long()),
    }
    e8 = getattr(torch, "float8_e8m0fnu", None)
    if e8 is not None:
        cases["e8m0 scales"] = (a2, b3, torch.full((M, K // 32), 127, dtype=torch.uint8).view(e8), torch.full((G, N, K // 32), 127, dtype=torch.uint8).view(e8), offs)
    patch.install()
    try:
        assert patch._original_scaled_grouped_mm is stub
        for name, (a, b, s1, s2, o) in cases.items():
            calls.clear()
            assert torch._scaled_grouped_mm(a, b, s1, s2, o, out_dtype=torch.bfloat16) == "original", name
            (args, kwargs), = calls
            flat = list(args) + list(kwargs.values())
            assert flat[0] is a and flat[1] is b and flat[2] is s1 and flat[3] is s2 and flat[4] is o, name
            assert torch.bfloat16 in flat, name
    finally:
        patch.uninstall()
    assert torch._scaled_grouped_mm is stub


def test_grouped_route_takes_only_the_moe_forward_layout():
    """grouped_route is a pure decision on shapes, dtypes and devices: meta tensors stand in for HIP ones."""
    import fp8_mps_patch as patch
    e4 = torch.float8_e4m3fn
    M, K, N, G = 16, 32, 16, 2

    def args(dev="meta"):
        return dict(input=torch.empty(M, K, dtype=e4, device=dev), mat2=torch.empty(G, N, K, dtype=e4, device=dev).transpose(1, 2),
                    scale_a=torch.empty(M, device=dev), scale_b=torch.empty(G, N, device=dev), offs=torch.empty(G, dtype=torch.int32, device=dev),
                    bias=None, scale_result=None, out_dtype=None)

    orig_dev = patch._DEV
    try:
        patch._DEV = "meta"
        assert patch.grouped_route(**args())
        for k, v in (("out_dtype", torch.bfloat16), ("out_dtype", torch.float32)):
            assert patch.grouped_route(**{**args(), k: v})
        bad = {
            "bias": torch.empty(N, device="meta"), "scale_result": torch.empty(1, device="meta"), "out_dtype": torch.float64,
            "scale_a": torch.empty(M, 1, device="meta"), "scale_b": torch.empty(G, device="meta"), "offs": torch.empty(G + 1, dtype=torch.int32, device="meta"),
            "input": torch.empty(M, K, dtype=torch.float8_e5m2, device="meta"), "mat2": torch.empty(N, K, dtype=e4, device="meta").t(),
        }
        for k, v in bad.items():
            assert not patch.grouped_route(**{**args(), k: v}), k
        assert not patch.grouped_route(**{**args(), "offs": None})
    finally:
        patch._DEV = orig_dev
    assert not patch.grouped_route(**args("cpu"))
