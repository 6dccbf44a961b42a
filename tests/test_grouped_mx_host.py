"""Grouped MXFP8 / MXFP4 GEMM and the MX scatter-quantiser on the host (no GPU): the new symbols are declared, exported and bound; every
argument error of fp8mi_scaled_mm_grouped_mxfp8 / _mxfp4 and fp8mi_moe_scatter_quantize_mx through the built library, from NULL or fake
pointers (each check runs before any HIP call); fp8mi_choose_kernel_grouped_mx against the single-problem MX choice."""
import os
import re

import pytest

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


def grouped_mx(lib, fp4, A=P, B=P, C=P, sa=P, ld_sa=None, sb=P, ld_sb=None, stride_sb=None, bias=None, sr=None, offs=P, G=4, M=64, N=32, K=256,
               lda=None, ldb=None, stride_b=None, ldc=None, out=L.BF16, bias_dtype=L.F32, nan=L.NAN_ZERO, kernel=L.KERNEL_AUTO):
    """K in elements; the operands' rows are K bytes (MXFP8) or K / 2 (MXFP4); the scales' rows round_up(K / 32, 4) bytes by default"""
    kb = K // 2 if fp4 else K
    pad = (K // 32 + 3) // 4 * 4
    lda, ldb, ldc = kb if lda is None else lda, kb if ldb is None else ldb, N if ldc is None else ldc
    ld_sa, ld_sb = pad if ld_sa is None else ld_sa, pad if ld_sb is None else ld_sb
    head = (A, B, C, sa, ld_sa, sb, ld_sb, N * ld_sb if stride_sb is None else stride_sb, bias, sr, offs, G, M, N, K, lda, ldb,
            N * ldb if stride_b is None else stride_b, ldc, out, bias_dtype)
    if fp4:
        return lib.fp8mi_scaled_mm_grouped_mxfp4(*head, kernel, None)
    return lib.fp8mi_scaled_mm_grouped_mxfp8(*head, nan, kernel, None)


@pytest.mark.parametrize("fp4", [False, True], ids=["mxfp8", "mxfp4"])
def test_grouped_mx_argument_errors_without_gpu(lib, fp4):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    call = lambda **kw: grouped_mx(lib, fp4, **kw)   # noqa: E731
    kb = 128 if fp4 else 256   # bytes of a default operand row
    for name in ("A", "B", "C", "sa", "sb"):
        assert call(**{name: None}) == E_NULL, name
        assert b"NULL" in err()
    assert call(offs=None) == E_NULL and b"offs" in err()
    # FP8MI_E_SHAPE
    assert call(K=48, lda=48, ldb=48) == E_SHAPE and b"multiple of the 32-element scale block" in err()
    assert call(K=16, lda=16, ldb=16) == E_SHAPE
    assert call(M=-1) == E_SHAPE and b"negative" in err()
    assert call(lda=kb - 1) == E_SHAPE and b"leading dimension" in err()
    assert call(ldb=kb - 1) == E_SHAPE and call(ldc=31) == E_SHAPE
    assert call(ld_sa=7) == E_SHAPE and b"ld_sa / ld_sb" in err()
    assert call(ld_sb=4) == E_SHAPE
    assert call(stride_b=31 * kb + kb - 1) == E_SHAPE and b"stride_b" in err()
    assert call(stride_b=-16) == E_SHAPE
    assert call(stride_sb=31 * 8 + 7) == E_SHAPE and b"stride_sb" in err()
    assert call(stride_sb=-4) == E_SHAPE and b"stride_sb" in err()
    assert call(G=0) == E_SHAPE and b"G=0" in err()
    assert call(G=-3) == E_SHAPE
    # FP8MI_E_ENUM
    assert call(out=3) == E_ENUM and call(bias=P, bias_dtype=7) == E_ENUM
    assert call(kernel=999) == E_ENUM and b"kernel id 999" in err()
    if not fp4:
        assert call(nan=2) == E_ENUM and b"nan mode" in err()
    # FP8MI_E_UNSUPPORTED: scale strides and pointers that would leave a rebased scale base off a 4-byte boundary
    assert call(ld_sa=9) == E_UNSUPPORTED and b"multiples of 4" in err()
    assert call(ld_sb=10, stride_sb=320) == E_UNSUPPORTED
    assert call(stride_sb=32 * 8 + 2) == E_UNSUPPORTED and b"stride_sb=258" in err()
    assert call(sa=P + 2) == E_UNSUPPORTED and call(sb=P + 1) == E_UNSUPPORTED and b"4-byte aligned" in err()
    assert call(G=1025) == E_UNSUPPORTED and b"G=1025" in err()
    assert call(K=0, lda=16, ldb=16) == E_UNSUPPORTED and b"K = 0" in err()
    assert call(bias=P, bias_dtype=L.F32 | L.EPILOGUE_TRANSPOSED) == E_UNSUPPORTED and b"TRANSPOSED" in err()
    for k in NOT_RING:
        assert call(kernel=k) == E_UNSUPPORTED, k
        assert b"no grouped form" in err()
    # operands the ring tiles cannot read (on the operands' bytes)
    assert call(lda=kb + 8) == E_UNSUPPORTED and b"multiples of 16" in err()
    assert call(stride_b=32 * kb + 8) == E_UNSUPPORTED
    assert call(A=P + 4) == E_UNSUPPORTED and call(B=P + 8) == E_UNSUPPORTED
    big = dict(M=1 << 31, N=1 << 31, ldc=1 << 31, G=1)
    assert call(**big) == E_UNSUPPORTED and b"slot grid" in err()
    # M_total = 0 or N = 0 is a no-op that needs no pointers - but not with bad sizes
    none = dict(A=None, B=None, C=None, sa=None, sb=None, offs=None)
    assert call(M=0, **none) == 0 and call(N=0, ldc=0, **none) == 0
    assert call(M=0, G=0, **none) == E_SHAPE and call(M=0, K=48, lda=48, ldb=48, **none) == E_SHAPE


def scatter_mx(lib, x=P, dtype=L.BF16, T=4, cols=128, ld_in=None, row_of=P, k=2, out=P, rows_out=8, ld_out=None, scales=P, ld_s=None, fmt=L.MX_FP8):
    row = cols // 2 if fmt == L.MX_FP4 else cols
    return lib.fp8mi_moe_scatter_quantize_mx(x, dtype, T, cols, cols if ld_in is None else ld_in, row_of, k, out, rows_out,
                                             row if ld_out is None else ld_out, scales, (cols // 32 + 3) // 4 * 4 if ld_s is None else ld_s, fmt, None)


@pytest.mark.parametrize("fmt", [L.MX_FP8, L.MX_FP4], ids=["mxfp8", "mxfp4"])
def test_scatter_mx_argument_errors_without_gpu(lib, fmt):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    call = lambda **kw: scatter_mx(lib, fmt=fmt, **kw)   # noqa: E731
    assert call(cols=48) == E_SHAPE and b"multiple of 32" in err()
    assert call(cols=16416) == E_UNSUPPORTED and b"16384" in err()
    assert call(T=-1) == E_SHAPE and call(k=-1) == E_SHAPE and call(rows_out=-1) == E_SHAPE
    assert call(ld_in=127) == E_SHAPE and b"leading dimension" in err()
    assert call(ld_out=(64 if fmt == L.MX_FP4 else 128) - 1) == E_SHAPE
    assert call(ld_s=3) == E_SHAPE
    assert call(dtype=5) == E_ENUM
    assert scatter_mx(lib, fmt=2) == E_ENUM and b"mx_format" in err()
    for name in ("x", "row_of", "out", "scales"):
        assert call(**{name: None}) == E_NULL, name
    assert call(x=P + 8) == E_UNSUPPORTED and b"16-byte loads" in err()
    assert call(out=P + 2) == E_UNSUPPORTED and call(row_of=P + 2) == E_UNSUPPORTED
    assert call(ld_in=132) == E_UNSUPPORTED   # bf16 rows 264 bytes apart
    assert call(ld_out=130) == E_UNSUPPORTED
    none = dict(x=None, row_of=None, out=None, scales=None)
    assert call(T=0, **none) == 0 and call(k=0, **none) == 0 and call(cols=0, **none) == 0


def test_choose_kernel_grouped_mx(lib):
    shapes = ((8, 64, 4096, 7168), (8, 4096, 4096, 7168), (8, 512, 7168, 2048), (1, 240, 200, 416), (256, 8192, 2048, 7168), (1024, 1024, 512, 128),
              (8, 8 * 1024, 4096, 7168), (3, 100, 200, 1312), (16, 16, 4096, 4096), (4, 4 * 256, 14336, 4096))
    same = 0
    for fmt, single in ((L.MX_FP8, lib.fp8mi_choose_kernel_mxfp8), (L.MX_FP4, lib.fp8mi_choose_kernel_mxfp4)):
        for (G, M, N, K) in shapes:
            kb = K // 2 if fmt == L.MX_FP4 else K
            got = lib.fp8mi_choose_kernel_grouped_mx(fmt, G, M, N, K, kb, kb, N, L.BF16)
            assert got in RING, (fmt, G, M, N, K, got)
            one = single((M + G - 1) // G, N, K, kb, kb, N, L.BF16, 0, 1)   # the single-problem MX choice for the average group
            if one in RING:
                assert got == one, (fmt, G, M, N, K, got, one)
                same += 1
    assert same > 0   # the comparison above ran
    c = lib.fp8mi_choose_kernel_grouped_mx
    assert c(2, 4, 64, 64, 128, 128, 128, 64, L.BF16) == E_ENUM
    assert c(L.MX_FP8, 0, 64, 64, 128, 128, 128, 64, L.BF16) == E_ENUM
    assert c(L.MX_FP8, 4, 64, 64, 144, 144, 144, 64, L.BF16) == E_ENUM
    assert c(L.MX_FP8, 4, 64, 64, 128, 128, 128, 64, 9) == E_ENUM
    assert c(L.MX_FP8, 2000, 64, 64, 128, 128, 128, 64, L.BF16) == E_UNSUPPORTED
    assert c(L.MX_FP4, 4, 64, 64, 0, 16, 16, 64, L.BF16) == E_UNSUPPORTED
    assert c(L.MX_FP8, 4, 64, 64, 128, 136, 128, 64, L.BF16) == E_UNSUPPORTED


def test_grouped_mx_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_scaled_mm_grouped_mxfp8", 24), ("fp8mi_scaled_mm_grouped_mxfp4", 23), ("fp8mi_choose_kernel_grouped_mx", 9),
                        ("fp8mi_moe_scatter_quantize_mx", 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_op_layer_exposes_the_mx_moe_ops():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_scaled_mm_grouped_mxfp8", "fp8_scaled_mm_grouped_mxfp4", "fp8_moe_linear_mxfp8", "fp8_moe_linear_mxfp4", "fp8_moe_mlp_mxfp8",
                 "fp8_moe_mlp_mxfp4", "fp8_moe_forward_mxfp8", "fp8_moe_forward_mxfp4"):
        assert callable(getattr(N, name)), name
        assert getattr(alias, name) is getattr(N, name), name
