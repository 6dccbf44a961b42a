"""MXW4A8 (e4m3 activations x e2m1 weights) on the host (no GPU): the new symbols are declared, exported and bound; the argument checks
of fp8mi_scaled_mm_mxw4a8 and fp8mi_scaled_mm_grouped_mxw4a8 through the built library, from NULL or fake pointers (every check runs
before any HIP call); the two choosers; the op layer's shape assertions, defaults and launch order with the C calls recorded; and, on the
very inputs the GPU edge tests build (tests/test_gpu_mx_edges.py, tests/mxw4a8_ref.py), what those tests rely on: the packing of the builders,
references that are fp32 values where the tests ask for equal bits, and epilogue sums inside float16's range."""
import os
import re

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = (L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_32x32,
        L.KERNEL_GEMM_128D)
NO_FORM = (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_SKINNY, L.KERNEL_GEMM_256, L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def mm(lib, M=64, N=64, K=256, lda=None, ldb=None, ldc=None, ld_sa=None, ld_sb=None, kernel=L.KERNEL_AUTO, out=L.F32, bias=L.F32,
       nan=L.NAN_ZERO, split=0, A=P, B=P, C=P, sa=P, sb=P):
    return lib.fp8mi_scaled_mm_mxw4a8(A, B, C, sa, K // 32 if ld_sa is None else ld_sa, sb, K // 32 if ld_sb is None else ld_sb, None, None,
                                      M, N, K, K if lda is None else lda, K // 2 if ldb is None else ldb, N if ldc is None else ldc,
                                      out, bias, nan, kernel, split, None, 0, None)


def test_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_scaled_mm_mxw4a8", 23), ("fp8mi_choose_kernel_mxw4a8", 9), ("fp8mi_scaled_mm_grouped_mxw4a8", 24),
                        ("fp8mi_choose_kernel_grouped_mxw4a8", 8)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert L.SIGNATURES["fp8mi_scaled_mm_mxw4a8"] == L.SIGNATURES["fp8mi_scaled_mm_mxfp8"]                    # the MXFP8 entry points' argument lists
    assert L.SIGNATURES["fp8mi_scaled_mm_grouped_mxw4a8"] == L.SIGNATURES["fp8mi_scaled_mm_grouped_mxfp8"]
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_scaled_mm_mxw4a8_validation(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    assert mm(lib, K=100) == E_SHAPE and b"multiple of the 32-element scale block" in err()
    assert mm(lib, K=48) == E_SHAPE
    assert mm(lib, K=-32) == E_SHAPE
    assert mm(lib, lda=255) == E_SHAPE and b"leading dimension" in err()    # lda < K bytes
    assert mm(lib, lda=128) == E_SHAPE                   # ... K / 2 is not enough on the e4m3 side
    assert mm(lib, ldb=127) == E_SHAPE                   # ldb < K / 2 bytes
    # ... and K / 2 is enough on the e2m1 side.  Asked of a forced tile with A off 16 bytes, which is refused behind the shape checks and
    # before any launch: a call that passes EVERY check launches, and where a GPU is present the kernel would then read and write at P
    assert mm(lib, ldb=128, A=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, ldb=127, A=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_SHAPE    # (the shape checks come first)
    assert mm(lib, ld_sa=7) == E_SHAPE and b"ld_sa / ld_sb" in err()
    assert mm(lib, ld_sb=7) == E_SHAPE
    assert mm(lib, ldc=10) == E_SHAPE
    assert mm(lib, M=-1) == E_SHAPE
    for name in ("A", "B", "C", "sa", "sb"):
        assert mm(lib, **{name: None}) == E_NULL, name
    assert mm(lib, out=7) == E_ENUM
    assert mm(lib, nan=2) == E_ENUM and b"nan mode" in err()
    assert mm(lib, split=-1) == E_ENUM
    assert mm(lib, kernel=999) == E_ENUM
    for k in NO_FORM:
        assert mm(lib, kernel=k) == E_UNSUPPORTED, k      # a kernel id without the form
        assert b"no MXW4A8 form" in err()
    # a forced ring tile with scales it cannot read in 4-byte pieces, or operands off 16 bytes
    assert mm(lib, K=160, ld_sa=5, ld_sb=8, kernel=L.KERNEL_GEMM_128x64) == E_UNSUPPORTED
    assert mm(lib, sa=P + 2, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, A=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, B=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, K=288, lda=296, kernel=L.KERNEL_GEMM_32x32) == E_UNSUPPORTED    # A's row stride 296 bytes: not 16-aligned
    assert mm(lib, K=288, ldb=152, kernel=L.KERNEL_GEMM_32x32) == E_UNSUPPORTED    # B's row stride 152 bytes
    assert mm(lib, M=0) == 0 and mm(lib, N=0) == 0          # no-ops
    assert mm(lib, M=0, A=None, B=None, C=None, sa=None, sb=None) == 0


def test_auto_choice_is_a_tile_with_the_form_or_generic(lib):
    c = lib.fp8mi_choose_kernel_mxw4a8
    for M in (1, 2, 7, 33, 64, 128, 300, 512, 4096):
        for N in (1, 64, 200, 3072, 4096):
            for K in (32, 96, 160, 4096, 4128, 12288, 14336):
                assert c(M, N, K, K, K // 2, N, L.BF16, 1, 0) in RING, (M, N, K)
    assert c(64, 64, 0, 0, 0, 64, L.F32, 0, 0) == L.KERNEL_GENERIC
    assert c(64, 64, 96, 96, 56, 64, L.F32, 0, 0) == L.KERNEL_GENERIC     # B's row stride is no multiple of 16
    assert c(64, 64, 96, 104, 48, 64, L.F32, 0, 0) == L.KERNEL_GENERIC    # A's
    assert c(64, 64, 100, 100, 50, 64, L.F32, 0, 0) < 0
    assert c(64, 64, 128, 128, 64, 64, 9, 0, 0) < 0
    # priced at the weights' byte depth: the MXFP4 choice for the same shape
    for (M, N, K) in ((64, 4096, 14336), (512, 4096, 4096), (1, 4096, 14336), (4096, 3072, 12288)):
        assert c(M, N, K, K, K // 2, N, L.BF16, 1, 0) == lib.fp8mi_choose_kernel_mxfp4(M, N, K, K // 2, K // 2, N, L.BF16, 1, 0)


def grouped(lib, A=P, B=P, C=P, sa=P, ld_sa=None, sb=P, ld_sb=None, stride_sb=None, bias=None, sr=None, offs=P, G=4, M=64, N=32, K=256,
            lda=None, ldb=None, stride_b=None, ldc=None, out=L.BF16, bias_dtype=L.F32, nan=L.NAN_ZERO, kernel=L.KERNEL_AUTO):
    """K in elements; A's rows are K bytes, B's K / 2; the scales' rows round_up(K / 32, 4) bytes by default"""
    pad = (K // 32 + 3) // 4 * 4
    lda, ldb, ldc = K if lda is None else lda, K // 2 if ldb is None else ldb, N if ldc is None else ldc
    ld_sa, ld_sb = pad if ld_sa is None else ld_sa, pad if ld_sb is None else ld_sb
    return lib.fp8mi_scaled_mm_grouped_mxw4a8(A, B, C, sa, ld_sa, sb, ld_sb, N * ld_sb if stride_sb is None else stride_sb, bias, sr, offs, G, M, N, K,
                                              lda, ldb, N * ldb if stride_b is None else stride_b, ldc, out, bias_dtype, nan, kernel, None)


def test_grouped_mxw4a8_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    call = lambda **kw: grouped(lib, **kw)   # noqa: E731
    for name in ("A", "B", "C", "sa", "sb"):
        assert call(**{name: None}) == E_NULL, name
        assert b"NULL" in err()
    assert call(offs=None) == E_NULL and b"offs" in err()
    assert call(K=48, lda=48, ldb=32) == E_SHAPE and b"multiple of the 32-element scale block" in err()
    assert call(M=-1) == E_SHAPE and b"negative" in err()
    assert call(lda=255) == E_SHAPE and b"leading dimension" in err()      # lda < K
    assert call(lda=128) == E_SHAPE                                          # (K / 2 is the weights' row)
    assert call(ldb=127) == E_SHAPE and call(ldc=31) == E_SHAPE
    assert call(ld_sa=7) == E_SHAPE and b"ld_sa / ld_sb" in err()           # below K / 32
    assert call(ld_sb=4) == E_SHAPE
    assert call(stride_b=31 * 128 + 127) == E_SHAPE and b"stride_b" in err()
    assert call(stride_sb=31 * 8 + 7) == E_SHAPE and b"stride_sb" in err()
    assert call(G=0) == E_SHAPE and b"G=0" in err()
    assert call(out=3) == E_ENUM and call(bias=P, bias_dtype=7) == E_ENUM
    assert call(kernel=999) == E_ENUM and b"kernel id 999" in err()
    assert call(nan=2) == E_ENUM and b"nan mode" in err()
    assert call(ld_sa=9) == E_UNSUPPORTED and b"multiples of 4" in err()    # not a multiple of 4
    assert call(ld_sb=10, stride_sb=320) == E_UNSUPPORTED
    assert call(stride_sb=32 * 8 + 2) == E_UNSUPPORTED
    assert call(sa=P + 2) == E_UNSUPPORTED and call(sb=P + 1) == E_UNSUPPORTED
    assert call(G=1025) == E_UNSUPPORTED and b"G=1025" in err()
    assert call(K=0, lda=16, ldb=16) == E_UNSUPPORTED and b"K = 0" in err()
    assert call(bias=P, bias_dtype=L.F32 | L.EPILOGUE_TRANSPOSED) == E_UNSUPPORTED and b"TRANSPOSED" in err()
    for k in NO_FORM + (L.KERNEL_GENERIC,):
        assert call(kernel=k) == E_UNSUPPORTED, k
        assert b"no grouped form" in err()
    assert call(lda=264) == E_UNSUPPORTED and b"multiples of 16" in err()
    assert call(ldb=136, stride_b=32 * 136) == E_UNSUPPORTED
    assert call(stride_b=32 * 128 + 8) == E_UNSUPPORTED
    assert call(A=P + 4) == E_UNSUPPORTED and call(B=P + 8) == E_UNSUPPORTED
    none = dict(A=None, B=None, C=None, sa=None, sb=None, offs=None)
    assert call(M=0, **none) == 0 and call(N=0, ldc=0, **none) == 0
    assert call(M=0, G=0, **none) == E_SHAPE


def test_choose_kernel_grouped_mxw4a8(lib):
    c = lib.fp8mi_choose_kernel_grouped_mxw4a8
    for (G, M, N, K) in ((8, 64, 4096, 7168), (8, 4096, 4096, 7168), (8, 512, 7168, 2048), (1, 240, 200, 416), (3, 100, 200, 1312),
                         (16, 16, 4096, 4096)):
        got = c(G, M, N, K, K, K // 2, N, L.BF16)
        assert got in RING, (G, M, N, K, got)
        assert got == lib.fp8mi_choose_kernel_grouped_mx(L.MX_FP4, G, M, N, K, K // 2, K // 2, N, L.BF16)   # the weights' byte depth
    assert c(0, 64, 64, 128, 128, 64, 64, L.BF16) == E_ENUM
    assert c(4, 64, 64, 144, 144, 72, 64, L.BF16) == E_ENUM                # K % 32
    assert c(4, 64, 64, 128, 128, 64, 64, 9) == E_ENUM
    assert c(2000, 64, 64, 128, 128, 64, 64, L.BF16) == E_UNSUPPORTED
    assert c(4, 64, 64, 0, 16, 16, 64, L.BF16) == E_UNSUPPORTED
    assert c(4, 64, 64, 128, 136, 64, 64, L.BF16) == E_UNSUPPORTED         # a row stride that is no multiple of 16
    assert c(4, 64, 64, 128, 128, 72, 64, L.BF16) == E_UNSUPPORTED
    # fp8mi_choose_kernel_grouped_mx keeps its two element formats
    assert lib.fp8mi_choose_kernel_grouped_mx(2, 4, 64, 64, 128, 128, 128, 64, L.BF16) == E_ENUM


def test_op_layer_exposes_the_ops():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_scaled_mm_mxw4a8", "fp8_linear_mxw4a8", "fp8_mlp_mxw4a8", "fp8_norm_linear_mxw4a8", "fp8_scaled_mm_grouped_mxw4a8",
                 "fp8_moe_linear_mxw4a8", "fp8_moe_mlp_mxw4a8", "fp8_moe_forward_mxw4a8"):
        assert callable(getattr(N, name)), name
        assert getattr(alias, name) is getattr(N, name), name
    assert "mxw4a8" in N._MOE_LAYER_RECIPE and N.MXW4A8_KERNELS == N.MXFP8_KERNELS
    # the recipe table names the activations' scale apart from the weights' packing; the old rows keep their launches
    assert N._MOE_RECIPES["mxw4a8"][3:] == (2, "mxfp8")
    assert [N._MOE_RECIPES[r][3:] for r in ("row", "block128", "mxfp8", "mxfp4")] == [(1, "row"), (1, "block128"), (1, "mxfp8"), (2, "mxfp4")]


class Recorder:
    """stands in for the library: records (entry, args) of every C call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fp8mi_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture()
def rec(monkeypatch):
    import fp8_mi355x_native as N
    r = Recorder()
    monkeypatch.setattr(N, "DEVICE_TYPE", "cpu")                      # stand in for the HIP device
    monkeypatch.setattr(N, "_stream", lambda dev: 0)
    monkeypatch.setattr(N._l, "load", lambda: r)
    return N, r


def test_scaled_mm_op_shapes_defaults_and_arguments(rec):
    N, r = rec
    M, Nn, K = 8, 24, 64
    A, B = torch.zeros(M, K, dtype=torch.uint8), torch.zeros(Nn, K // 2, dtype=torch.uint8)
    sa, sb = torch.full((M, K // 32), 127, dtype=torch.uint8), torch.full((Nn, K // 32), 127, dtype=torch.uint8)
    out = N.fp8_scaled_mm_mxw4a8(A, B, sa, sb, split_k=1)
    assert out.dtype == torch.float32 and tuple(out.shape) == (M, Nn)   # default out_dtype
    name, args = r.calls[-1]
    assert name == "fp8mi_scaled_mm_mxw4a8" and len(args) == 23
    assert args[9:15] == (M, Nn, K, K, K // 2, Nn)                      # M, N, K (elements), lda = K bytes, ldb = K / 2 bytes, ldc
    assert args[15:19] == (L.F32, L.F32, N.NAN_MODE, L.KERNEL_AUTO) and args[19:22] == (1, None, 0)
    N.fp8_scaled_mm_mxw4a8(A, B.view(torch.float4_e2m1fn_x2), sa.view(torch.float8_e8m0fnu), sb, out_dtype=torch.bfloat16, nan_mode=L.NAN_PROPAGATE,
                           bias=torch.zeros(M, dtype=torch.bfloat16), transposed_epilogue=True, split_k=1, kernel=L.KERNEL_GEMM_32x32)
    args = r.calls[-1][1]
    assert args[15:19] == (L.BF16, L.BF16 | L.EPILOGUE_TRANSPOSED, L.NAN_PROPAGATE, L.KERNEL_GEMM_32x32)
    with pytest.raises(AssertionError, match="e2m1 elements per row"):
        N.fp8_scaled_mm_mxw4a8(A, torch.zeros(Nn, K, dtype=torch.uint8), sa, sb)          # B as wide as A: not two per byte
    with pytest.raises(AssertionError, match="multiple of the 32-element"):
        N.fp8_scaled_mm_mxw4a8(torch.zeros(M, 48, dtype=torch.uint8), torch.zeros(Nn, 24, dtype=torch.uint8), sa, sb)
    with pytest.raises(AssertionError):
        N.fp8_scaled_mm_mxw4a8(A, B, sa[:, :1], sb)                                       # scales that do not hold (M, K / 32)
    n = len(r.calls)
    assert tuple(N.fp8_scaled_mm_mxw4a8(A[:0], B, sa[:0], sb).shape) == (0, Nn) and len(r.calls) == n    # M = 0: no call


def test_linear_mlp_and_norm_linear_compose_the_mxfp8_producers(rec):
    N, r = rec
    K, H, Nn = 64, 32, 16
    x = torch.zeros(2, 3, K, dtype=torch.bfloat16)
    w1, s1 = torch.zeros(2 * H, K // 2, dtype=torch.uint8), torch.full((2 * H, K // 32), 127, dtype=torch.uint8)
    w2, s2 = torch.zeros(Nn, H // 2, dtype=torch.uint8), torch.full((Nn, H // 32), 127, dtype=torch.uint8)
    y = N.fp8_linear_mxw4a8(x, w1, s1)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 3, 2 * H)                 # default out_dtype: x's
    assert [c[0] for c in r.calls] == ["fp8mi_quantize_mxfp8", "fp8mi_scaled_mm_mxw4a8"]
    assert N.fp8_linear_mxw4a8(x.float(), w1, s1, out_dtype=torch.float16).dtype == torch.float16
    with pytest.raises(AssertionError):
        N.fp8_linear_mxw4a8(torch.zeros(2, K // 2), w1, s1)                              # x as wide as the weights' BYTES
    del r.calls[:]
    y = N.fp8_mlp_mxw4a8(x, w1, s1, w2, s2)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 3, Nn)
    assert [c[0] for c in r.calls] == ["fp8mi_act_quantize_mx", "fp8mi_scaled_mm_mxw4a8", "fp8mi_act_quantize_mx", "fp8mi_scaled_mm_mxw4a8"]
    assert all(c[1][10] == L.MX_FP8 for c in r.calls if c[0] == "fp8mi_act_quantize_mx")   # both activations quantised to MXFP8
    with pytest.raises(AssertionError, match="hidden features"):
        N.fp8_mlp_mxw4a8(x, w1, s1, torch.zeros(Nn, H, dtype=torch.uint8), s2)           # w2 of H bytes = 2 H elements
    del r.calls[:]
    y = N.fp8_norm_linear_mxw4a8(x, w1, s1, weight=torch.ones(K))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 3, 2 * H)
    assert [c[0] for c in r.calls] == ["fp8mi_norm_quantize_mx", "fp8mi_scaled_mm_mxw4a8"]
    assert r.calls[0][1][22] == L.MX_FP8


def test_moe_ops_launch_what_the_mxfp8_layer_launches(rec):
    N, r = rec
    G, K, H, Nn, T, k = 4, 64, 32, 16, 5, 2
    x = torch.zeros(T, K, dtype=torch.bfloat16)
    w1, s1 = torch.zeros(G, 2 * H, K // 2, dtype=torch.uint8), torch.full((G, 2 * H, 4), 127, dtype=torch.uint8)[:, :, :K // 32]
    w2, s2 = torch.zeros(G, Nn, H // 2, dtype=torch.uint8), torch.full((G, Nn, 4), 127, dtype=torch.uint8)[:, :, :H // 32]
    w1_8, w2_8 = torch.zeros(G, 2 * H, K, dtype=torch.uint8), torch.zeros(G, Nn, H, dtype=torch.uint8)
    ids = torch.tensor([[0, 1], [2, 3], [1, 7], [0, 0], [3, 2]], dtype=torch.int32)
    logits = torch.zeros(T, G)
    names = lambda: [c[0] for c in r.calls]   # noqa: E731
    mixed = lambda n: n.replace("grouped_mxfp8", "grouped_mxw4a8")   # noqa: E731

    def launches(fn, *a, **kw):
        del r.calls[:]
        out = fn(*a, **kw)
        return out, names()

    offs = torch.tensor([2, 3, 4, 5], dtype=torch.int32)
    y, got = launches(N.fp8_moe_linear_mxw4a8, x, offs, w1, s1)
    _y8, want = launches(N.fp8_moe_linear_mxfp8, x, offs, w1_8, s1)
    assert got == [mixed(n) for n in want] and len(got) == 2 and tuple(y.shape) == (T, 2 * H) and y.dtype == torch.bfloat16
    y, got = launches(N.fp8_moe_mlp_mxw4a8, x, offs, w1, s1, w2, s2)
    _y8, want = launches(N.fp8_moe_mlp_mxfp8, x, offs, w1_8, s1, w2_8, s2)
    assert got == [mixed(n) for n in want] and len(got) == 4 and tuple(y.shape) == (T, Nn)
    y, got = launches(N.fp8_moe_forward_mxw4a8, x, ids, None, w1, s1, w2, s2)
    _y8, want = launches(N.fp8_moe_forward_mxfp8, x, ids, None, w1_8, s1, w2_8, s2)
    assert got == [mixed(n) for n in want] and tuple(y.shape) == (T, Nn) and y.dtype == torch.bfloat16
    assert sum(n.startswith("fp8mi_") and "workspace_bytes" not in n for n in got) == 6          # six launches up to 1024 assignments
    scatter = [c for c in r.calls if c[0] == "fp8mi_moe_scatter_quantize_mx"]
    _y, got7 = launches(N.fp8_moe_layer, x, logits, k, w1, s1, w2, s2, recipe="mxw4a8")
    assert [n for n in got7 if "workspace_bytes" not in n] == ["fp8mi_moe_gate"] + [n for n in got if "workspace_bytes" not in n]   # seven from the logits
    assert all(c[1][12] == L.MX_FP8 for c in r.calls if c[0] == "fp8mi_moe_scatter_quantize_mx") and len(scatter) <= 1
    assert all(c[1][10] == L.MX_FP8 for c in r.calls if c[0] == "fp8mi_act_quantize_mx")
    # T = 0: the empty tensor without a launch
    empty, got = launches(N.fp8_moe_forward_mxw4a8, x[:0], ids[:0], None, w1, s1, w2, s2)
    assert got == [] and tuple(empty.shape) == (0, Nn) and empty.dtype == torch.bfloat16
    with pytest.raises(AssertionError):
        N.fp8_moe_layer(x, logits, k, w1, s1, w2, s2, recipe="mxw8a4")
    with pytest.raises(AssertionError):
        N.fp8_moe_mlp_mxw4a8(x, offs, w1, s1, torch.zeros(G, Nn, H, dtype=torch.uint8), s2)    # w2 of H bytes = 2 H elements
    with pytest.raises(AssertionError):
        N.fp8_scaled_mm_grouped_mxw4a8(torch.zeros(5, K, dtype=torch.uint8), w1_8, torch.zeros(5, 2, dtype=torch.uint8), s1, offs)   # B as wide as A


# ---- the inputs of the GPU edge tests (tests/test_gpu_mx_edges.py on its MXW4A8 adapter): conditions on the inputs alone -----------------------

def test_edge_builders_hold_what_they_are_named_for():
    import mxfp4_ref
    import mxfp8_ref
    import mxw4a8_ref as R
    rng = np.random.default_rng(1)
    dec = mxfp8_ref.DEC_ZERO
    A = R.rand_a(rng, 64, 256)
    assert A.shape == (64, 256) and A.dtype == np.uint8 and not np.any((A & 0x7F) == 0x7F) and len(np.unique(A)) == 254   # every byte but the NaNs
    B = R.rand_b(rng, 64, 256)
    assert B.shape == (64, 128) and B.dtype == np.uint8 and len(np.unique(mxfp4_ref.unpack(B))) == 16
    ks = (37 * np.arange(64) + 5) % 256
    H = R.one_hot_a(64, 256, ks)
    assert H.shape == (64, 256) and np.count_nonzero(H) == 64 and np.all(H[np.arange(64), ks] == 0x38) and dec[0x38] == 1.0
    Ia = R.small_ints_a(rng, 64, 256)
    assert Ia.shape == (64, 256) and sorted(set(dec[Ia].ravel())) == [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    codes = R.INT_B_CODES[rng.integers(0, len(R.INT_B_CODES), (8, 64))]
    packed = R.pack_e2m1(codes)
    assert packed.shape == (8, 32) and np.array_equal(packed & 0xF, codes[:, 0::2]) and np.array_equal(packed >> 4, codes[:, 1::2])   # even k low
    assert np.array_equal(mxfp4_ref.unpack(packed), codes)
    Ib = R.small_ints_b(rng, 64, 256)
    vals = dec[R.w_as_e4m3(Ib)]
    assert Ib.shape == (64, 128) and sorted(set(vals.ravel())) == [-6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6]


def _is_fp32(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


def test_exact_edge_cases_have_fp32_references():
    """the selector (M = 128, N = 80, K = 512, scales in [90, 159]) and the small integers (M = 100, N = 136, K = 992, scales in [126, 128]):
    the GPU tests ask for mm_ref bit for bit, so mm_ref must be an fp32 value everywhere - and not mostly zero"""
    import test_gpu_mx_edges as E
    fx = E._MXW4A8
    A, B, sa, sb = E.selector_inputs(fx)
    assert A.shape == (128, 512) and B.shape == (80, 256) and sa.shape == (128, 16) and sb.shape == (80, 16)
    assert sa.min() >= 90 and sa.max() <= 159 and sb.min() >= 90 and sb.max() <= 159 and len(np.unique(sa)) > 60 and len(np.unique(sb)) > 60
    exact, _ = fx.ref(A, B, sa, sb)
    assert _is_fp32(exact) and np.count_nonzero(exact) > exact.size // 2
    A, B, sa, sb = E.small_int_inputs(fx)
    assert A.shape == (100, 992) and B.shape == (136, 496) and set(np.unique(sa)) == {126, 127, 128} == set(np.unique(sb))
    exact, bound = fx.ref(A, B, sa, sb)
    assert _is_fp32(exact) and np.count_nonzero(exact) > exact.size // 2
    # ... in any order of summation: every product is a multiple of 2^-2, and the sum of their magnitudes stays below 2^22
    a = mxfp8_scaled(A, sa)
    assert np.array_equal(a * 2, np.floor(a * 2)) and float(bound.max()) * 4 < 2 ** 24


def mxfp8_scaled(A, sa):
    import mxfp8_ref
    return mxfp8_ref.scaled_operand(A, sa, True)


# (M, N, K, seed) of every problem the edge tests draw with the epilogue scale range: test_epilogue_bias_scale_result_every_kernel,
# test_epilogue_single_and_odd_columns, test_transposed_epilogue, test_out_as_a_column_slice
EPILOGUE_SHAPES = [(300, 520, 384, 0), (512, 768, 384, 0), (70, 1, 256, 0), (130, 77, 384, 0), (1, 77, 256, 0), (72, 256, 768, 2), (200, 136, 256, 5)]


def test_epilogue_scale_range_keeps_the_sums_inside_float16():
    """scales 119 .. 125 (2^-8 .. 2^-2 per side, the range of tests/test_gpu_mxw4a8.py): max |exact| < 65504 at every epilogue shape, with room
    for the bias (make_bias: |bias| < max(M, N) + 20) and the scale_result (at most 1.5) the tests add"""
    import test_gpu_mx_edges as E
    fx = E._MXW4A8
    assert fx.epi_scales == (119, 125)
    for M, N, K, seed in EPILOGUE_SHAPES:
        A, B, sa, sb, exact, bound = E.problem(fx, M, N, K, *fx.epi_scales, seed=seed)
        assert A.shape == (M, K) and B.shape == (N, K // 2) and sa.min() >= 119 and sa.max() <= 125 and sb.min() >= 119 and sb.max() <= 125
        assert np.max(np.abs(exact)) < 65504.0, (M, N, K)
        assert (np.max(np.abs(exact)) + 1e-3 * np.max(bound) + max(M, N) + 20.0) * 1.5 < 65504.0, (M, N, K)
