"""MXFP8 on the host (no GPU): argument validation of the three C entry points (every check runs before any HIP call), the
patch's scale-layout / routing helpers, and the RCEIL restatement the GPU tests use as their reference."""
import math

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from mxfp8_ref import to_mxfp8_ref

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def mm(lib, M=64, N=64, K=128, lda=None, ldb=None, ldc=None, ld_sa=None, ld_sb=None, kernel=L.KERNEL_AUTO, out=L.F32, bias=L.F32,
       nan=L.NAN_ZERO, split=0, A=P, B=P, C=P, sa=P, sb=P):
    return lib.fp8mi_scaled_mm_mxfp8(A, B, C, sa, K // 32 if ld_sa is None else ld_sa, sb, K // 32 if ld_sb is None else ld_sb, None, None,
                                     M, N, K, K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc,
                                     out, bias, nan, kernel, split, None, 0, None)


def test_scaled_mm_mxfp8_validation(lib):
    assert mm(lib, K=100) == E_SHAPE                     # K % 32
    assert mm(lib, K=-32) == E_SHAPE
    assert mm(lib, ld_sa=3) == E_SHAPE                   # ld_sa < K/32
    assert mm(lib, ld_sb=3) == E_SHAPE
    assert mm(lib, lda=64) == E_SHAPE
    assert mm(lib, ldc=10) == E_SHAPE
    assert mm(lib, C=None) == E_NULL
    assert mm(lib, sa=None) == E_NULL
    assert mm(lib, out=7) == E_ENUM
    assert mm(lib, nan=2) == E_ENUM
    assert mm(lib, split=-1) == E_ENUM
    assert mm(lib, kernel=999) == E_ENUM
    for k in (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_SKINNY, L.KERNEL_GEMM_256, L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W):
        assert mm(lib, kernel=k) == E_UNSUPPORTED, k      # no block-scaled form
    # a forced ring tile with scales it cannot read in 4-byte K-steps
    assert mm(lib, K=160, ld_sa=5, ld_sb=8, kernel=L.KERNEL_GEMM_128x64) == E_UNSUPPORTED
    assert mm(lib, sa=P + 2, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, A=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, M=0) == 0 and mm(lib, N=0) == 0          # no-ops


def test_quantize_dequant_mxfp8_validation(lib):
    q = lib.fp8mi_quantize_mxfp8
    assert q(P, L.F32, 4, 48, 48, P, 48, P, 2, None) == E_SHAPE      # cols % 32
    assert q(P, L.F32, 4, 64, 32, P, 64, P, 2, None) == E_SHAPE      # ld_in
    assert q(P, L.F32, 4, 64, 64, P, 32, P, 2, None) == E_SHAPE      # ld_out
    assert q(P, L.F32, 4, 64, 64, P, 64, P, 1, None) == E_SHAPE      # ld_s
    assert q(P, 9, 4, 64, 64, P, 64, P, 2, None) == E_ENUM
    assert q(None, L.F32, 4, 64, 64, P, 64, P, 2, None) == E_NULL
    assert q(P, L.F32, 0, 64, 64, P, 64, P, 2, None) == 0
    d = lib.fp8mi_dequant_mxfp8
    assert d(P, 4, 64, 32, P, 2, P, L.F32, None) == E_SHAPE          # ld_in
    assert d(P, 4, 64, 64, P, 1, P, L.F32, None) == E_SHAPE          # ld_s < ceil(cols / 32)
    assert d(P, 4, 64, 64, P, 2, P, 9, None) == E_ENUM
    assert d(P, 4, 64, 64, None, 2, P, L.F32, None) == E_NULL
    assert d(P, -1, 64, 64, P, 2, P, L.F32, None) == E_SHAPE


def test_auto_choice_is_a_block_scaled_kernel(lib):
    ring = {L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
            L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D}
    for M, N, K in ((1, 4096, 4096), (64, 4096, 14336), (512, 4096, 4096), (4096, 3072, 12288), (300, 200, 160)):
        assert lib.fp8mi_choose_kernel_mxfp8(M, N, K, K, K, N, L.BF16, 1, 0) in ring, (M, N, K)
    assert lib.fp8mi_choose_kernel_mxfp8(64, 64, 0, 0, 0, 64, L.F32, 0, 0) == L.KERNEL_GENERIC
    assert lib.fp8mi_choose_kernel_mxfp8(64, 64, 100, 112, 112, 64, L.F32, 0, 0) < 0


E8 = torch.float8_e8m0fnu


def test_scale_layouts():
    import fp8_mi355x_native as N
    ld = N.mxfp8_scale_ld
    assert ld(torch.zeros(300, 5, dtype=torch.uint8), 300, 160) == 5                 # plain (rows, K/32)
    assert ld(torch.zeros(384, 8, dtype=torch.uint8), 300, 160) == 8                 # torch's padded 2-D allocation
    assert ld(torch.zeros(384 * 8, dtype=torch.uint8), 300, 160) == 8                # ... flattened
    assert ld(torch.zeros(300 * 5, dtype=torch.uint8), 300, 160) == 5
    assert ld(torch.zeros(299, 5, dtype=torch.uint8), 300, 160) is None              # too few rows
    assert ld(torch.zeros(300, 4, dtype=torch.uint8), 300, 160) is None              # too few blocks
    assert ld(torch.zeros(7, dtype=torch.uint8), 300, 160) is None
    assert ld(torch.zeros(300, 10, dtype=torch.uint8)[:, ::2], 300, 160) is None     # strided columns
    empty = torch.from_numpy(np.zeros((0, 2), np.uint8))                              # numpy hands empty arrays over with strides (0, 0)
    assert empty.stride() == (0, 0) and ld(empty, 0, 64) == 2                         # M = 0: no scale is read
    assert ld(torch.from_numpy(np.zeros((7, 0), np.uint8)), 7, 0) == 0                # K = 0
    assert ld(torch.from_numpy(np.zeros((0, 1), np.uint8)), 0, 64) is None            # still too few blocks


def test_transposed_epilogue_keyword_reaches_bias_dtype(monkeypatch):
    """The op layer on a CPU-only host with the library replaced by a recorder: transposed_epilogue ORs
    FP8MI_EPILOGUE_TRANSPOSED into bias_dtype (with or without a bias) and asks for a bias of length M."""
    import fp8_mi355x_native as N
    calls = []

    class Recorder:
        def fp8mi_scaled_mm_mxfp8(self, *args):
            calls.append(args)
            return 0

    monkeypatch.setattr(N, "DEVICE_TYPE", "cpu")                      # stand in for the HIP device
    monkeypatch.setattr(N, "_stream", lambda dev: 0)
    monkeypatch.setattr(N._l, "load", lambda: Recorder())
    M, Nn, K = 8, 24, 64
    A, B = torch.zeros(M, K // 1, dtype=torch.uint8), torch.zeros(Nn, K // 1, dtype=torch.uint8)
    sa, sb = torch.full((M, K // 32), 127, dtype=torch.uint8), torch.full((Nn, K // 32), 127, dtype=torch.uint8)
    bias_dtype = lambda: calls[-1][16]                                # (include/fp8mi.h: the 17th argument)
    mm = N.fp8_scaled_mm_mxfp8
    mm(A, B, sa, sb, bias=torch.arange(Nn, dtype=torch.bfloat16), split_k=1)
    assert bias_dtype() == L.BF16 and calls[-1][9:12] == (M, Nn, K)
    mm(A, B, sa, sb, bias=torch.arange(M, dtype=torch.bfloat16), split_k=1, transposed_epilogue=True)
    assert bias_dtype() == L.BF16 | L.EPILOGUE_TRANSPOSED
    mm(A, B, sa, sb, split_k=1, transposed_epilogue=True)
    assert bias_dtype() == L.F32 | L.EPILOGUE_TRANSPOSED and calls[-1][7] is None
    with pytest.raises(AssertionError, match=f"expected {M}"):
        mm(A, B, sa, sb, bias=torch.zeros(Nn), split_k=1, transposed_epilogue=True)
    with pytest.raises(AssertionError, match=f"expected {Nn}"):
        mm(A, B, sa, sb, bias=torch.zeros(M), split_k=1)
    assert len(calls) == 3


def test_patch_routes_by_scale_kind():
    import fp8_mps_patch as P_
    a = torch.zeros(64, 128, dtype=torch.float8_e4m3fn)
    b = torch.zeros(128, 32, dtype=torch.float8_e4m3fn)
    f1 = torch.ones(1)
    blk_a, blk_b = torch.zeros(128, 4, dtype=torch.uint8).view(E8), torch.zeros(128, 4, dtype=torch.uint8).view(E8)
    assert P_.scale_route(a, b, blk_a, blk_b) == "mxfp8"
    assert P_.scale_route(a, b, f1, f1) == "tensorwise"
    assert P_.scale_route(a, b, torch.ones(64, 1), torch.ones(1, 32)) == "tensorwise"
    assert P_.scale_route(a, b, blk_a, f1) == "original"                             # mixed kinds: torch's own op
    assert P_.scale_route(a, b, f1, blk_b) == "original"
    one = torch.tensor([127], dtype=torch.uint8).view(E8)
    assert P_.scale_route(a, b, one, f1) == "tensorwise"                             # a power of two per tensor: the route it always had


def _exact_exponent(descale: float) -> int:
    """clamp(ceil(log2(descale)), -127, 127) + 127 in exact arithmetic (descale is a float32 value, > 0 or 0 / inf)."""
    if descale == 0.0:
        return 0
    if math.isinf(descale):
        return 254
    m, e = math.frexp(descale)          # descale = m 2^e, 0.5 <= m < 1, exact
    c = e - 1 if m == 0.5 else e
    return min(max(c, -127), 127) + 127


def test_rceil_restatement_agrees_with_exact_except_just_above_powers_of_two():
    rng = np.random.default_rng(7)
    vals = list(np.float32(10.0) ** rng.uniform(-40, 38, 4000).astype(np.float32))
    for k in range(-30, 31):                                     # the adversarial blocks: 448 2^k (1 + j 2^-23)
        for j in range(0, 5):
            vals.append(np.float32(448.0 * 2.0 ** k * (1 + j * 2.0 ** -23)))
    vals += [np.float32(0.0), np.float32(np.inf), np.float32(1e-45), np.float32(3.4e38)]
    x = torch.zeros(len(vals), 32)
    x[:, 0] = torch.tensor(np.array(vals, dtype=np.float32))
    e, _ = to_mxfp8_ref(x)
    edge = 0
    for v, got in zip(vals, e[:, 0].tolist()):
        descale = float(np.float32(v) / np.float32(448.0))
        want = _exact_exponent(descale)
        if got != want:
            # only where float32 log2 rounds an exponent just above a power of two down to the power itself
            m, _ = math.frexp(descale)
            assert got == want - 1 and 0.5 < m < 0.5 * (1 + 2.0 ** -16), (v, descale, got, want)
            edge += 1
    assert edge > 0          # the documented edge exists (and is reproduced by the kernel: tests/test_gpu_mxfp8.py)
