"""Blockwise (1x128 / 128x128 fp32 scales) on the host (no GPU): argument validation of the four C entry points (every check runs
before any HIP call), the AUTO choice, the patch's scale route, and the torch restatement of the quantizer the GPU tests use."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from blockwise_ref import mm_ref, quantize_blockwise_ref

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
RING = {L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_32x32,
        L.KERNEL_GEMM_128D}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def mm(lib, M=64, N=64, K=256, lda=None, ldb=None, ldc=None, sa_sr=2, sa_sk=1, ba=1, sb_sr=2, sb_sk=1, bb=128, kernel=L.KERNEL_AUTO,
       out=L.F32, bias=L.F32, nan=L.NAN_ZERO, split=0, A=P, B=P, C=P, sa=P, sb=P):
    return lib.fp8mi_scaled_mm_blockwise(A, B, C, sa, sa_sr, sa_sk, ba, sb, sb_sr, sb_sk, bb, None, None, M, N, K,
                                         K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc,
                                         out, bias, nan, kernel, split, None, 0, None)


def test_blockwise_constants():
    assert (L.BLOCK_1, L.BLOCK_128) == (1, 128)


def test_scaled_mm_blockwise_validation(lib):
    assert mm(lib, M=-1) == E_SHAPE and mm(lib, N=-1) == E_SHAPE and mm(lib, K=-128) == E_SHAPE
    for kw in ({"sa_sr": -1}, {"sa_sk": -1}, {"sb_sr": -1}, {"sb_sk": -1}):
        assert mm(lib, **kw) == E_SHAPE, kw                 # negative scale strides
    for ba, bb in ((2, 128), (1, 64), (0, 1), (128, 256)):
        assert mm(lib, ba=ba, bb=bb) == E_ENUM, (ba, bb)    # blocks other than 1 and 128
    assert mm(lib, lda=128) == E_SHAPE and mm(lib, ldb=100) == E_SHAPE and mm(lib, ldc=10) == E_SHAPE
    assert mm(lib, C=None) == E_NULL
    for kw in ({"A": None}, {"B": None}, {"sa": None}, {"sb": None}):
        assert mm(lib, **kw) == E_NULL, kw
    assert mm(lib, K=0, lda=0, ldb=0, sa=None, sb=None, kernel=999) == E_ENUM   # (K = 0 takes NULL scales; the kernel id is still checked)
    assert mm(lib, out=7) == E_ENUM and mm(lib, nan=2) == E_ENUM and mm(lib, split=-1) == E_ENUM
    assert mm(lib, kernel=999) == E_ENUM
    for k in (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_SKINNY, L.KERNEL_GEMM_256, L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W):
        assert mm(lib, kernel=k) == E_UNSUPPORTED, k       # no blockwise form
    # forced ring tiles on operands they cannot stage, and on scale pointers that are not 4-byte aligned
    assert mm(lib, K=200, lda=208, ldb=208, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED     # K % 16
    assert mm(lib, A=P + 8, kernel=L.KERNEL_GEMM_128x64) == E_UNSUPPORTED
    assert mm(lib, lda=264, kernel=L.KERNEL_GEMM_32x32) == E_UNSUPPORTED                   # lda % 16
    assert mm(lib, sa=P + 2, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, sb=P + 1, kernel=L.KERNEL_GEMM_128) == E_UNSUPPORTED
    assert mm(lib, K=0, lda=0, ldb=0, sa=None, sb=None, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED   # the ring tiles need K > 0
    assert mm(lib, sa_sk=1 << 40, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED             # a scale extent past 32-bit offsets
    assert mm(lib, M=0) == 0 and mm(lib, N=0) == 0          # no-ops


def test_quantize_dequant_blockwise_validation(lib):
    q = lib.fp8mi_quantize_blockwise
    assert q(P, L.F32, -1, 256, 256, 1, P, 256, P, 2, 1, None) == E_SHAPE
    assert q(P, L.F32, 4, 256, 128, 1, P, 256, P, 2, 1, None) == E_SHAPE    # ld_in
    assert q(P, L.F32, 4, 256, 256, 1, P, 200, P, 2, 1, None) == E_SHAPE    # ld_out
    assert q(P, L.F32, 4, 256, 256, 1, P, 256, P, -2, 1, None) == E_SHAPE   # negative scale stride
    assert q(P, L.F32, 4, 256, 256, 2, P, 256, P, 2, 1, None) == E_ENUM     # block_rows
    assert q(P, 9, 4, 256, 256, 1, P, 256, P, 2, 1, None) == E_ENUM
    assert q(None, L.F32, 4, 256, 256, 1, P, 256, P, 2, 1, None) == E_NULL
    assert q(P, L.F32, 4, 256, 256, 128, P, 256, None, 2, 1, None) == E_NULL
    assert q(P, L.F32, 0, 256, 256, 1, P, 256, P, 2, 1, None) == 0
    d = lib.fp8mi_dequant_blockwise
    assert d(P, 4, 256, 128, 1, P, 2, 1, P, L.F32, None) == E_SHAPE         # ld_in
    assert d(P, 4, 256, 256, 1, P, 2, -1, P, L.F32, None) == E_SHAPE
    assert d(P, -1, 256, 256, 1, P, 2, 1, P, L.F32, None) == E_SHAPE
    assert d(P, 4, 256, 256, 3, P, 2, 1, P, L.F32, None) == E_ENUM
    assert d(P, 4, 256, 256, 1, P, 2, 1, P, 9, None) == E_ENUM
    assert d(P, 4, 256, 256, 1, None, 2, 1, P, L.F32, None) == E_NULL
    assert d(P, 4, 0, 256, 1, P, 2, 1, P, L.F32, None) == 0


def test_auto_choice_is_a_blockwise_ring_tile(lib):
    for M, N, K in ((1, 4096, 4096), (64, 4096, 14336), (512, 4096, 4096), (4096, 3072, 12288), (300, 200, 400)):
        for ba, bb in ((1, 128), (1, 1), (128, 1), (128, 128)):
            assert lib.fp8mi_choose_kernel_blockwise(M, N, K, K, K, N, L.BF16, ba, bb, 1, 0) in RING, (M, N, K, ba, bb)
    assert lib.fp8mi_choose_kernel_blockwise(64, 64, 0, 0, 0, 64, L.F32, 1, 128, 0, 0) == L.KERNEL_GENERIC       # K = 0
    assert lib.fp8mi_choose_kernel_blockwise(64, 64, 100, 100, 100, 64, L.F32, 1, 128, 0, 0) == L.KERNEL_GENERIC  # K % 16
    assert lib.fp8mi_choose_kernel_blockwise(64, 64, 128, 136, 128, 64, L.F32, 1, 128, 0, 0) == L.KERNEL_GENERIC  # lda % 16
    assert lib.fp8mi_choose_kernel_blockwise(64, 64, 128, 128, 128, 64, L.F32, 2, 128, 0, 0) < 0
    assert lib.fp8mi_choose_kernel_blockwise(-1, 64, 128, 128, 128, 64, L.F32, 1, 128, 0, 0) < 0


def test_patch_routes_blockwise_scales():
    import fp8_mps_patch as P_
    a = torch.zeros(64, 512, dtype=torch.float8_e4m3fn)
    b = torch.zeros(512, 256, dtype=torch.float8_e4m3fn)
    assert P_.scale_route(a, b, torch.ones(64, 4), torch.ones(4, 2)) == "blockwise"      # 1x128 x 128x128
    assert P_.scale_route(a, b, torch.ones(64, 4), torch.ones(4, 256)) == "blockwise"    # 1x128 x 1x128
    assert P_.scale_route(a, b, torch.ones(64, 4).t().contiguous().t(), torch.ones(2, 4).t()) == "blockwise"   # any strides
    assert P_.scale_route(a, b, torch.ones(1), torch.ones(1)) == "tensorwise"
    assert P_.scale_route(a, b, torch.ones(64, 1), torch.ones(1, 256)) == "tensorwise"   # rowwise
    assert P_.scale_route(a, b, torch.ones(64, 4, dtype=torch.float64), torch.ones(4, 2)) == "tensorwise"   # fp32 only: unchanged route
    assert P_.scale_route(a, b, torch.ones(64, 3), torch.ones(3, 2)) == "tensorwise"     # not a blockwise shape: unchanged route
    # K <= 128: (M, 1) / (1, N) are rowwise AND 1x128 x 1x128 shapes - matched as tensorwise first (the same math)
    a1 = torch.zeros(64, 128, dtype=torch.float8_e4m3fn)
    b1 = torch.zeros(128, 32, dtype=torch.float8_e4m3fn)
    assert P_.scale_route(a1, b1, torch.ones(64, 1), torch.ones(1, 32)) == "tensorwise"
    b2 = torch.zeros(128, 256, dtype=torch.float8_e4m3fn)
    assert P_.scale_route(a1, b2, torch.ones(64, 1), torch.ones(1, 2)) == "blockwise"    # rowwise a, 128x128 b: only blockwise reads it
    # the E8M0 routes are unchanged
    E8 = torch.float8_e8m0fnu
    blk = torch.zeros(128, 4, dtype=torch.uint8).view(E8)
    assert P_.scale_route(a1, b1, blk, blk) == "mxfp8"
    assert P_.scale_route(a1, b1, blk, torch.ones(1)) == "original"


def test_quantize_ref_recipe():
    x = torch.tensor([[0.0] * 127 + [448.0 * 3], [1.0] * 128])
    q, s = quantize_blockwise_ref(x, 1)
    assert s.tolist() == [[3.0], [float(np.float32(1.0) / np.float32(448.0))]]
    assert q[0, 127].item() == 0x7E and q[0, 0].item() == 0 and q[1, 0].item() == 0x7E
    q, s = quantize_blockwise_ref(torch.zeros(3, 130), 128)
    assert s.shape == (1, 2) and s.tolist() == [[1.0, 1.0]] and q.eq(0).all()
    x = torch.ones(2, 256)
    x[0, 5] = float("nan")
    x[1, 200] = float("inf")
    q, s = quantize_blockwise_ref(x, 1)
    assert torch.isnan(s[0, 0]) and s[0, 1] == 1.0 / 448.0 and s[1, 1] == float("inf")
    assert q[0, :128].eq(0x7F).all() and q[1, 200] == 0x7F and q[1, 128] == 0 and q[1, 0] == 0x7E
    # an amax whose quotient amax / 448 underflows to 0 in fp32 takes the all-zero block's scale of 1: finite input never yields
    # NaN bytes (with a scale of 0 the nonzero elements were +-448 and the zeros 0 / 0 = 0x7F)
    for amax in (1e-44, 1.4e-45):
        x = torch.zeros(130, 300)
        x[0, 3], x[5, 129], x[129, 299] = amax, -amax, amax
        assert (x.abs().max() / 448.0).item() == 0.0
        for block_rows in (1, 128):
            q, s = quantize_blockwise_ref(x, block_rows)
            assert s.eq(1.0).all() and q.eq(0).sum() == q.numel() - 1 and not (q & 0x7F).eq(0x7F).any()
            assert q[0, 3] == 0 and q[5, 129] == 0x80 and q[129, 299] == 0
    # one step above: a subnormal scale is kept, and the block's amax still quantizes to +-448
    x = torch.zeros(2, 128)
    x[0, 0], x[0, 1], x[1, 7] = 2.0 ** -140, -2.0 ** -141, -2.0 ** -126 * 448
    q, s = quantize_blockwise_ref(x, 1)
    assert s[0, 0].item() == 2.0 ** -149 and s[1, 0].item() == 2.0 ** -126
    assert q[0, 0] == 0x7E and q[0, 1] == 0xF8 and q[1, 7] == 0xFE and q[1, 0] == 0


def test_oracle_folds_scales_per_block():
    rng = np.random.default_rng(0)
    A = rng.integers(0, 0x70, size=(3, 300), dtype=np.uint8)
    B = rng.integers(0, 0x70, size=(5, 300), dtype=np.uint8)
    sa = np.full((3, 3), 2.0, np.float32)
    sb = np.full((1, 3), 0.5, np.float32)
    C, bound = mm_ref(A, B, sa, sb, 1, 128)
    from mxfp8_ref import DEC_ZERO
    assert np.allclose(C, DEC_ZERO[A] @ DEC_ZERO[B].T) and np.all(bound >= np.abs(C))
