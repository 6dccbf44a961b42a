"""MXFP4 on the host (no GPU): argument validation of the four C entry points (every check runs before any HIP call), AUTO's
choice, the patch's routing of fp4 operands, and known answers for the recipe restatement the GPU tests use as their reference."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from mxfp4_ref import E2M1, bf16_rne, e2m1_from_bf16, pack_uint4, to_mxfp4_ref, unpack

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
MX4_TILES = {L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
             L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def mm(lib, M=64, N=64, K=256, lda=None, ldb=None, ldc=None, ld_sa=None, ld_sb=None, kernel=L.KERNEL_AUTO, out=L.F32, bias=L.F32,
       split=0, A=P, B=P, C=P, sa=P, sb=P):
    return lib.fp8mi_scaled_mm_mxfp4(A, B, C, sa, K // 32 if ld_sa is None else ld_sa, sb, K // 32 if ld_sb is None else ld_sb, None, None,
                                     M, N, K, K // 2 if lda is None else lda, K // 2 if ldb is None else ldb, N if ldc is None else ldc,
                                     out, bias, kernel, split, None, 0, None)


def test_scaled_mm_mxfp4_validation(lib):
    assert mm(lib, K=100) == E_SHAPE                     # K % 32
    assert mm(lib, K=48) == E_SHAPE
    assert mm(lib, K=-32) == E_SHAPE
    assert mm(lib, lda=127) == E_SHAPE                   # lda < K/2 bytes
    assert mm(lib, ldb=127) == E_SHAPE
    assert mm(lib, ld_sa=7) == E_SHAPE                   # ld_sa < K/32
    assert mm(lib, ld_sb=7) == E_SHAPE
    assert mm(lib, ldc=10) == E_SHAPE
    assert mm(lib, C=None) == E_NULL
    assert mm(lib, sb=None) == E_NULL
    assert mm(lib, out=7) == E_ENUM
    assert mm(lib, split=-1) == E_ENUM
    assert mm(lib, kernel=999) == E_ENUM
    for k in (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_SKINNY, L.KERNEL_GEMM_256, L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W):
        assert mm(lib, kernel=k) == E_UNSUPPORTED, k      # no MXFP4 form
    # a forced ring tile with scales it cannot read in 4-byte pieces, or operands off 16 bytes
    assert mm(lib, K=160, ld_sa=5, ld_sb=8, kernel=L.KERNEL_GEMM_128x64) == E_UNSUPPORTED
    assert mm(lib, sa=P + 2, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, A=P + 8, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, K=288, lda=152, ldb=152, kernel=L.KERNEL_GEMM_32x32) == E_UNSUPPORTED   # row stride 152 bytes: not 16-aligned
    assert mm(lib, M=0) == 0 and mm(lib, N=0) == 0          # no-ops


def test_quantize_dequant_mxfp4_validation(lib):
    q = lib.fp8mi_quantize_mxfp4
    assert q(P, L.F32, 4, 48, 48, P, 24, P, 2, None) == E_SHAPE      # cols % 32
    assert q(P, L.F32, 4, 64, 32, P, 32, P, 2, None) == E_SHAPE      # ld_in
    assert q(P, L.F32, 4, 64, 64, P, 31, P, 2, None) == E_SHAPE      # ld_out < cols/2 bytes
    assert q(P, L.F32, 4, 64, 64, P, 32, P, 1, None) == E_SHAPE      # ld_s
    assert q(P, 9, 4, 64, 64, P, 32, P, 2, None) == E_ENUM
    assert q(None, L.F32, 4, 64, 64, P, 32, P, 2, None) == E_NULL
    assert q(P, L.F32, 0, 64, 64, P, 32, P, 2, None) == 0
    d = lib.fp8mi_dequant_mxfp4
    assert d(P, 4, 64, 31, P, 2, P, L.F32, None) == E_SHAPE          # ld_in < cols/2 bytes
    assert d(P, 4, 64, 32, P, 1, P, L.F32, None) == E_SHAPE          # ld_s < ceil(cols / 32)
    assert d(P, 4, 63, 32, P, 2, P, L.F32, None) == E_SHAPE          # odd cols
    assert d(P, 4, 64, 32, P, 2, P, 9, None) == E_ENUM
    assert d(P, 4, 64, 32, None, 2, P, L.F32, None) == E_NULL
    assert d(P, -1, 64, 32, P, 2, P, L.F32, None) == E_SHAPE
    assert d(P, 0, 64, 32, P, 2, P, L.F32, None) == 0


def test_auto_choice_is_an_fp4_kernel_or_generic(lib):
    for M in (1, 2, 7, 33, 64, 128, 300, 512, 4096):
        for N in (1, 64, 200, 3072, 4096):
            for K in (32, 96, 160, 4096, 4128, 12288, 14336):
                got = lib.fp8mi_choose_kernel_mxfp4(M, N, K, K // 2, K // 2, N, L.BF16, 1, 0)
                aligned = (K // 2) % 16 == 0
                assert got in (MX4_TILES if aligned else {L.KERNEL_GENERIC}), (M, N, K, got)
    assert lib.fp8mi_choose_kernel_mxfp4(64, 64, 0, 0, 0, 64, L.F32, 0, 0) == L.KERNEL_GENERIC
    assert lib.fp8mi_choose_kernel_mxfp4(64, 64, 96, 56, 56, 64, L.F32, 0, 0) == L.KERNEL_GENERIC   # unaligned row stride
    assert lib.fp8mi_choose_kernel_mxfp4(64, 64, 100, 50, 50, 64, L.F32, 0, 0) < 0


def test_every_e2m1_code_decodes_and_reencodes():
    vals = torch.tensor(E2M1, dtype=torch.float32)
    codes = e2m1_from_bf16(bf16_rne(vals))     # -0.0 keeps its sign bit: code 8
    assert torch.equal(codes, torch.arange(16, dtype=torch.uint8))
    assert E2M1[7] == 6.0 and E2M1[15] == -6.0 and E2M1[1] == 0.5


def test_rne_ties_saturation_and_double_rounding():
    enc = lambda v: e2m1_from_bf16(bf16_rne(torch.tensor([v], dtype=torch.float32)))[0].item()
    assert enc(0.25) == 0x0           # tie 0 / 0.5 -> even (0)
    assert enc(0.75) == 0x2           # tie 0.5 / 1.0 -> even (1.0)
    assert enc(1.25) == 0x2           # tie 1.0 / 1.5 -> 1.0
    assert enc(1.75) == 0x4           # tie 1.5 / 2.0 -> 2.0
    assert enc(2.5) == 0x4            # tie 2 / 3 -> 2
    assert enc(3.5) == 0x6            # tie 3 / 4 -> 4
    assert enc(5.0) == 0x6            # tie 4 / 6 -> 4
    assert enc(5.5) == 0x7
    assert enc(6.0) == 0x7 and enc(100.0) == 0x7 and enc(-1e30) == 0xF   # saturating
    assert enc(-0.5) == 0x9 and enc(-0.0) == 0x8
    assert enc(0.2578125) == 0x1      # above the tie (a bf16 value)
    # the recipe rounds to bfloat16 first: 2.5 + 2^-20 is bf16 2.5, which ties to 2.0; one rounding would give 3.0
    assert enc(2.5 + 2.0 ** -20) == 0x4
    assert enc(2.5 + 2.0 ** -6) == 0x5   # representable in bf16: above the tie
    assert enc(float("nan")) == 0xC     # bf16 0xFFFF through the integer path


def test_bf16_rounding_agrees_with_torch():
    g = torch.Generator().manual_seed(3)
    y = torch.cat([torch.randn(4096, generator=g) * 3, torch.tensor([2.5 + 2.0 ** -20, 2.0 ** -130, -0.0, 6.0, 1.00390625, 1.01171875])])
    want = y.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(bf16_rne(y), want)


def test_nibble_order_and_a_known_block():
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 31] = 1.0, -6.0, 0.5, 3.0       # amax 6: scale 2^0 (0x7F)
    s, q = to_mxfp4_ref(x)
    assert s.tolist() == [[127]]
    assert q.shape == (1, 16)
    assert q[0, 0].item() == 0xF2     # element 0 (1.0 = 0x2) in the low nibble, element 1 (-6 = 0xF) in the high one
    assert q[0, 1].item() == 0x01     # 0.5, then 0
    assert q[0, 15].item() == 0x50    # element 31 (3.0 = 0x5) high
    assert np.array_equal(unpack(q.numpy())[0, :3], [0x2, 0xF, 0x1])
    assert torch.equal(pack_uint4(torch.tensor([[1, 2, 3, 4]], dtype=torch.uint8)), torch.tensor([[0x21, 0x43]], dtype=torch.uint8))
    # amax 12: scale 2^1, the block divided by 2
    x[0, 5] = 12.0
    s, q = to_mxfp4_ref(x)
    assert s.tolist() == [[128]] and q[0, 2].item() == 0x70      # 12 / 2 = 6.0 in the high nibble of byte 2
    # a NaN block: scale 0xFF
    x[0, 7] = float("nan")
    s, _ = to_mxfp4_ref(x)
    assert s.tolist() == [[255]]


FP4 = torch.float4_e2m1fn_x2
E8 = torch.float8_e8m0fnu


def test_transposed_epilogue_keyword_reaches_bias_dtype(monkeypatch):
    """The op layer on a CPU-only host with the library replaced by a recorder: transposed_epilogue ORs
    FP8MI_EPILOGUE_TRANSPOSED into bias_dtype (with or without a bias) and asks for a bias of length M."""
    import fp8_mi355x_native as N
    calls = []

    class Recorder:
        def fp8mi_scaled_mm_mxfp4(self, *args):
            calls.append(args)
            return 0

    monkeypatch.setattr(N, "DEVICE_TYPE", "cpu")                      # stand in for the HIP device
    monkeypatch.setattr(N, "_stream", lambda dev: 0)
    monkeypatch.setattr(N._l, "load", lambda: Recorder())
    M, Nn, K = 8, 24, 64
    A, B = torch.zeros(M, K // 2, dtype=torch.uint8), torch.zeros(Nn, K // 2, dtype=torch.uint8)
    sa, sb = torch.full((M, K // 32), 127, dtype=torch.uint8), torch.full((Nn, K // 32), 127, dtype=torch.uint8)
    bias_dtype = lambda: calls[-1][16]                                # (include/fp8mi.h: the 17th argument)
    mm = N.fp8_scaled_mm_mxfp4
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


def test_patch_routes_fp4_operands_by_scale_kind():
    import fp8_mps_patch as P_
    a = torch.zeros(64, 64, dtype=torch.uint8).view(FP4)
    b = torch.zeros(32, 64, dtype=torch.uint8).view(FP4).t()           # (K/2, N), column-major
    blk_a, blk_b = torch.zeros(128, 4, dtype=torch.uint8).view(E8), torch.zeros(128, 4, dtype=torch.uint8).view(E8)
    f1 = torch.ones(1)
    assert P_.scale_route(a, b, blk_a, blk_b) == "mxfp4"
    assert P_.scale_route(a, b, f1, f1) == "original"                # fp4 with float scales: torch's own op, as before
    assert P_.scale_route(a, b, blk_a, f1) == "original"
    e4 = torch.zeros(64, 128, dtype=torch.float8_e4m3fn)
    assert P_.scale_route(e4, torch.zeros(128, 32, dtype=torch.float8_e4m3fn), blk_a, blk_b) == "mxfp8"   # e4m3 keeps its route
    assert P_.scale_route(e4, b, blk_a, blk_b) == "original"          # mixed e4m3 x e2m1: not served here


def test_patch_sends_fp4_with_float_scales_to_the_original_op(monkeypatch):
    """The patched _scaled_mm on a HIP-device fp4 call with float scales calls torch's original op (recorded here), and with
    E8M0 scales the MXFP4 op (recorded in place of the kernel)."""
    import fp8_mps_patch as P_
    calls = []
    monkeypatch.setattr(P_, "_original_scaled_mm", lambda *a, **k: calls.append("original") or "orig")

    class FakeNative:
        def fp8_scaled_mm_mxfp4(self, *a, **k):
            calls.append("mxfp4")
            return "mx4"

    monkeypatch.setattr(P_, "_native", lambda: FakeNative())
    monkeypatch.setattr(P_, "_DEV", "cpu")                            # stand in for the HIP device on a CPU-only host
    a = torch.zeros(64, 64, dtype=torch.uint8).view(FP4)
    b = torch.zeros(32, 64, dtype=torch.uint8).view(FP4).t()
    blk = torch.zeros(128, 4, dtype=torch.uint8).view(E8)
    assert P_._metal_scaled_mm(a, b, scale_a=torch.ones(1), scale_b=torch.ones(1)) == "orig"
    assert P_._metal_scaled_mm(a, b, scale_a=blk, scale_b=blk, out_dtype=torch.bfloat16) == "mx4"
    assert calls == ["original", "mxfp4"]
