"""float8_e5m2 on the host (no GPU): the reference's own self-checks, argument validation of the new C entry points through the built
library (every check runs before any HIP call), the patch's scale route and `take` rule on CPU tensors, and the symbol table."""
import math
import os
import re

import numpy as np
import pytest
import torch

import e5m2_ref as R
import fp8_mi355x_lib as L

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def mm(lib, M=64, N=64, K=256, lda=None, ldb=None, ldc=None, kernel=L.KERNEL_AUTO, out=L.F32, bias=L.F32, nan=L.NAN_PROPAGATE, split=0,
       sam=L.SCALE_TENSOR, sbm=L.SCALE_TENSOR, A=P, B=P, C=P, sa=P, sb=P, fa=L.FMT_E5M2, fb=L.FMT_E4M3):
    return lib.fp8mi_scaled_mm_fmt(A, B, C, sa, sb, None, None, M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                                   N if ldc is None else ldc, sam, sbm, out, bias, nan, kernel, split, None, 0, fa, fb, None)


# ---- the reference itself --------------------------------------------------------------------------------------------------

def test_decode_table_equals_the_closed_form():
    for b in range(256):
        want, got = R.closed_form_e5m2(b), float(R.DEC_E5M2[b])
        assert (math.isnan(want) and math.isnan(got)) or (want == got and math.copysign(1, want) == math.copysign(1, got)), (b, want, got)
    assert R.DEC_E5M2[0x7C] == float("inf") and R.DEC_E5M2[0xFC] == float("-inf")
    assert all(math.isnan(R.DEC_E5M2[b]) for b in (0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF))
    assert R.DEC_E5M2[0x7B] == 57344.0 and R.DEC_E5M2[0x01] == 2.0 ** -16 and R.DEC_E5M2[0x80] == 0.0 and math.copysign(1, R.DEC_E5M2[0x80]) == -1
    # an e5m2 byte is the high byte of an IEEE half
    halves = (np.arange(256, dtype=np.uint16) << 8).view(np.float16).astype(np.float64)
    assert np.array_equal(np.nan_to_num(halves, nan=1e99), np.nan_to_num(R.DEC_E5M2, nan=1e99))


def test_encode_ref_is_torchs_cast():
    x = torch.tensor([0.0, -0.0, 1.0, 57344.0, 61439.0, 61440.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -16, 2.0 ** -17, 1.5 * 2.0 ** -17])
    assert R.encode_ref(x).tolist() == [0x00, 0x80, 0x3C, 0x7B, 0x7B, 0x7C, 0x7C, 0xFC, 0x7F, 0x01, 0x00, 0x01]


def test_mm_ref_and_finite_bytes():
    rng = np.random.default_rng(0)
    for fmt in (R.FMT_E4M3, R.FMT_E5M2):
        b = R.finite_bytes(rng, (64, 256), fmt)
        assert np.isfinite(R.DEC[fmt][b]).all()
    A = np.array([[0x3C, 0x40]], dtype=np.uint8)   # e5m2 1, 2   (as e4m3: 1.5, 2)
    B = np.array([[0x38, 0x40]], dtype=np.uint8)   # e4m3 1, 2   (as e5m2: 0.5, 2)
    C, bound = R.mm_ref(A, B, [2.0], [0.5], R.FMT_E5M2, R.FMT_E4M3)
    assert C.tolist() == [[5.0]] and bound.tolist() == [[5.0]]
    C, _ = R.mm_ref(A, B, [1.0], [1.0], R.FMT_E4M3, R.FMT_E5M2)
    assert C.tolist() == [[1.5 * 0.5 + 4.0]]


def test_quantize_ref_recipe():
    q, amax, inv = R.quantize_ref(torch.tensor([0.0, 1.0, -2.0, 0.5]))
    assert amax == 2.0 and inv == np.float32(2.0 / 57344.0) and q.tolist() == [0x00, 0x77, 0xFB, 0x73]
    q, amax, inv = R.quantize_ref(torch.zeros(5))
    assert amax == 0.0 and inv == 1.0 and q.eq(0).all()


# ---- argument validation, through the built library --------------------------------------------------------------------------

def test_format_constants():
    assert (L.FMT_E4M3, L.FMT_E5M2) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    assert re.search(r"FP8MI_FMT_E4M3\s*=\s*0\s*,\s*FP8MI_FMT_E5M2\s*=\s*1", hdr)


def test_scaled_mm_fmt_validation(lib):
    for fa, fb in ((2, 0), (0, 2), (-1, 0), (1, 7)):
        assert mm(lib, fa=fa, fb=fb) == E_ENUM, (fa, fb)                      # unknown format
    for fa, fb in ((1, 0), (0, 1), (1, 1)):
        assert mm(lib, fa=fa, fb=fb, nan=L.NAN_ZERO) == E_UNSUPPORTED, (fa, fb)   # an e5m2 operand is OCP only
        assert b"PROPAGATE" in lib.fp8mi_last_error()
    # NULL / shape / enum errors as for fp8mi_scaled_mm_ws
    assert mm(lib, M=-1) == E_SHAPE and mm(lib, N=-1) == E_SHAPE and mm(lib, K=-16) == E_SHAPE
    assert mm(lib, lda=128) == E_SHAPE and mm(lib, ldb=100) == E_SHAPE and mm(lib, ldc=10) == E_SHAPE
    assert mm(lib, C=None) == E_NULL and mm(lib, sa=None) == E_NULL and mm(lib, sb=None) == E_NULL
    assert mm(lib, A=None) == E_NULL and mm(lib, B=None) == E_NULL
    assert mm(lib, out=7) == E_ENUM and mm(lib, nan=2) == E_ENUM and mm(lib, split=-1) == E_ENUM and mm(lib, sam=2) == E_ENUM
    assert mm(lib, kernel=999) == E_ENUM
    assert mm(lib, M=0) == 0 and mm(lib, N=0) == 0                              # no-ops
    # forced kernels outside their envelope, with an e5m2 operand as without
    assert mm(lib, kernel=L.KERNEL_GEMV) == E_UNSUPPORTED                      # M != 1
    assert mm(lib, kernel=L.KERNEL_GEMV_MX) == E_UNSUPPORTED                   # M > 8
    assert mm(lib, M=128, kernel=L.KERNEL_SKINNY) == E_UNSUPPORTED
    assert mm(lib, K=200, lda=208, ldb=208, kernel=L.KERNEL_GEMM_64x64) == E_UNSUPPORTED
    assert mm(lib, A=P + 8, kernel=L.KERNEL_GEMM_128x64) == E_UNSUPPORTED
    assert mm(lib, K=128, kernel=L.KERNEL_GEMM_256W) == E_UNSUPPORTED
    # both formats e4m3: the checks of fp8mi_scaled_mm_ws, NAN_ZERO allowed
    assert mm(lib, fa=0, fb=0, nan=L.NAN_ZERO, M=-1) == E_SHAPE
    assert mm(lib, fa=0, fb=0, nan=L.NAN_ZERO, kernel=999) == E_ENUM
    assert mm(lib, fa=0, fb=0, nan=L.NAN_ZERO, M=0) == 0


def test_e5m2_cast_validation(lib):
    e, d, q = lib.fp8mi_encode_e5m2, lib.fp8mi_dequant_e5m2, lib.fp8mi_quantize_e5m2
    assert e(P, L.F32, P, None, -1, None) == E_SHAPE and e(P, L.F32, P, None, 0, None) == 0
    assert e(None, L.F32, P, None, 4, None) == E_NULL and e(P, L.F32, None, None, 4, None) == E_NULL
    assert e(P, 9, P, None, 4, None) == E_ENUM
    assert d(P, P, None, -1, L.F16, None) == E_SHAPE and d(P, P, None, 0, L.F16, None) == 0
    assert d(None, P, None, 4, L.F16, None) == E_NULL and d(P, None, None, 4, L.F16, None) == E_NULL
    assert d(P, P, None, 4, 5, None) == E_ENUM
    assert q(P, L.F32, P, P, -1, None) == E_SHAPE
    assert q(P, L.F32, P, None, 4, None) == E_NULL and q(None, L.F32, P, P, 4, None) == E_NULL and q(P, L.F32, None, P, 4, None) == E_NULL
    assert q(P, 9, P, P, 4, None) == E_ENUM


def test_new_symbols_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_scaled_mm_fmt", 25), ("fp8mi_encode_e5m2", 6), ("fp8mi_dequant_e5m2", 6), ("fp8mi_quantize_e5m2", 6)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert len(L.SIGNATURES["fp8mi_scaled_mm_fmt"][1]) == len(L.SIGNATURES["fp8mi_scaled_mm_ws"][1]) + 2
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


# ---- the patch's routing, on CPU tensors -------------------------------------------------------------------------------------

def test_scale_route_of_e5m2_operands():
    import fp8_mps_patch as P_
    e4, e5, u8 = torch.float8_e4m3fn, torch.float8_e5m2, torch.uint8
    one = torch.ones(1)
    for da, db in ((e5, e4), (e4, e5), (e5, e5), (e5, u8), (u8, e5)):
        a, b = torch.zeros(64, 512, dtype=da), torch.zeros(512, 256, dtype=db)
        assert P_.scale_route(a, b, one, one) == "tensorwise", (da, db)
        assert P_.scale_route(a, b, torch.ones(64, 1), torch.ones(1, 256)) == "tensorwise", (da, db)      # rowwise
        assert P_.scale_route(a, b, None, None) == "tensorwise", (da, db)
        # blockwise-shaped float scales and E8M0 scales: the block kernels are e4m3 only -> torch's own op
        assert P_.scale_route(a, b, torch.ones(64, 4), torch.ones(4, 2)) == "original", (da, db)
        assert P_.scale_route(a, b, torch.ones(64, 4), torch.ones(4, 256)) == "original", (da, db)
        E8 = torch.float8_e8m0fnu
        blk_a = torch.full((128, 16), 127, dtype=u8).view(E8)
        blk_b = torch.full((256, 16), 127, dtype=u8).view(E8)
        assert P_.scale_route(a, b, blk_a, blk_b) == "original", (da, db)
        assert P_.scale_route(a, b, blk_a, one) == "original" and P_.scale_route(a, b, one, blk_b) == "original", (da, db)
        assert P_.scale_route(a, b, torch.full((1,), 127, dtype=u8).view(E8), one) == "original", (da, db)
    # the e4m3 routes are what they were
    a, b = torch.zeros(64, 512, dtype=e4), torch.zeros(512, 256, dtype=e4)
    assert P_.scale_route(a, b, one, one) == "tensorwise" and P_.scale_route(a, b, torch.ones(64, 4), torch.ones(4, 2)) == "blockwise"


def test_take_rule_cpu_tensors_reach_the_original():
    """On a CPU tensor nothing is taken, e5m2 or not: the call reaches the saved original with its arguments."""
    import fp8_mps_patch as P_
    seen = []

    def stub(input, other, **kw):
        seen.append((input.dtype, other.dtype, kw["out_dtype"]))
        return "original"

    saved = P_._original_scaled_mm
    P_._original_scaled_mm = stub
    try:
        for da, db in ((torch.float8_e5m2, torch.float8_e4m3fn), (torch.float8_e5m2, torch.float8_e5m2), (torch.float8_e4m3fn, torch.float8_e5m2)):
            a, b = torch.zeros(16, 32, dtype=da), torch.zeros(32, 16, dtype=db)
            assert P_._metal_scaled_mm(a, b, torch.ones(1), torch.ones(1), out_dtype=torch.bfloat16) == "original"
            assert seen[-1] == (da, db, torch.bfloat16)
    finally:
        P_._original_scaled_mm = saved
    assert len(seen) == 3


def test_to_and_copy_routing_of_e5m2_is_untouched():
    import fp8_mps_patch as P_
    f5 = torch.float8_e5m2
    assert P_._to_scenario(torch.float32, True, f5, None) == "original"
    assert P_._to_scenario(f5, True, torch.float16, None) == "original"
    assert P_._copy_scenario(f5, True, torch.float32) == "original"


def test_op_layer_takes_formats_from_dtype_or_keyword():
    import fp8_mi355x_native as N
    u = torch.zeros(4, 16, dtype=torch.uint8)
    assert N._operand_format(u, None, "A") == L.FMT_E4M3
    assert N._operand_format(u.view(torch.float8_e4m3fn), None, "A") == L.FMT_E4M3
    assert N._operand_format(u.view(torch.float8_e5m2), None, "A") == L.FMT_E5M2
    assert N._operand_format(u, L.FMT_E5M2, "A") == L.FMT_E5M2
    with pytest.raises(AssertionError):
        N._operand_format(u, 2, "A")
    with pytest.raises(AssertionError):
        N._operand_format(torch.zeros(4, 16), None, "A")
    for name in ("fp8_encode_e5m2", "fp8_dequantize_e5m2", "fp8_quantize_e5m2"):
        assert callable(getattr(N, name))


def test_fmt_loop_is_the_committed_product_loop_plus_format_codes():
    """The e5m2 instances of the one-wave-per-SIMD kernels run `gen_gemm256_loop.py --fmt` (generated at build time, not committed): it must be
    the committed product loops, instruction for instruction, with nothing but ` cbsz:%c[fw] blgp:%c[fx]` behind every MFMA and the two
    immediate operands added - and the generator's plain output stays the committed file (tests/test_abi_and_host.py checks that)."""
    import subprocess
    import sys
    gen = os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "gen", "gen_gemm256_loop.py")
    inc = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_gemm256_loop.inc")).read()
    fmt = subprocess.run([sys.executable, gen, "--fmt"], capture_output=True, text=True, check=True).stdout

    def macro(text, name):
        start = text.index(f"#define {name}() \\\n")
        return text[start:text.index("\n\n", start)].split("\n")[1:]

    for plain_name, fmt_name in (("FP8MI_GEMM256_LOOP", "FP8MI_GEMM256_LOOP_FMT"), ("FP8MI_GEMM256_LOOP_N128", "FP8MI_GEMM256_LOOP_N128_FMT")):
        plain, coded = macro(inc, plain_name), macro(fmt, fmt_name)
        assert len(plain) == len(coded) > 500
        n_mfma = sum("v_mfma_scale_f32_16x16x128_f8f6f4" in l for l in plain)
        assert n_mfma >= 64 and sum(" cbsz:%c[fw] blgp:%c[fx]" in l for l in coded) == n_mfma
        back = [l.replace(" cbsz:%c[fw] blgp:%c[fx]", "").replace(', [fw] "n"(kFW), [fx] "n"(kFX)', "") for l in coded]
        assert back == plain, [(a, b) for a, b in zip(plain, back) if a != b][:3]
    assert fmt.count("#define ") == 2 and "SCRUB" not in fmt   # no scrubbing loop for the OCP-only instances
