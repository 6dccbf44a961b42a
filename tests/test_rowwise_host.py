"""Per-row dynamic quantisation on the host (no GPU): argument validation of fp8mi_quantize_rowwise / fp8mi_dequant_rowwise through the
built library (every check runs before any HIP call), the reference of tests/rowwise_ref.py against the oracle and against torch's CPU
casts, and the numerical case for the recipe measured on the reference alone."""
import os
import re

import numpy as np
import pytest
import torch

import e5m2_ref
import fp8_mi355x_lib as L
import rowwise_ref as R

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4, E5 = L.FMT_E4M3, L.FMT_E5M2


@pytest.fixture(scope="module")
def lib():
    return L.load()


def quant(lib, rows=4, cols=64, ld_in=None, ld_out=None, inp=P, out=P, inv=P, amax=None, dtype=L.BF16, fmt=E4, mode=L.ENC_REFERENCE):
    return lib.fp8mi_quantize_rowwise(inp, dtype, rows, cols, cols if ld_in is None else ld_in, out, cols if ld_out is None else ld_out, inv, amax,
                                      fmt, mode, None)


def dequant(lib, rows=4, cols=64, ld_in=None, inp=P, scales=P, out=P, fmt=E4, dtype=L.F32):
    return lib.fp8mi_dequant_rowwise(inp, rows, cols, cols if ld_in is None else ld_in, scales, fmt, out, dtype, None)


# ---- argument validation, through the built library --------------------------------------------------------------------------

def test_quantize_rowwise_argument_errors_without_gpu(lib):
    assert quant(lib, inp=None) == E_NULL and b"NULL" in lib.fp8mi_last_error()
    assert quant(lib, out=None) == E_NULL and quant(lib, inv=None) == E_NULL
    assert quant(lib, cols=0, inp=None, out=None, inv=None) == E_NULL            # the scales are still written for empty rows
    assert quant(lib, rows=-1) == E_SHAPE and quant(lib, cols=-1, ld_in=0, ld_out=0) == E_SHAPE
    assert quant(lib, ld_in=63) == E_SHAPE and b"leading dimension" in lib.fp8mi_last_error()
    assert quant(lib, ld_out=63) == E_SHAPE
    assert quant(lib, dtype=3) == E_ENUM and quant(lib, dtype=-1) == E_ENUM
    assert quant(lib, fmt=2) == E_ENUM and quant(lib, fmt=-1) == E_ENUM
    assert quant(lib, mode=2) == E_ENUM and quant(lib, mode=-1) == E_ENUM and quant(lib, fmt=E5, mode=7) == E_ENUM
    assert quant(lib, fmt=E5, mode=L.ENC_REFERENCE) == E_UNSUPPORTED and b"OCP" in lib.fp8mi_last_error()
    # rows == 0 is a no-op that accepts NULL pointers, for both formats - but not bad enums or shapes
    assert quant(lib, rows=0, inp=None, out=None, inv=None) == 0
    assert quant(lib, rows=0, cols=0, inp=None, out=None, inv=None, fmt=E5, mode=L.ENC_RNE) == 0
    assert quant(lib, rows=0, dtype=9) == E_ENUM and quant(lib, rows=0, ld_in=1) == E_SHAPE
    assert quant(lib, rows=0, fmt=E5, mode=L.ENC_REFERENCE) == E_UNSUPPORTED


def test_dequant_rowwise_argument_errors_without_gpu(lib):
    assert dequant(lib, inp=None) == E_NULL and dequant(lib, scales=None) == E_NULL and dequant(lib, out=None) == E_NULL
    assert dequant(lib, rows=-1) == E_SHAPE and dequant(lib, cols=-2, ld_in=0) == E_SHAPE and dequant(lib, ld_in=10) == E_SHAPE
    assert dequant(lib, fmt=2) == E_ENUM and dequant(lib, dtype=3) == E_ENUM
    assert dequant(lib, rows=0, inp=None, scales=None, out=None) == 0 and dequant(lib, cols=0, inp=None, scales=None, out=None) == 0


def test_new_symbols_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_quantize_rowwise", 12), ("fp8mi_dequant_rowwise", 9)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_op_layer_exposes_the_rowwise_ops():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_quantize_rowwise", "fp8_dequantize_rowwise", "fp8_linear_rowwise"):
        assert callable(getattr(N, name)), name
    assert callable(alias.fp8_quantize) and callable(N.fp8_linear)
    # the row view: a column slice is used in place, anything else is flattened
    w = torch.zeros(6, 40)
    v, rows, cols, ld = N._rows_view(w[:, 8:24])
    assert v.data_ptr() == w[:, 8:24].data_ptr() and (rows, cols, ld) == (6, 16, 40)
    v, rows, cols, ld = N._rows_view(torch.zeros(2, 3, 16))
    assert (rows, cols, ld) == (6, 16, 16) and v.is_contiguous()
    v, rows, cols, ld = N._rows_view(w.t())
    assert (rows, cols, ld) == (40, 6, 6) and v.is_contiguous()
    v, rows, cols, ld = N._rows_view(torch.zeros(16))
    assert (rows, cols, ld) == (1, 16, 16)


# ---- the reference against the oracle and torch --------------------------------------------------------------------------------

def _data(rng, rows, cols):
    return (rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-12, 12, size=(rows, 1)))).astype(np.float32)


def test_ref_rows_equal_the_oracles_per_tensor_quantize(oracle):
    rng = np.random.default_rng(1)
    x = _data(rng, 19, 333)
    x[4] = 0.0
    q, amax, inv = R.quantize_rowwise_ref(x, E4, R.ENC_REFERENCE)
    assert q.shape == x.shape and q.dtype == np.uint8 and amax.dtype == np.float32 and inv.dtype == np.float32
    for r in range(x.shape[0]):
        wq, winv = oracle.quantize(x[r])
        assert np.array_equal(q[r], wq), r
        assert inv[r] == winv and amax[r] == np.max(np.abs(x[r])), r
    assert inv[4] == 1.0 and amax[4] == 0.0 and not q[4].any()
    # 16-bit inputs are widened first
    xb = torch.from_numpy(x).to(torch.bfloat16)
    qb, _, invb = R.quantize_rowwise_ref(xb, E4, R.ENC_REFERENCE)
    for r in (0, 7, 18):
        wq, winv = oracle.quantize(xb[r].float().numpy())
        assert np.array_equal(qb[r], wq) and invb[r] == winv


def test_ref_rne_bytes_are_torchs_casts():
    rng = np.random.default_rng(2)
    x = _data(rng, 23, 257)
    q, amax, inv = R.quantize_rowwise_ref(x, E4, R.ENC_RNE)
    scale = np.array([np.float32(448.0 / float(a)) for a in amax], np.float32)
    want = (torch.from_numpy(x) * torch.from_numpy(scale)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(q, want)
    assert np.array_equal(inv, np.array([np.float32(1.0 / (448.0 / float(a))) for a in amax], np.float32))
    q5, amax5, inv5 = R.quantize_rowwise_ref(x, E5, R.ENC_RNE)
    for r in range(x.shape[0]):
        wq, wamax, winv = e5m2_ref.quantize_ref(torch.from_numpy(x[r]))
        assert np.array_equal(q5[r], wq.numpy()) and amax5[r] == wamax and inv5[r] == winv, r


def test_ref_ignores_nans_in_the_amax_and_handles_empty_rows():
    x = np.array([[1.0, np.nan, -2.0, 0.5], [np.nan, np.nan, np.nan, np.nan]], np.float32)
    q, amax, inv = R.quantize_rowwise_ref(x, E4, R.ENC_RNE)
    assert amax.tolist() == [2.0, 0.0] and inv[1] == 1.0 and inv[0] == np.float32(1.0 / 224.0)
    assert q[0].tolist() == [0x76, 0x7F, 0xFE, 0x6E] and (q[1] & 0x7F).tolist() == [0x7F] * 4
    q, amax, inv = R.quantize_rowwise_ref(np.zeros((3, 0), np.float32), E5, R.ENC_RNE)
    assert q.shape == (3, 0) and amax.tolist() == [0, 0, 0] and inv.tolist() == [1, 1, 1]
    d = R.dequant_rowwise_ref(np.array([[0x38, 0x7F], [0xC0, 0x00]], np.uint8), [2.0, 0.5], E4, torch.float16)
    assert d.dtype == torch.float16 and d[0, 0] == 2.0 and torch.isnan(d[0, 1]) and d[1, 0] == -1.0


# ---- why the recipe exists -------------------------------------------------------------------------------------------------------

def test_rowwise_keeps_small_rows_that_per_tensor_scaling_loses(oracle):
    """Rows whose magnitudes differ by up to 2^24 (row r of N(0,1) times 2^-(r % 25)): with one scale per row every row keeps e4m3's
    relative precision; with one scale for the tensor the rows 2^-18 and below fall under the format's range and are lost."""
    x = np.random.default_rng(20261017).standard_normal((256, 1024))
    mult = np.exp2(-(np.arange(256) % 25).astype(np.float64))
    x = (x * mult[:, None]).astype(np.float32)
    for mode in (R.ENC_REFERENCE, R.ENC_RNE):
        q, _, inv = R.quantize_rowwise_ref(x, E4, mode)
        back = oracle.decode(q) * inv[:, None]
        rel = R.rel_rms_rows(back, x)
        print(f"[rowwise] mode {mode}: worst row rel rms {rel.max():.4f}")
        assert np.all(rel < 0.05), float(rel.max())
    qt, invt = oracle.quantize(x)
    rel_t = R.rel_rms_rows(oracle.decode(qt) * invt, x)
    small = mult <= 2.0 ** -18
    print(f"[rowwise] per tensor: best small row rel rms {rel_t[small].min():.4f}")
    assert small.sum() >= 60 and np.all(rel_t[small] > 0.5), float(rel_t[small].min())
