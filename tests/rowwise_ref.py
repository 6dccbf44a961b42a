"""Host-side reference for the per-row quantisation tests (not a test module), written from the formulas of include/fp8mi.h
(fp8mi_quantize_rowwise / fp8mi_dequant_rowwise) with numpy and torch CPU, on top of the oracle's encoders:

  row_scales            amax -> (scale, inverse scale): FMAX / amax and 1 / (FMAX / amax) in double, each rounded to float32; 1 for amax == 0
  quantize_rowwise_ref  (bytes, amax, inv): NaN-ignoring amax per row, float32(x) * scale in float32, then oracle.encode (reference mode),
                        oracle.encode_torch_rne (RNE) or torch CPU's float8_e5m2 cast of the value clamped to +-57344
  dequant_rowwise_ref   OCP decode (torch CPU's tables) times the row's scale in float32, then torch's cast to the output type
"""
import numpy as np
import torch

import fp8_oracle as oracle
from e5m2_ref import DEC, FMT_E4M3, FMT_E5M2, encode_ref as encode_e5m2_ref

ENC_REFERENCE, ENC_RNE = 0, 1
FMAX = {FMT_E4M3: 448.0, FMT_E5M2: 57344.0}


def as_f32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(torch.float32).numpy()
    return np.asarray(x, dtype=np.float32)


def row_scales(amax, fmt):
    """amax float32[rows] -> (scale float32[rows], inv float32[rows]); the divisions in double, as Python float arithmetic."""
    amax = np.asarray(amax, dtype=np.float32)
    scale = np.ones(amax.shape, np.float32)
    inv = np.ones(amax.shape, np.float32)
    pos = amax > 0
    with np.errstate(divide="ignore", over="ignore"):
        s = np.float64(FMAX[fmt]) / amax[pos].astype(np.float64)
        scale[pos] = s.astype(np.float32)
        inv[pos] = (np.float64(1.0) / s).astype(np.float32)
    return scale, inv


def quantize_rowwise_ref(x, fmt=FMT_E4M3, mode=ENC_REFERENCE):
    """x (rows, cols) f32 / f16 / bf16 (torch or numpy) -> (bytes uint8 (rows, cols), amax float32[rows], inv float32[rows])."""
    xf = as_f32(x)
    assert xf.ndim == 2
    rows, cols = xf.shape
    a = np.abs(xf)
    a = np.where(np.isnan(a), np.float32(0), a)
    amax = a.max(axis=1).astype(np.float32) if cols else np.zeros(rows, np.float32)
    scale, inv = row_scales(amax, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (xf * scale[:, None]).astype(np.float32)
    # A NaN that the multiply itself generates (inf * 0: a row whose amax is inf has scale 0) has no sign defined by IEEE 754, and the RNE /
    # e5m2 encodings copy that bit.  x86 and gfx950 both generate the quiet NaN with the sign bit SET (0xFFC00000), which is what
    # fp8mi_quantize stores for such input (tests/test_gpu_rowwise.py compares with it row by row); the reference pins that pattern so
    # that it does not depend on the host it runs on.  A NaN INPUT keeps its own sign through the multiply.
    y = np.where(np.isnan(y) & ~np.isnan(xf), np.array([0xFFC00000], np.uint32).view(np.float32)[0], y).astype(np.float32)
    if fmt == FMT_E5M2:
        assert mode == ENC_RNE, "e5m2 is OCP only"
        q = encode_e5m2_ref(torch.clamp(torch.from_numpy(y), min=-57344.0, max=57344.0)).numpy()
    elif mode == ENC_REFERENCE:
        q = oracle.encode(y)
    else:
        q = oracle.encode_torch_rne(y)
    return q.reshape(rows, cols), amax, inv


def dequant_rowwise_ref(q, scales, fmt=FMT_E4M3, out_dtype=torch.float32) -> torch.Tensor:
    """bytes (rows, cols), one scale per row -> torch tensor of out_dtype: float32(dec(q)) * scale rounded to float32, then cast."""
    q = np.asarray(q, dtype=np.uint8)
    s = np.asarray(scales, dtype=np.float32).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        prod = (DEC[fmt][q].astype(np.float32) * s).astype(np.float32)
    return torch.from_numpy(prod).to(out_dtype)


def rel_rms_rows(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.sqrt(np.mean((got - want) ** 2, axis=1)) / np.sqrt(np.mean(want ** 2, axis=1))
