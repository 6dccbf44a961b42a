"""Host-side reference for the float8_e5m2 tests (not a test module).  Everything comes from torch's CPU implementation of the
dtype and from float64 arithmetic:

  DEC_E5M2 / DEC_E4M3   256-entry decode tables, uint8.view(float8_*).float() widened to float64 (OCP: inf and NaN entries kept)
  mm_ref                float64 matmul of the decoded operands with the sum|a||b| bound the GEMM tolerances are stated against
  encode_ref            torch CPU's x.to(torch.float8_e5m2), as bytes
  quantize_ref          the amax-scaled recipe of include/fp8mi.h (fp8mi_quantize_e5m2) restated with torch CPU ops
"""
import numpy as np
import torch

FMT_E4M3, FMT_E5M2 = 0, 1
_ALL = torch.arange(256, dtype=torch.int16).to(torch.uint8)
DEC_E5M2 = _ALL.view(torch.float8_e5m2).float().double().numpy()
DEC_E4M3 = _ALL.view(torch.float8_e4m3fn).float().double().numpy()
DEC = {FMT_E4M3: DEC_E4M3, FMT_E5M2: DEC_E5M2}
TORCH_DTYPE = {FMT_E4M3: torch.float8_e4m3fn, FMT_E5M2: torch.float8_e5m2}

# tolerances of the existing suite (tests/test_gpu_parity.py): fp32-FMA kernels and exact matrix-core cases; the matrix-core
# truncation bound (7 addends of a group of 8, each up to 2^-13 of the largest: 8.5e-4) and its rms gate
MM_TOL = 4e-6
MFMA_TOL = 1e-3
MFMA_RMS_TOL = 1e-4


def closed_form_e5m2(b: int) -> float:
    """Value of e5m2 byte b from the format's definition: 1 sign, 5 exponent (bias 15), 2 mantissa bits; exponent 31 is inf / NaN."""
    s, e, m = b >> 7, (b >> 2) & 31, b & 3
    if e == 31:
        v = float("inf") if m == 0 else float("nan")
    elif e == 0:
        v = m / 4.0 * 2.0 ** -14
    else:
        v = (1 + m / 4.0) * 2.0 ** (e - 15)
    return -v if s else v


def finite_bytes(rng, shape, fmt):
    """Random bytes of format fmt without inf / NaN encodings: e5m2 bytes with (b & 0x7C) == 0x7C and e4m3 0x7F / 0xFF are redrawn
    as the same byte with one exponent bit cleared."""
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if fmt == FMT_E5M2:
        return np.where((b & 0x7C) == 0x7C, b & 0xBF, b).astype(np.uint8)
    return np.where((b & 0x7F) == 0x7F, b & 0xF7, b).astype(np.uint8)


def mm_ref(A, B, sa, sb, fa, fb, bias=None, scale_result=None):
    """-> (C, bound) float64: C = ((dec_fa(A) @ dec_fb(B).T) * sa[:, None] * sb[None, :] + bias) * scale_result and
    bound = (|dec(A)| @ |dec(B)|.T) * |sa sb| * |scale_result| (the bias adds no error of the sum).  sa: 1 or M values, sb: 1 or N."""
    a, b = DEC[fa][A], DEC[fb][B]
    sa = np.asarray(sa, dtype=np.float64).reshape(-1, 1)
    sb = np.asarray(sb, dtype=np.float64).reshape(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        C = (a @ b.T) * sa * sb
        bound = (np.abs(a) @ np.abs(b).T) * np.abs(sa * sb)
        if bias is not None:
            C = C + np.asarray(bias, dtype=np.float64).reshape(1, -1)
        if scale_result is not None:
            C = C * float(scale_result)
            bound = bound * abs(float(scale_result))
    return C, bound


def encode_ref(x: torch.Tensor) -> torch.Tensor:
    """torch CPU's cast, as uint8 bytes."""
    return x.cpu().to(torch.float8_e5m2).view(torch.uint8)


def quantize_ref(x: torch.Tensor):
    """-> (bytes, amax, inv_scale): amax = max|x| in fp32 (NaNs ignored); scale = 57344 / amax in double (1 when amax == 0), rounded to fp32;
    q = e5m2_rne(clamp(fp32(x) * scale, +-57344)); inv_scale = fp32(1 / (57344 / amax))."""
    xf = x.cpu().to(torch.float32)
    finite = torch.where(torch.isnan(xf), torch.zeros_like(xf), xf.abs())
    amax = float(finite.max()) if xf.numel() else 0.0
    scale = np.float32(57344.0 / amax) if amax > 0 else np.float32(1.0)
    inv = np.float32(1.0 / (57344.0 / amax)) if amax > 0 else np.float32(1.0)
    y = torch.clamp(xf * torch.tensor(scale), min=-57344.0, max=57344.0)
    return encode_ref(y), np.float32(amax), inv
