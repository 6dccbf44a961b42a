"""Host-side references for the MXFP8 tests (not a test module): torch's MXFP8 quantisation recipe restated with torch CPU ops,
and an exact float64 block-scaled matmul in numpy."""
import numpy as np
import torch


def to_mxfp8_ref(x: torch.Tensor):
    """torch.testing._internal.common_quantized.to_mxfp(x, 32, "mxfp8") restated (torchao's RCEIL), for float32 / bfloat16 /
    float16 (x, CPU) of shape (rows, cols): -> (uint8 scales (rows, cols/32), uint8 e4m3 bytes (rows, cols))."""
    rows, cols = x.shape
    blocks = x.reshape(rows, cols // 32, 32)
    max_abs = torch.amax(torch.abs(blocks), -1).unsqueeze(-1).to(torch.float32)
    data = blocks.to(torch.float32)
    descale = max_abs / 448.0
    exponent = torch.where(torch.isnan(descale), 0xFF,
                           (torch.clamp(torch.ceil(torch.log2(descale)), min=-127, max=127) + 127).to(torch.uint8))
    factor = torch.where(exponent == 0, 1.0, torch.exp2(127 - exponent.to(torch.float32)))
    data_lp = torch.clamp(data * factor, min=-448.0, max=448.0).to(torch.float8_e4m3fn)
    return exponent.reshape(rows, cols // 32).to(torch.uint8), data_lp.reshape(rows, cols).view(torch.uint8)


def _decode_table(nan_zero: bool) -> np.ndarray:
    t = np.zeros(256)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        if (b & 0x7F) == 0x7F:
            v = 0.0 if nan_zero else np.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


DEC_ZERO = _decode_table(True)
DEC_NAN = _decode_table(False)


def scaled_operand(q: np.ndarray, s: np.ndarray, nan_zero: bool = True) -> np.ndarray:
    """dec(q) x 2^(s - 127) per 32-element block, float64 (exact), NaN where the scale is 0xFF."""
    d = (DEC_ZERO if nan_zero else DEC_NAN)[q]
    f = np.repeat(np.where(s == 0xFF, np.nan, np.ldexp(1.0, s.astype(np.int64) - 127)), 32, axis=1)[:, :q.shape[1]]
    return d * f


def mm_ref(A, B, sa, sb, nan_zero=True):
    """-> (exact C (M, N) float64, bound sum |a 2^sa| |b 2^sb|)."""
    a = scaled_operand(A, sa, nan_zero)
    b = scaled_operand(B, sb, nan_zero)
    with np.errstate(invalid="ignore", over="ignore"):
        return a @ b.T, np.abs(a) @ np.abs(b).T
