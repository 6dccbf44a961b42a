"""Host-side references for the blockwise tests (not a test module): the blockwise quantisation recipe of include/fp8mi.h
restated with torch CPU ops, and a float64 oracle of the blockwise matmul (fp8mi_scaled_mm_blockwise) in numpy."""
import numpy as np
import torch

from mxfp8_ref import DEC_NAN, DEC_ZERO


def quantize_blockwise_ref(x: torch.Tensor, block_rows: int):
    """(rows, cols) float32 / float16 / bfloat16 CPU tensor -> (uint8 e4m3 bytes (rows, cols), float32 scales (ceil(rows / block_rows),
    ceil(cols / 128))):  amax = max|x| of the block in fp32 (NaN if it holds one);  s = amax / 448 (1 where that quotient is 0: an
    all-zero block, or an f32 amax so small that the division underflows);
    q = e4m3_rne(clamp(x / s, -448, 448)), a NaN quotient as 0x7F; a NaN scale is the quiet NaN 0x7FC00000."""
    rows, cols = x.shape
    nrb, ncb = -(-rows // block_rows), -(-cols // 128)
    xf = x.to(torch.float32)
    pad = torch.zeros(nrb * block_rows, ncb * 128)
    pad[:rows, :cols] = xf
    blocks = pad.reshape(nrb, block_rows, ncb, 128)
    amax = torch.amax(torch.abs(blocks), dim=(1, 3))                      # NaN propagates
    nan = torch.tensor(float("nan"))
    s = amax / 448.0
    s = torch.where(s == 0, torch.tensor(1.0), s)
    s = torch.where(torch.isnan(s), nan, s)
    full = s.repeat_interleave(block_rows, 0).repeat_interleave(128, 1)[:rows, :cols]
    y = torch.clamp(xf / full, min=-448.0, max=448.0)
    y = torch.where(torch.isnan(y), nan, y)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), s


def expand_scales(s: np.ndarray, rows: int, K: int, block: int) -> np.ndarray:
    """(ceil(rows / block), ceil(K / 128)) scales -> (rows, ceil(K / 128)) float64, one row per operand row."""
    return np.repeat(np.asarray(s, dtype=np.float64), block, axis=0)[:rows]


def mm_ref(A, B, sa, sb, block_a=1, block_b=128, nan_zero=True):
    """-> (C (M, N) float64 of sum_b fl32(sa sb) P_b with exact P_b, bound sum_b |fl32(sa sb)| sum_k |a b|, and the largest
    |fl32(sa sb) P_b| over b of each output - the fold's own rounding is bounded by a few ulps of the running sums)."""
    M, K = A.shape
    Nn = B.shape[0]
    dec = DEC_ZERO if nan_zero else DEC_NAN
    a, b = dec[A], dec[B]
    nkb = -(-K // 128)
    ea, eb = expand_scales(sa, M, K, block_a), expand_scales(sb, Nn, K, block_b)
    C = np.zeros((M, Nn))
    bound = np.zeros((M, Nn))
    with np.errstate(invalid="ignore", over="ignore"):
        for blk in range(nkb):
            ks = slice(128 * blk, min(128 * blk + 128, K))
            pb = a[:, ks] @ b[:, ks].T
            ab = np.abs(a[:, ks]) @ np.abs(b[:, ks]).T
            s = (ea[:, blk:blk + 1].astype(np.float32) * eb[:, blk].astype(np.float32)[None, :]).astype(np.float64)
            C += s * pb
            bound += np.abs(s) * ab
    return C, bound
