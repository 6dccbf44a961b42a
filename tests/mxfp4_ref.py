"""Host-side references for the MXFP4 tests (not a test module): torch's MXFP4 quantisation recipe restated with torch CPU ops,
the 16-code e2m1 decode table, and an exact float64 block-scaled matmul in numpy."""
import numpy as np
import torch

# OCP e2m1: code -> value (bit 3 sign, bits 2-1 exponent (bias 1), bit 0 mantissa); no NaN, no inf
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


def bf16_rne(y: torch.Tensor) -> torch.Tensor:
    """float32 -> bfloat16 bits (int32 in 0..0xFFFF), round to nearest even; every NaN -> 0xFFFF, what torch's CPU cast
    (`.to(torch.bfloat16)`) writes for a NaN."""
    u = y.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(torch.isnan(y), torch.full_like(r, 0xFFFF), r).to(torch.int32)


def e2m1_from_bf16(bf: torch.Tensor) -> torch.Tensor:
    """bfloat16 bits -> e2m1 codes: torchao's _f32_to_floatx_unpacked(x, ebits=2, mbits=1) (torch's
    torch/testing/_internal/common_quantized.py) restated: RNE, saturating to 6.0, int32 arithmetic, uint8 results."""
    x = (bf.to(torch.int64) << 16).to(torch.int64)
    x = torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)      # the float32 bits as int32
    sign = x & torch.tensor(-2 ** 31, dtype=torch.int32)
    x = x ^ sign
    xf = x.view(torch.float32)
    saturate = xf >= 6.0
    denormal = torch.logical_and(torch.logical_not(saturate), xf < 1.0)
    normal = torch.logical_not(torch.logical_or(saturate, denormal))
    denorm_mask_int = 149 << 23
    denormal_x = (xf + torch.tensor(denorm_mask_int, dtype=torch.int32).view(torch.float32)).view(torch.int32) - denorm_mask_int
    denormal_x = denormal_x.to(torch.uint8)
    mant_odd = (x >> 22) & 1
    normal_x = (x + (((1 - 127) << 23) + (2 ** 21 - 1)) + mant_odd) >> 22
    normal_x = normal_x.to(torch.uint8)
    out = torch.full_like(x, 7, dtype=torch.uint8)
    out = torch.where(denormal, denormal_x, out)
    out = torch.where(normal, normal_x, out)
    sign_lp = ((sign >> 28).to(torch.uint8)) & 8
    return out | sign_lp


def pack_uint4(codes: torch.Tensor) -> torch.Tensor:
    """(rows, cols) uint8 codes -> (rows, cols/2) bytes, the even column in the low nibble (torch's pack_uint4)."""
    return ((codes[:, 1::2] << 4) | codes[:, ::2]).to(torch.uint8)


def to_mxfp4_ref(x: torch.Tensor):
    """torch.testing._internal.common_quantized.to_mxfp(x, 32, "mxfp4") restated for float32 / bfloat16 / float16 (x, CPU) of
    shape (rows, cols): -> (uint8 scales (rows, cols/32), uint8 packed e2m1 bytes (rows, cols/2))."""
    rows, cols = x.shape
    blocks = x.reshape(rows, cols // 32, 32)
    max_abs = torch.amax(torch.abs(blocks), -1).unsqueeze(-1).to(torch.float32)
    data = blocks.to(torch.float32)
    descale = max_abs / 6.0
    exponent = torch.where(torch.isnan(descale), 0xFF,
                           (torch.clamp(torch.ceil(torch.log2(descale)), min=-127, max=127) + 127).to(torch.uint8))
    factor = torch.where(exponent == 0, 1.0, torch.exp2(127 - exponent.to(torch.float32)))
    data_lp = torch.clamp(data * factor, min=-6.0, max=6.0).reshape(rows, cols)
    codes = e2m1_from_bf16(bf16_rne(data_lp))
    return exponent.reshape(rows, cols // 32).to(torch.uint8), pack_uint4(codes)


def unpack(q: np.ndarray) -> np.ndarray:
    """(rows, cols/2) packed bytes -> (rows, cols) codes."""
    out = np.empty((q.shape[0], 2 * q.shape[1]), dtype=np.uint8)
    out[:, 0::2] = q & 15
    out[:, 1::2] = q >> 4
    return out


def scaled_operand(q: np.ndarray, s: np.ndarray) -> np.ndarray:
    """e2m1(q) x 2^(s - 127) per 32-element block, float64 (exact), NaN where the scale is 0xFF; q packed (rows, K/2)."""
    d = E2M1[unpack(q)]
    f = np.repeat(np.where(s == 0xFF, np.nan, np.ldexp(1.0, s.astype(np.int64) - 127)), 32, axis=1)[:, :d.shape[1]]
    return d * f


def mm_ref(A, B, sa, sb):
    """-> (exact C (M, N) float64, bound sum |a 2^sa| |b 2^sb|); A (M, K/2), B (N, K/2) packed."""
    a = scaled_operand(A, sa)
    b = scaled_operand(B, sb)
    with np.errstate(invalid="ignore", over="ignore"):
        return a @ b.T, np.abs(a) @ np.abs(b).T
