"""Host-side reference for the fused activation + quantisation tests (not a test module), from the formulas of include/fp8mi.h
(fp8mi_act_quantize): y is computed on the CPU and handed to the existing references,

  act_y             y float32 (rows, C): act(x), or act(gate) * up for x = [gate | up]
  act_quantize_ref  scale "row":      rowwise_ref.quantize_rowwise_ref(y, fmt, mode)    -> (bytes, scales (rows,), amax (rows,))
                    scale "block128": blockwise_ref.quantize_blockwise_ref(y, 1)        -> (bytes, scales (rows, ceil(C / 128)), None)

act "none": y is the float32 widening of x, or the float32 product of the two widened halves - nothing else, so those modes are
compared byte for byte.  The other acts: the function's value in float64 on the widened input, the gate product included, rounded ONCE
to float32.  The float64 evaluation uses the forms that do not cancel,

  silu       g sigma(g)                                          sigma(w) = 1 / (1 + e^-w) for w >= 0, e^w / (1 + e^w) for w < 0
  gelu_tanh  0.5 g (1 + tanh(u)) = g sigma(2u),                  u = sqrt(2/pi) (g + 0.044715 g^3)
  gelu_erf   0.5 g (1 + erf(g / sqrt 2)) = 0.5 g erfc(-g / sqrt 2)

because 1 + tanh(u) and 1 + erf(.) evaluated literally lose every digit in float64 once g is below about -6 (they round to 0 or to a
single ulp of 1), and a row of large negative gates would then have a reference amax of noise.  literal64 evaluates the formulas as
written, for the check that both agree wherever the literal form has digits left."""
import math

import numpy as np
import torch

import blockwise_ref
import rowwise_ref
from rowwise_ref import ENC_REFERENCE, ENC_RNE, FMT_E4M3, FMT_E5M2  # noqa: F401

ACTS = ("none", "silu", "gelu_tanh", "gelu_erf")
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def widen(x) -> torch.Tensor:
    """-> float32 CPU tensor (f16 / bf16 widened exactly)"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.asarray(x))
    return x.detach().cpu().to(torch.float32)


def _sigmoid64(w: torch.Tensor) -> torch.Tensor:
    e = torch.exp(-w.abs())
    return torch.where(w >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act64(g: torch.Tensor, act: str) -> torch.Tensor:
    """act(g) in float64, g float64"""
    if act == "silu":
        return g * _sigmoid64(g)
    if act == "gelu_tanh":
        return g * _sigmoid64(2.0 * SQRT_2_OVER_PI * (g + 0.044715 * g ** 3))
    if act == "gelu_erf":
        return 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))
    raise ValueError(act)


def literal64(g: torch.Tensor, act: str) -> torch.Tensor:
    """the formulas exactly as include/fp8mi.h writes them, float64"""
    if act == "silu":
        return g / (1.0 + torch.exp(-g))
    if act == "gelu_tanh":
        return 0.5 * g * (1.0 + torch.tanh(SQRT_2_OVER_PI * (g + 0.044715 * g ** 3)))
    if act == "gelu_erf":
        return 0.5 * g * (1.0 + torch.special.erf(g / math.sqrt(2.0)))
    raise ValueError(act)


def split(x, gated: bool):
    xf = widen(x)
    assert xf.dim() == 2
    if not gated:
        return xf, None
    assert xf.shape[1] % 2 == 0
    C = xf.shape[1] // 2
    return xf[:, :C], xf[:, C:]


def act_y(x, act: str = "none", gated: bool = False, fn=act64) -> torch.Tensor:
    """x (rows, C) or (rows, 2C) f32 / f16 / bf16 -> y float32 (rows, C)"""
    assert act in ACTS, act
    g, u = split(x, gated)
    if act == "none":
        if not gated:
            return g.clone()
        y = g * u                                        # float32 arithmetic: one rounding
        # 0 * inf: IEEE 754 leaves the sign of a generated NaN open; x86 and gfx950 both give 0xFFC00000, pinned here as in rowwise_ref
        made = torch.isnan(y) & ~torch.isnan(g) & ~torch.isnan(u)
        return _pin_nan(y, made)
    y = fn(g.double(), act)
    if gated:
        y = y * u.double()
    y = y.to(torch.float32)
    if not gated:
        y = torch.where(torch.isnan(g), g, y)            # a NaN gate stays the NaN it was, as in the "none" mode
    return y


def _pin_nan(y: torch.Tensor, where: torch.Tensor) -> torch.Tensor:
    bits = y.view(torch.int32).clone()
    bits[where] = -0x400000                              # 0xFFC00000
    return bits.view(torch.float32)


def act_quantize_ref(x, act: str = "none", gated: bool = False, scale: str = "row", fmt=FMT_E4M3, mode=ENC_REFERENCE, y=None):
    """-> (bytes uint8 (rows, C), scales float32, amax float32 (rows,) or None); `y` may be passed when it has been computed already"""
    if y is None:
        y = act_y(x, act, gated)
    if scale == "row":
        q, amax, inv = rowwise_ref.quantize_rowwise_ref(y, fmt, mode)
        return q, inv, amax
    assert scale == "block128" and fmt == FMT_E4M3 and mode == ENC_RNE
    rows, cols = y.shape
    if cols == 0:
        return np.zeros((rows, 0), np.uint8), np.zeros((rows, 0), np.float32), None
    q, s = blockwise_ref.quantize_blockwise_ref(y, 1)
    return q.numpy(), s.numpy(), None
