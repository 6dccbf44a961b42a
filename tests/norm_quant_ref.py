"""Host-side reference for the fused normalisation + quantisation tests (not a test module), from the formula of include/fp8mi.h
(fp8mi_norm_quantize):

  make_rows          the tests' input generator: N(0,1) rows with magnitudes 2^-8 .. 2^7, plus a per-row offset of up to eight standard
                     deviations for LayerNorm
  norm_h             step 1: h float32 (and what is stored to h_out) - x, or x + residual in float32 rounded to x's dtype by torch
  norm_stats64       step 2 in float64: (mean or None, rstd)
  norm_y             steps 1 - 3 in numpy float32, ONE operation at a time (numpy fuses nothing), with the statistics it is given - the
                     kernel's own - or the float64 ones rounded to float32
  norm_quantize_ref  y handed to rowwise_ref / blockwise_ref, as act_quant_ref does

A NaN that one of these operations GENERATES (inf * 0, inf - inf) has no sign defined by IEEE 754; it is pinned to 0xFFC00000, what x86
and gfx950 give, as in rowwise_ref / act_quant_ref.  A NaN that comes in through an operand (the input, a statistic) is left as it is."""
import numpy as np
import torch

import blockwise_ref
import rowwise_ref
from rowwise_ref import ENC_REFERENCE, ENC_RNE, FMT_E4M3, FMT_E5M2  # noqa: F401

F32 = np.float32
PINNED = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


def make_rows(rng, rows, cols, dt, layer=False):
    """test_gpu_act_quant.make()'s rows; layer: every row shifted by up to eight of its standard deviations"""
    s = np.exp2(rng.integers(-8, 8, size=(rows, 1)))
    x = rng.standard_normal((rows, cols)) * s
    if layer:
        x = x + rng.uniform(-8.0, 8.0, size=(rows, 1)) * s
    return torch.from_numpy(x.astype(np.float32)).to(dt)


def make_params(rng, n, cols, dt, centre=0.0):
    """n rows of parameters around `centre` (weights: 1, everything else: 0)"""
    return torch.from_numpy((centre + 0.5 * rng.standard_normal((n, cols))).astype(np.float32)).to(dt)


def widen(x) -> np.ndarray:
    """-> float32 numpy array (f16 / bf16 widened exactly); None stays None"""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.asarray(x))
    return x.detach().cpu().to(torch.float32).numpy()


def norm_h(x: torch.Tensor, residual=None):
    """-> (h float32 numpy, h as stored: a tensor of x's dtype, or None without a residual)"""
    if residual is None:
        return widen(x), None
    with np.errstate(invalid="ignore", over="ignore"):
        s = (widen(x) + widen(residual)).astype(F32)
    stored = torch.from_numpy(s).to(x.dtype)           # round to nearest even, as torch's own x + residual
    return widen(stored), stored


def norm_stats64(h, norm: str, eps: float):
    """h float32 (rows, cols) -> (mean float64[rows] or None, rstd float64[rows]); LayerNorm's variance about the float64 mean"""
    h64 = np.asarray(h, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if norm == "rms":
            return None, 1.0 / np.sqrt(np.mean(h64 * h64, axis=1) + np.float64(F32(eps)))
        mean = np.mean(h64, axis=1)
        d = h64 - mean[:, None]
        return mean, 1.0 / np.sqrt(np.mean(d * d, axis=1) + np.float64(F32(eps)))


def norm_y(x, norm="rms", weight=None, bias=None, eps=1e-6, residual=None, mod_scale=None, mod_shift=None, rows_per_mod=1, mean=None, rstd=None):
    """-> (y float32 (rows, cols), h float32, h as stored or None).  mean / rstd: float32[rows], the statistics to compute with."""
    assert norm in ("rms", "layer")
    h, stored = norm_h(x, residual)
    rows, cols = h.shape
    if rstd is None:
        m64, r64 = norm_stats64(h, norm, eps)
        rstd = r64.astype(F32)
        mean = None if m64 is None else m64.astype(F32)
    rstd = np.asarray(rstd, dtype=F32).reshape(rows, 1)
    operand_nan = np.isnan(h) | np.isnan(rstd)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if norm == "layer":
            mean = np.asarray(mean, dtype=F32).reshape(rows, 1)
            operand_nan = operand_nan | np.isnan(mean)
            d = (h - mean).astype(F32)
        else:
            d = h
        z = (d * rstd).astype(F32)
        if weight is not None:
            w = widen(weight).reshape(1, cols)
            z = (z * w).astype(F32)
            operand_nan = operand_nan | np.isnan(w)
        if bias is not None:
            b = widen(bias).reshape(1, cols)
            z = (z + b).astype(F32)
            operand_nan = operand_nan | np.isnan(b)
        if mod_scale is not None:
            g = np.arange(rows) // rows_per_mod
            sc, sh = widen(mod_scale).reshape(-1, cols)[g], widen(mod_shift).reshape(-1, cols)[g]
            t = (F32(1.0) + sc).astype(F32)
            z = (z * t).astype(F32)
            z = (z + sh).astype(F32)
            operand_nan = operand_nan | np.isnan(sc) | np.isnan(sh)
    y = np.where(np.isnan(z) & ~operand_nan, PINNED, z).astype(F32)
    return y, h, stored


def two_nan_elements(x, norm, residual=None, mean=None, rstd=None):
    """The elements where TWO NaNs meet in d * rstd (a NaN d - a NaN element, or LayerNorm's h - mean with a NaN or inf - inf - and a NaN
    rstd): the one place where the sign of y's NaN is not specified.  Everywhere else a NaN y is generated (pinned) or is its single NaN
    operand's."""
    h, _ = norm_h(x, residual)
    rows = h.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (h - np.asarray(mean, dtype=F32).reshape(rows, 1)).astype(F32) if norm == "layer" else h
    return np.isnan(d) & np.isnan(np.asarray(rstd, dtype=F32).reshape(rows, 1))


def norm_quantize_ref(x, norm="rms", weight=None, bias=None, eps=1e-6, residual=None, mod_scale=None, mod_shift=None, rows_per_mod=1, scale="row",
                      fmt=FMT_E4M3, mode=ENC_REFERENCE, mean=None, rstd=None):
    """-> ((bytes uint8 (rows, cols), scales float32, amax float32 (rows,) or None), y, h as stored or None)"""
    y, _, stored = norm_y(x, norm, weight, bias, eps, residual, mod_scale, mod_shift, rows_per_mod, mean, rstd)
    if scale == "row":
        q, amax, inv = rowwise_ref.quantize_rowwise_ref(y, fmt, mode)
        return (q, inv, amax), y, stored
    assert scale == "block128" and fmt == FMT_E4M3 and mode == ENC_RNE
    rows, cols = y.shape
    if cols == 0:
        return (np.zeros((rows, 0), np.uint8), np.zeros((rows, 0), np.float32), None), y, stored
    q, s = blockwise_ref.quantize_blockwise_ref(torch.from_numpy(y), 1)
    return (q.numpy(), s.numpy(), None), y, stored


# ---- the statistics caps of tests/test_gpu_norm_quant.py (conditions, not measurements) ------------------------------------------------

STAT_CAP = 2.0 ** -18   # the project's scale cap: 64 fp32 ulps


def stat_ratios(h, norm, eps, mean, rstd):
    """The returned statistics against float64, as multiples of the caps: (mean ratio or 0, rstd ratio), the largest over the rows.
    mean: |mean - mean64| <= 2^-18 mean_c |h|.  rstd: |rstd - rstd64| <= 2^-18 rstd64, with rstd64 from mean(h^2) (RMS) or from
    mean64(d^2), d = fl32(h - mean) formed from the RETURNED mean (LayerNorm: a reference about the float64 mean would test the data's
    conditioning - rows of 2 or 129 columns show it).  A NaN statistic must be NaN in both (ratio 0) - else inf."""
    h64 = np.asarray(h, dtype=np.float64)
    rstd = np.asarray(rstd, dtype=np.float64).reshape(-1)
    e64 = np.float64(F32(eps))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mr = 0.0
        if norm == "layer":
            mean = np.asarray(mean, dtype=F32).reshape(-1)
            mean64 = np.mean(h64, axis=1)
            r = np.abs(mean.astype(np.float64) - mean64) / (STAT_CAP * np.mean(np.abs(h64), axis=1))
            r = np.where(mean.astype(np.float64) == mean64, 0.0, r)
            r = np.where(np.isnan(mean64) | np.isnan(mean), np.where(np.isnan(mean64) & np.isnan(mean), 0.0, np.inf), r)
            mr = float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0
            d = (np.asarray(h, dtype=F32) - mean[:, None]).astype(F32).astype(np.float64)
        else:
            d = h64
        rstd64 = 1.0 / np.sqrt(np.mean(d * d, axis=1) + e64)
        r = np.abs(rstd - rstd64) / (STAT_CAP * rstd64)
        r = np.where(rstd == rstd64, 0.0, r)
        r = np.where(np.isnan(rstd64) | np.isnan(rstd), np.where(np.isnan(rstd64) & np.isnan(rstd), 0.0, np.inf), r)
        rr = float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0
    return mr, rr


def lane_sum32(v):
    """float32 sums along the rows the way a wave forms them at the least: 64 strided partial sums, each sequential, then added in order"""
    v = np.asarray(v, dtype=F32)
    rows, cols = v.shape
    pad = (-cols) % 64
    v = np.concatenate([v, np.zeros((rows, pad), F32)], axis=1).reshape(rows, -1, 64)
    part = np.zeros((rows, 64), F32)
    for i in range(v.shape[1]):
        part = (part + v[:, i, :]).astype(F32)
    tot = np.zeros(rows, F32)
    for lane in range(64):
        tot = (tot + part[:, lane]).astype(F32)
    return tot


def stats32(h, norm, eps):
    """the statistics by lane_sum32, every other operation as the contract writes it: (mean or None, rstd), float32"""
    h = np.asarray(h, dtype=F32)
    cols = F32(h.shape[1])
    if norm == "layer":
        mean = (lane_sum32(h) / cols).astype(F32)
        d = (h - mean[:, None]).astype(F32)
    else:
        mean, d = None, h
    ms = (lane_sum32((d * d).astype(F32)) / cols).astype(F32)
    rstd = (F32(1.0) / np.sqrt((ms + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    return mean, rstd
