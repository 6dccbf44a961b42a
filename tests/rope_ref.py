"""The rotary embedding of fp8mi_rope_kv_cache_append / fp8mi_mla_rope_cache_append on the CPU (include/fp8mi.h states it): rotate32 is the
definition in float32, every operation a separately rounded elementwise one; rotate64 the same in float64 with the optional RMSNorm in front.
A plain module: no fixtures, no tests."""
import numpy as np
import torch


def _partners(rot_dim, style):
    half = rot_dim // 2
    return (slice(0, half), slice(half, rot_dim)) if style == "neox" else (slice(0, rot_dim, 2), slice(1, rot_dim, 2))


def rotate32(x, cos_sin, positions, rot_dim, style):
    """x (T, H, D) of any float dtype, cos_sin (max_pos, >= rot_dim), positions (T,) inside the table -> y (T, H, D) float32:
    y_a = fl(fl(x_a c) - fl(x_b s)), y_b = fl(fl(x_b c) + fl(x_a s)); channels at or beyond rot_dim pass through"""
    x, half = x.detach().cpu().float(), rot_dim // 2
    row = cos_sin.detach().cpu().float()[positions.cpu().long()]
    c, s = row[:, None, :half], row[:, None, half:rot_dim]
    ia, ib = _partners(rot_dim, style)
    a, b = x[..., ia], x[..., ib]
    y = x.clone()
    y[..., ia] = a * c - b * s
    y[..., ib] = b * c + a * s
    return y


def rotate64(x, cos_sin, positions, rot_dim, style, weight=None, eps=1e-6):
    """-> (y, mag) float64 numpy: the norm n = x / sqrt(mean(x^2) + eps) * weight over the last axis (weight None: n = x), then the rotation;
    mag is |n_a c| + |n_b s| for a rotated channel and |n| for one that passes through"""
    n, half = x.detach().cpu().double().numpy(), rot_dim // 2
    if weight is not None:
        n = n / np.sqrt((n * n).mean(axis=-1, keepdims=True) + eps) * weight.detach().cpu().double().numpy()
    row = cos_sin.detach().cpu().double().numpy()[positions.cpu().long().numpy()]
    c, s = row[:, None, :half], row[:, None, half:rot_dim]
    ia, ib = _partners(rot_dim, style)
    a, b = n[..., ia], n[..., ib]
    y, mag = n.copy(), np.abs(n)
    y[..., ia], y[..., ib] = a * c - b * s, b * c + a * s
    mag[..., ia], mag[..., ib] = np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)
    return y, mag
