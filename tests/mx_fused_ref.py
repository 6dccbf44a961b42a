"""Host-side reference of the fused producers with MXFP8 / MXFP4 output (fp8mi_act_quantize_mx / fp8mi_norm_quantize_mx; not a test
module).  It composes what exists: y from act_quant_ref.act_y or norm_quant_ref.norm_y (the latter fed with the statistics the GPU
returned), then mxfp8_ref.to_mxfp8_ref / mxfp4_ref.to_mxfp4_ref on that float32 y.

For the transcendental activations the kernel's y is a few fp32 ulps from the float64-derived one, so a block whose
descale = fl32(amax / max_pos) sits on a power of two can take the neighbouring exponent: `window` finds those blocks (descale within
2^-18 relative of a power of two), `allowed_exponents` the two bytes such a block may get, and `requantize` re-evaluates the recipe's
element step with a given exponent."""
import numpy as np
import torch

import act_quant_ref as A
import mxfp4_ref
import mxfp8_ref
import norm_quant_ref as NR

FORMATS = ("mxfp8", "mxfp4")
MAX_POS = {"mxfp8": 448.0, "mxfp4": 6.0}
WINDOW = 2.0 ** -18          # the project's scale cap
BYTE_SHARE = 1e-3            # the project's cap on the share of element codes that may be one step off
BLOCK_SHARE = 0.02           # excused blocks: at most max(1 block, 2 %) of a tensor's blocks

# the transcendental grid of tests/test_gpu_mx_fused.py, shared with the host test that checks the window share on the reference alone
T_ACTS = ("silu", "gelu_tanh", "gelu_erf")
T_COLS = (32, 224, 1024, 4128, 16416)
T_ROWS = (3, 257)
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def make(rng, rows, cols, dt):
    """test_gpu_act_quant.make(): N(0,1) rows with magnitudes spread over 2^-8 .. 2^7, in dtype dt"""
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-8, 8, size=(rows, 1)))
    return torch.from_numpy(x.astype(np.float32)).to(dt)


def t_seed(act, gated, dt):
    return 8000 + 100 * T_ACTS.index(act) + 10 * int(gated) + DT_CODE[dt]


def t_inputs(act, gated, dt):
    """the inputs of one case of the transcendental grid, in the order the GPU test draws them: yields (rows, cols, x)"""
    rng = np.random.default_rng(t_seed(act, gated, dt))
    for cols in T_COLS:
        for rows in T_ROWS:
            yield rows, cols, make(rng, rows, 2 * cols if gated else cols, dt)


def as_f32(y) -> torch.Tensor:
    if not isinstance(y, torch.Tensor):
        y = torch.from_numpy(np.ascontiguousarray(np.asarray(y, dtype=np.float32)))
    return y.detach().cpu().to(torch.float32).contiguous()


def to_mx_ref(y, fmt: str):
    """float32 y (rows, cols), cols % 32 == 0 -> (scale bytes uint8 (rows, cols/32), element bytes uint8 (rows, cols) or (rows, cols/2))"""
    assert fmt in FORMATS
    y = as_f32(y)
    rows, cols = y.shape
    assert cols % 32 == 0
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols // 32), np.uint8), np.zeros((rows, cols // (2 if fmt == "mxfp4" else 1)), np.uint8)
    s, q = (mxfp8_ref.to_mxfp8_ref if fmt == "mxfp8" else mxfp4_ref.to_mxfp4_ref)(y)
    return s.numpy(), q.numpy()


def act_mx_ref(x, act="none", gated=False, fmt="mxfp8", y=None):
    """-> (scale bytes, element bytes, y)"""
    if y is None:
        y = A.act_y(x, act, gated)
    s, q = to_mx_ref(y, fmt)
    return s, q, y


def norm_mx_ref(x, norm="rms", fmt="mxfp8", mean=None, rstd=None, **kw):
    """-> (scale bytes, element bytes, y, h as stored or None); mean / rstd: the statistics the GPU returned"""
    y, _, stored = NR.norm_y(x, norm, mean=mean, rstd=rstd, **kw)
    s, q = to_mx_ref(y, fmt)
    return s, q, y, stored


def descale(y, fmt: str) -> np.ndarray:
    """fl32(amax / max_pos) of every block, float32 (rows, cols/32)"""
    y = as_f32(y)
    rows, cols = y.shape
    amax = torch.amax(torch.abs(y.reshape(rows, cols // 32, 32)), -1)
    return (amax / MAX_POS[fmt]).numpy()


def window(y, fmt: str):
    """-> (inside: bool (rows, cols/32) - the block's descale lies within 2^-18 relative of a power of two 2^k; k: int (rows, cols/32))"""
    d = descale(y, fmt).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.rint(np.log2(d))
        k = np.where(np.isfinite(k), k, 0.0)
        inside = np.isfinite(d) & (d > 0) & (np.abs(d / np.exp2(k) - 1.0) <= WINDOW)
    return inside, k.astype(np.int64)


def allowed_exponents(k: np.ndarray):
    """the two scale bytes a block inside the window around 2^k may get: RCEIL just below or on the power (k) and just above it (k + 1)"""
    return np.clip(k, -127, 127) + 127, np.clip(k + 1, -127, 127) + 127


def requantize(y, e: np.ndarray, fmt: str) -> np.ndarray:
    """the recipe's element step with the exponent bytes e (rows, cols/32) in place of its own: fl32(y * 2^(127 - e)) (factor 1 for
    e == 0), clamped, rounded as to_mxfp*_ref rounds"""
    y = as_f32(y)
    rows, cols = y.shape
    ef = torch.from_numpy(np.ascontiguousarray(e).astype(np.float32)).reshape(rows, cols // 32, 1)
    factor = torch.where(ef == 0, torch.tensor(1.0), torch.exp2(127 - ef))
    data = y.reshape(rows, cols // 32, 32) * factor
    if fmt == "mxfp8":
        return torch.clamp(data, min=-448.0, max=448.0).to(torch.float8_e4m3fn).reshape(rows, cols).view(torch.uint8).numpy()
    lp = torch.clamp(data, min=-6.0, max=6.0).reshape(rows, cols)
    return mxfp4_ref.pack_uint4(mxfp4_ref.e2m1_from_bf16(mxfp4_ref.bf16_rne(lp))).numpy()


def codes(q: np.ndarray, fmt: str) -> np.ndarray:
    """element bytes -> one integer code per element (MXFP4: the two nibbles of a byte side by side), as int32"""
    q = np.asarray(q, dtype=np.uint8)
    if fmt == "mxfp8":
        return q.astype(np.int32)
    return np.stack([q & 0xF, q >> 4], axis=-1).reshape(q.shape[0], -1).astype(np.int32)


def compare_transcendental(y_ref, s_gpu, q_gpu, fmt: str):
    """The conditions of the transcendental grid.  -> dict(blocks, excused, wrong_scale, off_by_one, far): the number of blocks, of blocks
    inside the window, of blocks whose scale byte is not allowed (outside the window: not the reference's; inside: neither of the two
    neighbours of the power of two), of element codes one step from the reference recipe evaluated with the GPU's exponent, and of
    codes further off than that."""
    s_ref, _ = to_mx_ref(y_ref, fmt)
    inside, k = window(y_ref, fmt)
    lo, hi = allowed_exponents(k)
    s_gpu = np.asarray(s_gpu, dtype=np.uint8).reshape(s_ref.shape)
    ok = np.where(inside, (s_gpu == lo) | (s_gpu == hi), s_gpu == s_ref)
    assert (np.where(inside, (s_ref == lo) | (s_ref == hi), True)).all(), "the reference's own exponent is one of the two"
    want = requantize(y_ref, s_gpu, fmt)
    d = np.abs(codes(np.asarray(q_gpu).reshape(want.shape), fmt) - codes(want, fmt))
    return dict(blocks=int(s_ref.size), excused=int(inside.sum()), wrong_scale=int((~ok).sum()), off_by_one=int((d == 1).sum()),
                far=int((d > 1).sum()), elements=int(d.size))
