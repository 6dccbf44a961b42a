"""The fused producers with MXFP8 / MXFP4 output on the host (no GPU): argument validation of fp8mi_act_quantize_mx and
fp8mi_norm_quantize_mx through the built library (every check runs before any HIP call), the symbols declared and bound with the ABI
version unmoved, the op layer's keyword validation, the reference of tests/mx_fused_ref.py against the references it builds on, and the
condition tests/test_gpu_mx_fused.py puts on the transcendental grid - how many blocks may be excused - checked on the reference alone."""
import os
import re

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import mx_fused_ref as MX
import mxfp4_ref
import mxfp8_ref

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8, FP4 = L.MX_FP8, L.MX_FP4


@pytest.fixture(scope="module")
def lib():
    return L.load()


def act_call(lib, rows=4, cols=64, ld_in=None, act=L.ACT_SILU, ld_out=None, inp=P, out=P, scales=P, ld_s=None, dtype=L.BF16, fmt=FP8):
    width = 2 * cols if act & L.ACT_GATED else cols
    ocols = cols // 2 if fmt == FP4 else cols
    return lib.fp8mi_act_quantize_mx(inp, dtype, rows, cols, width if ld_in is None else ld_in, act, out, ocols if ld_out is None else ld_out, scales,
                                     cols // 32 if ld_s is None else ld_s, fmt, None)


def norm_call(lib, rows=4, cols=64, ld_in=None, norm=L.NORM_RMS, eps=1e-6, weight=None, bias=None, msc=None, msh=None, ld_mod=None, rpm=1, pdt=L.BF16,
              res=None, ld_res=None, h=None, ld_h=None, ld_out=None, inp=P, out=P, scales=P, ld_s=None, dtype=L.BF16, fmt=FP8, mean=None, rstd=None):
    d = lambda v: cols if v is None else v   # noqa: E731
    ocols = cols // 2 if fmt == FP4 else cols
    return lib.fp8mi_norm_quantize_mx(inp, dtype, rows, cols, d(ld_in), norm, eps, weight, bias, msc, msh, d(ld_mod), rpm, pdt, res, d(ld_res), h, d(ld_h), out,
                                      ocols if ld_out is None else ld_out, scales, cols // 32 if ld_s is None else ld_s, fmt, mean, rstd, None)


# ---- argument validation, through the built library --------------------------------------------------------------------------

def test_act_quantize_mx_argument_errors_without_gpu(lib):
    err = lib.fp8mi_last_error
    for fmt in (FP8, FP4):
        assert act_call(lib, inp=None, fmt=fmt) == E_NULL and b"fp8mi_act_quantize_mx" in err() and b"NULL" in err()
        assert act_call(lib, out=None, fmt=fmt) == E_NULL and act_call(lib, scales=None, fmt=fmt) == E_NULL
        assert act_call(lib, rows=-1, fmt=fmt) == E_SHAPE and b"negative" in err()
        assert act_call(lib, cols=-32, ld_in=0, ld_out=0, ld_s=0, fmt=fmt) == E_SHAPE
        for cols in (1, 31, 33, 48, 100):
            assert act_call(lib, cols=cols, fmt=fmt) == E_SHAPE and b"multiple of 32" in err()
        assert act_call(lib, ld_in=63, fmt=fmt) == E_SHAPE and b"leading dimension" in err()
        assert act_call(lib, ld_out=(31 if fmt == FP4 else 63), fmt=fmt) == E_SHAPE
        assert act_call(lib, ld_s=1, fmt=fmt) == E_SHAPE
        # gated: the input is 2 cols wide
        assert act_call(lib, act=L.ACT_SILU | L.ACT_GATED, ld_in=127, fmt=fmt) == E_SHAPE and b"2 cols" in err()
        assert act_call(lib, act=L.ACT_NONE | L.ACT_GATED, ld_in=64, fmt=fmt) == E_SHAPE
        assert act_call(lib, act=4, fmt=fmt) == E_ENUM and b"act" in err()
        assert act_call(lib, act=-1, fmt=fmt) == E_ENUM and act_call(lib, act=0x200, fmt=fmt) == E_ENUM and act_call(lib, act=0x104, fmt=fmt) == E_ENUM
        assert act_call(lib, dtype=3, fmt=fmt) == E_ENUM and b"in_dtype" in err()
        assert act_call(lib, dtype=-1, fmt=fmt) == E_ENUM
        # rows == 0 or cols == 0 is a no-op that accepts NULL pointers - but not bad enums or shapes
        assert act_call(lib, rows=0, inp=None, out=None, scales=None, fmt=fmt) == 0
        assert act_call(lib, cols=0, inp=None, out=None, scales=None, fmt=fmt) == 0
        assert act_call(lib, rows=0, cols=0, inp=None, out=None, scales=None, act=L.ACT_GATED, fmt=fmt) == 0
        assert act_call(lib, rows=0, dtype=9, fmt=fmt) == E_ENUM and act_call(lib, rows=0, ld_in=1, fmt=fmt) == E_SHAPE
        assert act_call(lib, rows=0, act=77, fmt=fmt) == E_ENUM and act_call(lib, rows=0, cols=40, fmt=fmt) == E_SHAPE
        assert act_call(lib, cols=0, dtype=9, inp=None, out=None, scales=None, fmt=fmt) == E_ENUM
    assert act_call(lib, fmt=2) == E_ENUM and b"mx_format" in err()
    assert act_call(lib, fmt=-1) == E_ENUM and act_call(lib, rows=0, fmt=7) == E_ENUM
    # MXFP4 rows are cols / 2 bytes long
    assert act_call(lib, rows=0, ld_out=32, fmt=FP4) == 0 and act_call(lib, rows=0, ld_out=32, fmt=FP8) == E_SHAPE


def test_norm_quantize_mx_argument_errors_without_gpu(lib):
    err = lib.fp8mi_last_error
    for fmt in (FP8, FP4):
        assert norm_call(lib, inp=None, fmt=fmt) == E_NULL and b"fp8mi_norm_quantize_mx" in err() and b"NULL" in err()
        assert norm_call(lib, out=None, fmt=fmt) == E_NULL and norm_call(lib, scales=None, fmt=fmt) == E_NULL
        assert norm_call(lib, rows=-1, fmt=fmt) == E_SHAPE and b"negative" in err()
        for cols in (1, 31, 33, 48, 100):
            assert norm_call(lib, cols=cols, fmt=fmt) == E_SHAPE and b"multiple of 32" in err()
        assert norm_call(lib, ld_in=63, fmt=fmt) == E_SHAPE and b"leading dimension" in err()
        assert norm_call(lib, ld_out=(31 if fmt == FP4 else 63), fmt=fmt) == E_SHAPE
        assert norm_call(lib, ld_s=1, fmt=fmt) == E_SHAPE
        assert norm_call(lib, res=P, h=P, ld_res=63, fmt=fmt) == E_SHAPE and norm_call(lib, res=P, h=P, ld_h=63, fmt=fmt) == E_SHAPE
        assert norm_call(lib, msc=P, msh=P, ld_mod=63, fmt=fmt) == E_SHAPE
        assert norm_call(lib, msc=P, msh=P, rpm=0, fmt=fmt) == E_SHAPE and b"rows_per_mod" in err()
        assert norm_call(lib, norm=2, fmt=fmt) == E_ENUM and b"norm" in err()
        assert norm_call(lib, dtype=3, fmt=fmt) == E_ENUM and b"in_dtype" in err()
        assert norm_call(lib, pdt=3, fmt=fmt) == E_ENUM and b"param_dtype" in err()
        assert norm_call(lib, pdt=L.F16, fmt=fmt) == E_UNSUPPORTED and b"param_dtype" in err()
        assert norm_call(lib, pdt=L.F32, rows=0, fmt=fmt) == 0
        assert norm_call(lib, mean=P, fmt=fmt) == E_UNSUPPORTED and b"mean" in err()
        assert norm_call(lib, msc=P, fmt=fmt) == E_NULL and b"mod_scale" in err()
        assert norm_call(lib, msh=P, fmt=fmt) == E_NULL
        assert norm_call(lib, res=P, fmt=fmt) == E_NULL and b"residual" in err()
        assert norm_call(lib, h=P, fmt=fmt) == E_NULL
        # rows == 0 or cols == 0 is a no-op that accepts NULL pointers - but not bad enums or shapes
        assert norm_call(lib, rows=0, inp=None, out=None, scales=None, fmt=fmt) == 0
        assert norm_call(lib, cols=0, inp=None, out=None, scales=None, fmt=fmt) == 0
        assert norm_call(lib, rows=0, norm=5, fmt=fmt) == E_ENUM and norm_call(lib, rows=0, ld_in=1, fmt=fmt) == E_SHAPE
        assert norm_call(lib, cols=0, dtype=9, inp=None, out=None, scales=None, fmt=fmt) == E_ENUM
        assert norm_call(lib, rows=0, cols=40, fmt=fmt) == E_SHAPE
    assert norm_call(lib, fmt=2) == E_ENUM and b"mx_format" in err()
    assert norm_call(lib, fmt=-1) == E_ENUM and norm_call(lib, rows=0, fmt=7) == E_ENUM


def test_new_symbols_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    assert re.search(r"\bint\s+fp8mi_act_quantize_mx\s*\(", hdr) and re.search(r"\bint\s+fp8mi_norm_quantize_mx\s*\(", hdr)
    assert len(L.SIGNATURES["fp8mi_act_quantize_mx"][1]) == 12 and lib.fp8mi_act_quantize_mx.argtypes == L.SIGNATURES["fp8mi_act_quantize_mx"][1]
    assert len(L.SIGNATURES["fp8mi_norm_quantize_mx"][1]) == 26 and lib.fp8mi_norm_quantize_mx.argtypes == L.SIGNATURES["fp8mi_norm_quantize_mx"][1]
    for name, value in (("FP8MI_MX_FP8", L.MX_FP8), ("FP8MI_MX_FP4", L.MX_FP4)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", hdr), name
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move
    # the two existing entry points did not grow a third scale mode
    assert lib.fp8mi_act_quantize(P, L.BF16, 4, 64, 64, L.ACT_SILU, P, 64, P, 1, 1, None, 2, L.FMT_E4M3, L.ENC_RNE, None) == E_ENUM


def test_op_layer_exposes_the_ops_and_validates_keywords():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_mlp_mxfp8", "fp8_mlp_mxfp4", "fp8_norm_linear_mxfp8", "fp8_norm_linear_mxfp4"):
        assert callable(getattr(N, name)) and getattr(alias, name) is getattr(N, name), name
    x = torch.zeros(4, 64)
    for scale in MX.FORMATS:
        for f in (N.fp8_act_quantize, N.fp8_norm_quantize):
            with pytest.raises(AssertionError, match="out_format"):
                f(x, scale=scale, out_format=L.FMT_E5M2)
            with pytest.raises(AssertionError, match="encode_mode"):
                f(x, scale=scale, encode_mode=L.ENC_RNE)
        with pytest.raises(AssertionError, match="amax"):
            N.fp8_act_quantize(x, scale=scale, return_amax=True)
        with pytest.raises(AssertionError, match="unknown act"):
            N.fp8_act_quantize(x, act="relu", scale=scale)
        with pytest.raises(AssertionError, match="unknown norm"):
            N.fp8_norm_quantize(x, norm="group", scale=scale)
    with pytest.raises(AssertionError, match="unknown scale"):
        N.fp8_act_quantize(x, scale="tensor")
    with pytest.raises(AssertionError, match="unknown scale"):
        N.fp8_norm_quantize(x, scale="tensor")
    with pytest.raises(AssertionError, match="unknown scale"):
        N.fp8_act_quantize(x, scale="mxfp6")


# ---- the reference against the references it builds on -----------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_ref_none_reduces_to_the_existing_references(dt):
    rng = np.random.default_rng(5)
    x = MX.make(rng, 9, 2 * 224, dt)
    x[3, 7] = float("nan")
    x[4] = 0.0
    x[5, 40] = float("inf")
    prod = x[:, :224].float() * x[:, 224:].float()
    for fmt, ref in (("mxfp8", mxfp8_ref.to_mxfp8_ref), ("mxfp4", mxfp4_ref.to_mxfp4_ref)):
        s, q, y = MX.act_mx_ref(x, "none", False, fmt)
        ws, wq = ref(x)
        assert np.array_equal(s, ws.numpy()) and np.array_equal(q, wq.numpy()) and s.shape == (9, 14)
        assert torch.equal(y.view(torch.int32), x.float().view(torch.int32))
        assert s[3, 0] == 0xFF and (s[3, 1:] != 0xFF).all() and (s[4] == 0).all() and s[5, 1] == 254
        s, q, _ = MX.act_mx_ref(x, "none", True, fmt)
        ws, wq = ref(prod)
        assert s.shape == (9, 7) and q.shape == (9, 224 // (2 if fmt == "mxfp4" else 1))
        assert np.array_equal(s, ws.numpy()) and np.array_equal(q, wq.numpy())
        # the recipe's element step with the recipe's own exponents is the recipe
        assert np.array_equal(MX.requantize(x.float(), MX.act_mx_ref(x, "none", False, fmt)[0], fmt), MX.act_mx_ref(x, "none", False, fmt)[1])
    assert MX.to_mx_ref(torch.zeros(0, 64), "mxfp4")[1].shape == (0, 32) and MX.to_mx_ref(torch.zeros(3, 0), "mxfp8")[0].shape == (3, 0)


def test_window_finds_the_blocks_on_a_power_of_two():
    y = torch.zeros(1, 128)
    y[0, 0] = 28.0                                  # 28 / 448 = 2^-4 exactly: inside
    y[0, 32] = 28.0 * (1 + 2.0 ** -20)              # just above: inside; the RCEIL quirk keeps 2^-4 for the first ulps only
    y[0, 64] = 30.0                                 # far from a power of two
    inside, k = MX.window(y, "mxfp8")               # (block 3 is all zero: descale 0, never inside)
    assert inside.tolist() == [[True, True, False, False]] and k[0, 0] == -4 and k[0, 1] == -4
    lo, hi = MX.allowed_exponents(k)
    assert lo[0, 0] == 123 and hi[0, 0] == 124
    s, _ = MX.to_mx_ref(y, "mxfp8")
    assert s[0, 0] == 123 and s[0, 1] == 124 and s[0, 3] == 0
    # silu(28) is 28 to fp32: the example of a 16-bit input whose block sits on the power exactly
    assert float(torch.nn.functional.silu(torch.tensor(28.0, dtype=torch.float64)).float()) == 28.0


# ---- the condition of the GPU test's transcendental grid, on the reference alone ------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("act", MX.T_ACTS)
def test_excused_blocks_stay_under_their_cap_on_the_gpu_tests_inputs(act, dt):
    """For the seeds, shapes and dtypes tests/test_gpu_mx_fused.py uses: the blocks whose descale lies within 2^-18 of a power of two are at
    most max(1 block, 2 %) of every tensor's blocks - the inputs, not the kernel, leave that room."""
    worst = 0.0
    for gated in (False, True):
        for rows, cols, x in MX.t_inputs(act, gated, dt):
            y = MX.A.act_y(x, act, gated)
            for fmt in MX.FORMATS:
                inside, _ = MX.window(y, fmt)
                n, blocks = int(inside.sum()), inside.size
                worst = max(worst, n / blocks)
                print(f"[mx_fused window] {act} gated={gated} {dt} {fmt} {rows}x{cols}: {n} of {blocks} blocks inside ({n / blocks:.2%})")
                assert n <= max(1, MX.BLOCK_SHARE * blocks), (act, gated, dt, fmt, rows, cols, n, blocks)
    print(f"[mx_fused window] {act} {dt}: largest share {worst:.2%}")
