"""Fused normalisation + quantisation on the host (no GPU): argument validation of fp8mi_norm_quantize through the built library (every
check runs before any HIP call), the binding, the op layer's keyword validation, the reference of tests/norm_quant_ref.py against torch's
own layer_norm / rms_norm, and the statistics caps tests/test_gpu_norm_quant.py holds the kernel to, checked on the CPU alone."""
import os
import re

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import norm_quant_ref as NR

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4, E5 = L.FMT_E4M3, L.FMT_E5M2
ROW, GROUP = L.QSCALE_ROW, L.QSCALE_GROUP128
N_ARGS = 30   # the flat argument list of include/fp8mi.h (the issue's own list, counted: 30)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def call(lib, rows=4, cols=64, ld_in=None, norm=L.NORM_LAYER, eps=1e-6, weight=None, bias=None, mod_scale=None, mod_shift=None, ld_mod=None,
         rows_per_mod=1, pdtype=None, residual=None, ld_res=None, h_out=None, ld_h=None, inp=P, out=P, ld_out=None, scales=P, s_sr=1, s_sk=1,
         amax=None, smode=ROW, fmt=E4, mode=L.ENC_RNE, mean=None, rstd=None, dtype=L.BF16):
    d = lambda v: cols if v is None else v   # noqa: E731
    return lib.fp8mi_norm_quantize(inp, dtype, rows, cols, d(ld_in), norm, eps, weight, bias, mod_scale, mod_shift, d(ld_mod), rows_per_mod,
                                   dtype if pdtype is None else pdtype, residual, d(ld_res), h_out, d(ld_h), out, d(ld_out), scales, s_sr, s_sk, amax,
                                   smode, fmt, mode, mean, rstd, None)


# ---- argument validation, through the built library --------------------------------------------------------------------------

def test_norm_quantize_argument_errors_without_gpu(lib):
    err = lib.fp8mi_last_error
    for smode in (ROW, GROUP):
        for norm in (L.NORM_RMS, L.NORM_LAYER):
            kw = dict(smode=smode, norm=norm)
            assert call(lib, inp=None, **kw) == E_NULL and b"fp8mi_norm_quantize" in err() and b"NULL" in err()
            assert call(lib, out=None, **kw) == E_NULL and call(lib, scales=None, **kw) == E_NULL
            # one of a pair missing
            assert call(lib, mod_scale=P, **kw) == E_NULL and b"mod_scale and mod_shift" in err()
            assert call(lib, mod_shift=P, **kw) == E_NULL
            assert call(lib, residual=P, **kw) == E_NULL and b"h_out" in err()
            assert call(lib, h_out=P, **kw) == E_NULL
            assert call(lib, rows=-1, **kw) == E_SHAPE and b"negative" in err()
            assert call(lib, cols=-1, **kw) == E_SHAPE
            assert call(lib, ld_in=63, **kw) == E_SHAPE and b"leading dimension" in err()
            assert call(lib, ld_out=63, **kw) == E_SHAPE
            assert call(lib, residual=P, h_out=P, ld_res=63, **kw) == E_SHAPE and call(lib, residual=P, h_out=P, ld_h=63, **kw) == E_SHAPE
            assert call(lib, mod_scale=P, mod_shift=P, ld_mod=63, **kw) == E_SHAPE
            assert call(lib, rows=0, ld_res=0, ld_h=0, ld_mod=0, **kw) == 0   # the leading dimensions of absent arrays are not looked at
            assert call(lib, mod_scale=P, mod_shift=P, rows_per_mod=0, **kw) == E_SHAPE and b"rows_per_mod" in err()
            assert call(lib, mod_scale=P, mod_shift=P, rows_per_mod=-3, **kw) == E_SHAPE
            assert call(lib, s_sr=-1, **kw) == E_SHAPE and b"stride" in err()
            assert call(lib, s_sk=-1, **kw) == E_SHAPE
            assert call(lib, dtype=3, pdtype=L.F32, **kw) == E_ENUM and b"in_dtype" in err()
            assert call(lib, dtype=-1, pdtype=L.F32, **kw) == E_ENUM
            assert call(lib, pdtype=3, **kw) == E_ENUM and b"param_dtype" in err()
            assert call(lib, fmt=2, **kw) == E_ENUM and b"out_format" in err()
            assert call(lib, mode=2, **kw) == E_ENUM and b"encode mode" in err()
            # one param_dtype: the input's or fp32
            assert call(lib, dtype=L.BF16, pdtype=L.F16, weight=P, **kw) == E_UNSUPPORTED and b"param_dtype" in err()
            assert call(lib, dtype=L.F32, pdtype=L.BF16, **kw) == E_UNSUPPORTED
            # rows == 0 is a no-op that accepts NULL pointers - but not bad enums or shapes
            assert call(lib, rows=0, inp=None, out=None, scales=None, **kw) == 0
            assert call(lib, rows=0, inp=None, out=None, scales=None, residual=P, mod_shift=P, **kw) == 0
            assert call(lib, rows=0, dtype=9, **kw) == E_ENUM and call(lib, rows=0, ld_in=1, **kw) == E_SHAPE
        assert call(lib, norm=2, smode=smode) == E_ENUM and b"norm" in err()
        assert call(lib, norm=-1, smode=smode) == E_ENUM and call(lib, rows=0, norm=7, smode=smode) == E_ENUM
        # the mean belongs to LayerNorm
        assert call(lib, norm=L.NORM_RMS, mean=P, smode=smode) == E_UNSUPPORTED and b"mean" in err()
        assert call(lib, norm=L.NORM_RMS, rows=0, mean=P, smode=smode) == E_UNSUPPORTED
    assert call(lib, smode=2) == E_ENUM and b"scale_mode" in err()
    assert call(lib, smode=-1) == E_ENUM
    # one scale per row: e4m3 with either encode mode, e5m2 with OCP rounding only; the scales are still written for empty rows
    assert call(lib, fmt=E5, mode=L.ENC_REFERENCE) == E_UNSUPPORTED and b"OCP" in err()
    assert call(lib, rows=0, fmt=E5, mode=L.ENC_REFERENCE) == E_UNSUPPORTED
    assert call(lib, cols=0, inp=None, out=None, scales=None) == E_NULL
    # one scale per 128 columns: e4m3 / RNE only, no amax output; nothing to write for empty rows
    assert call(lib, smode=GROUP, mode=L.ENC_REFERENCE) == E_UNSUPPORTED and b"GROUP128" in err()
    assert call(lib, smode=GROUP, fmt=E5) == E_UNSUPPORTED
    assert call(lib, smode=GROUP, amax=P) == E_UNSUPPORTED and b"amax" in err()
    assert call(lib, smode=GROUP, rows=0, amax=P) == E_UNSUPPORTED
    assert call(lib, smode=GROUP, cols=0, inp=None, out=None, scales=None) == 0


def test_new_symbol_is_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    m = re.search(r"\bint\s+fp8mi_norm_quantize\s*\((.*?)\);", hdr, flags=re.S)
    assert m
    declared = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    sig = L.SIGNATURES["fp8mi_norm_quantize"][1]
    assert len(declared) == N_ARGS and len(sig) == N_ARGS and lib.fp8mi_norm_quantize.argtypes == sig
    import ctypes
    assert sig[6] is ctypes.c_float and "float eps" in declared[6]
    for name, value in (("FP8MI_NORM_RMS", L.NORM_RMS), ("FP8MI_NORM_LAYER", L.NORM_LAYER)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", hdr), name
    assert lib.fp8mi_version() == 0x000400   # a new entry point only: the ABI version does not move


def test_op_layer_exposes_the_ops_and_validates_keywords():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_norm_quantize", "fp8_norm_linear_rowwise", "fp8_norm_linear_blockwise"):
        assert callable(getattr(N, name)) and getattr(alias, name) is getattr(N, name), name
    x = torch.zeros(4, 64)
    with pytest.raises(AssertionError, match="unknown norm"):
        N.fp8_norm_quantize(x, norm="group")
    with pytest.raises(AssertionError, match="unknown scale"):
        N.fp8_norm_quantize(x, scale="tensor")
    with pytest.raises(AssertionError, match="out_format"):
        N.fp8_norm_quantize(x, out_format=5)
    with pytest.raises(AssertionError, match="come together"):
        N.fp8_norm_quantize(x, mod_scale=torch.zeros(4, 64))


# ---- the reference against torch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_ref_with_its_own_statistics_agrees_with_torch_in_float64(dt):
    rng = np.random.default_rng(3)
    F = torch.nn.functional
    for rows, cols in ((9, 200), (4, 3072), (5, 2)):
        for layer in (False, True):
            x = NR.make_rows(rng, rows, cols, dt, layer)
            w, b = NR.make_params(rng, 1, cols, dt, 1.0)[0], NR.make_params(rng, 1, cols, dt)[0]
            sc, sh = NR.make_params(rng, 3, cols, dt), NR.make_params(rng, 3, cols, dt)
            x64, w64, b64 = x.double(), w.double(), b.double()
            eps = float(np.float32(1e-5))
            for kw, want in ((dict(), lambda n: n), (dict(weight=w), lambda n: n * w64), (dict(weight=w, bias=b), lambda n: n * w64 + b64),
                             (dict(mod_scale=sc, mod_shift=sh, rows_per_mod=4),
                              lambda n: n * (1.0 + sc.double()[torch.arange(rows) // 4]) + sh.double()[torch.arange(rows) // 4])):
                y, _, _ = NR.norm_y(x, "layer" if layer else "rms", eps=eps, **kw)
                n64 = F.layer_norm(x64, (cols,), eps=eps) if layer else F.rms_norm(x64, (cols,), eps=eps)
                w64y = want(n64).numpy()
                rel = np.abs(y.astype(np.float64) - w64y).max() / np.abs(w64y).max()
                # every one of the chain's five float32 roundings is below 2^-24 of the row's largest value; the centring of LayerNorm
                # in float32 adds 2^-24 of up to nine standard deviations
                assert rel <= 1e-6, (dt, rows, cols, layer, sorted(kw), rel)


def test_ref_with_residual_is_the_ref_on_torchs_sum():
    rng = np.random.default_rng(4)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x, res = NR.make_rows(rng, 7, 300, dt, True), NR.make_rows(rng, 7, 300, dt)
        w = NR.make_params(rng, 1, 300, dt, 1.0)[0]
        for norm in ("rms", "layer"):
            for scale, fmt, mode in (("row", E4, L.ENC_REFERENCE), ("row", E5, L.ENC_RNE), ("block128", E4, L.ENC_RNE)):
                (q, s, _), y, stored = NR.norm_quantize_ref(x, norm, weight=w, residual=res, scale=scale, fmt=fmt, mode=mode)
                summed = x + res
                (wq, ws, _), wy, none = NR.norm_quantize_ref(summed, norm, weight=w, scale=scale, fmt=fmt, mode=mode)
                assert none is None and stored.dtype == dt and torch.equal(stored.view(torch.uint8), summed.view(torch.uint8))
                assert np.array_equal(q, wq) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(y.view(np.uint32), wy.view(np.uint32))


def test_ref_pins_generated_nans_and_leaves_operand_nans():
    x = torch.tensor([[1.0, float("inf"), -2.0, 0.5], [1.0, 2.0, 3.0, 4.0]])
    y, _, _ = NR.norm_y(x, "rms")                                   # ms = inf, rstd = 0: finite elements 0, inf * 0 a generated NaN
    assert y[0, [0, 2, 3]].tolist() == [0.0, -0.0, 0.0] and y[0:1, 1].view(np.uint32)[0] == 0xFFC00000 and np.isfinite(y[1]).all()
    pos = np.array([0x7FC00001], np.uint32).view(np.float32)
    y, _, _ = NR.norm_y(x, "rms", rstd=np.array([pos[0], 1.0], np.float32))
    assert np.isnan(y[0]).all() and (y[0].view(np.uint32) >> 31 == 0).all()   # the statistic's own NaN, sign kept


# ---- the statistics caps of the GPU test, on the CPU alone -------------------------------------------------------------------------

@pytest.mark.parametrize("norm", ["rms", "layer"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_statistics_caps_hold_for_lane_ordered_float32_sums(norm, dt):
    """The GPU test's generator and shapes; float32 sums as 64 strided partial sums followed by a sequential sum stay within a QUARTER of
    the caps (a failure here is the generator's, never the cap's)."""
    import test_gpu_norm_quant as G
    eps = 1e-6
    for cols in G.COLS:
        worst = [0.0, 0.0]
        for rows in G.ROWS:
            rng = np.random.default_rng(G.seed(norm, dt, cols, rows))
            h = NR.widen(NR.make_rows(rng, rows, cols, dt, norm == "layer"))
            mean, rstd = NR.stats32(h, norm, eps)
            mr, rr = NR.stat_ratios(h, norm, eps, mean, rstd)
            worst = [max(worst[0], mr), max(worst[1], rr)]
        print(f"[norm_quant caps] {norm} {dt} cols {cols}: mean at {worst[0]:.3f} of its cap, rstd at {worst[1]:.3f}")
        assert worst[0] <= 0.25 and worst[1] <= 0.25, (norm, dt, cols, worst)
