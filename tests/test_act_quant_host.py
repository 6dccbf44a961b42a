"""Fused activation + quantisation on the host (no GPU): argument validation of fp8mi_act_quantize through the built library (every check
runs before any HIP call), the op layer's keyword validation, the reference of tests/act_quant_ref.py against the references it builds
on, and the conditions tests/test_gpu_act_quant.py holds the transcendental activations to, checked on the CPU alone."""
import os
import re

import numpy as np
import pytest
import torch

import act_quant_ref as A
import blockwise_ref
import fp8_mi355x_lib as L
import rowwise_ref as R

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4, E5 = L.FMT_E4M3, L.FMT_E5M2
ROW, GROUP = L.QSCALE_ROW, L.QSCALE_GROUP128


@pytest.fixture(scope="module")
def lib():
    return L.load()


def call(lib, rows=4, cols=64, ld_in=None, act=L.ACT_SILU, ld_out=None, inp=P, out=P, scales=P, s_sr=1, s_sk=1, amax=None, dtype=L.BF16, smode=ROW,
         fmt=E4, mode=L.ENC_RNE):
    width = 2 * cols if act & L.ACT_GATED else cols
    return lib.fp8mi_act_quantize(inp, dtype, rows, cols, width if ld_in is None else ld_in, act, out, cols if ld_out is None else ld_out, scales, s_sr,
                                  s_sk, amax, smode, fmt, mode, None)


# ---- argument validation, through the built library --------------------------------------------------------------------------

def test_act_quantize_argument_errors_without_gpu(lib):
    err = lib.fp8mi_last_error
    for smode in (ROW, GROUP):
        assert call(lib, inp=None, smode=smode) == E_NULL and b"fp8mi_act_quantize" in err() and b"NULL" in err()
        assert call(lib, out=None, smode=smode) == E_NULL and call(lib, scales=None, smode=smode) == E_NULL
        assert call(lib, rows=-1, smode=smode) == E_SHAPE and b"negative" in err()
        assert call(lib, cols=-1, ld_in=0, ld_out=0, smode=smode) == E_SHAPE
        assert call(lib, ld_in=63, smode=smode) == E_SHAPE and b"leading dimension" in err()
        assert call(lib, ld_out=63, smode=smode) == E_SHAPE
        # gated: the input is 2 cols wide
        assert call(lib, act=L.ACT_SILU | L.ACT_GATED, ld_in=127, smode=smode) == E_SHAPE and b"2 cols" in err()
        assert call(lib, act=L.ACT_NONE | L.ACT_GATED, ld_in=64, smode=smode) == E_SHAPE
        assert call(lib, s_sr=-1, smode=smode) == E_SHAPE and b"stride" in err()
        assert call(lib, s_sk=-1, smode=smode) == E_SHAPE
        assert call(lib, act=4, smode=smode) == E_ENUM and b"act" in err()
        assert call(lib, act=-1, smode=smode) == E_ENUM and call(lib, act=0x200, smode=smode) == E_ENUM and call(lib, act=0x104, smode=smode) == E_ENUM
        assert call(lib, dtype=3, smode=smode) == E_ENUM and b"in_dtype" in err()
        assert call(lib, dtype=-1, smode=smode) == E_ENUM
        assert call(lib, fmt=2, smode=smode) == E_ENUM and b"out_format" in err()
        assert call(lib, mode=2, smode=smode) == E_ENUM and b"encode mode" in err()
        # rows == 0 is a no-op that accepts NULL pointers - but not bad enums or shapes
        assert call(lib, rows=0, inp=None, out=None, scales=None, smode=smode) == 0
        assert call(lib, rows=0, cols=0, inp=None, out=None, scales=None, act=L.ACT_GATED, smode=smode) == 0
        assert call(lib, rows=0, dtype=9, smode=smode) == E_ENUM and call(lib, rows=0, ld_in=1, smode=smode) == E_SHAPE
        assert call(lib, rows=0, act=77, smode=smode) == E_ENUM
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
    assert re.search(r"\bint\s+fp8mi_act_quantize\s*\(", hdr)
    assert len(L.SIGNATURES["fp8mi_act_quantize"][1]) == 16 and lib.fp8mi_act_quantize.argtypes == L.SIGNATURES["fp8mi_act_quantize"][1]
    for name, value in (("FP8MI_ACT_NONE", L.ACT_NONE), ("FP8MI_ACT_SILU", L.ACT_SILU), ("FP8MI_ACT_GELU_TANH", L.ACT_GELU_TANH),
                        ("FP8MI_ACT_GELU_ERF", L.ACT_GELU_ERF), ("FP8MI_QSCALE_ROW", L.QSCALE_ROW), ("FP8MI_QSCALE_GROUP128", L.QSCALE_GROUP128)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", hdr), name
    assert re.search(r"#define\s+FP8MI_ACT_GATED\s+0x100\b", hdr) and L.ACT_GATED == 0x100
    assert lib.fp8mi_version() == 0x000400   # a new entry point only: the ABI version does not move


def test_op_layer_exposes_the_ops_and_validates_keywords():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_act_quantize", "fp8_mlp_rowwise", "fp8_mlp_blockwise"):
        assert callable(getattr(N, name)) and getattr(alias, name) is getattr(N, name), name
    x = torch.zeros(4, 64)
    with pytest.raises(AssertionError, match="unknown act"):
        N.fp8_act_quantize(x, act="relu")
    with pytest.raises(AssertionError, match="unknown scale"):
        N.fp8_act_quantize(x, scale="tensor")
    with pytest.raises(AssertionError, match="out_format"):
        N.fp8_act_quantize(x, out_format=5)
    with pytest.raises(AssertionError, match="amax"):
        N.fp8_act_quantize(x, scale="block128", return_amax=True)
    with pytest.raises(AssertionError, match="even"):
        N.fp8_act_quantize(torch.zeros(4, 63), act="silu", gated=True)


# ---- the reference against the references it builds on -----------------------------------------------------------------------------

def _data(rng, rows, cols, dt):
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-8, 8, size=(rows, 1)))
    return torch.from_numpy(x.astype(np.float32)).to(dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_ref_none_modes_reduce_to_the_existing_references(dt):
    rng = np.random.default_rng(5)
    x = _data(rng, 9, 2 * 200, dt)
    x[3, 7] = float("nan")
    x[4] = 0.0
    for fmt, mode in ((E4, R.ENC_REFERENCE), (E4, R.ENC_RNE), (E5, R.ENC_RNE)):
        q, inv, amax = A.act_quantize_ref(x, "none", False, "row", fmt, mode)
        wq, wamax, winv = R.quantize_rowwise_ref(x, fmt, mode)
        assert np.array_equal(q, wq) and np.array_equal(inv.view(np.uint32), winv.view(np.uint32)) and np.array_equal(amax, wamax)
        prod = x[:, :200].float() * x[:, 200:].float()
        q, inv, amax = A.act_quantize_ref(x, "none", True, "row", fmt, mode)
        wq, wamax, winv = R.quantize_rowwise_ref(prod, fmt, mode)
        assert q.shape == (9, 200) and np.array_equal(q, wq) and np.array_equal(inv.view(np.uint32), winv.view(np.uint32))
    q, s, none = A.act_quantize_ref(x, "none", False, "block128", E4, R.ENC_RNE)
    wq, ws = blockwise_ref.quantize_blockwise_ref(x, 1)
    assert none is None and np.array_equal(q, wq.numpy()) and s.shape == (9, 4)
    assert np.array_equal(s.view(np.uint32), ws.numpy().view(np.uint32))
    assert np.isnan(s[3, 0]) and (q[3, :128] == 0x7F).all() and not np.isnan(s[3, 1:]).any() and s[4].tolist() == [1.0] * 4
    q, s, _ = A.act_quantize_ref(x, "none", True, "block128", E4, R.ENC_RNE)
    wq, ws = blockwise_ref.quantize_blockwise_ref(prod, 1)
    assert q.shape == (9, 200) and s.shape == (9, 2) and np.array_equal(q, wq.numpy())
    assert np.array_equal(s.view(np.uint32), ws.numpy().view(np.uint32))
    # 0 * inf in the gate product is a NaN element
    z = torch.tensor([[0.0, 1.0, float("inf"), 2.0]], dtype=dt)
    y = A.act_y(z, "none", True)
    assert torch.isnan(y[0, 0]) and y[0, 1] == 2.0


def test_ref_forms_agree_with_the_formulas_as_written_where_those_have_digits():
    g = torch.linspace(-4.0, 30.0, 20001, dtype=torch.float64)
    for act in ("silu", "gelu_tanh", "gelu_erf"):
        a, b = A.act64(g, act), A.literal64(g, act)
        rel = ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()
        assert rel < 1e-10, (act, rel)     # (1 + tanh, 1 + erf at g = -4 are about 1e-5: eleven digits left of float64's sixteen)
    # ... and where they have none: the formulas as written give -0 or noise, the reference the function's value
    far = torch.tensor([-9.0, -12.0], dtype=torch.float64)
    assert (A.literal64(far, "gelu_tanh") == 0).all() and (A.act64(far, "gelu_tanh")[0] < 0)
    assert abs(A.act64(far, "gelu_erf")[0].item() / (-9.0 * 1.1285884059538408e-19) - 1.0) < 1e-9    # -9 Phi(-9)


# ---- the conditions of the GPU test, on the CPU alone ------------------------------------------------------------------------------

def _f32_eval(x, act, gated):
    """an independent float32 evaluation of the same formulas with torch CPU ops"""
    xf = x.float()
    C = xf.shape[1] // 2 if gated else xf.shape[1]
    g = xf[:, :C]
    F = torch.nn.functional
    y = {"silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "gelu_erf": F.gelu}[act](g)
    return y * xf[:, C:] if gated else y


def conditions(q, s, wq, ws):
    """-> (share of bytes that differ, largest byte distance, largest relative scale distance)"""
    d = np.abs(q.astype(np.int32) - wq.astype(np.int32))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(s.astype(np.float64) - ws.astype(np.float64)) / np.abs(ws.astype(np.float64))
    rel = np.where(s.view(np.uint32) == ws.view(np.uint32), 0.0, rel)
    return float((d != 0).mean()), int(d.max()), float(rel.max())


@pytest.mark.parametrize("act", ["silu", "gelu_tanh", "gelu_erf"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_caps_hold_between_float64_and_float32_evaluations(act, dt):
    """The caps of the GPU test - at most 1e-3 of the bytes differ, each by 1, scales within 2^-18 - between the float64-derived
    reference and a float32 evaluation, and under a simulated +-16 ulp error of y: the inputs, not the kernel, keep the caps honest.
    (OCP rounding: under the reference encoder a y that underflowed to -0 is 0x00 and a tiny negative y 0x80, which no cap on |y| sees.)"""
    rng = np.random.default_rng(11)
    x = _data(rng, 64, 2 * 3072, dt)
    y64 = A.act_y(x, act, True)
    y32 = _f32_eval(x, act, True)
    # a relative error of up to 16 ulp (2^-23 each): zeros stay zeros, signs stay signs
    y16 = (y64.double() * (1.0 + torch.from_numpy(rng.integers(-16, 17, size=tuple(y64.shape))).double() * 2.0 ** -23)).float()
    for name, other in (("float32 evaluation", y32), ("+-16 ulp", y16)):
        for scale in ("row", "block128"):
            wq, ws, _ = A.act_quantize_ref(None, scale=scale, mode=R.ENC_RNE, y=y64)
            q, s, _ = A.act_quantize_ref(None, scale=scale, mode=R.ENC_RNE, y=other)
            share, dist, rel = conditions(q, s, wq, ws)
            print(f"[act_quant caps] {act} {dt} {scale} {name}: share {share:.2e} distance {dist} scales {rel:.2e}")
            assert share <= 1e-3 and dist <= 1 and rel <= 2.0 ** -18, (act, dt, scale, name, share, dist, rel)
