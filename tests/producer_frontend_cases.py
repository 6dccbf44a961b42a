"""What the fused producers and the dense layer ops do with their arguments, enumerated for tests/test_producer_frontend_host.py (no GPU):

  c_front_end(lib, L)  the return code of every faulty call of the 6 fused-producer entry points (fp8mi_act_quantize, fp8mi_norm_quantize,
                       fp8mi_moe_scatter_quantize and their *_mx forms; the MX forms once per mx_format): each single fault and each pair of a
                       per-entry list, on a small base call with fake aligned pointers (rows = 4, cols = 64; scatter: T = 4, k = 2); and, for
                       each single fault, whether fp8mi_last_error() begins with the entry point's name;
  op_layer(native)     the library calls (entry point and full argument tuple, in order), the results and the text of what is raised of
                       fp8_act_quantize, fp8_norm_quantize, fp8_moe_scatter_quantize and the sixteen dense layer ops (six fp8_linear*, five
                       fp8_mlp_*, five fp8_norm_linear_*), with the library replaced by gemm_frontend_cases' recorder.  The sequence of calls
                       per function is what shows that no launch was added, dropped or rerouted.

    python tests/producer_frontend_cases.py record [PACKAGE_DIR]
writes both as tests/golden/producer_frontend_{c,op}.json from the package in PACKAGE_DIR (default: this tree's).  The fixtures are the
behaviour of the commit BEFORE a change to the front end: record them there, then run the test on the change.

The pair rule: every two faults of an entry's list that set different arguments (a pair that sets the same argument is not a pair).  Three
empty inputs launch by design - cols = 0 with FP8MI_QSCALE_ROW in fp8mi_act_quantize, fp8mi_norm_quantize and fp8mi_moe_scatter_quantize
(every row publishes inv_scale = 1) - and are in no list here: where there is a GPU such a call would write through the fake pointer.  The
GPU suites cover them.  cols = 0 is listed for FP8MI_QSCALE_GROUP128 and the MX forms, which return 0 before they look at a pointer.  The
misaligned ld_out of the scatter forms is 68 where a piece is stored as 8 bytes (e4m3, MXFP8) and 34 for MXFP4, whose store is 4 bytes
wide (68 is a multiple of 4: that call is valid and would launch)."""
import itertools
import json
import os
import sys

from cast_frontend_cases import views
from gemm_frontend_cases import GOLDEN, P, recorder


# ---- the C front end ------------------------------------------------------------------------------------------------------------

def _entries(L):
    """-> {entry point: (argument order, {variant: (base arguments, {fault: overrides})})}; every call gets a NULL stream as its last argument"""
    ROW, GROUP, E4, E5, RNE, REF = L.QSCALE_ROW, L.QSCALE_GROUP128, L.FMT_E4M3, L.FMT_E5M2, L.ENC_RNE, L.ENC_REFERENCE
    null = lambda *names: {f"NULL {n}": {n: None} for n in names}   # noqa: E731
    sizes = {"negative rows": dict(rows=-1), "negative cols": dict(cols=-32), "rows = 0": dict(rows=0)}
    bad_in = {"bad in_dtype": dict(in_dtype=3)}
    strides = {"negative scale row stride": dict(s_sr=-1), "negative scale k stride": dict(s_sk=-1)}
    # what the e4m3 forms take behind q: float32 scales with two strides, the scale mode, the element format, the rounding
    e4m3_enums = {"bad scale_mode": dict(scale_mode=2), "bad out_format": dict(out_format=2), "bad encode_mode": dict(mode=2),
                  "negative encode_mode": dict(mode=-1)}
    group = {"GROUP128 with ENC_REFERENCE": dict(scale_mode=GROUP, mode=REF), "GROUP128, cols = 0": dict(scale_mode=GROUP, cols=0)}
    e4m3_pairs = {"e5m2 with ENC_REFERENCE": dict(out_format=E5, mode=REF), "GROUP128 with e5m2": dict(scale_mode=GROUP, out_format=E5),
                  "GROUP128 with an amax pointer": dict(scale_mode=GROUP, amax=P), **group}
    mx_width = {"cols = 0": dict(cols=0), "cols % 32": dict(cols=40), "cols = 48": dict(cols=48), "bad mx_format": dict(mx_format=2)}

    def mx_variants(base, faults, ld_out_small, extra=None):
        """the MX form of an entry point on both element formats: MXFP4 rows are cols / 2 bytes"""
        extra = extra or {}
        return {"mxfp8": (dict(base, mx_format=L.MX_FP8, ld_out=64, ld_s=2),
                          {**faults, **mx_width, "ld_out too small": dict(ld_out=63), "ld_s too small": dict(ld_s=1), **extra.get("mxfp8", {})}),
                "mxfp4": (dict(base, mx_format=L.MX_FP4, ld_out=32, ld_s=2),
                          {**faults, **mx_width, "ld_out too small": dict(ld_out=ld_out_small), "ld_s too small": dict(ld_s=1), **extra.get("mxfp4", {})})}

    act_base = dict({"in": P}, in_dtype=L.BF16, rows=4, cols=64, ld_in=64, act=L.ACT_SILU, out=P, scales=P, s_sr=1, s_sk=1, amax=None, scale_mode=ROW,
                    out_format=E4, mode=RNE)
    act_faults = {**sizes, **bad_in, **null("in", "out", "scales"), "ld_in too small": dict(ld_in=63),
                  "gated, ld_in too small": dict(act=L.ACT_SILU | L.ACT_GATED, ld_in=127), "bad act": dict(act=4), "bad act under the gate bit": dict(act=0x104)}

    gated_base = dict(act=L.ACT_SILU | L.ACT_GATED, ld_in=128)
    norm_base = dict({"in": P}, in_dtype=L.BF16, rows=4, cols=64, ld_in=64, norm=L.NORM_LAYER, eps=1e-6, weight=None, bias=None, mod_scale=None,
                     mod_shift=None, ld_mod=64, rows_per_mod=1, param_dtype=L.BF16, residual=None, ld_res=64, h_out=None, ld_h=64, out=P, scales=P,
                     s_sr=1, s_sk=1, amax=None, scale_mode=ROW, out_format=E4, mode=RNE, mean_out=None, rstd_out=None)
    mod, res = dict(mod_scale=P, mod_shift=P), dict(residual=P, h_out=P)
    norm_faults = {**sizes, **bad_in, **null("in", "out", "scales"), "ld_in too small": dict(ld_in=63), "ld_res too small": dict(res, ld_res=63),
                   "ld_h too small": dict(res, ld_h=63), "ld_mod too small": dict(mod, ld_mod=63), "rows_per_mod = 0": dict(mod, rows_per_mod=0),
                   "bad norm": dict(norm=2), "bad param_dtype": dict(param_dtype=3), "RMS with mean_out": dict(norm=L.NORM_RMS, mean_out=P),
                   "param_dtype neither in_dtype nor F32": dict(param_dtype=L.F16, weight=P), "mod_scale without mod_shift": dict(mod_scale=P, mod_shift=None),
                   "mod_shift without mod_scale": dict(mod_scale=None, mod_shift=P), "residual without h_out": dict(residual=P, h_out=None), "h_out without residual": dict(residual=None, h_out=P)}

    sc_base = dict({"in": P}, in_dtype=L.BF16, T=4, cols=64, ld_in=64, row_of=P, k=2, out=P, rows_out=8, scales=P, s_sr=1, s_sk=1, scale_mode=ROW,
                   out_format=E4, mode=RNE)
    wide = lambda cols, per_byte=1: dict(cols=cols, ld_in=cols, ld_out=cols // per_byte, ld_s=(cols + 31) // 32)   # noqa: E731
    sc_faults = {"negative T": dict(T=-1), "negative cols": dict(cols=-32), "negative k": dict(k=-1), "negative rows_out": dict(rows_out=-8),
                 "T = 0": dict(T=0), "k = 0": dict(k=0), **bad_in, **null("in", "row_of", "out", "scales"), "ld_in too small": dict(ld_in=63),
                 "in at P + 8": {"in": P + 8}, "out at P + 2": dict(out=P + 2), "row_of at P + 2": dict(row_of=P + 2), "ld_in of 136 bytes": dict(ld_in=68)}

    act_order = ("in", "in_dtype", "rows", "cols", "ld_in", "act", "out", "ld_out")
    norm_order = ("in", "in_dtype", "rows", "cols", "ld_in", "norm", "eps", "weight", "bias", "mod_scale", "mod_shift", "ld_mod", "rows_per_mod",
                  "param_dtype", "residual", "ld_res", "h_out", "ld_h", "out", "ld_out")
    sc_order = ("in", "in_dtype", "T", "cols", "ld_in", "row_of", "k", "out", "rows_out", "ld_out")
    e4m3_tail, mx_tail = ("scales", "s_sr", "s_sk", "amax", "scale_mode", "out_format", "mode"), ("scales", "ld_s", "mx_format")
    e4m3 = lambda base, faults: {"e4m3": (dict(base, ld_out=64), {**faults, "ld_out too small": dict(ld_out=63), **strides, **e4m3_enums})}   # noqa: E731
    gated = lambda variants: {f"{v}, gated": (dict(b, **gated_base), {k: f for k, f in fl.items() if "act" not in f})   # noqa: E731
                              for v, (b, fl) in variants.items()}
    act_e4m3, act_mx = e4m3(act_base, {**act_faults, **e4m3_pairs}), mx_variants(act_base, act_faults, 31)
    return {
        "fp8mi_act_quantize": (act_order + e4m3_tail, {**act_e4m3, **gated(act_e4m3)}),
        "fp8mi_act_quantize_mx": (act_order + mx_tail, {**act_mx, **gated(act_mx)}),
        "fp8mi_norm_quantize": (norm_order + e4m3_tail + ("mean_out", "rstd_out"), e4m3(norm_base, {**norm_faults, **e4m3_pairs})),
        "fp8mi_norm_quantize_mx": (norm_order + mx_tail + ("mean_out", "rstd_out"), mx_variants(norm_base, norm_faults, 31)),
        "fp8mi_moe_scatter_quantize": (sc_order + tuple(a for a in e4m3_tail if a != "amax"),
                                       e4m3(sc_base, {**sc_faults, **group, "e5m2": dict(out_format=E5), "cols % 16": dict(cols=40),
                                                      "cols = 16400": wide(16400), "ld_out = 68": dict(ld_out=68), "scales at P + 2": dict(scales=P + 2)})),
        "fp8mi_moe_scatter_quantize_mx": (sc_order + mx_tail, mx_variants(sc_base, sc_faults, 31, {
            "mxfp8": {"cols = 16400": wide(16400), "cols = 16416": wide(16416), "ld_out = 68": dict(ld_out=68)},
            "mxfp4": {"cols = 16400": wide(16400, 2), "cols = 16416": wide(16416, 2), "ld_out = 34": dict(ld_out=34)}})),
    }


def c_front_end(lib, L):
    """-> {entry point: {variant: {fault: [return code, whether the message it left begins with the entry point's name (None after a 0),
    {second fault: the return code of the pair}]}}}; a pair is filed under the fault that the list has first.  A pair whose faults set the same
    argument is not a pair and is left out.  Asserts, before anything is compared, that no case got as far as a launch (a HIP code, or 0 from
    anything but an empty problem): a test must never launch on P."""
    out = {}
    for entry, (order, variants) in _entries(L).items():
        out[entry] = {}

        def call(variant, name, base, over):
            args = {**base, **over}
            rc = getattr(lib, entry)(*(args[k] for k in order), None)
            empty = 0 in [args[k] for k in ("rows", "T", "k", "cols") if k in order]
            assert rc < 0 or (rc == 0 and empty), f"{entry}, {variant}: '{name}' reached a launch (returned {rc})"
            return rc

        for variant, (base, faults) in variants.items():
            filed = out[entry][variant] = {}
            for name, over in faults.items():
                rc = call(variant, name, base, over)
                filed[name] = [rc, lib.fp8mi_last_error().decode().startswith(entry + ":") if rc else None, {}]
            for (n1, o1), (n2, o2) in itertools.combinations(faults.items(), 2):
                if not set(o1) & set(o2):
                    filed[n1][2][n2] = call(variant, f"{n1} + {n2}", base, {**o1, **o2})
    return out


def count(entry_cases):
    """the calls recorded for one entry point"""
    return sum(1 + len(pairs) for faults in entry_cases.values() for _rc, _named, pairs in faults.values())


# ---- the op layer ---------------------------------------------------------------------------------------------------------------

DENSE = {  # recipe -> (linear, mlp, norm-linear: the functions' names; elements per weight byte; the weight scales of a (rows, K) weight)
    "tensor": ("fp8_linear", None, None, 1, lambda torch, rows, K: torch.ones(1)),
    "rowwise": ("fp8_linear_rowwise", "fp8_mlp_rowwise", "fp8_norm_linear_rowwise", 1, lambda torch, rows, K: torch.ones(rows)),
    "blockwise": ("fp8_linear_blockwise", "fp8_mlp_blockwise", "fp8_norm_linear_blockwise", 1,
                  lambda torch, rows, K: torch.ones((rows + 127) // 128, (K + 127) // 128)),
    "mxfp8": ("fp8_linear_mxfp8", "fp8_mlp_mxfp8", "fp8_norm_linear_mxfp8", 1, lambda torch, rows, K: torch.full((rows, K // 32), 127, dtype=torch.uint8)),
    "mxfp4": ("fp8_linear_mxfp4", "fp8_mlp_mxfp4", "fp8_norm_linear_mxfp4", 2, lambda torch, rows, K: torch.full((rows, K // 32), 127, dtype=torch.uint8)),
    "mxw4a8": ("fp8_linear_mxw4a8", "fp8_mlp_mxw4a8", "fp8_norm_linear_mxw4a8", 2, lambda torch, rows, K: torch.full((rows, K // 32), 127, dtype=torch.uint8)),
}


def op_layer(native):
    """-> {"function: case": what gemm_frontend_cases.recorder()'s run files} for the 19 functions"""
    import torch
    u8, f32, f16, bf16, f64, i32, i64 = torch.uint8, torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32, torch.int64
    E5 = torch.float8_e5m2
    L = native._l
    results = {}
    floats = lambda dt=f32: (lambda shape: torch.zeros(shape, dtype=dt))   # noqa: E731
    scales = ("row", "block128", "mxfp8", "mxfp4")

    with recorder(native) as run:
        def cases_of(fn, names=("x",)):
            def case(label, *args, **kw):
                assert f"{fn.__name__}: {label}" not in results, label
                run(results, f"{fn.__name__}: {label}", fn, *args, names=names, **kw)
                filed = results[f"{fn.__name__}: {label}"]
                if not filed["workspace_asked"]:
                    del filed["workspace_asked"]   # (filed only where a GEMM asked for the split-K workspace)
                result = filed.get("result")
                if fn.__name__.startswith("fp8_norm_linear") and result and isinstance(result[1], list):
                    # (y, h): the recorder places a result among the LAST call's arguments, and h is memory of the call before it
                    result[1][2] = "fresh"
            return case

        # fp8_act_quantize
        case = cases_of(native.fp8_act_quantize)
        x = torch.zeros(4, 64)
        for scale in scales:
            for gated in (False, True):
                for label, t in views(floats(), 128 if gated else 64).items():
                    case(f"{scale}{', gated' if gated else ''}, {label}", t, "silu", gated, scale)
            for dt in (bf16, i32):
                case(f"{scale}, {dt}", floats(dt)((4, 64)), scale=scale)
            case(f"{scale}, return_amax", x, scale=scale, return_amax=True)
            case(f"{scale}, e5m2", x, scale=scale, out_format=L.FMT_E5M2)
            case(f"{scale}, e5m2 with ENC_REFERENCE", x, scale=scale, out_format=L.FMT_E5M2, encode_mode=L.ENC_REFERENCE)
            case(f"{scale}, encode_mode ENC_REFERENCE", x, scale=scale, encode_mode=L.ENC_REFERENCE)
            case(f"{scale}, out_format 5", x, scale=scale, out_format=5)
            case(f"{scale}, an odd gated width", torch.zeros(4, 63), "silu", True, scale)
            case(f"{scale}, 48 columns", torch.zeros(4, 48), scale=scale)
            case(f"{scale}, 0-d", torch.zeros(()), scale=scale)
        for act in ("none", "gelu_tanh", "gelu_erf", "relu"):
            case(f"act {act}", x, act)
        case("3-D, return_amax", torch.zeros(2, 3, 64), return_amax=True)
        case("e5m2, return_amax", x, "none", False, "row", L.FMT_E5M2, None, True)
        case("encode_mode ENC_RNE", x, encode_mode=L.ENC_RNE)
        case("gated, 200 columns, float16", torch.zeros(3, 400, dtype=f16), "gelu_erf", True, "block128")
        case("scale tensor", x, scale="tensor")
        case("scale mxfp6", x, scale="mxfp6")

        # fp8_norm_quantize
        case = cases_of(native.fp8_norm_quantize)
        x, x3 = torch.zeros(4, 64, dtype=bf16), torch.zeros(2, 3, 64, dtype=bf16)
        w = lambda dt=bf16: torch.ones(64, dtype=dt)   # noqa: E731
        for scale, other in zip(scales, ("layer", "rms", "layer", "rms")):
            for norm in ("rms", "layer"):
                for label, t in views(floats(bf16)).items():
                    case(f"{scale}, {norm}, {label}", t, norm, scale=scale)
            norm = other   # the parameters: on one of the two normalisations per scale
            case(f"{scale}, {norm}, weight and bias, eps", x, norm, weight=w(), bias=w(), eps=1e-5, scale=scale)
            case(f"{scale}, {norm}, float32 parameters", x, norm, weight=w(f32), bias=w(f32), scale=scale)
            case(f"{scale}, {norm}, 3-D, residual", x3, norm, weight=w(), residual=torch.zeros(2, 3, 64, dtype=bf16), scale=scale)
            case(f"{scale}, {norm}, residual a column slab", x, norm, residual=torch.zeros(4, 128, dtype=bf16)[:, 64:], scale=scale)
            case(f"{scale}, {norm}, modulation (B, C)", x3, norm, mod_scale=torch.zeros(2, 64, dtype=bf16), mod_shift=torch.zeros(2, 64, dtype=bf16),
                 scale=scale)
            case(f"{scale}, {norm}, modulation (B, 1, C), float32", x3, norm, weight=w(f32), mod_scale=torch.zeros(2, 1, 64),
                 mod_shift=torch.zeros(2, 1, 64), scale=scale)
            case(f"{scale}, {norm}, modulation, zero rows", torch.zeros(0, 3, 64, dtype=bf16), norm, mod_scale=torch.zeros(0, 64, dtype=bf16),
                 mod_shift=torch.zeros(0, 64, dtype=bf16), scale=scale)
            case(f"{scale}, rms, return_stats", x, "rms", scale=scale, return_stats=True)
            case(f"{scale}, layer, 3-D, residual, return_stats", x3, "layer", residual=torch.zeros(2, 3, 64, dtype=bf16), scale=scale, return_stats=True)
            case(f"{scale}, float32", torch.zeros(4, 64), scale=scale)
            case(f"{scale}, e5m2", x, scale=scale, out_format=L.FMT_E5M2)
            case(f"{scale}, e5m2 with ENC_REFERENCE", x, scale=scale, out_format=L.FMT_E5M2, encode_mode=L.ENC_REFERENCE)
            case(f"{scale}, encode_mode ENC_REFERENCE", x, scale=scale, encode_mode=L.ENC_REFERENCE)
            case(f"{scale}, out_format 5", x, scale=scale, out_format=5)
            case(f"{scale}, 48 columns", torch.zeros(4, 48, dtype=bf16), scale=scale)
            case(f"{scale}, 0-d", torch.zeros((), dtype=bf16), scale=scale)
        case("int32", torch.zeros(4, 64, dtype=i32))
        case("encode_mode ENC_RNE", x, encode_mode=L.ENC_RNE)
        case("200 columns", torch.zeros(3, 200, dtype=f16), scale="block128")
        case("modulation on 2-D x", x, mod_scale=torch.zeros(4, 64, dtype=bf16), mod_shift=torch.zeros(4, 64, dtype=bf16))
        case("norm batch", x, "batch")
        case("mod_scale without mod_shift", x, mod_scale=torch.zeros(4, 64, dtype=bf16))
        case("parameters of two dtypes", x, weight=torch.ones(64, dtype=bf16), bias=torch.ones(64))
        case("float16 parameters with bfloat16 x", x, weight=torch.ones(64, dtype=f16))
        case("weight of the wrong shape", x, weight=torch.ones(63, dtype=bf16))
        case("bias of the wrong shape", x, bias=torch.ones(1, 64, dtype=bf16))
        case("modulation on 1-D x", torch.zeros(64, dtype=bf16), mod_scale=torch.zeros(1, 64, dtype=bf16), mod_shift=torch.zeros(1, 64, dtype=bf16))
        case("modulation of the wrong shape", x3, mod_scale=torch.zeros(6, 64, dtype=bf16), mod_shift=torch.zeros(6, 64, dtype=bf16))
        case("residual of the wrong shape", x, residual=torch.zeros(64, 4, dtype=bf16))
        case("residual of the wrong dtype", x, residual=torch.zeros(4, 64))
        case("scale tensor", x, scale="tensor")

        # fp8_moe_scatter_quantize
        case = cases_of(native.fp8_moe_scatter_quantize, ("x", "row_of"))
        plan = lambda T=4, k=2, dt=i32: torch.zeros(T, k, dtype=dt)   # noqa: E731
        x = torch.zeros(4, 64, dtype=bf16)
        for scale in scales:
            case(f"{scale}, plain", x, plan(), scale)
            case(f"{scale}, float64", torch.zeros(4, 64, dtype=f64), plan(), scale)
            case(f"{scale}, T = 0", torch.zeros(0, 64, dtype=bf16), plan(0), scale)
            case(f"{scale}, k = 1", x, plan(4, 1), scale)
            case(f"{scale}, k = 0", x, plan(4, 0), scale)
            case(f"{scale}, a column slab of a wider buffer", torch.zeros(4, 128, dtype=bf16)[:, 64:], plan(), scale)
            case(f"{scale}, zero columns", torch.zeros(4, 0, dtype=bf16), plan(), scale)
            case(f"{scale}, 48 columns", torch.zeros(4, 48, dtype=bf16), plan(), scale)
            case(f"{scale}, row_of int64, a transposed view", x, torch.zeros(2, 4, dtype=i64).t(), scale)
            case(f"{scale}, row_of of the wrong length", x, plan(5), scale)
            case(f"{scale}, row_of 1-D", x, torch.zeros(8, dtype=i32), scale)
            case(f"{scale}, encode_mode ENC_RNE", x, plan(), scale, L.ENC_RNE)
            case(f"{scale}, encode_mode ENC_REFERENCE", x, plan(), scale, encode_mode=L.ENC_REFERENCE)
        case("a transposed view", torch.zeros(64, 4, dtype=bf16).t(), plan())
        case("x 3-D", torch.zeros(2, 2, 64, dtype=bf16), plan())
        case("scale tensor", x, plan(), "tensor")

        # the sixteen dense layer ops: K = 64, N = 32, MLP hidden 32 (a gated w1 has 64 rows)
        K, N, H = 64, 32, 32
        xs = {"plain": torch.zeros(4, K, dtype=bf16), "3-D, float32": torch.zeros(2, 3, K), "zero rows": torch.zeros(0, K, dtype=bf16),
              "a column slab of a wider buffer": torch.zeros(4, 2 * K, dtype=bf16)[:, K:], "int32": torch.zeros(4, K, dtype=i32)}
        x, x3 = xs["plain"], xs["3-D, float32"]
        for recipe, (linear, mlp, norm_linear, per_byte, w_scales) in DENSE.items():
            weight = lambda rows, k: (torch.zeros(rows, k // per_byte, dtype=u8), w_scales(torch, rows, k))   # noqa: E731
            e5m2 = recipe in ("tensor", "rowwise")

            w, ws = weight(N, K)
            case = cases_of(getattr(native, linear), ("x", "w", "w_scales"))
            for label, t in xs.items():
                case(label, t, w, ws)
            case("3-D, bias, out_dtype", x3, w, ws, bias=torch.zeros(N), out_dtype=f16)
            case("the wrong feature count for x", torch.zeros(4, K + 32, dtype=bf16), w, ws)
            case("a 3-D weight", x, w[None], ws)
            case("a float32 weight", x, w.float(), ws)   # (where each function looks at the weight's type: before or behind its first launch)
            if e5m2:
                case("an e5m2 weight", x, w.view(E5), ws)
                case("weight_format FMT_E5M2", x, w, ws, weight_format=L.FMT_E5M2)

            if mlp is not None:
                case = cases_of(getattr(native, mlp), ("x", "w1", "w1_scales", "w2", "w2_scales"))
                (w1, w1s), (w1u, w1us), (w2, w2s) = weight(2 * H, K), weight(H, K), weight(N, H)
                for label, t in xs.items():
                    case(label, t, w1, w1s, w2, w2s)
                case("3-D, biases, out_dtype", x3, w1, w1s, w2, w2s, bias1=torch.zeros(2 * H), bias2=torch.zeros(N), out_dtype=f16)
                case("ungated, gelu_tanh, bias1 alone", x, w1u, w1us, w2, w2s, "gelu_tanh", False, bias1=torch.zeros(H, dtype=bf16))
                case("act relu", x, w1, w1s, w2, w2s, "relu")
                case("the wrong feature count for x", torch.zeros(4, K + 32, dtype=bf16), w1, w1s, w2, w2s)
                case("the wrong feature count for w2", x, w1, w1s, *weight(N, 2 * H))
                case("a 3-D w2", x, w1, w1s, w2[None], w2s)
                case("a float32 w1", x, w1.float(), w1s, w2, w2s)
                case("a float32 w2", x, w1, w1s, w2.float(), w2s)
                if e5m2:
                    case("e5m2 weights", x, w1.view(E5), w1s, w2.view(E5), w2s)

            if norm_linear is not None:
                case = cases_of(getattr(native, norm_linear), ("x", "w", "w_scales"))
                for label, t in xs.items():
                    case(label, t, w, ws)
                case("3-D, layer, parameters, bias, out_dtype", x3, w, ws, "layer", weight=torch.ones(K), norm_bias=torch.ones(K), eps=1e-5,
                     bias=torch.zeros(N), out_dtype=f16)
                case("residual", x, w, ws, residual=torch.zeros(4, K, dtype=bf16))
                case("3-D, modulation, residual, bias", x3, w, ws, "layer", residual=torch.zeros(2, 3, K), mod_scale=torch.zeros(2, K),
                     mod_shift=torch.zeros(2, 1, K), bias=torch.zeros(N))
                case("the wrong feature count for x", torch.zeros(4, K + 32, dtype=bf16), w, ws)
                case("a 3-D weight", x, w[None], ws)
                case("a float32 weight", x, w.float(), ws)
                if e5m2:
                    case("an e5m2 weight", x, w.view(E5), ws)
    return results


def compact(data, depth):
    """JSON text with one line per value `depth` levels down (a case of the op layer; a fault with its pairs in the C front end), keys sorted:
    what json.load reads is what json.dump(data) would have written"""
    def text(value, level):
        if level == depth:
            return json.dumps(value, sort_keys=True)
        return "{\n" + ",\n".join(f"{json.dumps(k)}: {text(value[k], level + 1)}" for k in sorted(value)) + "\n}"
    return text(data, 0) + "\n"


if __name__ == "__main__":
    assert len(sys.argv) >= 2 and sys.argv[1] == "record", __doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "fp8-mps-metal_amd"))
    import fp8_mi355x_lib
    import fp8_mi355x_native
    for name, data in (("c", c_front_end(fp8_mi355x_lib.load(), fp8_mi355x_lib)), ("op", op_layer(fp8_mi355x_native))):
        with open(os.path.join(GOLDEN, f"producer_frontend_{name}.json"), "w") as f:
            f.write(compact(data, 3 if name == "c" else 1))
        print(f"producer_frontend_{name}.json: {sum(count(v) for v in data.values()) if name == 'c' else len(data)} cases")
