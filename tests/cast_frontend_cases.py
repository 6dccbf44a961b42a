"""What the stand-alone casts and quantisers do with their arguments, enumerated for tests/test_cast_frontend_host.py (no GPU):

  c_front_end(lib, L)  the return code of every faulty call of the 16 cast entry points (fp8mi_dequant and its alias fp8mi_dequant_f16,
                       fp8mi_encode, fp8mi_amax, fp8mi_quantize, the three *_e5m2, and the quantise / dequant pairs of MXFP8, MXFP4, blockwise and rowwise): each single
                       fault and each pair of a per-entry list, on a small base call with fake aligned pointers; and, for each single fault,
                       whether fp8mi_last_error() begins with the name the entry point reports under;
  op_layer(native)     the entry point and the full argument tuple that the 15 fp8_* cast functions of fp8_mi355x_native hand to the library,
                       their results and the text of what they raise, with the library replaced by gemm_frontend_cases' recorder.

    python tests/cast_frontend_cases.py record [PACKAGE_DIR]
writes both as tests/golden/cast_frontend_{c,op}.json from the package in PACKAGE_DIR (default: this tree's).  The fixtures are the
behaviour of the commit BEFORE a change to the front end: record them there, then run the test on the change.

Four empty inputs launch by design - fp8mi_amax, fp8mi_quantize and fp8mi_quantize_e5m2 with count = 0 (they publish amax = 0 and
inv_scale = 1), fp8mi_quantize_rowwise with cols = 0 (the same, per row) - and are in no list here: where there is a GPU such a call
would write through the fake pointer.  The GPU suites cover them."""
import itertools
import json
import os
import sys

from gemm_frontend_cases import GOLDEN, P, recorder


# ---- the C front end ------------------------------------------------------------------------------------------------------------

def _entries(L):
    """-> {entry point: (the name its messages begin with, argument order, base arguments, {fault: overrides})}; every call gets a NULL
    stream as its last argument"""
    neg_count, no_count = {"negative count": dict(count=-1)}, {"count = 0": dict(count=0)}
    null = lambda *names: {f"NULL {n}": {n: None} for n in names}   # noqa: E731
    bad_in, bad_out = {"bad in_dtype": dict(in_dtype=3)}, {"bad out_dtype": dict(out_dtype=-1)}
    bad_mode = {"bad encode_mode": dict(mode=2), "negative encode_mode": dict(mode=-1)}
    sizes = {"negative rows": dict(rows=-1), "negative cols": dict(cols=-32), "rows = 0": dict(rows=0)}
    no_cols = {"cols = 0": dict(cols=0)}
    ld = lambda **small: {f"{n} too small": {n: v} for n, v in small.items()}   # noqa: E731
    bad_block = {"bad block_rows": dict(block_rows=64), "block_rows = 0": dict(block_rows=0)}
    neg_strides = {"negative scale row stride": dict(s_sr=-1), "negative scale k stride": dict(s_sk=-1)}

    flat_dq = ("in", "out", "scale", "count", "out_dtype")
    flat_dq_base = dict({"in": P}, out=P, scale=P, count=64, out_dtype=L.F16)
    flat_dq_faults = {**neg_count, **no_count, **null("in", "out"), **bad_out}
    enc_base = dict({"in": P}, in_dtype=L.F32, out=P, prescale=P, scales=P, count=64, mode=L.ENC_RNE)
    two_d = dict({"in": P}, in_dtype=L.F32, out_dtype=L.F32, rows=4, cols=64, ld_in=64, out=P, ld_out=64, scales=P, ld_s=2, block_rows=1, s_sr=1,
                 s_sk=1, amax=P, out_format=L.FMT_E4M3, in_format=L.FMT_E4M3, mode=L.ENC_RNE)
    mx_q = ("in", "in_dtype", "rows", "cols", "ld_in", "out", "ld_out", "scales", "ld_s")
    mx_dq = ("in", "rows", "cols", "ld_in", "scales", "ld_s", "out", "out_dtype")
    mx_q_faults = {**sizes, **no_cols, **null("in", "out", "scales"), **bad_in, "cols % 32": dict(cols=48)}
    mx_dq_faults = {**sizes, **no_cols, **null("in", "scales", "out"), **bad_out}
    return {
        "fp8mi_dequant": ("fp8mi_dequant", flat_dq, flat_dq_base, flat_dq_faults),
        "fp8mi_dequant_f16": ("fp8mi_dequant", flat_dq, flat_dq_base, flat_dq_faults),   # the alias reports under the one name
        "fp8mi_encode": ("fp8mi_encode", ("in", "in_dtype", "out", "prescale", "count", "mode"), enc_base,
                         {**neg_count, **no_count, **null("in", "out"), **bad_in, **bad_mode}),
        "fp8mi_amax": ("fp8mi_amax", ("in", "in_dtype", "out", "count"), enc_base, {**neg_count, **null("in", "out"), **bad_in}),
        "fp8mi_quantize": ("fp8mi_quantize", ("in", "in_dtype", "out", "scales", "count", "mode"), enc_base,
                           {**neg_count, **null("in", "out", "scales"), **bad_in, **bad_mode}),
        "fp8mi_encode_e5m2": ("fp8mi_encode_e5m2", ("in", "in_dtype", "out", "prescale", "count"), enc_base,
                              {**neg_count, **no_count, **null("in", "out"), **bad_in}),
        "fp8mi_dequant_e5m2": ("fp8mi_dequant_e5m2", flat_dq, flat_dq_base, flat_dq_faults),
        "fp8mi_quantize_e5m2": ("fp8mi_quantize_e5m2", ("in", "in_dtype", "out", "scales", "count"), enc_base,
                                {**neg_count, **null("in", "out", "scales"), **bad_in}),
        "fp8mi_quantize_mxfp8": ("fp8mi_quantize_mxfp8", mx_q, two_d, {**mx_q_faults, **ld(ld_in=63, ld_out=63, ld_s=1)}),
        "fp8mi_dequant_mxfp8": ("fp8mi_dequant_mxfp8", mx_dq, two_d, {**mx_dq_faults, **ld(ld_in=63, ld_s=1)}),
        "fp8mi_quantize_mxfp4": ("fp8mi_quantize_mxfp4", mx_q, dict(two_d, ld_out=32), {**mx_q_faults, **ld(ld_in=63, ld_out=31, ld_s=1)}),
        "fp8mi_dequant_mxfp4": ("fp8mi_dequant_mxfp4", mx_dq, dict(two_d, ld_in=32), {**mx_dq_faults, **ld(ld_in=31, ld_s=1), "odd cols": dict(cols=63)}),
        "fp8mi_quantize_blockwise": ("fp8mi_quantize_blockwise",
                                     ("in", "in_dtype", "rows", "cols", "ld_in", "block_rows", "out", "ld_out", "scales", "s_sr", "s_sk"), two_d,
                                     {**sizes, **no_cols, **null("in", "out", "scales"), **bad_in, **bad_block, **ld(ld_in=63, ld_out=63), **neg_strides}),
        "fp8mi_dequant_blockwise": ("fp8mi_dequant_blockwise", ("in", "rows", "cols", "ld_in", "block_rows", "scales", "s_sr", "s_sk", "out", "out_dtype"),
                                    two_d, {**sizes, **no_cols, **null("in", "scales", "out"), **bad_out, **bad_block, **ld(ld_in=63), **neg_strides}),
        "fp8mi_quantize_rowwise": ("fp8mi_quantize_rowwise",
                                   ("in", "in_dtype", "rows", "cols", "ld_in", "out", "ld_out", "scales", "amax", "out_format", "mode"), two_d,
                                   {**sizes, **null("in", "out", "scales"), **bad_in, **bad_mode, **ld(ld_in=63, ld_out=63),
                                    "bad out_format": dict(out_format=2), "e5m2 with ENC_REFERENCE": dict(out_format=L.FMT_E5M2, mode=L.ENC_REFERENCE)}),
        "fp8mi_dequant_rowwise": ("fp8mi_dequant_rowwise", ("in", "rows", "cols", "ld_in", "scales", "in_format", "out", "out_dtype"), two_d,
                                  {**sizes, **no_cols, **null("in", "scales", "out"), **bad_out, **ld(ld_in=63), "bad in_format": dict(in_format=2)}),
    }


def c_front_end(lib, L):
    """-> {entry point: {"fault" or "fault + fault": return code}}.  A pair whose faults set the same argument is not a pair and is left out.
    Asserts that no case got as far as a launch (a HIP code, or 0 from anything but an empty problem) - a test must never launch on P - and
    that after each single fault fp8mi_last_error() begins with the entry point's name."""
    out = {}
    for entry, (reports, order, base, faults) in _entries(L).items():
        cases = {name: over for name, over in faults.items()}
        for (n1, o1), (n2, o2) in itertools.combinations(faults.items(), 2):
            if not set(o1) & set(o2):
                cases[f"{n1} + {n2}"] = {**o1, **o2}
        codes = {}
        for name, over in cases.items():
            args = {**base, **over}
            rc = getattr(lib, entry)(*(args[k] for k in order), None)
            empty = 0 in [args[k] for k in ("count", "rows", "cols") if k in order]
            assert rc < 0 or (rc == 0 and empty), f"{entry}: '{name}' reached a launch (returned {rc})"
            if rc and name in faults:
                message = lib.fp8mi_last_error().decode()
                assert message.startswith(reports + ":"), f"{entry}: '{name}' left the message '{message}'"
            codes[name] = rc
        out[entry] = codes
    return out


# ---- the op layer ---------------------------------------------------------------------------------------------------------------

def views(make, cols=64):
    """the layouts every function is shown: make(shape) -> a tensor of the function's input type"""
    return {"plain": make((4, cols)), "3-D": make((2, 3, cols)), "1-D": make((cols,)),
            "a column slab of a wider buffer": make((4, 2 * cols))[:, cols:], "a transposed view": make((cols, 4)).t(),
            "one row": make((1, cols)), "one row of a wider buffer": make((1, 2 * cols))[:, cols:], "zero rows": make((0, cols)),
            "zero columns": make((4, 0)), "every second column": make((4, 2 * cols))[:, ::2]}


def op_layer(native):
    """-> {"function: case": what gemm_frontend_cases.recorder()'s run files} for the 15 fp8_* cast functions"""
    import torch
    u8, f32, f16, bf16, f64, i32 = torch.uint8, torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32
    E4, E5, E8, FP4 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e8m0fnu, torch.float4_e2m1fn_x2
    L = native._l
    results = {}

    floats = lambda dt=f32: (lambda shape: torch.zeros(shape, dtype=dt))   # noqa: E731
    in_dtypes = {str(dt): floats(dt)((4, 64)) for dt in (f16, bf16, f64, i32)}
    out_dtypes = {f"out_dtype {dt}": dict(out_dtype=dt) for dt in (f32, f16, bf16, f64)}

    with recorder(native) as run:
        def cases_of(fn, names):
            def case(label, *args, **kw):
                run(results, f"{fn.__name__}: {label}", fn, *args, names=names, **kw)
            return case

        # the flat casts: fp8_dequantize, fp8_dequantize_e5m2 (bytes in), fp8_encode, fp8_encode_e5m2, fp8_quantize, fp8_quantize_e5m2, fp8_amax
        for fn, byte_types in ((native.fp8_dequantize, (E4, E5, f32)), (native.fp8_dequantize_e5m2, (E5, E4, f32))):
            case = cases_of(fn, ("input", "scale"))
            for label, t in views(floats(u8)).items():
                case(label, t)
            for dt in byte_types:
                case(f"input {dt}", torch.zeros(4, 64, dtype=u8).view(dt) if dt is not f32 else torch.zeros(4, 64))
            q = torch.zeros(4, 64, dtype=u8)
            for label, kw in out_dtypes.items():
                case(label, q, **kw)
            case("scale f32", q, torch.ones(1))
            case("scale f64, 0-d", q, torch.ones((), dtype=f64))
            case("scale of two elements", q, torch.ones(2))
            case("scale, zero rows", torch.zeros(0, 64, dtype=u8), torch.ones(1))
        for fn in (native.fp8_encode, native.fp8_quantize, native.fp8_amax, native.fp8_encode_e5m2, native.fp8_quantize_e5m2):
            case = cases_of(fn, ("input", "prescale"))
            for label, t in {**views(floats()), **in_dtypes}.items():
                case(label, t)
            if fn in (native.fp8_encode, native.fp8_quantize):
                case("encode_mode ENC_RNE", torch.zeros(4, 64), L.ENC_RNE)
                case("encode_mode ENC_REFERENCE", torch.zeros(4, 64), encode_mode=L.ENC_REFERENCE)
            if fn is native.fp8_encode_e5m2:
                case("prescale f32", torch.zeros(4, 64), torch.ones(1))
                case("prescale bf16, (1, 1)", torch.zeros(4, 64), torch.ones(1, 1, dtype=bf16))
                case("prescale of two elements", torch.zeros(4, 64), torch.ones(2))
                case("prescale, zero rows", torch.zeros(0, 64), torch.ones(1))

        # the MX pairs
        for q_fn, dq_fn, per_byte, packed in ((native.fp8_quantize_mxfp8, native.fp8_dequantize_mxfp8, 1, E4),
                                              (native.fp8_quantize_mxfp4, native.fp8_dequantize_mxfp4, 2, FP4)):
            case = cases_of(q_fn, ("x",))
            for label, t in {**views(floats()), **in_dtypes}.items():
                case(label, t)
            case("48 columns", torch.zeros(4, 48))
            case("3-D, 48 columns", torch.zeros(2, 3, 48))
            case("1024 columns", torch.zeros(2, 1024, dtype=bf16))
            case = cases_of(dq_fn, ("q", "scales"))
            sc = lambda rows=4, nb=2: torch.full((rows, nb), 127, dtype=u8)   # noqa: E731
            for label, t in views(floats(u8), 64 // per_byte).items():
                rows = t.shape[0] if t.dim() == 2 else 4
                case(label, t, sc(rows, 2 if t.shape[-1] else 0))
            q = torch.zeros(4, 64 // per_byte, dtype=u8)
            case(f"q {packed}", q.view(packed), sc())
            case("q float32", torch.zeros(4, 64 // per_byte), sc())
            case("40 columns", torch.zeros(4, 40 // per_byte, dtype=u8), sc())
            for label, kw in out_dtypes.items():
                case(label, q, sc(), **kw)
            case("scales float8_e8m0fnu", q, sc().view(E8))
            case("scales float32", q, torch.ones(4, 2))
            case("scales of the wrong shape", q, sc(4, 1))
            case("scales of too few rows", q, sc(3, 2))
            case("scales flat", q, sc().reshape(-1))
            case("scales flat, of the wrong count", q, sc(4, 3).reshape(-1))
            case("scales flat, torch's padded size", q, torch.full((128 * 4,), 127, dtype=u8))
            case("scales in a padded row", q, sc(4, 8)[:, :2])
            case("scales wider than needed", q, sc(4, 4))
            case("scales a transposed view", q, sc(2, 4).t())
            case("scales 3-D", q, sc()[None])
            case("one row, scales in a padded row", q[:1], sc(1, 8)[:, :2])

        # the blockwise pair
        case = cases_of(native.fp8_quantize_blockwise, ("x",))
        for label, t in {**views(floats(), 192), **in_dtypes}.items():
            case(label, t)
            if label in ("plain", "3-D", "a column slab of a wider buffer", "zero rows", "zero columns"):
                case(f"{label}, block_rows 128", t, 128)
        case("130 rows, block_rows 128", torch.zeros(130, 192), block_rows=128)
        case("200 columns", torch.zeros(4, 200))
        case("block_rows 64", torch.zeros(4, 192), 64)
        case = cases_of(native.fp8_dequantize_blockwise, ("q", "scales"))
        for label, t in views(floats(u8), 192).items():
            rows = t.shape[0] if t.dim() == 2 else 4
            case(label, t, torch.ones(rows, (t.shape[-1] + 127) // 128))
        q = torch.zeros(4, 192, dtype=u8)
        case("q float8_e4m3fn", q.view(E4), torch.ones(4, 2))
        case("q float32", torch.zeros(4, 192), torch.ones(4, 2))
        for label, kw in out_dtypes.items():
            case(label, q, torch.ones(4, 2), **kw)
        case("block_rows 128", q, torch.ones(1, 2), 128)
        case("130 rows, block_rows 128", torch.zeros(130, 192, dtype=u8), torch.ones(2, 2), block_rows=128)
        case("block_rows 64", q, torch.ones(4, 2), 64)
        case("scales of the wrong shape", q, torch.ones(4, 3))
        case("scales for another block_rows", q, torch.ones(1, 2))
        case("scales flat", q, torch.ones(8))
        case("scales float64", q, torch.ones(4, 2, dtype=f64))
        case("scales a transposed view", q, torch.ones(2, 4).t())
        case("scales in a padded row", q, torch.ones(4, 8)[:, :2])

        # the rowwise pair
        case = cases_of(native.fp8_quantize_rowwise, ("x",))
        for label, t in {**views(floats()), **in_dtypes, "0-d": torch.zeros(())}.items():
            case(label, t)
        x = torch.zeros(4, 64)
        case("return_amax", x, return_amax=True)
        case("3-D, return_amax", torch.zeros(2, 3, 64), return_amax=True)
        case("zero rows, return_amax", torch.zeros(0, 64), return_amax=True)
        case("e5m2", x, L.FMT_E5M2)
        case("e5m2, return_amax", x, L.FMT_E5M2, None, True)
        case("e5m2 with ENC_REFERENCE", x, L.FMT_E5M2, L.ENC_REFERENCE)
        case("encode_mode ENC_RNE", x, encode_mode=L.ENC_RNE)
        case("encode_mode ENC_REFERENCE", x, encode_mode=L.ENC_REFERENCE)
        case("out_format 2", x, 2)
        case("50 columns", torch.zeros(4, 50))
        case = cases_of(native.fp8_dequantize_rowwise, ("q", "scales"))
        for label, t in {**views(floats(u8)), "0-d": torch.zeros((), dtype=u8)}.items():
            case(label, t, torch.ones(t.numel() // t.shape[-1] if t.dim() and t.shape[-1] else (4 if t.dim() == 2 else 1)))
        q = torch.zeros(4, 64, dtype=u8)
        for dt in (E4, E5):
            case(f"q {dt}", q.view(dt), torch.ones(4, 1))
        case("q float32", torch.zeros(4, 64), torch.ones(4))
        case("q float16, in_format given", torch.zeros(4, 64, dtype=f16), torch.ones(4), in_format=L.FMT_E4M3)
        case("in_format FMT_E5M2 on uint8", q, torch.ones(4), in_format=L.FMT_E5M2)
        case("in_format FMT_E4M3 on float8_e5m2", q.view(E5), torch.ones(4), in_format=L.FMT_E4M3)
        case("in_format 2", q, torch.ones(4), in_format=2)
        for label, kw in out_dtypes.items():
            case(label, q, torch.ones(4), **kw)
        case("scales (4, 1)", q, torch.ones(4, 1))
        case("scales float64", q, torch.ones(4, dtype=f64))
        case("scales a strided view", q, torch.ones(4, 2)[:, 0])
        case("scales of the wrong count", q, torch.ones(5))
        case("scales of one element", q, torch.ones(1))
        case("3-D, scales (2, 3, 1)", torch.zeros(2, 3, 64, dtype=u8), torch.ones(2, 3, 1))
        case("50 columns", torch.zeros(4, 50, dtype=u8), torch.ones(4))
    return results


if __name__ == "__main__":
    assert len(sys.argv) >= 2 and sys.argv[1] == "record", __doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "fp8-mps-metal_amd"))
    import fp8_mi355x_lib
    import fp8_mi355x_native
    for name, data in (("c", c_front_end(fp8_mi355x_lib.load(), fp8_mi355x_lib)), ("op", op_layer(fp8_mi355x_native))):
        with open(os.path.join(GOLDEN, f"cast_frontend_{name}.json"), "w") as f:
            json.dump(data, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"cast_frontend_{name}.json: {sum(len(v) for v in data.values()) if name == 'c' else len(data)} cases")
