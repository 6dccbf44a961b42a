"""What the GEMM front end does with its arguments, enumerated for tests/test_gemm_frontend_host.py (no GPU):

  c_front_end(lib)   the return code of every faulty call of the four fp8mi_scaled_mm_* entry points and of their four grouped forms
                     (fp8mi_scaled_mm_grouped*): each single fault and each pair of a per-family list, on the base call of
                     tests/test_mxfp8_host.py (M = N = 64, K = 128, fake aligned pointers; grouped: M_total = 64, G = 2);
  c_choosers(lib)    what fp8mi_choose_kernel_grouped / _grouped_mx return over a small list, the error returns included;
  op_layer(native)   the entry point and the full argument tuple that the GEMM functions of fp8_mi355x_native - the four
                     single-problem ones, scaled_mm_colmajor, the four grouped ones, the fp8_moe_linear_* / _mlp_* / _forward_* and
                     scaled_grouped_mm_colmajor - hand to the library, with the library replaced by a recorder.

    python tests/gemm_frontend_cases.py record [PACKAGE_DIR]
writes both as tests/golden/gemm_frontend_{c,op}.json from the package in PACKAGE_DIR (default: this tree's).  The fixtures are the
behaviour of the commit BEFORE a change to the front end: record them there, then run the test on the change."""
import contextlib
import itertools
import json
import os
import sys

P = 0x100000   # a 16-byte aligned fake device pointer: every enumerated call must fail before anything dereferences it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the C front end ------------------------------------------------------------------------------------------------------------

def _families(L):
    """-> {family: (call(lib, **args), base args, {fault: overrides})}"""
    common = dict(A=P, B=P, C=P, sa=P, sb=P, bias=None, sr=None, M=64, N=64, K=128, lda=None, ldb=None, ldc=None, out=L.F32, bias_dtype=L.F32,
                  nan=L.NAN_ZERO, kernel=L.KERNEL_AUTO, split=0)
    shared = {
        "negative M": dict(M=-1), "negative K": dict(K=-32), "M = 0": dict(M=0), "N = 0": dict(N=0), "NULL C": dict(C=None),
        "NULL B": dict(B=None), "NULL scale_a": dict(sa=None), "lda too small": dict(lda=16), "ldb too small": dict(ldb=16),
        "ldc too small": dict(ldc=10), "bad out_dtype": dict(out=7), "bad bias_dtype with a bias": dict(bias=P, bias_dtype=7),
        "bad nan mode": dict(nan=2), "split_k = -1": dict(split=-1), "unknown kernel id": dict(kernel=999),
        "forced ring tile, misaligned A": dict(kernel=L.KERNEL_GEMM_64x64, A=P + 8),
    }
    no_block_form = {f"kernel {k} has no form": dict(kernel=k) for k in (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX, L.KERNEL_SKINNY,
                                                                        L.KERNEL_GEMM_256, L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W)}
    mx_faults = {"K % 32": dict(K=100), "ld_sa too small": dict(ld_sa=3), "ld_sb too small": dict(ld_sb=3),
                 "forced ring tile, misaligned scale pointer": dict(kernel=L.KERNEL_GEMM_32x64, sb=P + 2),
                 "forced ring tile, ld_sa % 4": dict(kernel=L.KERNEL_GEMM_128x64, K=160, ld_sa=5, ld_sb=8)}

    def ld(a, per_byte=1):
        k = a["K"] // per_byte
        return (k if a["lda"] is None else a["lda"], k if a["ldb"] is None else a["ldb"], a["N"] if a["ldc"] is None else a["ldc"])

    def tensorwise(lib, a):
        return lib.fp8mi_scaled_mm_fmt(a["A"], a["B"], a["C"], a["sa"], a["sb"], a["bias"], a["sr"], a["M"], a["N"], a["K"], *ld(a), a["sa_mode"],
                                       a["sb_mode"], a["out"], a["bias_dtype"], a["nan"], a["kernel"], a["split"], None, 0, a["a_format"],
                                       a["b_format"], None)

    def mx(name, per_byte):
        def call(lib, a):
            nb = a["K"] // 32
            args = [a["A"], a["B"], a["C"], a["sa"], nb if a["ld_sa"] is None else a["ld_sa"], a["sb"], nb if a["ld_sb"] is None else a["ld_sb"],
                    a["bias"], a["sr"], a["M"], a["N"], a["K"], *ld(a, per_byte), a["out"], a["bias_dtype"]]
            if per_byte == 1:
                args.append(a["nan"])
            return getattr(lib, name)(*args, a["kernel"], a["split"], None, 0, None)
        return call

    def blockwise(lib, a):
        return lib.fp8mi_scaled_mm_blockwise(a["A"], a["B"], a["C"], a["sa"], a["sa_sr"], a["sa_sk"], a["block_a"], a["sb"], a["sb_sr"], a["sb_sk"],
                                             a["block_b"], a["bias"], a["sr"], a["M"], a["N"], a["K"], *ld(a), a["out"], a["bias_dtype"], a["nan"],
                                             a["kernel"], a["split"], None, 0, None)

    # tensorwise has a form of every kernel id: the ids below are those whose own envelope turns the base shape away (M = 64, K = 128)
    tw_faults = {f"kernel {k} does not take the shape": dict(kernel=k) for k in (L.KERNEL_GEMV, L.KERNEL_GEMV_FP32, L.KERNEL_GEMV_MX,
                                                                                 L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W)}
    tw_faults.update({"bad a_format": dict(a_format=2), "bad b_format": dict(b_format=-1), "bad scale_a mode": dict(sa_mode=2),
                      "bad scale_b mode": dict(sb_mode=3), "e5m2 with NAN_ZERO": dict(a_format=L.FMT_E5M2), "NULL scale_b": dict(sb=None)})
    mxfp4_shared = {k: v for k, v in shared.items() if k != "bad nan mode"}   # (fp8mi_scaled_mm_mxfp4 has no nan_mode)

    # the grouped forms: M is M_total; no split-K and no workspace; B_gnk's experts stride_b bytes apart (None: N dense rows)
    g_common = dict(common, offs=P, G=2, stride_b=None)
    g_shared = {k: v for k, v in shared.items() if k != "split_k = -1"}
    g_shared.update({"NULL offs": dict(offs=None), "NULL scale_b": dict(sb=None), "G = 0": dict(G=0), "G = 1025": dict(G=1025), "K = 0": dict(K=0),
                     "negative stride_b": dict(stride_b=-16), "stride_b smaller than an expert": dict(stride_b=1024),
                     "stride_b % 16": dict(stride_b=64 * 128 + 8), "transposed epilogue": dict(bias_dtype=L.F32 | L.EPILOGUE_TRANSPOSED),
                     f"kernel {L.KERNEL_GENERIC} has no form": dict(kernel=L.KERNEL_GENERIC), **no_block_form})
    g_mxfp4_shared = {k: v for k, v in g_shared.items() if k != "bad nan mode"}
    g_mx_faults = {"K % 32": dict(K=100), "ld_sa too small": dict(ld_sa=3), "ld_sb too small": dict(ld_sb=3), "negative stride_sb": dict(stride_sb=-4),
                   "stride_sb smaller than an expert": dict(stride_sb=4), "stride_sb % 4": dict(stride_sb=64 * 4 + 2),
                   "misaligned scale pointer": dict(sb=P + 2), "ld_sa % 4": dict(K=160, ld_sa=5, ld_sb=8, stride_sb=64 * 8)}

    def g_ld(a, per_byte=1):
        lda, ldb, ldc = ld(a, per_byte)
        return lda, ldb, a["N"] * ldb if a["stride_b"] is None else a["stride_b"], ldc

    def g_tensorwise(lib, a):
        return lib.fp8mi_scaled_mm_grouped(a["A"], a["B"], a["C"], a["sa"], a["sb"], a["bias"], a["sr"], a["offs"], a["G"], a["M"], a["N"], a["K"],
                                           *g_ld(a), a["sa_mode"], a["sb_mode"], a["out"], a["bias_dtype"], a["nan"], a["kernel"], None)

    def g_blockwise(lib, a):
        return lib.fp8mi_scaled_mm_grouped_blockwise(a["A"], a["B"], a["C"], a["sa"], a["sa_sr"], a["sa_sk"], a["block_a"], a["sb"], a["sb_sr"], a["sb_sk"],
                                                     a["sb_se"], a["block_b"], a["bias"], a["sr"], a["offs"], a["G"], a["M"], a["N"], a["K"], *g_ld(a),
                                                     a["out"], a["bias_dtype"], a["nan"], a["kernel"], None)

    def g_mx(name, per_byte):
        def call(lib, a):
            nb = a["K"] // 32
            ld_sb = nb if a["ld_sb"] is None else a["ld_sb"]
            args = [a["A"], a["B"], a["C"], a["sa"], nb if a["ld_sa"] is None else a["ld_sa"], a["sb"], ld_sb,
                    a["N"] * ld_sb if a["stride_sb"] is None else a["stride_sb"], a["bias"], a["sr"], a["offs"], a["G"], a["M"], a["N"], a["K"],
                    *g_ld(a, per_byte), a["out"], a["bias_dtype"]]
            if per_byte == 1:
                args.append(a["nan"])
            return getattr(lib, name)(*args, a["kernel"], None)
        return call

    g_mx_base = dict(g_common, ld_sa=None, ld_sb=None, stride_sb=None)
    grouped = {
        "grouped": (g_tensorwise, dict(g_common, sa_mode=0, sb_mode=0), {**g_shared, "bad scale_a mode": dict(sa_mode=2), "bad scale_b mode": dict(sb_mode=3)}),
        "grouped_blockwise": (g_blockwise, dict(g_common, sa_sr=1, sa_sk=1, sb_sr=1, sb_sk=1, sb_se=1, block_a=1, block_b=128),
                              {**g_shared, "negative scale stride": dict(sa_sk=-1), "negative scale_b stride": dict(sb_sr=-1),
                               "negative expert scale stride": dict(sb_se=-1), "bad block_a": dict(block_a=64), "bad block_b": dict(block_b=0),
                               "block_a = 128": dict(block_a=128), "misaligned scale pointer": dict(sb=P + 2)}),
        "grouped_mxfp8": (g_mx("fp8mi_scaled_mm_grouped_mxfp8", 1), g_mx_base, {**g_shared, **g_mx_faults}),
        "grouped_mxfp4": (g_mx("fp8mi_scaled_mm_grouped_mxfp4", 2), g_mx_base, {**g_mxfp4_shared, **g_mx_faults}),
    }
    return {
        **grouped,
        "tensorwise": (tensorwise, dict(common, sa_mode=0, sb_mode=0, a_format=L.FMT_E4M3, b_format=L.FMT_E4M3), {**shared, **tw_faults}),
        "mxfp8": (mx("fp8mi_scaled_mm_mxfp8", 1), dict(common, ld_sa=None, ld_sb=None), {**shared, **no_block_form, **mx_faults}),
        "mxfp4": (mx("fp8mi_scaled_mm_mxfp4", 2), dict(common, ld_sa=None, ld_sb=None), {**mxfp4_shared, **no_block_form, **mx_faults}),
        "blockwise": (blockwise, dict(common, sa_sr=1, sa_sk=1, sb_sr=1, sb_sk=1, block_a=1, block_b=128),
                      {**shared, **no_block_form, "negative scale stride": dict(sa_sk=-1), "negative scale_b stride": dict(sb_sr=-1),
                       "bad block_a": dict(block_a=64), "bad block_b": dict(block_b=0)}),
    }


def c_front_end(lib, L):
    """-> {family: {"fault" or "fault + fault": return code}}.  A pair whose faults set the same argument is not a pair and is left out.
    Asserts that no case got as far as a launch (a HIP code, or 0 from anything but an empty problem): a test must never launch on P."""
    out = {}
    for family, (call, base, faults) in _families(L).items():
        cases = {name: over for name, over in faults.items()}
        for (n1, o1), (n2, o2) in itertools.combinations(faults.items(), 2):
            if not set(o1) & set(o2):
                cases[f"{n1} + {n2}"] = {**o1, **o2}
        codes = {}
        for name, over in cases.items():
            args = {**base, **over}
            rc = call(lib, args)
            assert rc < 0 or (rc == 0 and (args["M"] == 0 or args["N"] == 0)), f"{family}: '{name}' reached a launch (returned {rc})"
            codes[name] = rc
        out[family] = codes
    return out


def c_choosers(lib, L):
    """-> {"grouped" / "grouped_mx": {"arguments": return value}} of fp8mi_choose_kernel_grouped / _grouped_mx (host-only)"""
    shapes = {"G = 8, M_total = 4096, N = 4096, K = 7168": (8, 4096, 4096, 7168), "G = 2, M_total = 64, N = 64, K = 128": (2, 64, 64, 128),
              "G = 64, M_total = 512, N = 2048, K = 1024": (64, 512, 2048, 1024), "G = 1, M_total = 8192, N = 8192, K = 8192": (1, 8192, 8192, 8192),
              "G = 4, M_total = 3, N = 256, K = 256": (4, 3, 256, 256),
              "G = 0": (0, 64, 64, 128), "G = 1025": (1025, 64, 64, 128), "K = 0": (4, 64, 64, 0), "M_total = 0": (4, 0, 64, 128),
              "N = 0": (4, 64, 0, 128), "negative M_total": (4, -1, 64, 128), "K % 32": (4, 64, 64, 112), "unaligned K": (4, 64, 64, 72),
              "K = 96": (4, 64, 64, 96)}
    out = {"grouped": {}, "grouped_mx": {}}
    for name, (G, M, N, K) in shapes.items():
        out["grouped"][name] = lib.fp8mi_choose_kernel_grouped(G, M, N, K, K, K, N, L.BF16)
        for fmt, per_byte in ((L.MX_FP8, 1), (L.MX_FP4, 2)):
            out["grouped_mx"][f"format {fmt}, {name}"] = lib.fp8mi_choose_kernel_grouped_mx(fmt, G, M, N, K, K // per_byte, K // per_byte, N, L.BF16)
    out["grouped"]["bad out_dtype"] = lib.fp8mi_choose_kernel_grouped(4, 64, 64, 128, 128, 128, 64, 9)
    out["grouped_mx"]["bad out_dtype"] = lib.fp8mi_choose_kernel_grouped_mx(L.MX_FP8, 4, 64, 64, 128, 128, 128, 64, 9)
    out["grouped_mx"]["bad format"] = lib.fp8mi_choose_kernel_grouped_mx(2, 4, 64, 64, 128, 128, 128, 64, L.BF16)
    out["grouped_mx"]["format 1, a row stride that is no multiple of 16"] = lib.fp8mi_choose_kernel_grouped_mx(L.MX_FP4, 4, 64, 64, 128, 72, 64, 64, L.BF16)
    return out


# ---- the op layer ---------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def recorder(native):
    """-> run(results, label, fn, *args, names=, **kw), which files {"calls": [[entry point, [arguments]]], "workspace_asked": bool,
    "result" / "returned_none" / "raised": ...} under results[label], with the module's device type, stream, library and workspace replaced
    as in test_transposed_epilogue_keyword_reaches_bias_dtype.  A pointer argument is written "<input tensor>+<byte offset>", "fresh" (memory
    the op layer allocated) or None.  A tensor result is [shape, dtype, pointer]; a tuple of results is the list of those, and there a
    pointer into memory that the call received as its argument i reads "arg<i>+<byte offset>"."""
    import torch
    L = native._l
    saved = (native.DEVICE_TYPE, native._stream, L.load, native._workspace_on)
    calls, raw, asked, named = [], [], [], {}
    workspace = torch.zeros(64, dtype=torch.uint8)

    class Recorder:
        def __getattr__(self, entry):
            def record(*args):
                calls.append([entry, [describe(a) for a in args]])
                raw[:] = args
                return 0
            return record

    def describe(a):
        if not isinstance(a, int) or isinstance(a, bool) or a < (1 << 24):   # (no size, stride or code of these calls comes near a heap address)
            return a
        for name, t in named.items():
            st = t.untyped_storage()
            if st.data_ptr() <= a < st.data_ptr() + max(st.nbytes(), 1):
                return f"{name}+{a - st.data_ptr()}"
        return "fresh"

    def in_call(p):
        """a result's pointer: into an input, or "arg<i>+<offset>" for the nearest fresh pointer at or below it among the last call's arguments"""
        d = describe(p)
        below = [(p - a, i) for i, a in enumerate(raw) if isinstance(a, int) and not isinstance(a, bool) and describe(a) == "fresh" and a <= p]
        return "arg%d+%d" % min(below)[::-1] if d == "fresh" and below else d

    def run(results, label, fn, *args, names=("A", "B", "scale_a", "scale_b"), **kw):
        del calls[:], raw[:], asked[:]
        named.clear()
        tensors = dict(zip(names, args), **kw, workspace=workspace)
        named.update({k: v for k, v in tensors.items() if isinstance(v, torch.Tensor) and v.numel() > 0})
        entry = {}
        try:
            ret = fn(*args, **kw)
            if ret is None:
                entry["returned_none"] = True
            elif isinstance(ret, tuple):
                entry["result"] = [[list(r.shape), str(r.dtype), in_call(r.data_ptr()) if r.numel() else None] for r in ret]
            else:
                entry["result"] = [list(ret.shape), str(ret.dtype), describe(ret.data_ptr()) if ret.numel() else None]
        except AssertionError as e:
            entry["raised"] = str(e)
        except KeyError as e:   # (a dtype that a function looks up without a check of its own)
            entry["raised"] = f"KeyError: {e}"
        results[label] = dict(entry, calls=[c for c in calls], workspace_asked=bool(asked))

    native.DEVICE_TYPE, native._stream, L.load = "cpu", (lambda dev: 0), (lambda: Recorder())
    native._workspace_on = lambda dev, stream: (asked.append(1), workspace)[1]
    try:
        yield run
    finally:
        native.DEVICE_TYPE, native._stream, L.load, native._workspace_on = saved


def op_layer(native):
    """-> {"function: case": what recorder()'s run files} for the GEMM functions of the op layer"""
    import torch
    with recorder(native) as run:
        results = {}
        u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16
        E4, E5, FP4 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2
        one = lambda: torch.ones(1)   # noqa: E731

        def operands(family, M, N, K):
            """-> (A, B, scale_a, scale_b, bytes per operand row)"""
            kb = K // 2 if family == "mxfp4" else K
            A, B = torch.zeros(M, kb, dtype=u8), torch.zeros(N, kb, dtype=u8)
            if family in ("tensorwise", "colmajor"):
                return A, B, one(), one(), kb
            if family == "blockwise":
                return A, B, torch.ones(M, (K + 127) // 128), torch.ones((N + 127) // 128, (K + 127) // 128), kb
            return A, B, torch.full((M, K // 32), 127, dtype=u8), torch.full((N, K // 32), 127, dtype=u8), kb

        fns = {"tensorwise": native.fp8_scaled_mm, "mxfp8": native.fp8_scaled_mm_mxfp8, "mxfp4": native.fp8_scaled_mm_mxfp4,
               "blockwise": native.fp8_scaled_mm_blockwise,
               "colmajor": lambda A, B, sa, sb, **kw: native.scaled_mm_colmajor(A, B.t(), sa, sb, **kw)}
        for family, fn in fns.items():
            M, N, K = 8, 24, 64
            col = family == "colmajor"   # (scaled_mm_colmajor has torch._scaled_mm's keywords only)
            f8 = FP4 if family == "mxfp4" else E4

            def case(label, *args, **kw):
                run(results, f"{family}: {label}", fn, *args, **kw)

            A, B, sa, sb, kb = operands(family, M, N, K)
            case("plain", A, B, sa, sb)
            case("A a column slab of a wider buffer", torch.zeros(M, 2 * kb, dtype=u8)[:, kb:], B, sa, sb)
            case("A a transposed view", torch.zeros(kb, M, dtype=u8).t(), B, sa, sb)
            case("out_dtype bf16", A, B, sa, sb, out_dtype=bf16)
            for dt in (f32, bf16, torch.float64):
                case(f"bias {dt}", A, B, sa, sb, bias=torch.zeros(N, dtype=dt))
            case("bias shaped (1, N)", A, B, sa, sb, bias=torch.zeros(1, N))
            case("bias of the wrong length", A, B, sa, sb, bias=torch.zeros(N + 1))
            case("scale_result f32", A, B, sa, sb, scale_result=torch.ones(1))
            case("scale_result f64", A, B, sa, sb, scale_result=torch.ones(1, dtype=torch.float64))
            case("float8 operands", A.view(f8), B.view(f8), sa, sb)
            A0 = operands(family, 0, N, K)
            case("M = 0", A0[0], B, A0[2], sb)
            A1, B1, sa1, sb1, _ = operands(family, 1, N, 1024)
            case("M = 1, K = 1024", A1, B1, sa1, sb1)
            Ak, Bk, sak, sbk, _ = operands(family, M, N, 1024)
            case("K = 1024", Ak, Bk, sak, sbk)
            if family in ("tensorwise", "colmajor"):
                case("e5m2 A", A.view(E5), B, sa, sb)
                case("e5m2 B, e4m3 A", A.view(E4), B.view(E5), sa, sb)
                Ap, Bp, sap, sbp, _ = operands(family, 32, 64, 2052)
                case("the padded path, M = 32, N = 64, K = 2052", Ap, Bp, sap, sbp)
            if col:
                continue
            case("out with a padded row stride", A, B, sa, sb, out=torch.zeros(M, N + 8)[:, :N])
            case("out of the wrong shape", A, B, sa, sb, out=torch.zeros(M, N + 1))
            case("out of the wrong dtype", A, B, sa, sb, out=torch.zeros(M, N, dtype=bf16))
            case("out with a column stride", A, B, sa, sb, out=torch.zeros(M, 2 * N)[:, ::2])
            case("transposed_epilogue with a bias", A, B, sa, sb, bias=torch.zeros(M, dtype=bf16), transposed_epilogue=True)
            case("transposed_epilogue without a bias", A, B, sa, sb, transposed_epilogue=True)
            case("transposed_epilogue with a bias of N elements", A, B, sa, sb, bias=torch.zeros(N), transposed_epilogue=True)
            case("K = 1024, split_k = 1", Ak, Bk, sak, sbk, split_k=1)
            case("K = 1024, split_k = 4", Ak, Bk, sak, sbk, split_k=4)
            if family == "mxfp4":
                A2, B2, sa2, sb2, _ = operands(family, M, N, 2048)
                case("K = 2048", A2, B2, sa2, sb2)
        _grouped_op_cases(native, lambda label, fn, *args, **kw: run(results, label, fn, *args, **kw))
        return results


def _grouped_op_cases(native, run):
    """The grouped GEMM functions, the MoE linears, MLPs and forwards and scaled_grouped_mm_colmajor: run(label, fn, *args, names=, **kw)."""
    import torch
    L = native._l
    u8, f32, bf16, i32 = torch.uint8, torch.float32, torch.bfloat16, torch.int32
    mx_of = {"mxfp8": 1, "mxfp4": 2}   # elements per operand byte of the MX recipes

    def offs_of(M, G, dtype=i32):
        return torch.tensor([M * (g + 1) // G for g in range(G)], dtype=dtype)

    def weights(recipe, G, rows, K):
        """-> (w_q (G, rows, K bytes), its scales as the recipe's functions take them)"""
        w = torch.zeros(G, rows, K // mx_of.get(recipe, 1), dtype=u8)
        if recipe == "row":
            return w, torch.ones(G, rows)
        if recipe == "block128":
            return w, torch.ones(G, (rows + 127) // 128, (K + 127) // 128)
        return w, torch.full((G, rows, K // 32), 127, dtype=u8)

    def acts(recipe, M, K):
        """-> (A (M, K bytes), scale_a) of the recipe's grouped GEMM"""
        A = torch.zeros(M, K // mx_of.get(recipe, 1), dtype=u8)
        if recipe == "row":
            return A, torch.ones(M)
        if recipe == "block128":
            return A, torch.ones(M, (K + 127) // 128)
        return A, torch.full((M, K // 32), 127, dtype=u8)

    def padded(w):   # the same values with padded row and expert strides
        G, rows, kb = w.shape
        return torch.zeros(G, rows + 1, kb + 16, dtype=w.dtype)[:, :rows, :kb]

    def transposed(w):   # a layout the kernels cannot read: K is not the unit-stride dimension
        G, rows, kb = w.shape
        return torch.zeros(G, kb, rows, dtype=w.dtype).transpose(1, 2)

    gemms = {"row": ("grouped", native.fp8_scaled_mm_grouped), "block128": ("grouped_blockwise", native.fp8_scaled_mm_grouped_blockwise),
             "mxfp8": ("grouped_mxfp8", native.fp8_scaled_mm_grouped_mxfp8), "mxfp4": ("grouped_mxfp4", native.fp8_scaled_mm_grouped_mxfp4)}
    M, G, N, K, H = 8, 2, 24, 128, 128
    for recipe, (family, fn) in gemms.items():
        def case(label, *args, **kw):
            run(f"{family}: {label}", fn, *args, names=("A", "B", "scale_a", "scale_b", "offs"), **kw)

        (A, sa), (B, sb), offs = acts(recipe, M, K), weights(recipe, G, N, K), offs_of(M, G)
        case("plain", A, B, sa, sb, offs)
        case("B with padded row and expert strides", A, padded(B), sa, sb, offs)
        case("B that must be copied", A, transposed(B), sa, sb, offs)
        case("A a column slab of a wider buffer", torch.zeros(M, 2 * A.shape[1], dtype=u8)[:, A.shape[1]:], B, sa, sb, offs)
        case("offs int64", A, B, sa, sb, offs_of(M, G, torch.int64))
        case("offs of the wrong length", A, B, sa, sb, offs_of(M, G + 1))
        for dt in (f32, bf16, torch.float64):
            case(f"bias {dt}", A, B, sa, sb, offs, bias=torch.zeros(G, N, dtype=dt))
        case("bias of the wrong length", A, B, sa, sb, offs, bias=torch.zeros(G, N + 1))
        case("scale_result f32", A, B, sa, sb, offs, scale_result=torch.ones(1))
        case("out_dtype bf16", A, B, sa, sb, offs, out_dtype=bf16)
        case("out given", A, B, sa, sb, offs, out=torch.zeros(M, N))
        case("out with a padded row stride", A, B, sa, sb, offs, out=torch.zeros(M, N + 8)[:, :N])
        case("out of the wrong shape", A, B, sa, sb, offs, out=torch.zeros(M, N + 1))
        A0, sa0 = acts(recipe, 0, K)
        case("M_total = 0", A0, B, sa0, sb, offs)
        B1, sb1 = weights(recipe, 1, N, K)
        case("G = 1", A, B1, sa, sb1, offs_of(M, 1))
        if recipe != "mxfp4":   # (fp8_scaled_mm_grouped_mxfp4 has no nan_mode)
            case("nan_mode NAN_PROPAGATE", A, B, sa, sb, offs, nan_mode=L.NAN_PROPAGATE)
            case("nan_mode NAN_ZERO", A, B, sa, sb, offs, nan_mode=L.NAN_ZERO)
        case("kernel GEMM_64x64", A, B, sa, sb, offs, kernel=L.KERNEL_GEMM_64x64)
        if recipe == "row":
            case("one scale per tensor and per expert", A, B, torch.ones(1), torch.ones(G), offs)
            case("scale_b a strided view", A, B, sa, torch.ones(G, 2 * N)[:, ::2], offs)
            case("scale_b of the wrong length", A, B, sa, torch.ones(G, N + 1), offs)
            case("e5m2 A", A.view(torch.float8_e5m2), B, sa, sb, offs)
        if recipe == "block128":
            case("block_b = 1", A, B, sa, torch.ones(G, N, 1), offs, block_b=1)
            case("scale_b with strides of its own", A, B, sa, torch.ones(1, 1, G).permute(2, 0, 1), offs)
            case("scale_a outer-dim-major", A, B, torch.ones(1, M).t(), sb, offs)
            case("scale_b of the wrong shape", A, B, sa, torch.ones(G, 2, 1), offs)
        if recipe in mx_of:
            nb = K // 32
            case("scales in padded rows, read in place", A, B, torch.full((M, 2 * nb), 127, dtype=u8)[:, :nb],
                 torch.full((G, N + 1, 2 * nb), 127, dtype=u8)[:, :N, :nb], offs)
            case("scale_b with a row stride that is no multiple of 4, copied", A, B, sa, torch.full((G, N, nb + 1), 127, dtype=u8)[:, :, :nb], offs)
            case("scale_b at a misaligned base, copied", A, B, sa, torch.full((G * N * nb + 4,), 127, dtype=u8)[2:2 + G * N * nb].view(G, N, nb), offs)
            case("scale_a transposed, copied", A, B, torch.full((nb, M), 127, dtype=u8).t(), sb, offs)
            case("scales float8_e8m0fnu", A, B, sa.view(torch.float8_e8m0fnu), sb.view(torch.float8_e8m0fnu), offs)
            A64, sa64 = acts(recipe, M, 64)
            B64, sb64 = weights(recipe, G, N, 64)
            case("K = 64: scale rows of 2 bytes, copied", A64, B64, sa64, sb64, offs)
            case("K % 32", torch.zeros(M, 80 // mx_of[recipe], dtype=u8), torch.zeros(G, N, 80 // mx_of[recipe], dtype=u8), sa, sb, offs)

    suffix = {"row": "rowwise", "block128": "blockwise", "mxfp8": "mxfp8", "mxfp4": "mxfp4"}
    for recipe, name in suffix.items():
        linear, mlp, forward = (getattr(native, f"fp8_moe_{kind}_{name}") for kind in ("linear", "mlp", "forward"))
        w, ws = weights(recipe, G, N, K)
        w1, s1 = weights(recipe, G, 2 * H, K)
        w1u, s1u = weights(recipe, G, H, K)
        w2, s2 = weights(recipe, G, N, H)
        x, offs = torch.zeros(M, K), offs_of(M, G)

        def lin(label, *args, **kw):
            run(f"moe_linear_{name}: {label}", linear, *args, names=("x", "offs", "w_q", "w_scale"), **kw)

        lin("plain", x, offs, w, ws)
        lin("x bf16", x.to(bf16), offs, w, ws)
        lin("x float64", x.double(), offs, w, ws)
        lin("w_q with padded row and expert strides", x, offs, padded(w), ws)
        lin("w_q that must be copied", x, offs, transposed(w), ws)
        lin("offs int64", x, offs_of(M, G, torch.int64), w, ws)
        for dt in (f32, bf16, torch.float64):
            lin(f"bias {dt}", x, offs, w, ws, bias=torch.zeros(G, N, dtype=dt))
        lin("bias of the wrong length", x, offs, w, ws, bias=torch.zeros(G, N + 1))
        lin("out_dtype bf16", x, offs, w, ws, out_dtype=bf16)
        lin("M_total = 0", torch.zeros(0, K), offs, w, ws)
        lin("G = 1", x, offs_of(M, 1), *weights(recipe, 1, N, K))
        lin("kernel GEMM_64x64", x, offs, w, ws, kernel=L.KERNEL_GEMM_64x64)
        lin("x of the wrong width", torch.zeros(M, K + 32), offs, w, ws)

        def ml(label, *args, **kw):
            run(f"moe_mlp_{name}: {label}", mlp, *args, names=("x", "offs", "w1", "w1_scale", "w2", "w2_scale"), **kw)

        ml("gated", x, offs, w1, s1, w2, s2)
        ml("ungated", x, offs, w1u, s1u, w2, s2, gated=False)
        ml("act gelu_tanh, ungated", x, offs, w1u, s1u, w2, s2, "gelu_tanh", False)
        ml("w2 of the wrong hidden size", x, offs, w1u, s1u, w2, s2)
        ml("x bf16", x.to(bf16), offs, w1, s1, w2, s2)
        ml("w1 with padded strides, w2 that must be copied", x, offs, padded(w1), s1, transposed(w2), s2)
        ml("offs int64", x, offs_of(M, G, torch.int64), w1, s1, w2, s2)
        ml("biases", x, offs, w1, s1, w2, s2, bias1=torch.zeros(G, 2 * H), bias2=torch.zeros(G, N, dtype=bf16))
        ml("bias1 of the wrong length", x, offs, w1, s1, w2, s2, bias1=torch.zeros(G, H))
        ml("out_dtype f32 from bf16", x.to(bf16), offs, w1, s1, w2, s2, out_dtype=f32)
        ml("M_total = 0", torch.zeros(0, K), offs, w1, s1, w2, s2)
        ml("G = 1", x, offs_of(M, 1), *weights(recipe, 1, 2 * H, K), *weights(recipe, 1, N, H))
        ml("kernel GEMM_64x64", x, offs, w1, s1, w2, s2, kernel=L.KERNEL_GEMM_64x64)
        ml("x of the wrong width", torch.zeros(M, K + 32), offs, w1, s1, w2, s2)

        def fw(label, *args, **kw):
            run(f"moe_forward_{name}: {label}", forward, *args, names=("x", "topk_ids", "topk_weights", "w1", "w1_scale", "w2", "w2_scale"), **kw)

        T, k = 4, 2
        xt, ids, tw = torch.zeros(T, K), torch.tensor([[0, 1], [1, 0], [0, 1], [1, 1]]), torch.ones(T, k)
        fw("plain", xt, ids, tw, w1, s1, w2, s2)
        fw("topk_weights=None", xt, ids, None, w1, s1, w2, s2)
        fw("T = 0", torch.zeros(0, K), ids[:0], tw[:0], w1, s1, w2, s2)
        fw("T = 0, out_dtype bf16", torch.zeros(0, K), ids[:0], None, w1, s1, w2, s2, out_dtype=bf16)
        fw("ids int32, weights bf16", xt, ids.to(i32), tw.to(bf16), w1, s1, w2, s2)
        fw("x bf16", xt.to(bf16), ids, tw, w1, s1, w2, s2)
        fw("ungated", xt, ids, tw, w1u, s1u, w2, s2, gated=False)
        fw("w2 of the wrong hidden size", xt, ids, tw, w1u, s1u, w2, s2)
        fw("biases", xt, ids, tw, w1, s1, w2, s2, bias1=torch.zeros(G, 2 * H), bias2=torch.zeros(G, N))
        fw("out_dtype bf16", xt, ids, tw, w1, s1, w2, s2, out_dtype=bf16)
        fw("G = 1", xt, ids, tw, *weights(recipe, 1, 2 * H, K), *weights(recipe, 1, N, H))
        fw("kernel GEMM_64x64", xt, ids, tw, w1, s1, w2, s2, kernel=L.KERNEL_GEMM_64x64)
        fw("ids of another token count", xt, ids[:3], tw[:3], w1, s1, w2, s2)
        fw("x of the wrong width", torch.zeros(T, K + 32), ids, tw, w1, s1, w2, s2)

    def col(label, *args, **kw):
        run(f"grouped_colmajor: {label}", native.scaled_grouped_mm_colmajor, *args, names=("input", "mat2", "scale_a", "scale_b", "offs"), **kw)

    A, sa = acts("row", M, K)
    sb, offs = torch.ones(G, N), offs_of(M, G)
    mat2 = torch.zeros(G, N, K, dtype=u8).transpose(1, 2)   # (G, K, N), every expert column-major
    col("plain", A, mat2, sa, sb, offs)
    col("out_dtype bf16", A, mat2, sa, sb, offs, out_dtype=bf16)
    col("float8 operands", A.view(torch.float8_e4m3fn), mat2.view(torch.float8_e4m3fn), sa, sb, offs, out_dtype=bf16)
    col("mat2 with padded column and expert strides", A, torch.zeros(G, N + 1, K + 16, dtype=u8)[:, :N, :K].transpose(1, 2), sa, sb, offs)
    col("mat2 row-major", A, torch.zeros(G, K, N, dtype=u8), sa, sb, offs)
    col("input a transposed view", torch.zeros(K, M, dtype=u8).t(), mat2, sa, sb, offs)
    col("input a column slab of a wider buffer", torch.zeros(M, 2 * K, dtype=u8)[:, K:], mat2, sa, sb, offs)
    col("input 3D", A[None], mat2, sa, sb, offs)
    col("M_total = 0", A[:0], mat2, sa[:0], sb, offs)
    col("G = 1", A, mat2[:1], sa, sb[:1], offs_of(M, 1))
    col("offs int64", A, mat2, sa, sb, offs_of(M, G, torch.int64))
    col("K = 0", A[:, :0], mat2[:, :0], sa, sb, offs)


if __name__ == "__main__":
    assert len(sys.argv) >= 2 and sys.argv[1] == "record", __doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "fp8-mps-metal_amd"))
    import fp8_mi355x_lib
    import fp8_mi355x_native
    lib = fp8_mi355x_lib.load()
    for name, data in (("c", dict(c_front_end(lib, fp8_mi355x_lib), choosers=c_choosers(lib, fp8_mi355x_lib))), ("op", op_layer(fp8_mi355x_native))):
        with open(os.path.join(GOLDEN, f"gemm_frontend_{name}.json"), "w") as f:
            json.dump(data, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"gemm_frontend_{name}.json: {sum(len(v) for k, v in data.items() if k != 'choosers') if name == 'c' else len(data)} cases")
