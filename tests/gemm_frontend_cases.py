"""What the GEMM front end does with its arguments, enumerated for tests/test_gemm_frontend_host.py (no GPU):

  c_front_end(lib)   the return code of every faulty call of the four fp8mi_scaled_mm_* entry points: each single fault and each pair
                     of a per-family list, on the base call of tests/test_mxfp8_host.py (M = N = 64, K = 128, fake aligned pointers);
  op_layer(native)   the entry point and the full argument tuple that the four GEMM functions of fp8_mi355x_native and
                     scaled_mm_colmajor hand to the library, with the library replaced by a recorder.

    python tests/gemm_frontend_cases.py record [PACKAGE_DIR]
writes both as tests/golden/gemm_frontend_{c,op}.json from the package in PACKAGE_DIR (default: this tree's).  The fixtures are the
behaviour of the commit BEFORE a change to the front end: record them there, then run the test on the change."""
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
    return {
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


# ---- the op layer ---------------------------------------------------------------------------------------------------------------

def op_layer(native):
    """-> {"function: case": {"calls": [[entry point, [arguments]]], "workspace_asked": bool, "returned_none" / "raised": ...}} with the module's
    device type, stream, library and workspace replaced as in test_transposed_epilogue_keyword_reaches_bias_dtype.  A pointer argument is
    written "<input tensor>+<byte offset>", "fresh" (memory the op layer allocated) or None."""
    import torch
    L = native._l
    saved = (native.DEVICE_TYPE, native._stream, L.load, native._workspace_on)
    calls, asked, named = [], [], {}
    workspace = torch.zeros(64, dtype=torch.uint8)

    class Recorder:
        def __getattr__(self, entry):
            def record(*args):
                calls.append([entry, [describe(a) for a in args]])
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

    def run(results, label, fn, *args, **kw):
        del calls[:], asked[:]
        named.clear()
        tensors = dict(zip(("A", "B", "scale_a", "scale_b"), args), **{k: v for k, v in kw.items() if isinstance(v, torch.Tensor)}, workspace=workspace)
        named.update({k: v for k, v in tensors.items() if v.numel() > 0})
        entry = {}
        try:
            ret = fn(*args, **kw)
            if ret is None:
                entry["returned_none"] = True
            else:
                entry["result"] = [list(ret.shape), str(ret.dtype), describe(ret.data_ptr()) if ret.numel() else None]
        except AssertionError as e:
            entry["raised"] = str(e)
        results[label] = dict(entry, calls=[c for c in calls], workspace_asked=bool(asked))

    native.DEVICE_TYPE, native._stream, L.load = "cpu", (lambda dev: 0), (lambda: Recorder())
    native._workspace_on = lambda dev, stream: (asked.append(1), workspace)[1]
    try:
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
        return results
    finally:
        native.DEVICE_TYPE, native._stream, L.load, native._workspace_on = saved


if __name__ == "__main__":
    assert len(sys.argv) >= 2 and sys.argv[1] == "record", __doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "fp8-mps-metal_amd"))
    import fp8_mi355x_lib
    import fp8_mi355x_native
    for name, data in (("c", c_front_end(fp8_mi355x_lib.load(), fp8_mi355x_lib)), ("op", op_layer(fp8_mi355x_native))):
        with open(os.path.join(GOLDEN, f"gemm_frontend_{name}.json"), "w") as f:
            json.dump(data, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"gemm_frontend_{name}.json: {sum(len(v) for v in data.values()) if name == 'c' else len(data)} cases")
