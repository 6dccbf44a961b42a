"""The cases of tests/test_gpu_gemm_entry.py and the generator of its fixture (not a test module).

The ring-tile GEMMs' kernel entry (tile map, descriptors, first stages' DMA) and tail (NaN verdict, split-K flag, epilogue scalars) may be
rearranged, but no output bit may change.  The fixture tests/golden/gemm_entry_parent.json holds the sha256 of every case's output bytes as
computed by the commit BEFORE such a change:

    python tests/make_gemm_entry_golden.py            (on an MI355X, on that commit's build)

Inputs come from numpy generators seeded by the case's name, never from the device RNG; the scales keep every output inside the range
of float16 (random e4m3 bytes at K = 1040 sum to ~1e6).  The cases are the smallest at which the entry
and tail can go wrong, pairwise rather than as a cross product (about 170 launches):

  kernels    the seven product ring tiles, the 256x256 ring tile, AUTO
  K          16 (one partial K-step, fewer stages than the prologue issues), 256 (one two-step stage), 272 (a stage and a tail),
             768 (three stages: the ring's depth), 1040 (the ring wraps, and a tail)
  extent     exactly one tile; one tile + 8 rows + 4 columns (masked rows, the unstaged epilogue)
  epilogue   scale_result and bias present / absent, row scales on / off, f32 / bf16 / f16 - rotated over the cases
  split-K    2 and 3 slices at K = 1040 (uneven slices that do not start at K = 0)
  NaN        a 0x7F byte in A's first K-step or in B's last, under NAN_ZERO (the scrubbed redo pass stages for itself) and propagated
  families   MXFP8, MXFP4, MXW4A8, blockwise and an e5m2 operand on the 128x64 tile at a stage (MXW4A8: two) and a tail of their own K units
  graph      eight launches captured as one graph, two C buffers over four weight buffers; each equals its eager result
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p in (os.path.join(ROOT, "fp8-mps-metal_amd"), os.path.join(ROOT, "oracle"), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fp8_mi355x_lib as L  # noqa: E402

FIXTURE = os.path.join(TESTS, "golden", "gemm_entry_parent.json")
MFMA_TOL = 1.0e-3       # tests/test_gpu_parity.py: the matrix core's truncation bound, any input
MFMA_RMS_TOL = 1.0e-4   # ... and its rms gate on random inputs

# kernel id -> (name, BM, BN); AUTO gets the 128x64 tile's extents (whatever it picks, the shape is one tile of the flagship kernel)
TILES = [(L.KERNEL_GEMM_128, "128x128", 128, 128), (L.KERNEL_GEMM_128x64, "128x64", 128, 64), (L.KERNEL_GEMM_64x128, "64x128", 64, 128),
         (L.KERNEL_GEMM_64x64, "64x64", 64, 64), (L.KERNEL_GEMM_32x64, "32x64", 32, 64), (L.KERNEL_GEMM_32x32, "32x32", 32, 32),
         (L.KERNEL_GEMM_128D, "128D", 128, 128), (L.KERNEL_GEMM_256, "256x256", 256, 256), (L.KERNEL_AUTO, "auto", 128, 64)]
KS = [16, 256, 272, 768, 1040]
OUTS = ["f32", "bf16", "f16"]
TORCH_OUT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _epilogue(i):
    """the i-th combination of (out dtype, bias, scale_result, row scales): 3 x 2 x 2 x 2, every pair of values within any 12 consecutive i"""
    return dict(out=OUTS[i % 3], bias=bool(i & 1), sr=bool((i >> 1) & 1), rows=bool((i >> 2) & 1))


def cases():
    out = []
    i = 0
    for kernel, name, bm, bn in TILES:
        for K in KS:
            for ragged in (False, True):
                out.append(dict(id=f"tw-{name}-K{K}-{'ragged' if ragged else 'tile'}", family="tw", kernel=kernel, M=bm + 8 * ragged, N=bn + 4 * ragged,
                                K=K, split=1, nan=None, nan_mode=L.NAN_ZERO, **_epilogue(i)))
                i += 1
    for kernel, name, bm, bn in TILES:
        for split in (2, 3):
            ragged = bool(i & 1)
            out.append(dict(id=f"tw-{name}-K1040-split{split}", family="tw", kernel=kernel, M=bm + 8 * ragged, N=bn + 4 * ragged, K=1040, split=split,
                            nan=None, nan_mode=L.NAN_ZERO, **_epilogue(i)))
            i += 1
    for kernel, name, bm, bn in TILES:
        for where in ("A-first", "B-last"):
            for mode, mname in ((L.NAN_ZERO, "zero"), (L.NAN_PROPAGATE, "propagate")):
                K = 1040 if name in ("128x64", "128D") else 272
                ragged = bool(i & 1)
                out.append(dict(id=f"tw-{name}-K{K}-nan-{where}-{mname}", family="tw", kernel=kernel, M=bm + 8 * ragged, N=bn + 4 * ragged, K=K, split=1,
                                nan=where, nan_mode=mode, **_epilogue(i)))
                i += 1
    # the other families on the 128x64 tile: one stage (two K-steps of 128 bytes) and a tail, in each family's units
    for family, K in (("mxfp8", 288), ("mxfp4", 544), ("bw", 272), ("e5m2", 272), ("mxw4a8", 544)):
        for ragged in (False, True):
            e = _epilogue(i)
            e["rows"] = e["rows"] and family == "e5m2"    # (the scaled families carry their scales per block)
            out.append(dict(id=f"{family}-128x64-K{K}-{'ragged' if ragged else 'tile'}", family=family, kernel=L.KERNEL_GEMM_128x64, M=128 + 8 * ragged,
                            N=64 + 4 * ragged, K=K, split=1, nan=None, nan_mode=L.NAN_PROPAGATE if family == "e5m2" else L.NAN_ZERO, **e))
            i += 1
    return out


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _clean(b, e5m2=False):
    if e5m2:
        return np.where((b & 0x7C) == 0x7C, b & 0xBF, b).astype(np.uint8)   # no inf / NaN encodings
    b = b.copy()
    b[(b & 0x7F) == 0x7F] ^= 1   # no e4m3 NaN bytes unless the case asks for them
    return b


def inputs(c):
    """-> dict of numpy arrays: A, B (bytes), sa, sb, bias (or None), sr (float or None)"""
    rng = _rng(c["id"])
    M, N, K, fam = c["M"], c["N"], c["K"], c["family"]
    kb = K // 2 if fam == "mxfp4" else K
    A = rng.integers(0, 256, size=(M, kb), dtype=np.uint8)
    B = rng.integers(0, 256, size=(N, K // 2 if fam == "mxw4a8" else kb), dtype=np.uint8)
    if fam == "mxw4a8":
        A = _clean(A)
    elif fam != "mxfp4":   # (e2m1 has no NaN encoding)
        A, B = _clean(A, fam == "e5m2"), _clean(B)
    if c["nan"] == "A-first":
        A[M // 3, 5] = 0x7F
    elif c["nan"] == "B-last":
        B[N // 2, K - 3] = 0x7F
    if fam in ("mxfp8", "mxfp4", "mxw4a8"):
        sa = rng.integers(108, 123, size=(M, K // 32), dtype=np.uint8)   # 2^-19 .. 2^-5
        sb = rng.integers(108, 123, size=(N, K // 32), dtype=np.uint8)
    elif fam == "bw":
        nkb = -(-K // 128)
        sa = np.exp2(rng.uniform(-9, -5, size=(M, nkb))).astype(np.float32)
        sb = (np.exp2(rng.uniform(-9, -5, size=(-(-N // 128), nkb))) * rng.choice([-1.0, 1.0], size=(-(-N // 128), nkb))).astype(np.float32)
    else:
        sa = (rng.uniform(0.25, 2.0, size=M if c["rows"] else 1) / 32).astype(np.float32)
        sb = (rng.uniform(0.25, 2.0, size=N if c["rows"] else 1) / 32).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) * 64 if c["bias"] else None
    sr = float(np.float32(rng.uniform(0.3, 3.0))) if c["sr"] else None
    return dict(A=A, B=B, sa=sa, sb=sb, bias=bias, sr=sr)


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def launch(native, c, x, dev, **more):
    """one launch of the case through the op layer (a thin wrapper of the C ABI: pointers, strides and the stream); x: device tensors"""
    kw = dict(kernel=c["kernel"], split_k=c["split"], out_dtype=TORCH_OUT[c["out"]], **more)
    if x["bias"] is not None:
        kw["bias"] = x["bias"]
    if x["sr"] is not None:
        kw["scale_result"] = x["sr"]
    fam = c["family"]
    if fam == "mxfp8":
        return native.fp8_scaled_mm_mxfp8(x["A"], x["B"], x["sa"], x["sb"], nan_mode=c["nan_mode"], **kw)
    if fam == "mxfp4":
        return native.fp8_scaled_mm_mxfp4(x["A"], x["B"], x["sa"], x["sb"], **kw)
    if fam == "mxw4a8":
        return native.fp8_scaled_mm_mxw4a8(x["A"], x["B"], x["sa"], x["sb"], nan_mode=c["nan_mode"], **kw)
    if fam == "bw":
        return native.fp8_scaled_mm_blockwise(x["A"], x["B"], x["sa"], x["sb"], block_a=1, block_b=128, nan_mode=c["nan_mode"], **kw)
    if fam == "e5m2":
        return native.fp8_scaled_mm(x["A"], x["B"], x["sa"], x["sb"], nan_mode=c["nan_mode"], a_format=L.FMT_E5M2, b_format=L.FMT_E4M3, **kw)
    return native.fp8_scaled_mm(x["A"], x["B"], x["sa"], x["sb"], nan_mode=c["nan_mode"], **kw)


def to_device(inp, dev):
    x = {k: (_dev(v, dev) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    if inp["sr"] is not None:
        x["sr"] = torch.full((1,), inp["sr"], dtype=torch.float32, device=dev)
    return x


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run_case(native, c, dev):
    """-> (output tensor, numpy inputs)"""
    inp = inputs(c)
    out = launch(native, c, to_device(inp, dev), dev)
    torch.cuda.synchronize()
    return out, inp


def reference(c, inp, oracle):
    """-> (exact, bound, eps, tiny, lanes that must be NaN): float64, the suite's oracles and bounds (tests/test_gpu_parity.py check_mm and
    the families' *_ref.py): |got - exact| <= tol x bound + eps x |exact| + tiny."""
    A, B, fam = inp["A"], inp["B"], c["family"]
    tol = MFMA_TOL
    if fam == "mxfp8":
        import mxfp8_ref
        exact, bound = mxfp8_ref.mm_ref(A, B, inp["sa"], inp["sb"], True)
    elif fam == "mxfp4":
        import mxfp4_ref
        exact, bound = mxfp4_ref.mm_ref(A, B, inp["sa"], inp["sb"])
    elif fam == "mxw4a8":
        import mxw4a8_ref
        exact, bound = mxw4a8_ref.mm_ref(A, B, inp["sa"], inp["sb"], True)
    elif fam == "bw":
        import blockwise_ref
        exact, bound = blockwise_ref.mm_ref(A, B, inp["sa"], inp["sb"], 1, 128, True)
        tol = MFMA_TOL + -(-c["K"] // 128) * 2.0 ** -23     # (tests/test_gpu_blockwise.py: the fold's own roundings)
    elif fam == "e5m2":
        import e5m2_ref
        exact, bound = e5m2_ref.mm_ref(A, B, inp["sa"], inp["sb"], 1, 0)
    else:
        exact = oracle.scaled_mm(A, B, inp["sa"], inp["sb"], accumulate="f64")     # (decodes NaN bytes to 0.0, the reference's rule)
        bound = oracle.abs_dot_bound(A, B, inp["sa"], inp["sb"])
    exact, bound = np.asarray(exact, np.float64), np.asarray(bound, np.float64)
    if inp["bias"] is not None:
        exact = exact + inp["bias"].astype(np.float64)[None, :]
        bound = bound + np.abs(inp["bias"].astype(np.float64))[None, :]
    if inp["sr"] is not None:
        exact, bound = exact * inp["sr"], bound * abs(inp["sr"])
    nan = np.zeros(exact.shape, bool)
    if c["nan"] and c["nan_mode"] == L.NAN_PROPAGATE:   # the row of A / of B_nk that holds the NaN byte poisons its outputs, and only those
        if c["nan"] == "A-first":
            nan[c["M"] // 3, :] = True
        else:
            nan[:, c["N"] // 2] = True
    eps = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[c["out"]]
    tiny = 2.0 ** -24 if c["out"] == "f16" else 0.0
    return exact, bound * tol, eps, tiny, nan


# ---- the graph case: the benchmark's replay pattern at one C3-shaped tile grid in small ----
GRAPH = dict(id="graph", family="tw", kernel=L.KERNEL_GEMM_128x64, M=256, N=128, K=768, split=1, nan=None, nan_mode=L.NAN_ZERO, out="f32", bias=False,
             sr=False, rows=False)
GRAPH_LAUNCHES, GRAPH_WEIGHTS, GRAPH_OUTS = 8, 4, 2


def graph_inputs():
    inp = inputs(GRAPH)
    rng = _rng("graph-weights")
    Bs = [_clean(rng.integers(0, 256, size=(GRAPH["N"], GRAPH["K"]), dtype=np.uint8)) for _ in range(GRAPH_WEIGHTS)]
    return inp, Bs


def run_graph(native, dev):
    """-> (eager outputs, graph outputs): launch i multiplies by weight buffer i mod 4 into C buffer i mod 2; a copy node keeps each result"""
    inp, Bs = graph_inputs()
    x = to_device(inp, dev)
    Bd = [_dev(b, dev) for b in Bs]
    Cs = [torch.zeros(GRAPH["M"], GRAPH["N"], dtype=torch.float32, device=dev) for _ in range(GRAPH_OUTS)]
    eager = []
    for i in range(GRAPH_LAUNCHES):
        launch(native, GRAPH, dict(x, B=Bd[i % GRAPH_WEIGHTS]), dev, out=Cs[i % GRAPH_OUTS])
        eager.append(Cs[i % GRAPH_OUTS].clone())
    torch.cuda.synchronize()
    for C in Cs:
        C.zero_()
    kept = [torch.zeros_like(Cs[0]) for _ in range(GRAPH_LAUNCHES)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(GRAPH_LAUNCHES):
            launch(native, GRAPH, dict(x, B=Bd[i % GRAPH_WEIGHTS]), dev, out=Cs[i % GRAPH_OUTS])
            kept[i].copy_(Cs[i % GRAPH_OUTS])
    g.replay()
    torch.cuda.synchronize()
    return eager, kept, inp, Bs


def main():
    import fp8_mi355x_native as native
    dev = torch.device("cuda:0")
    L.load()
    hashes = {}
    for c in cases():
        out, _ = run_case(native, c, dev)
        hashes[c["id"]] = digest(out)
    eager, _, _, _ = run_graph(native, dev)
    for i, t in enumerate(eager):
        hashes[f"graph-{i}"] = digest(t)
    with open(FIXTURE, "w") as f:
        json.dump(hashes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{os.path.basename(FIXTURE)}: {len(hashes)} outputs")


if __name__ == "__main__":
    main()
