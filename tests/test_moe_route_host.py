"""MoE routing on the host (no GPU): the reference of tests/moe_route_ref.py against a brute-force count, the index arithmetic host and
kernels share (csrc/fp8mi_moe_route.h) as a program of its own, every argument error of fp8mi_moe_route / _scatter_quantize / _combine through
the built library (each check runs before any HIP call), the workspace size, and the bindings."""
import os
import random
import re
import subprocess

import pytest
import torch

import fp8_mi355x_lib as L
from moe_route_ref import combine_f64, combine_ref, route_brute, route_ref

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------

def test_route_reference_equals_the_brute_force_count():
    """A few hundred random small cases (n <= 40, G <= 9) with dropped ids mixed in, and the edge cases by hand."""
    rng = random.Random(20250)
    special = [-1, INT32_MIN, INT32_MAX, (1 << 32) + 1, -(1 << 40)]
    cases = [([], 3), ([0], 1), ([5], 3), ([2, 2, 2, 2], 3), ([-1, 7, 3], 3)]
    for _ in range(300):
        G = rng.randint(1, 9)
        n = rng.randint(0, 40)
        cases.append(([rng.choice(special + [G]) if rng.random() < 0.15 else rng.randrange(G) for _ in range(n)], G))
    for ids, G in cases:
        offs, row_of, src = route_ref(torch.tensor(ids, dtype=torch.int64), G)
        b_offs, b_row_of, b_src = route_brute(ids, G)
        assert offs.tolist() == b_offs and row_of.tolist() == b_row_of and src.tolist() == b_src, (ids, G)


def test_route_reference_on_the_issue_example():
    ids = torch.tensor([[1, 0], [1, 1], [2, 5], [0, -1], [1, 2]])   # T = 5, k = 2, G = 3; the token (1, 1) owns two rows; 5 and -1 are dropped
    offs, row_of, src = route_ref(ids, 3)
    assert offs.tolist() == [2, 6, 8]
    assert row_of.tolist() == [2, 0, 3, 4, 6, -1, 1, -1, 5, 7]
    assert src.tolist() == [1, 6, 0, 2, 3, 8, 4, 9, -1, -1]


def test_combine_reference_is_the_sequential_float32_loop():
    y = torch.tensor([[1.0, 2.0], [3.0, 4.0], [1e8, -1e8]])
    row_of = torch.tensor([[2, 0, 1], [-1, 7, -1], [1, -1, 1]])
    w = torch.tensor([[1.0, 0.5, 2.0], [1.0, 1.0, 1.0], [0.25, 9.0, 0.25]])
    out = combine_ref(y, row_of, w, torch.float32)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    assert out[0, 0] == (f32(1e8) + f32(0.5)) + f32(6.0) and out[1].tolist() == [0.0, 0.0] and out[2].tolist() == [1.5, 2.0]
    total, mag = combine_f64(y, row_of, w)
    assert total[0, 0] == 1e8 + 0.5 + 6.0 and mag[0, 1] == 1e8 + 1.0 + 8.0
    assert combine_ref(y, row_of, None, torch.bfloat16)[2].tolist() == [6.0, 8.0]


# ---- the shared index header, as a host program ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_index_arithmetic_program(tmp_path, flags):
    """csrc/fp8mi_moe_route.h under g++: the form choice, the walk over workgroups / waves / lanes in assignment order, the workspace
    layout and its size (tests/c/moe_route_index.cpp); once more as a stand-alone program with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "moe_route_index")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "fp8-mps-metal_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "moe_route_index.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok 144", out.stdout + out.stderr


def test_exported_constants_match_the_header_and_the_index_header():
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    idx = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_moe_route.h")).read()
    assert int(re.search(r"#define FP8MI_MOE_ROUTE_CHUNK (\d+)", hdr).group(1)) == L.MOE_ROUTE_CHUNK
    assert int(re.search(r"#define FP8MI_MOE_ROUTE_SINGLE_MAX (\d+)", hdr).group(1)) == L.MOE_ROUTE_SINGLE_MAX
    assert "kMoeRouteSingleMax = kMoeRouteChunk" in idx and L.MOE_ROUTE_SINGLE_MAX == L.MOE_ROUTE_CHUNK   # (the .hip file static_asserts the values)


# ---- argument errors, before any HIP call ---------------------------------------------------------------------------------------------------

def route(lib, ids=P, id_bytes=8, n=64, G=8, offs=P, row_of=P, src=P, ws=None, ws_bytes=0):
    return lib.fp8mi_moe_route(ids, id_bytes, n, G, offs, row_of, src, ws, ws_bytes, None)


def scatter(lib, x=P, dtype=L.BF16, T=4, cols=128, ld_in=None, row_of=P, k=2, out=P, rows_out=8, ld_out=None, scales=P, s_sr=1, s_sk=1,
            mode=L.QSCALE_ROW, fmt=L.FMT_E4M3, enc=L.ENC_RNE):
    return lib.fp8mi_moe_scatter_quantize(x, dtype, T, cols, cols if ld_in is None else ld_in, row_of, k, out, rows_out,
                                          cols if ld_out is None else ld_out, scales, s_sr, s_sk, mode, fmt, enc, None)


def combine(lib, y=P, y_dtype=L.BF16, rows=8, N=64, ld_y=None, row_of=P, w=P, T=4, k=2, out=P, out_dtype=L.BF16, ld_out=None):
    return lib.fp8mi_moe_combine(y, y_dtype, rows, N, N if ld_y is None else ld_y, row_of, w, T, k, out, out_dtype, N if ld_out is None else ld_out, None)


def test_route_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("ids", "offs", "row_of"):
        assert route(lib, **{name: None}) == E_NULL, name
        assert b"NULL" in err()
    big = L.MOE_ROUTE_SINGLE_MAX + 1
    need = lib.fp8mi_moe_route_workspace_bytes(big, 8)
    assert route(lib, n=big, ws=None, ws_bytes=need) == E_NULL and b"workspace" in err()
    assert route(lib, n=big, ws=P, ws_bytes=need - 1) == E_SHAPE and b"workspace" in err()
    assert route(lib, n=-1) == E_SHAPE and b"negative" in err()
    assert route(lib, ws_bytes=-1) == E_SHAPE
    assert route(lib, G=0) == E_SHAPE and b"G=0" in err()
    assert route(lib, G=-2) == E_SHAPE
    assert route(lib, G=1025) == E_UNSUPPORTED and b"G=1025" in err()
    assert route(lib, n=1 << 31) == E_UNSUPPORTED and b"int32" in err()
    for width in (0, 1, 2, 3, 5, 16, -4):
        assert route(lib, id_bytes=width) == E_ENUM, width
        assert b"int32 (4) or int64 (8)" in err()
    assert route(lib, ids=P + 4, id_bytes=8) == E_UNSUPPORTED and b"aligned" in err()
    assert route(lib, ids=P + 2, id_bytes=4) == E_UNSUPPORTED
    assert route(lib, offs=P + 2) == E_UNSUPPORTED and route(lib, row_of=P + 1) == E_UNSUPPORTED and route(lib, src=P + 3) == E_UNSUPPORTED
    # n = 0 is a no-op that needs no pointers - but still validates
    none = dict(ids=None, offs=None, row_of=None, src=None)
    assert route(lib, n=0, **none) == 0
    assert route(lib, n=0, G=0, **none) == E_SHAPE and route(lib, n=0, G=1025, **none) == E_UNSUPPORTED and route(lib, n=0, id_bytes=2, **none) == E_ENUM


def test_route_workspace_bytes(lib):
    ws = lib.fp8mi_moe_route_workspace_bytes
    chunk, single = L.MOE_ROUTE_CHUNK, L.MOE_ROUTE_SINGLE_MAX
    # the one-launch form needs none
    for n in (0, 1, 512, single):
        for G in (1, 8, 1024):
            assert ws(n, G) == 0, (n, G)
    assert ws(single + 1, 1) > 0
    # non-decreasing in n and in G; room for a count per (workgroup, expert) and a total per expert
    ns = [0, 1, single - 1, single, single + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 5, 65536, 10 ** 6, (1 << 31) - 1]
    Gs = [1, 2, 8, 9, 64, 65, 256, 1024]
    for G in Gs:
        sizes = [ws(n, G) for n in ns]
        assert sizes == sorted(sizes) and all(s >= 0 and s % 16 == 0 for s in sizes), (G, sizes)
    for n in ns:
        sizes = [ws(n, G) for G in Gs]
        assert sizes == sorted(sizes), (n, sizes)
        if n > single:
            assert all(s >= 4 * (-(-n // chunk) * G + G) for s, G in zip(sizes, Gs)), (n, sizes)
    # the sizes fp8mi_moe_route rejects
    assert ws(-1, 8) == E_SHAPE and ws(64, 0) == E_SHAPE and ws(64, 1025) == E_UNSUPPORTED and ws(1 << 31, 8) == E_UNSUPPORTED


def test_scatter_quantize_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("x", "row_of", "out", "scales"):
        assert scatter(lib, **{name: None}) == E_NULL, name
        assert b"NULL" in err()
    for name in ("T", "cols", "k", "rows_out"):
        assert scatter(lib, **{name: -1}) == E_SHAPE, name
    assert scatter(lib, ld_in=112) == E_SHAPE and b"leading dimension" in err()
    assert scatter(lib, ld_out=127) == E_SHAPE
    assert scatter(lib, s_sr=-1) == E_SHAPE and scatter(lib, mode=L.QSCALE_GROUP128, s_sk=-1) == E_SHAPE
    assert scatter(lib, dtype=3) == E_ENUM and b"in_dtype" in err()
    assert scatter(lib, mode=2) == E_ENUM and b"scale_mode" in err()
    assert scatter(lib, fmt=2) == E_ENUM and b"out_format" in err()
    assert scatter(lib, enc=2) == E_ENUM and b"encode mode" in err()
    # no generic form: FP8MI_E_UNSUPPORTED
    for cols in (8, 24, 120, 127, 4104):
        assert scatter(lib, cols=cols) == E_UNSUPPORTED, cols
        assert b"multiple of 16" in err()
    assert scatter(lib, cols=16400) == E_UNSUPPORTED and b"16384" in err()
    assert scatter(lib, x=P + 8) == E_UNSUPPORTED and b"16-byte loads" in err()
    assert scatter(lib, out=P + 4) == E_UNSUPPORTED
    assert scatter(lib, ld_in=132) == E_UNSUPPORTED          # 264 bytes per bf16 row
    assert scatter(lib, ld_in=130, dtype=L.F32) == E_UNSUPPORTED
    assert scatter(lib, ld_out=132) == E_UNSUPPORTED
    assert scatter(lib, row_of=P + 2) == E_UNSUPPORTED and scatter(lib, scales=P + 2) == E_UNSUPPORTED
    assert scatter(lib, fmt=L.FMT_E5M2) == E_UNSUPPORTED and b"e4m3 only" in err()
    assert scatter(lib, mode=L.QSCALE_GROUP128, enc=L.ENC_REFERENCE) == E_UNSUPPORTED and b"FP8MI_ENC_RNE" in err()
    # T = 0 or k = 0 is a no-op that needs no pointers - but still validates
    none = dict(x=None, row_of=None, out=None, scales=None)
    assert scatter(lib, T=0, **none) == 0 and scatter(lib, k=0, **none) == 0
    assert scatter(lib, T=0, cols=24, **none) == E_UNSUPPORTED and scatter(lib, k=0, dtype=9, **none) == E_ENUM


def test_combine_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("y", "row_of", "out"):
        assert combine(lib, **{name: None}) == E_NULL, name
        assert b"NULL" in err()
    for name in ("rows", "N", "T", "k"):
        assert combine(lib, **{name: -1}) == E_SHAPE, name
    assert combine(lib, ld_y=63) == E_SHAPE and b"leading dimension" in err()
    assert combine(lib, ld_out=63) == E_SHAPE
    assert combine(lib, y_dtype=3) == E_ENUM and b"y_dtype" in err()
    assert combine(lib, out_dtype=-1) == E_ENUM and b"out_dtype" in err()
    assert combine(lib, y=P + 1) == E_UNSUPPORTED and b"aligned" in err()
    assert combine(lib, out=P + 2, out_dtype=L.F32) == E_UNSUPPORTED
    assert combine(lib, row_of=P + 2) == E_UNSUPPORTED and combine(lib, w=P + 2) == E_UNSUPPORTED
    none = dict(y=None, row_of=None, w=None, out=None)
    assert combine(lib, T=0, **none) == 0 and combine(lib, N=0, ld_y=0, ld_out=0, **none) == 0
    assert combine(lib, T=0, N=-1, **none) == E_SHAPE and combine(lib, T=0, y_dtype=7, **none) == E_ENUM


# ---- bindings ---------------------------------------------------------------------------------------------------------------------------------

def test_moe_route_symbols_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, nargs in (("fp8mi_moe_route_workspace_bytes", 2), ("fp8mi_moe_route", 10), ("fp8mi_moe_scatter_quantize", 17), ("fp8mi_moe_combine", 13)):
        assert re.search(r"\bint(64_t)?\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_op_layer_exposes_the_routing_ops():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_moe_route", "fp8_moe_scatter_quantize", "fp8_moe_combine", "fp8_moe_forward_rowwise", "fp8_moe_forward_blockwise"):
        assert callable(getattr(N, name)), name
        assert getattr(alias, name) is getattr(N, name), name
