"""The MoE gate on the host (no GPU): the two forms of the reference (tests/moe_gate_ref.py) against each other and against examples worked
by hand, the ordered-key map and sort word host and kernel share (csrc/fp8mi_moe_gate.h) as a program of its own, every argument error of
fp8mi_moe_gate through the built library (each check runs before any HIP call), the bindings and the op layer's assertions, and the share
of tokens the reference flags `close` on the scored-form inputs of tests/test_gpu_moe_gate.py and tests/test_gpu_moe_gate_edges.py."""
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from moe_gate_ref import (EDGE_CASES, EDGE_SEED, SCORED_CASES, SKIP_CAP, T_SCORED, as_logit_dtype, edge_dtypes, edge_inputs, edge_kwargs, gate_brute,
                          gate_ref, scored_inputs, scored_kwargs)

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------

def test_vectorised_reference_equals_the_brute_force_order():
    """A few hundred small random cases of every form, with ties, NaN, +-inf and +-0 mixed in."""
    rng = random.Random(20251)
    pool = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, 1.0, -1.0, 0.5, 2.0, -2.5, 3.0e38, -3.0e38, 1e-40, -1e-40]
    done = 0
    while done < 400:
        n_group = rng.choice([1, 1, 2, 3, 4])
        gs = rng.randint(1, 5)
        G = n_group * gs if n_group > 1 else rng.randint(1, 12)
        group_score = rng.choice(["max", "top2"])
        if n_group > 1 and group_score == "top2" and gs < 2:
            continue
        topk_group = rng.randint(1, n_group)
        k = rng.randint(1, topk_group * gs if n_group > 1 else G)
        T = rng.randint(1, 4)
        special = rng.random()
        x = np.array([[rng.choice(pool) if rng.random() < special else rng.uniform(-4, 4) for _ in range(G)] for _ in range(T)], dtype=np.float32)
        bias = None if rng.random() < 0.5 else np.array([rng.choice([0.0, 0.0, 0.25, -0.25, 1.0]) for _ in range(G)], dtype=np.float32)
        kw = dict(k=k, scoring=rng.choice(["softmax", "sigmoid"]), bias=bias, n_group=n_group, topk_group=topk_group, group_score=group_score)
        r = gate_ref(x, **kw)
        assert r.ids.tolist() == gate_brute(x, **kw), (x.tolist(), kw)
        assert all(len(set(row)) == k and all(0 <= e < G for e in row) for row in r.ids.tolist())
        done += 1


def test_plain_softmax_by_hand():
    x = np.array([[1.0, 3.0, 2.0, 0.0]], dtype=np.float32)
    e = [math.exp(v - 3.0) for v in (1.0, 3.0, 2.0, 0.0)]
    r = gate_ref(x, 2, "softmax")
    assert r.ids.tolist() == [[1, 2]] and not r.close.any()
    np.testing.assert_allclose(r.weights[0], [e[1] / sum(e), e[2] / sum(e)], rtol=1e-14)
    r = gate_ref(x, 2, "softmax", renormalize=True, scale=2.5)   # a softmax followed by the top-k, renormalised over the k
    np.testing.assert_allclose(r.weights[0], [2.5 * e[1] / (e[1] + e[2]), 2.5 * e[2] / (e[1] + e[2])], rtol=1e-14)


def test_bias_changes_the_selection_and_not_the_weights():
    x = np.array([[2.0, 1.0, 0.0, -1.0]], dtype=np.float32)
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))   # noqa: E731
    plain = gate_ref(x, 2, "sigmoid")
    assert plain.ids.tolist() == [[0, 1]]
    biased = gate_ref(x, 2, "sigmoid", bias=np.array([0.0, 0.0, 0.0, 5.0], dtype=np.float32))
    assert biased.ids.tolist() == [[3, 0]]   # the key of expert 3 is sigmoid(-1) + 5 ...
    np.testing.assert_allclose(biased.weights[0], [sig(-1.0), sig(2.0)], rtol=1e-14)   # ... its weight is the score
    assert gate_brute(x, 2, "sigmoid", bias=np.array([0.0, 0.0, 0.0, 5.0], dtype=np.float32)) == [[3, 0]]


def test_group_limited_max_and_top2_by_hand():
    # group 0 = experts 0..2 holds the largest score, group 1 = experts 3..5 the largest sum of two
    x = np.array([[3.0, -3.0, -3.0, 2.0, 1.5, -3.0]], dtype=np.float32)
    by_max = gate_ref(x, 2, "sigmoid", n_group=2, topk_group=1, group_score="max")
    by_top2 = gate_ref(x, 2, "sigmoid", n_group=2, topk_group=1, group_score="top2")
    assert by_max.ids.tolist() == [[0, 1]] and by_max.eligible.tolist() == [[True] * 3 + [False] * 3]   # (experts 1 and 2 tie: the lower index)
    assert by_top2.ids.tolist() == [[3, 4]] and by_top2.eligible.tolist() == [[False] * 3 + [True] * 3]
    assert gate_brute(x, 2, "sigmoid", n_group=2, topk_group=1, group_score="max") == [[0, 1]]
    assert gate_brute(x, 2, "sigmoid", n_group=2, topk_group=1, group_score="top2") == [[3, 4]]
    # both groups kept: nothing is excluded, the order is the ungrouped one on the same keys
    assert gate_ref(x, 3, "sigmoid", n_group=2, topk_group=2).ids.tolist() == [[0, 3, 4]]


def test_plain_ids_equal_torch_topk_on_tie_free_finite_inputs():
    g = torch.Generator().manual_seed(7)
    for G, k in ((8, 2), (64, 8), (257, 64), (1000, 8)):
        x = torch.randperm(G * 16, generator=g).reshape(16, G).float() * 0.01 - 3.0   # distinct values
        for scoring in ("softmax", "sigmoid"):
            r = gate_ref(x.numpy(), k, scoring)
            assert torch.equal(torch.from_numpy(r.ids), torch.topk(x, k).indices), (G, k)


def test_reference_ties_and_special_values():
    nan, inf = float("nan"), float("inf")
    assert gate_ref(np.zeros((1, 9), dtype=np.float32), 4).ids.tolist() == [[0, 1, 2, 3]]
    assert gate_ref(np.full((1, 9), -inf, dtype=np.float32), 4).ids.tolist() == [[0, 1, 2, 3]]
    assert gate_ref(np.array([[0.0, -0.0, 0.0, -0.0]], dtype=np.float32), 3).ids.tolist() == [[0, 1, 2]]
    assert gate_ref(np.array([[1.0, nan, inf, 5.0, -nan]], dtype=np.float32), 4).ids.tolist() == [[1, 4, 2, 3]]


# ---- the shared key header, as a host program -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_key_map_program(tmp_path, flags):
    """csrc/fp8mi_moe_gate.h under g++ (tests/c/moe_gate_key.cpp): the ordered-key map, the sort word and the launch geometry; once more as a
    stand-alone program with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "moe_gate_key")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "fp8-mps-metal_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "moe_gate_key.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"ok \d+", out.stdout.strip()), out.stdout + out.stderr


# ---- argument errors, before any HIP call ---------------------------------------------------------------------------------------------------

def gate(lib, logits=P, dtype=L.BF16, T=4, G=64, ld=None, bias=None, k=8, scoring=L.GATE_SOFTMAX, renorm=1, scale=1.0, n_group=1, topk_group=1,
         group_score=L.GATE_GROUP_MAX, ids=P, weights=P):
    return lib.fp8mi_moe_gate(logits, dtype, T, G, G if ld is None else ld, bias, k, scoring, renorm, scale, n_group, topk_group, group_score, ids,
                              weights, None)


def test_gate_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("logits", "ids", "weights"):
        assert gate(lib, **{name: None}) == E_NULL, name
        assert b"NULL" in err() and name.encode() in err()
    assert gate(lib, T=-1) == E_SHAPE and b"T=-1" in err()
    assert gate(lib, G=0) == E_SHAPE and b"G=0" in err()
    assert gate(lib, G=-3) == E_SHAPE
    assert gate(lib, k=0) == E_SHAPE and b"k=0" in err()
    assert gate(lib, k=-1) == E_SHAPE
    assert gate(lib, G=4, k=5) == E_SHAPE and b"k=5" in err()
    assert gate(lib, ld=63) == E_SHAPE and b"ld=63" in err()
    assert gate(lib, n_group=0) == E_SHAPE and b"n_group=0" in err()
    assert gate(lib, n_group=-2) == E_SHAPE
    assert gate(lib, n_group=3, topk_group=1) == E_SHAPE and b"n_group=3" in err()   # 64 % 3 != 0
    assert gate(lib, n_group=8, topk_group=0) == E_SHAPE and b"topk_group=0" in err()
    assert gate(lib, n_group=8, topk_group=9) == E_SHAPE and b"topk_group=9" in err()
    assert gate(lib, topk_group=2) == E_SHAPE                                         # n_group = 1
    assert gate(lib, n_group=8, topk_group=1, k=9) == E_SHAPE and b"k=9" in err()     # one group of 8 experts
    assert gate(lib, G=8, k=2, n_group=8, topk_group=4, group_score=L.GATE_GROUP_TOP2) == E_SHAPE and b"GROUP_TOP2" in err()
    assert gate(lib, dtype=3) == E_ENUM and b"dtype" in err()
    assert gate(lib, dtype=-1) == E_ENUM
    assert gate(lib, scoring=2) == E_ENUM and b"scoring" in err()
    assert gate(lib, group_score=2) == E_ENUM and b"group_score" in err()
    assert gate(lib, group_score=-1) == E_ENUM
    assert gate(lib, G=1025, ld=1025) == E_UNSUPPORTED and b"G=1025" in err()
    assert gate(lib, G=128, k=65) == E_UNSUPPORTED and b"k=65" in err()
    assert gate(lib, G=130, n_group=65, topk_group=65) == E_UNSUPPORTED and b"n_group=65" in err()
    assert gate(lib, T=1 << 28, k=8) == E_UNSUPPORTED and b"int32" in err()          # T k = 2^31
    assert gate(lib, T=(1 << 31) - 1, k=1, ids=None) == E_NULL                       # T k = 2^31 - 1 passes the size check
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert gate(lib, scale=bad) == E_UNSUPPORTED and b"scale" in err()
    assert gate(lib, logits=P + 1) == E_UNSUPPORTED and b"aligned" in err()
    assert gate(lib, logits=P + 2, dtype=L.F32) == E_UNSUPPORTED
    assert gate(lib, bias=P + 2) == E_UNSUPPORTED and gate(lib, ids=P + 2) == E_UNSUPPORTED and gate(lib, weights=P + 1) == E_UNSUPPORTED
    # T = 0 is a no-op that needs no pointers - but still validates
    none = dict(logits=None, ids=None, weights=None)
    assert gate(lib, T=0, **none) == 0
    assert gate(lib, T=0, n_group=8, topk_group=4, group_score=L.GATE_GROUP_TOP2, bias=None, **none) == 0
    assert gate(lib, T=0, k=65, G=128, **none) == E_UNSUPPORTED and gate(lib, T=0, G=0, **none) == E_SHAPE and gate(lib, T=0, scoring=7, **none) == E_ENUM
    assert gate(lib, T=0, scale=float("nan"), **none) == E_UNSUPPORTED


# ---- bindings and ops -------------------------------------------------------------------------------------------------------------------------

def test_gate_symbol_and_constants_match_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name in ("GATE_SOFTMAX", "GATE_SIGMOID", "GATE_GROUP_MAX", "GATE_GROUP_TOP2", "MOE_GATE_MAX_K"):
        assert int(re.search(r"#define FP8MI_" + name + r"\s+(\d+)", hdr).group(1)) == getattr(L, name), name
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_moe_gate.h")).read()
    assert int(re.search(r"kMoeGateMaxK = (\d+)", shared).group(1)) == L.MOE_GATE_MAX_K   # (the .hip file static_asserts it against the header)
    assert re.search(r"\bint\s+fp8mi_moe_gate\s*\(", hdr)
    assert len(L.SIGNATURES["fp8mi_moe_gate"][1]) == 16 and lib.fp8mi_moe_gate.argtypes == L.SIGNATURES["fp8mi_moe_gate"][1]
    assert lib.fp8mi_version() == 0x000400   # a new entry point only: the ABI version does not move


def test_op_layer_exposes_the_gate_and_asserts_its_arguments():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_moe_gate", "fp8_moe_layer"):
        assert callable(getattr(N, name)) and getattr(alias, name) is getattr(N, name), name
    x = torch.zeros(4, 8)
    with pytest.raises(AssertionError, match="scoring"):
        N.fp8_moe_gate(x, 2, scoring="tanh")
    with pytest.raises(AssertionError, match="group_score"):
        N.fp8_moe_gate(x, 2, group_score="top3")
    with pytest.raises(AssertionError, match="bias"):
        N.fp8_moe_gate(x, 2, bias=torch.zeros(7))
    with pytest.raises(AssertionError, match="k=65"):
        N.fp8_moe_gate(torch.zeros(4, 128), 65)
    with pytest.raises(AssertionError, match="recipe"):
        N.fp8_moe_layer(x, x, 2, None, None, None, None, recipe="tensorwise")


# ---- the skip cap of the scored-form GPU cases ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCORED_CASES))
def test_reference_alone_stays_under_the_skip_cap(name):
    """On the inputs tests/test_gpu_moe_gate.py runs (seed 0) and on two more seeds: the share of tokens whose selection the bounds of
    tests/moe_gate_ref.py cannot decide stays under SKIP_CAP, so the id comparison there covers at least 98 % of every case."""
    for seed in (0, 1, 2):
        x, bias = scored_inputs(name, seed)
        r = gate_ref(x, bias=bias, **scored_kwargs(name))
        assert x.shape[0] == T_SCORED
        share = float(r.close.mean())
        print(f"{name} seed {seed}: {100 * share:.2f} % of the tokens flagged close")
        assert share <= SKIP_CAP, (name, seed, share)


@pytest.mark.parametrize("name,dtype", [(n, d) for n in sorted(EDGE_CASES) for d in edge_dtypes(n)])
def test_reference_alone_stays_under_the_skip_cap_on_the_edge_cases(name, dtype):
    """The same for every (case, logit type) tests/test_gpu_moe_gate_edges.py runs, on the values after the conversion to the logit type: its
    seed and the three of the test above."""
    for seed in sorted({EDGE_SEED, 0, 1, 2}):
        x, bias = edge_inputs(name, seed)
        r = gate_ref(as_logit_dtype(x, dtype).float().numpy(), bias=bias, **edge_kwargs(name))
        assert x.shape[0] == T_SCORED
        share = float(r.close.mean())
        print(f"{name} {dtype} seed {seed}: {100 * share:.2f} % of the tokens flagged close")
        assert share <= SKIP_CAP, (name, dtype, seed, share)


def test_edge_case_table_covers_every_geometry_the_gate_has():
    """The table's own claims (no GPU): every E, power-of-two and other n_group, gs a multiple of E and not, gs < L, L = 1 at E > 1, lanes
    without a group, a NULL bias with groups, both scorings with both values of renormalize and of scale; every case a valid call."""
    seen = set()
    for name, (G, k, scoring, sigma, n_group, topk_group, group_score, renorm, scale) in EDGE_CASES.items():
        E, L_ = 1, 1
        while 64 * E < G:
            E *= 2
        while 2 * L_ * n_group <= 64:
            L_ *= 2
        gs = G // n_group
        assert G % n_group == 0 and 1 <= topk_group <= n_group and 1 <= k <= min(64, topk_group * gs if n_group > 1 else G), name
        assert group_score == "max" or gs >= 2, name
        seen |= {("E", E), (scoring, renorm), (scoring, scale), ("bias", sigma is not None, n_group > 1)}
        if n_group > 1:
            seen |= {("pow2", n_group & (n_group - 1) == 0), ("gs % E", gs % E == 0, E), ("gs < L", gs < L_), ("L", L_ == 1, E > 1),
                     ("idle lanes", n_group * L_ < 64)}
    want = {("E", e) for e in (1, 2, 4, 8, 16)} | {(s, v) for s in ("softmax", "sigmoid") for v in (True, False, 1.0, 2.5)}
    want |= {("bias", True, True), ("bias", True, False), ("bias", False, True), ("pow2", True), ("pow2", False), ("gs < L", True), ("L", True, True),
             ("idle lanes", True), ("gs % E", False, 2), ("gs % E", False, 4), ("gs % E", False, 8), ("gs % E", False, 16), ("gs % E", True, 8)}
    assert want <= seen, sorted(map(str, want - seen))
