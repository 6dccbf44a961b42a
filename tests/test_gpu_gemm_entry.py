"""GPU (MI355X): the ring-tile GEMMs' kernel entry and tail compute what the previous commit computed, bit for bit.

The cases (tests/make_gemm_entry_golden.py says which and why) run once per module; each is checked against the float64 oracle with
the suite's matrix-core bound (tests/test_gpu_parity.py: 1e-3 x sum|a||b|, one more rounding for 16-bit outputs, rms gate 1e-4 on
random data) and against the sha256 of the previous commit's output bytes (tests/golden/gemm_entry_parent.json)."""
import json

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import make_gemm_entry_golden as G

pytestmark = pytest.mark.gpu

CASES = G.cases()


@pytest.fixture(scope="module")
def parent():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_case_list_covers_what_it_says():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids) and len(ids) <= 200
    tw = [c for c in CASES if c["family"] == "tw"]
    for kernel, name, _, _ in G.TILES:
        mine = [c for c in tw if c["kernel"] == kernel]
        assert {c["K"] for c in mine} == set(G.KS), name
        assert {c["split"] for c in mine} == {1, 2, 3}, name
        assert {(c["nan"], c["nan_mode"]) for c in mine if c["nan"]} == {(w, m) for w in ("A-first", "B-last") for m in (L.NAN_ZERO, L.NAN_PROPAGATE)}, name
        assert {c["out"] for c in mine} == set(G.OUTS) and {c["bias"] for c in mine} == {c["sr"] for c in mine} == {c["rows"] for c in mine} == {False, True}, name
    assert {c["family"] for c in CASES} == {"tw", "mxfp8", "mxfp4", "mxw4a8", "bw", "e5m2"}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_entry_case(native, cuda, oracle, parent, c):
    out, inp = G.run_case(native, c, cuda)
    assert out.shape == (c["M"], c["N"]) and out.dtype == G.TORCH_OUT[c["out"]]
    got = out.float().cpu().numpy().astype(np.float64)
    exact, allow, eps, tiny, nan = G.reference(c, inp, oracle)
    assert np.array_equal(np.isnan(got), nan), "NaN outputs are exactly those of the poisoned row / column"
    fin = ~nan
    err = np.abs(got - exact)[fin]
    lim = (allow + eps * np.abs(exact) + tiny + 1e-30)[fin]
    assert np.all(err <= lim), f"max err / allowed = {np.max(err / lim):.3e}"
    if c["out"] == "f32" and c["family"] in ("tw", "e5m2") and not c["nan"] and c["K"] >= 256:
        rms = np.sqrt(np.mean(err ** 2)) / (np.sqrt(np.mean((allow[fin] / G.MFMA_TOL) ** 2)) + 1e-300)
        assert rms <= G.MFMA_RMS_TOL, f"rms err / rms bound = {rms:.3e}"
    assert G.digest(out) == parent[c["id"]], "output bytes differ from the previous commit's"


def test_graph_of_eight_launches_equals_eager(native, cuda, oracle, parent):
    eager, kept, inp, Bs = G.run_graph(native, cuda)
    for i, (e, k) in enumerate(zip(eager, kept)):
        B = Bs[i % G.GRAPH_WEIGHTS]
        exact = oracle.scaled_mm(inp["A"], B, inp["sa"], inp["sb"], accumulate="f64")
        bound = oracle.abs_dot_bound(inp["A"], B, inp["sa"], inp["sb"])
        assert np.all(np.abs(e.cpu().numpy().astype(np.float64) - exact) <= G.MFMA_TOL * bound + 1e-30), i
        assert torch.equal(e, k), f"launch {i}: the graph's result differs from the eager one"
        assert G.digest(k) == parent[f"graph-{i}"], f"launch {i}: output bytes differ from the previous commit's"
