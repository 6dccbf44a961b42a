"""The fused producers and the dense layer ops on the host (no GPU) against their recorded behaviour: the return code of every faulty call -
each fault and each pair of faults - of the 6 fused-producer entry points of the C ABI, and the exact sequence of library calls, the results
and the assertion texts of fp8_act_quantize, fp8_norm_quantize, fp8_moe_scatter_quantize and the sixteen fp8_linear* / fp8_mlp_* /
fp8_norm_linear_* functions of the op layer.  The expectations (tests/golden/producer_frontend_{c,op}.json) were recorded from the commit
before the two families were moved onto shared front ends (tests/producer_frontend_cases.py says how, and states the pair rule): the drift
between the entry points that they hold - each one's order of checks, which launches each recipe makes - is recorded behaviour, not a
model (DESIGN.md 5.19 lists it)."""
import json
import os

import fp8_mi355x_lib as L
import producer_frontend_cases as cases

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h


def golden(name):
    with open(os.path.join(cases.GOLDEN, f"producer_frontend_{name}.json")) as f:
        return json.load(f)


def test_c_front_end_return_codes():
    """No enumerated call reaches a launch (c_front_end asserts it before any comparison); each call returns what it always has, and a
    single fault's message begins with the entry point's name wherever it did."""
    got, want = cases.c_front_end(L.load(), L), golden("c")
    assert sorted(got) == sorted(want) and len(want) == 6
    for entry in want:
        assert cases.count(want[entry]) >= 10 and sorted(got[entry]) == sorted(want[entry]), entry
        for variant, faults in want[entry].items():
            assert sorted(got[entry][variant]) == sorted(faults), (entry, variant)
            wrong = {k: (got[entry][variant][k], faults[k]) for k in faults if got[entry][variant][k] != faults[k]}
            assert not wrong, f"{entry}, {variant}: (returned, recorded) {wrong}"
            assert all(named for rc, named, _pairs in faults.values() if rc), (entry, variant)
    # the drift between the entry points, spelled out.  fp8mi_act_quantize looks at act ahead of scale_mode ahead of in_dtype (its messages
    # name what it refused); the scatter forms look at the cols envelope only behind every enum
    lib = L.load()
    assert lib.fp8mi_act_quantize(cases.P, 3, 4, 64, 64, 4, cases.P, 64, cases.P, 1, 1, None, 2, 0, L.ENC_RNE, None) == E_ENUM
    assert b"unknown act" in lib.fp8mi_last_error()
    assert lib.fp8mi_act_quantize(cases.P, 3, 4, 64, 64, L.ACT_SILU, cases.P, 64, cases.P, 1, 1, None, 2, 0, L.ENC_RNE, None) == E_ENUM
    assert b"scale_mode" in lib.fp8mi_last_error()
    def pair(entry, variant, a, b):
        faults = want[entry][variant]
        return faults[a][2][b] if b in faults[a][2] else faults[b][2][a]

    assert pair("fp8mi_moe_scatter_quantize", "e4m3", "bad encode_mode", "cols % 16") == E_ENUM
    assert pair("fp8mi_moe_scatter_quantize", "e4m3", "e5m2", "cols % 16") == E_UNSUPPORTED
    assert pair("fp8mi_moe_scatter_quantize", "e4m3", "negative scale row stride", "cols % 16") == E_SHAPE
    assert pair("fp8mi_moe_scatter_quantize_mx", "mxfp8", "bad in_dtype", "cols = 16416") == E_ENUM
    # the norm forms report a half-given pair of pointers between the two empty problems: behind rows = 0, ahead of cols = 0
    for entry, variant, no_cols in (("fp8mi_norm_quantize", "e4m3", "GROUP128, cols = 0"), ("fp8mi_norm_quantize_mx", "mxfp4", "cols = 0")):
        assert pair(entry, variant, "rows = 0", "mod_scale without mod_shift") == 0
        assert pair(entry, variant, "mod_scale without mod_shift", no_cols) == E_NULL
        assert pair(entry, variant, "residual without h_out", no_cols) == E_NULL and pair(entry, variant, "NULL in", no_cols) == 0
    # ... where the activation forms end an empty problem of either kind before they look at a pointer
    assert pair("fp8mi_act_quantize_mx", "mxfp8", "NULL in", "cols = 0") == 0
    assert pair("fp8mi_act_quantize", "e4m3", "NULL scales", "GROUP128, cols = 0") == 0


def test_op_layer_calls():
    import fp8_mi355x_native as native
    got, want = cases.op_layer(native), golden("op")
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], label
    dense = {name for names in cases.DENSE.values() for name in names[:3] if name}
    assert len(dense) == 16
    assert {label.split(":")[0] for label in want} == dense | {"fp8_act_quantize", "fp8_norm_quantize", "fp8_moe_scatter_quantize"}
    # the launch choices of the recipes, spelled out: which quantiser each function runs on x
    first = lambda label: want[label]["calls"][0][0]   # noqa: E731
    assert first("fp8_linear_blockwise: plain") == "fp8mi_quantize_blockwise" and first("fp8_mlp_blockwise: plain") == "fp8mi_act_quantize"
    assert first("fp8_linear_mxfp8: plain") == "fp8mi_quantize_mxfp8" and first("fp8_mlp_mxfp8: plain") == "fp8mi_act_quantize_mx"
    assert first("fp8_linear_mxw4a8: plain") == "fp8mi_quantize_mxfp8" and first("fp8_linear_mxfp4: plain") == "fp8mi_quantize_mxfp4"
    assert first("fp8_mlp_rowwise: plain") == "fp8mi_quantize_rowwise" and first("fp8_norm_linear_rowwise: plain") == "fp8mi_norm_quantize"
    assert [c[0] for c in want["fp8_mlp_mxw4a8: plain"]["calls"]] == ["fp8mi_act_quantize_mx", "fp8mi_scaled_mm_mxw4a8"] * 2
    # fp8_mlp_rowwise takes its first layer from fp8_linear_rowwise: a wrong feature count names the weight as that function does
    assert "weight expects" in want["fp8_mlp_rowwise: the wrong feature count for x"]["raised"]
    assert "w1 expects" in want["fp8_mlp_blockwise: the wrong feature count for x"]["raised"]
