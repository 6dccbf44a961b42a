"""The GEMM front end on the host (no GPU) against its recorded behaviour: the return code of every faulty call - each fault and each
pair of faults - of the four fp8mi_scaled_mm_* entry points, and the exact library call the op layer's GEMM functions make.  The
expectations (tests/golden/gemm_frontend_{c,op}.json) were recorded from the commit before the four families' front ends were merged
into shared helpers (tests/gemm_frontend_cases.py says how): the drift between the families that they hold - only the tensorwise path
skips the workspace for M = 1, MXFP4 compares its workspace threshold against bytes - is recorded behaviour, not a model.
The four grouped entry points, the two grouped choosers and the grouped / MoE functions of the op layer were recorded in the same way from
the commit before THEIR front ends were merged (DESIGN.md 5.13 lists the drift between the recipes that the fixtures hold)."""
import json
import os

import fp8_mi355x_lib as L
import gemm_frontend_cases as cases


def golden(name):
    with open(os.path.join(cases.GOLDEN, f"gemm_frontend_{name}.json")) as f:
        return json.load(f)


def test_c_front_end_return_codes():
    """No enumerated call reaches a launch (c_front_end asserts it before any comparison), and each returns what it always has."""
    got, want = cases.c_front_end(L.load(), L), golden("c")
    assert cases.c_choosers(L.load(), L) == want.pop("choosers")   # fp8mi_choose_kernel_grouped / _grouped_mx, the error returns included
    assert sorted(got) == sorted(want) and len(want) == 8
    for family in want:
        assert len(want[family]) > 200 and sorted(got[family]) == sorted(want[family]), family
        wrong = {k: (got[family][k], want[family][k]) for k in want[family] if got[family][k] != want[family][k]}
        assert not wrong, f"{family}: (returned, recorded) {wrong}"


def test_op_layer_calls():
    import fp8_mi355x_native as native
    got, want = cases.op_layer(native), golden("op")
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], label
    # the drift between the families, spelled out: who asks for a split-K workspace
    asked = {label: want[label]["workspace_asked"] for label in want}
    assert not asked["tensorwise: M = 1, K = 1024"] and asked["mxfp8: M = 1, K = 1024"] and asked["blockwise: M = 1, K = 1024"]
    assert not asked["mxfp4: K = 1024"] and asked["mxfp4: K = 2048"]
    assert want["tensorwise: e5m2 A"]["calls"][0][0] == "fp8mi_scaled_mm_fmt" and want["tensorwise: e5m2 A"]["calls"][0][1][17] == L.NAN_PROPAGATE
