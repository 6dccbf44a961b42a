"""The stand-alone casts and quantisers on the host (no GPU) against their recorded behaviour: the return code of every faulty call - each
fault and each pair of faults - of the 16 cast entry points of the C ABI, and the exact library call, the results and the assertion texts
of the 15 fp8_* cast functions of the op layer.  The expectations (tests/golden/cast_frontend_{c,op}.json) were recorded from the commit
before the family's three layers were merged into shared bodies (tests/cast_frontend_cases.py says how): the drift between the recipes
that they hold - each entry point's order of checks, the words of the assertions, which empty inputs still reach the library - is
recorded behaviour, not a model (DESIGN.md 5.15 lists it)."""
import json
import os

import fp8_mi355x_lib as L
import cast_frontend_cases as cases


def golden(name):
    with open(os.path.join(cases.GOLDEN, f"cast_frontend_{name}.json")) as f:
        return json.load(f)


def test_c_front_end_return_codes():
    """No enumerated call reaches a launch and every single fault leaves a message that begins with the entry point's name (c_front_end
    asserts both before any comparison); each call returns what it always has."""
    got, want = cases.c_front_end(L.load(), L), golden("c")
    assert sorted(got) == sorted(want) and len(want) == 16   # fp8mi_dequant_f16, the alias, is one of them
    for entry in want:
        assert len(want[entry]) >= 10 and sorted(got[entry]) == sorted(want[entry]), entry
        wrong = {k: (got[entry][k], want[entry][k]) for k in want[entry] if got[entry][k] != want[entry][k]}
        assert not wrong, f"{entry}: (returned, recorded) {wrong}"
    assert want["fp8mi_dequant_f16"] == want["fp8mi_dequant"]
    # the drift between the entry points, spelled out: a NULL pointer is reported ahead of a bad enum by the flat casts and behind it by the
    # 2-D ones, which also look at sizes and leading dimensions before the empty problem
    assert want["fp8mi_encode"]["NULL in + bad in_dtype"] == -1 and want["fp8mi_quantize_mxfp8"]["NULL in + bad in_dtype"] == -3
    assert want["fp8mi_dequant"]["count = 0 + bad out_dtype"] == 0 and want["fp8mi_dequant_mxfp8"]["rows = 0 + bad out_dtype"] == -3


def test_op_layer_calls():
    import fp8_mi355x_native as native
    got, want = cases.op_layer(native), golden("op")
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], label
    assert {label.split(":")[0] for label in want} == {
        "fp8_dequantize", "fp8_encode", "fp8_quantize", "fp8_amax", "fp8_encode_e5m2", "fp8_dequantize_e5m2", "fp8_quantize_e5m2",
        "fp8_quantize_mxfp8", "fp8_quantize_mxfp4", "fp8_dequantize_mxfp8", "fp8_dequantize_mxfp4", "fp8_quantize_blockwise",
        "fp8_dequantize_blockwise", "fp8_quantize_rowwise", "fp8_dequantize_rowwise"}
    # the drift between the functions, spelled out: which empty inputs still reach the library
    reaches = {label: bool(want[label]["calls"]) for label in want}
    assert not reaches["fp8_dequantize: zero rows"] and not reaches["fp8_encode: zero rows"] and not reaches["fp8_encode_e5m2: zero rows"]
    assert reaches["fp8_quantize: zero rows"] and reaches["fp8_amax: zero rows"] and reaches["fp8_quantize_e5m2: zero rows"]
    assert reaches["fp8_quantize_mxfp8: zero rows"] and reaches["fp8_dequantize_blockwise: zero columns"] and reaches["fp8_quantize_rowwise: zero rows"]
