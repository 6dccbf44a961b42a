"""The MLA reference (tests/mla_ref.py) and the split rule, on the CPU."""
import os
import sys

import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle")]
import mla_ref as R  # noqa: E402


def test_E_mla_is_what_the_model_measures():
    e = R.measure_E()
    assert e <= R.E_mla < e * 1.001 and R.TOL_mla == 2 * R.E_mla, e


def test_the_rope_dominant_case_catches_a_kernel_without_its_fifth_k_step():
    c, ref, vmax = R.case("rope-dominant")
    assert R.ratio(R.attention_ref(c, rope=False)[0], ref, vmax) > R.TOL_mla


@pytest.mark.parametrize("B,Hq,max_seq,ws,want", [(1, 16, 512, 1 << 40, 1), (1, 16, 8192, 1 << 40, 16), (1, 128, 32768, 1 << 40, 64),
                                                  (64, 128, 32768, 1 << 40, 4), (8, 65, 4096, 8 * 65 * 3 * 514 * 4, 3), (512, 16, 32768, 1 << 40, 1)])
def test_split_rule(B, Hq, max_seq, ws, want):
    """fp8mi_attn_auto_splits_mla (csrc/fp8mi_attn.h) at 256 compute units, restated in mla_ref.auto_splits, against values worked out by hand;
    tests/test_gpu_mla.py holds the library to the restatement on the device's own count"""
    assert R.auto_splits(B, Hq, max_seq, ws, 256) == want
