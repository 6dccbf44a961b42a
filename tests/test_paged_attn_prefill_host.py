"""fp8mi_paged_attention_prefill on the host, no GPU: E_prefill recomputed and pinned; the split choice pinned."""
import fp8_mi355x_lib as L
import paged_attn_prefill_ref as P
import paged_attn_ref as R


def test_model_with_one_owner_per_split_stays_within_E_prefill():
    worst = P.measure_E_prefill()
    assert P.E_prefill - 1e-5 <= worst <= P.E_prefill and P.TOL_prefill == 2 * P.E_prefill and P.E_prefill < 2.0 ** -4, worst
    assert len(P.PREFILL_CASES) == 16 + 5 + 1 + 4 + 3 + 3 + 4 + 3 + 1 and R.WAVES == 4
    assert all(c.q.shape[0] > 0 and (vmax > 0).any() for c, _e, _ref, vmax in map(P.prefill_case, P.PREFILL_CASES))


def test_split_choice_pinned():   # two workgroups per CU (256, with or without a device), no split below four steps, no more than the workspace holds
    f, big = L.load().fp8mi_paged_attention_prefill_splits, 1 << 62
    assert f(512, 1, 512, 32, 8, 128, 8192, big) == 4      # 16 tiles x 8 KV heads = 128 workgroups
    assert f(512, 1, 512, 32, 8, 128, 8192, R.workspace_bytes(512, 32, 128, 3)) == 3 and f(512, 1, 512, 32, 8, 128, 8192, 0) == 1
    assert f(8, 8, 1, 4, 4, 128, 1 << 17, big) == 16 and f(40, 3, 33, 32, 8, 128, 512, big) == 1 and f(40, 3, 33, 5, 1, 128, 1300, big) == 3
    assert f(8, 1, 8, 34, 2, 128, 8192, big) == 0
