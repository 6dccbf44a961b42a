"""The sparse MLA attention (fp8mi_mla_attention_sparse) on the host, no GPU: E_mla_sparse recomputed and pinned, the masked model against
mla_ref.attention_model on the compaction, the ABI's symbols, the split choice against its restatement, the argument checks through the built
library (each runs before any HIP call)."""
import inspect

import numpy as np
import pytest

import fp8_mi355x_lib as L
import mla_ref as R
import mla_sparse_ref as S

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_E_mla_sparse_is_what_the_model_measures():
    e = S.measure_E()
    assert e <= S.E_mla_sparse < e * 1.001 and S.TOL == 2 * S.E_mla_sparse, e


@pytest.mark.parametrize("name", S.PREFIX_CASES)
def test_the_masked_model_on_a_hole_free_list_is_the_decode_model_on_the_compaction(name):
    c = S.case(name)[0]
    assert S.prefix_n(c, 0) is not None and np.array_equal(S.masked_model(c), R.attention_model(S.compact(c, 0)))


def test_symbols_bindings_and_op_layer_arguments(lib):
    for name, n in (("fp8mi_mla_attention_sparse", 29), ("fp8mi_mla_attention_sparse_splits", 6)):
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    import fp8_mi355x_native as N
    params = inspect.signature(N.fp8_mla_paged_attention).parameters
    assert "indices" in params and params["indices"].default is None


def test_split_choice_restated(lib):
    """fp8mi_attn_auto_splits_mla_sparse through fp8mi_mla_attention_sparse_splits (without a device the library counts 256 compute units)"""
    info = L.DeviceInfo()
    cus = info.compute_units if lib.fp8mi_device_info(0, info) == 0 and info.compute_units > 0 else 256
    big, seen, f = 1 << 40, set(), lib.fp8mi_mla_attention_sparse_splits
    for Hq in (1, 16, 65, 128):
        for T, B, mq in ((1, 1, 1), (8, 8, 1), (12, 8, 2), (7, 2, 100), (64, 64, 1)):
            for topk in (1, 512, 513, 2048, 1 << 15):
                for ws in (big, T * Hq * 2 * 514 * 4, T * Hq * 2 * 514 * 4 - 1, 0):
                    assert f(T, B, mq, Hq, topk, ws) == S.auto_splits(T, B, min(mq, T), Hq, topk, ws, cus), (T, B, mq, Hq, topk, ws)
                    seen.add(f(T, B, mq, Hq, topk, ws))
    assert {1, 2, 4, 64} <= seen
    assert S.auto_splits(1, 1, 1, 16, 2048, big, 256) == 4 and S.auto_splits(64, 64, 1, 128, 2048, big, 256) == 4   # the four-step floor
    assert f(8, 8, 1, 129, 2048, big) == 0 and f(8, 8, 1, 16, 0, big) == 0 and f(-1, 1, 1, 4, 2048, big) == 0 and f(0, 1, 1, 4, 2048, big) == 1


def sparse(lib, ql=P, qp=P, q_dtype=L.BF16, T=6, B=2, cu=P, max_q_len=4, Hq=8, idx=P, topk=200, ld_idx=None, cache=P, nb=8, bs=16, bt=P, max_blocks=4, lens=P,
           kvs=P, splits=1, out=P):
    return lib.fp8mi_mla_attention_sparse(ql, qp, q_dtype, T, B, cu, max_q_len, Hq, Hq * 512, Hq * 64, idx, topk, topk if ld_idx is None else ld_idx, cache, nb, bs, bt,
                                          max_blocks, max_blocks, lens, kvs, 0.1, splits, None, 0, out, L.BF16, Hq * 512, None)


def test_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    assert sparse(lib, idx=None) == E_NULL and b"fp8mi_mla_attention_sparse: NULL" in err() and sparse(lib, out=None) == E_NULL
    assert sparse(lib, topk=0) == E_SHAPE and b"topk" in err() and sparse(lib, topk=-1) == E_SHAPE
    assert sparse(lib, ld_idx=199) == E_SHAPE and b"ld_idx" in err() and sparse(lib, ld_idx=208, out=None) == E_NULL
    assert sparse(lib, Hq=0) == E_SHAPE and sparse(lib, Hq=129) == E_UNSUPPORTED and b"MLA_MAX_HEADS" in err() and sparse(lib, Hq=128, out=None) == E_NULL
    assert sparse(lib, cu=None) == E_SHAPE and b"cu_seqlens_q" in err() and sparse(lib, cu=None, T=2, idx=None) == E_NULL   # the decode form: T = B
    assert sparse(lib, idx=P + 2) == E_UNSUPPORTED and b"indices" in err() and sparse(lib, topk=1 << 31) == E_UNSUPPORTED
    assert sparse(lib, nb=1 << 28) == E_UNSUPPORTED and b"cache rows" in err() and sparse(lib, splits=3) == E_UNSUPPORTED and b"workspace" in err()
    none = dict(ql=None, qp=None, cu=None, idx=None, cache=None, bt=None, lens=None, kvs=None, out=None)
    assert sparse(lib, B=0, T=0, **none) == 0 and sparse(lib, B=0, T=0, topk=0, **none) == E_SHAPE   # a no-op that still validates
