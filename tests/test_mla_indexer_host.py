"""The lightning indexer (fp8mi_mla_index_*) on the host, no GPU: the ABI's symbols and bindings, the op layer's parameters, the argument checks
through the built library (each runs before any HIP call), and topk_ref against a brute-force selection."""
import functools
import inspect

import numpy as np
import pytest

import fp8_mi355x_lib as L
import mla_indexer_ref as I

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_symbols_bindings_and_op_layer_parameters(lib):
    for name, n in (("fp8mi_mla_index_cache_bytes", 2), ("fp8mi_mla_index_cache_append", 11), ("fp8mi_mla_index_logits", 21), ("fp8mi_mla_index_topk", 12)):
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_mla_index_cache_bytes(3, 64) == 3 * 64 * 132 and lib.fp8mi_mla_index_cache_bytes(3, 48) == 0 and lib.fp8mi_mla_index_cache_bytes(-1, 16) == 0
    import fp8_mi355x_native as N
    want = {"fp8_mla_index_cache_alloc": ["num_blocks", "block_size"], "fp8_mla_index_cache_append": ["k", "cache", "slot_mapping", "encode_mode"],
            "fp8_mla_index_logits": ["q", "weights", "cache", "block_table", "seq_lens", "cu_seqlens_q", "max_q_len", "max_seq_len", "out"],
            "fp8_mla_index_topk": ["logits", "seq_lens", "topk", "cu_seqlens_q", "max_q_len", "out"],
            "fp8_mla_indexer": ["q", "weights", "cache", "block_table", "seq_lens", "topk", "cu_seqlens_q", "max_q_len", "max_seq_len", "logits"]}
    for fn, names in want.items():
        assert [p for p in inspect.signature(getattr(N, fn)).parameters if p != "device"] == names, fn


def append(lib, k=P, dtype=L.BF16, T=4, ld_k=128, cache=P, nb=8, bs=16, slots=P, slot_bytes=8, mode=L.ENC_RNE):
    return lib.fp8mi_mla_index_cache_append(k, dtype, T, ld_k, cache, nb, bs, slots, slot_bytes, mode, None)


def logits(lib, q=P, dtype=L.BF16, w=P, T=6, B=2, cu=P, max_q_len=4, Hi=64, ld_q=None, ld_w=None, cache=P, nb=8, bs=16, bt=P, ld_bt=4, max_blocks=4, lens=P,
           max_seq_len=64, out=P, ld_logits=64):
    return lib.fp8mi_mla_index_logits(q, dtype, w, T, B, cu, max_q_len, Hi, Hi * 128 if ld_q is None else ld_q, Hi if ld_w is None else ld_w, cache, nb, bs, bt, ld_bt,
                                      max_blocks, lens, max_seq_len, out, ld_logits, None)


def topk(lib, x=P, ld_logits=64, n_cols=64, T=6, B=2, cu=P, max_q_len=4, lens=P, k=8, idx=P, ld_idx=8):
    return lib.fp8mi_mla_index_topk(x, ld_logits, n_cols, T, B, cu, max_q_len, lens, k, idx, ld_idx, None)


def test_shape_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    assert append(lib, T=-1) == E_SHAPE and b"fp8mi_mla_index_cache_append: negative" in err() and append(lib, bs=48) == E_SHAPE and append(lib, ld_k=127) == E_SHAPE
    assert logits(lib, Hi=48) == E_SHAPE and b"Hi=48" in err() and logits(lib, Hi=128) == E_SHAPE and logits(lib, bs=8) == E_SHAPE
    assert logits(lib, ld_q=64 * 128 - 1) == E_SHAPE and b"ld_q" in err() and logits(lib, ld_w=63) == E_SHAPE and logits(lib, ld_bt=3) == E_SHAPE
    assert logits(lib, ld_logits=63) == E_SHAPE and logits(lib, max_seq_len=32, ld_logits=32, out=None) == E_NULL   # min(max_blocks bs, max_seq_len) columns
    assert logits(lib, cu=None) == E_SHAPE and b"cu_seqlens_q" in err() and logits(lib, cu=None, T=2, out=None) == E_NULL   # the decode form: T = B
    assert topk(lib, k=0) == E_SHAPE and b"topk" in err() and topk(lib, ld_idx=7) == E_SHAPE and topk(lib, ld_logits=63) == E_SHAPE and topk(lib, cu=None) == E_SHAPE


def test_enum_errors_without_gpu(lib):
    assert append(lib, dtype=7) == E_ENUM and b"dtype" in lib.fp8mi_last_error() and append(lib, mode=5) == E_ENUM and append(lib, slot_bytes=2) == E_ENUM
    assert logits(lib, dtype=9) == E_ENUM


def test_unsupported_errors_without_gpu(lib):
    assert append(lib, cache=P + 8) == E_UNSUPPORTED and b"aligned" in lib.fp8mi_last_error() and append(lib, k=P + 1) == E_UNSUPPORTED
    assert append(lib, slots=P + 4) == E_UNSUPPORTED and append(lib, slots=P + 4, slot_bytes=4, cache=None) == E_NULL and append(lib, nb=1 << 27) == E_UNSUPPORTED
    assert logits(lib, w=P + 2) == E_UNSUPPORTED and logits(lib, cache=P + 4) == E_UNSUPPORTED and logits(lib, nb=1 << 28) == E_UNSUPPORTED
    assert topk(lib, idx=P + 2) == E_UNSUPPORTED and topk(lib, k=1 << 31, ld_idx=1 << 31) == E_UNSUPPORTED
    assert topk(lib, n_cols=1 << 31, ld_logits=1 << 31) == E_UNSUPPORTED and b"2^31" in lib.fp8mi_last_error()


def test_null_errors_and_no_ops_without_gpu(lib):
    assert append(lib, k=None) == E_NULL and b"fp8mi_mla_index_cache_append: NULL" in lib.fp8mi_last_error() and append(lib, slots=None) == E_NULL
    assert logits(lib, w=None) == E_NULL and logits(lib, lens=None) == E_NULL and logits(lib, bt=None) == E_NULL
    assert topk(lib, x=None) == E_NULL and topk(lib, idx=None) == E_NULL and topk(lib, lens=None) == E_NULL
    assert append(lib, T=0, k=None, cache=None, slots=None) == 0 and append(lib, T=0, bs=3) == E_SHAPE   # a no-op that still validates
    none = dict(q=None, w=None, cu=None, cache=None, bt=None, lens=None, out=None)
    assert logits(lib, T=0, B=0, **none) == 0 and logits(lib, T=0, B=0, Hi=8, **none) == E_SHAPE
    assert topk(lib, T=0, B=0, x=None, cu=None, lens=None, idx=None) == 0 and topk(lib, T=0, B=0, k=0) == E_SHAPE


def test_topk_ref_is_the_brute_force_selection():
    """ties, +-0, +-inf and NaNs of both signs: a selection sort under a comparison written out case by case"""
    row = np.array([1, np.nan, -0.0, 0.0, np.inf, -np.inf, 1, 1, -np.nan, 0.0, -0.0, -3, 2, 2], np.float32)

    def first(i, j):   # < 0: element i is selected ahead of element j
        (a, b), (na, nb) = row[[i, j]], np.isnan(row[[i, j]])
        if na != nb:
            return 1 if na else -1
        if not na and a != b:
            return -1 if a > b else 1
        if not na and np.signbit(a) != np.signbit(b):
            return 1 if np.signbit(a) else -1
        return i - j
    for limit in (0, 5, len(row)):
        for k in (1, 4, 9, len(row), len(row) + 2):
            picked = sorted(range(limit), key=functools.cmp_to_key(first))[:k]
            assert I.topk_ref(row, limit, k).tolist() == sorted(picked) + [-1] * (k - len(picked)), (limit, k)
