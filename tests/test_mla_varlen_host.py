"""The multi-token MLA attention (fp8mi_mla_attention_varlen) on the host, no GPU: the ABI's symbols, the split choice against its
restatement, the argument checks through the built library (each runs before any HIP call), E_mla_varlen recomputed and pinned."""
import inspect

import pytest

import fp8_mi355x_lib as L
import mla_ref as R
import mla_varlen_ref as V

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_E_mla_varlen_is_what_the_model_measures():
    e = V.measure_E()
    assert e <= V.E_mla_varlen < e * 1.001 and V.TOL == 2 * V.E_mla_varlen, e


def test_symbols_bindings_and_op_layer_arguments(lib):
    for name, n in (("fp8mi_mla_attention_varlen", 27), ("fp8mi_mla_attention_varlen_splits", 6)):
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    import fp8_mi355x_native as N
    import fp8_mps_native as M
    params = inspect.signature(N.fp8_mla_paged_attention).parameters
    assert list(params)[-3:] == ["workspace", "cu_seqlens_q", "max_q_len"] and params["cu_seqlens_q"].default is None and params["max_q_len"].default is None
    assert M.fp8_mla_paged_attention is N.fp8_mla_paged_attention


def test_split_choice_restated(lib):
    """fp8mi_attn_auto_splits_mla_varlen through fp8mi_mla_attention_varlen_splits (without a device the library counts 256 compute units,
    with one its own count); one token per sequence is the decode choice"""
    info = L.DeviceInfo()
    cus = info.compute_units if lib.fp8mi_device_info(0, info) == 0 and info.compute_units > 0 else 256
    big, seen, f = 1 << 40, set(), lib.fp8mi_mla_attention_varlen_splits
    for Hq in (1, 5, 16, 20, 128):
        for T, B, mq in ((8, 8, 1), (32, 8, 4), (40, 3, 33), (512, 1, 512), (7, 2, 100)):
            for ms in (300, 513, 1300, 8192, 1 << 17):
                for ws in (big, T * Hq * 2 * 514 * 4, T * Hq * 2 * 514 * 4 - 1, 0):
                    assert f(T, B, mq, Hq, ms, ws) == V.auto_splits(T, B, min(mq, T), Hq, ms, ws, cus), (T, B, mq, Hq, ms, ws)
                    seen.add(f(T, B, mq, Hq, ms, ws))
                assert f(B, B, 1, Hq, ms, big) == lib.fp8mi_mla_attention_splits(B, Hq, ms, big) == R.auto_splits(B, Hq, ms, big, cus)
    assert {1, 2, 3, 64} <= seen
    assert V.auto_splits(4, 1, 4, 16, 8192, big, 256) == 16      # Hq = 16: four tokens are ONE workgroup tile -> min(512, 16 by steps)
    assert V.auto_splits(128, 64, 2, 128, 32768, big, 256) == 2  # 64 x 4 tiles
    assert f(8, 1, 8, 129, 8192, big) == 0 and f(-1, 1, 8, 4, 8192, big) == 0 and f(0, 1, 8, 4, 8192, big) == 1


def varlen(lib, ql=P, qp=P, q_dtype=L.BF16, T=6, B=2, cu=P, max_q_len=4, Hq=8, ld_ql=None, ld_qp=None, cache=P, nb=8, bs=16, bt=P, ld_bt=None, max_blocks=4, lens=P,
           max_seq_len=64, kvs=P, scale=0.1, splits=1, ws=None, ws_bytes=0, out=P, out_dtype=L.BF16, ld_out=None):
    return lib.fp8mi_mla_attention_varlen(ql, qp, q_dtype, T, B, cu, max_q_len, Hq, Hq * 512 if ld_ql is None else ld_ql, Hq * 64 if ld_qp is None else ld_qp, cache, nb,
                                          bs, bt, max_blocks if ld_bt is None else ld_bt, max_blocks, lens, max_seq_len, kvs, scale, splits, ws, ws_bytes, out,
                                          out_dtype, Hq * 512 if ld_out is None else ld_out, None)


def test_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("ql", "qp", "cu", "cache", "bt", "lens", "kvs", "out"):
        assert varlen(lib, **{name: None}) == E_NULL and b"fp8mi_mla_attention_varlen: NULL" in err(), name
    for neg in ("T", "max_q_len", "B", "nb", "max_blocks", "max_seq_len", "ws_bytes", "splits"):
        assert varlen(lib, **{neg: -1}) == E_SHAPE, neg
    assert varlen(lib, Hq=0) == E_SHAPE and varlen(lib, bs=48) == E_SHAPE
    assert varlen(lib, ld_ql=4095) == E_SHAPE and varlen(lib, ld_qp=511) == E_SHAPE and varlen(lib, ld_out=4095) == E_SHAPE and varlen(lib, ld_bt=3) == E_SHAPE
    assert varlen(lib, q_dtype=3) == E_ENUM and varlen(lib, out_dtype=-1) == E_ENUM
    assert varlen(lib, Hq=129) == E_UNSUPPORTED and b"MLA_MAX_HEADS" in err() and varlen(lib, Hq=128, out=None) == E_NULL
    assert varlen(lib, splits=L.ATTN_MAX_SPLITS + 1, ws=P, ws_bytes=1 << 40) == E_UNSUPPORTED and b"MAX_SPLITS" in err()
    assert varlen(lib, scale=float("inf")) == E_UNSUPPORTED and varlen(lib, scale=float("nan")) == E_UNSUPPORTED
    need = lib.fp8mi_mla_attention_workspace_bytes(6, 8, 3)   # the workspace is per query ROW: T in place of B
    assert need == 6 * 8 * 3 * 514 * 4 and varlen(lib, splits=3) == E_UNSUPPORTED and b"workspace" in err()
    assert varlen(lib, splits=3, ws=P, ws_bytes=need - 1) == E_UNSUPPORTED and varlen(lib, splits=3, ws=P + 4, ws_bytes=need) == E_UNSUPPORTED
    assert varlen(lib, splits=3, ws=P, ws_bytes=need, out=None) == E_NULL   # ... enough: the next check
    assert varlen(lib, ql=P + 1) == E_UNSUPPORTED and varlen(lib, cache=P + 8) == E_UNSUPPORTED and varlen(lib, cu=P + 2) == E_UNSUPPORTED and b"cu_seqlens_q" in err()
    # sizes at or beyond 2^31: the query rows, the grid, the combine's grid
    assert varlen(lib, T=1 << 28, Hq=8) == E_UNSUPPORTED and b"query rows" in err()
    assert varlen(lib, T=1 << 20, B=1 << 29, max_q_len=256, Hq=1) == E_UNSUPPORTED and b"workgroups" in err()
    assert varlen(lib, T=1 << 20, B=1 << 12, max_q_len=1 << 20, Hq=1) == E_UNSUPPORTED and b"combine" in err()
    none = dict(ql=None, qp=None, cu=None, cache=None, bt=None, lens=None, kvs=None, out=None)
    for empty in (dict(T=0), dict(B=0), dict(max_q_len=0)):   # a no-op that still validates
        assert varlen(lib, **empty, **none) == 0 and varlen(lib, Hq=0, **empty, **none) == E_SHAPE and varlen(lib, q_dtype=5, **empty, **none) == E_ENUM
