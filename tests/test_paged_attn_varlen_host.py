"""The multi-token paged attention (fp8mi_paged_attention_varlen) on the host, no GPU: E_varlen recomputed and pinned, the expansion's
limits against a causal attention written directly, the restated split choice against the library's, every argument error of the new
entry through the built library (each check runs before any HIP call), the binding and the op layer's new arguments."""
import inspect
import os
import re

import numpy as np
import pytest

import fp8_mi355x_lib as L
import paged_attn_ref as R
import paged_attn_varlen_ref as V

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_model_stays_within_E_varlen_on_every_case_and_no_case_compares_nothing():
    """E_varlen is the measurement over VARLEN_CASES, rounded up in its fourth digit, and TOL_varlen twice it: what the GPU test asks of
    the kernel, the model of its roundings meets on every case before anything runs on a GPU."""
    worst = 0.0
    for name in V.VARLEN_CASES:
        c, e, ref, vmax = V.varlen_case(name)
        assert e.q.shape[0] == c.q.shape[0] == int(c.cu[-1]) > 0 and (vmax > 0).any(), name   # rows to compare, some of them live
        r = R.ratio(R.attention_model(e), ref, vmax)
        assert r <= V.E_varlen, (name, r)
        worst = max(worst, r)
    assert V.E_varlen - 1e-5 <= worst <= V.E_varlen, worst
    assert V.TOL_varlen == 2 * V.E_varlen and V.E_varlen < 2.0 ** -4
    assert len(V.VARLEN_CASES) == len(set(V.VARLEN_CASES)) == 48 + 4 + 2 + 3 + 3 + 3 + 2 + 2 + 4 + 3 + 1 + 2


def test_case_table_is_what_the_docstrings_say():
    assert [V.mapping_q_len(1, i) for i in range(4)] == [15, 16, 17, 33] and [V.mapping_q_len(5, i) for i in range(4)] == [2, 3, 4, 7]
    assert [V.mapping_q_len(16, i) for i in range(4)] == [0, 1, 2, 3] and V.tile_tokens(5, 1) == 3 and V.tile_tokens(32, 2) == 1
    c = V.varlen_case("mapping G=1 Hkv=2 q_len=33")[0]
    assert tuple(c.q_lens) == (33, 2) and tuple(c.seq_lens) == (73, 42) and tuple(c.cu) == (0, 33, 35)
    # step edge: the limits of (130, 4) are 127 .. 130: tokens 0 and 1 own nothing of the second step [128, 256), which wave 1 takes
    assert tuple(V.limits_of([130], [4])) == (127, 128, 129, 130)
    # pass edge: (514, 4) -> 511 .. 514: wave 0's second pass [512, 640) is fully masked for tokens 0 and 1, whose m is finite by then
    assert tuple(V.limits_of([514], [4])) == (511, 512, 513, 514) and R.WAVES * R.STEP == 512
    # split edge: chunk 256 at 2 splits of 512: split 1 = [256, ..) owns nothing of the tokens with limits 255 and 256
    assert R.chunk_of(512, 2) == 256 and tuple(V.limits_of([258], [4])) == (255, 256, 257, 258)
    assert R.chunk_of(512, 3) == 256 and R.chunk_of(512, 8) == 128
    assert tuple(V.expand(V.varlen_case("q_len = seq_len + 3")[0]).seq_lens) == (0, 0, 0, 1, 2, 3, 4, 5, 19, 20)
    e = V.varlen_case("q_len = 0 and seq_len = 0 in a batch")[1]
    assert tuple(e.seq_lens) == (48, 49, 50, 0, 0, 19) and tuple(e.seq_of) == (0, 0, 0, 2, 2, 4)
    e = V.varlen_case("mixed batch splits=3")[1]
    assert e.num_splits == 3 and e.max_seq_len == 300 and e.q.shape[0] == 42 and tuple(e.seq_lens[:9]) == (300, 1, 2, 3, 4, 5, 6, 7, 1)
    assert (e.block_table[1:8] == e.block_table[1]).all()


@pytest.mark.parametrize("name", ("mixed batch splits=1", "q_len = seq_len + 3"))
def test_expansion_equals_a_causal_attention_written_directly(name):
    """attention_ref on expand(case) - the definition every GPU result is held to - against the q_len x seq_len masked softmax"""
    c, e, ref, _vmax = V.varlen_case(name)
    Hq = c.q.shape[1]
    for b in range(len(c.q_lens)):
        rows = slice(int(c.cu[b]), int(c.cu[b + 1]))
        for hq in range(Hq):
            want = V.dense_causal(c, b, hq)
            assert np.allclose(ref[rows, hq], want, rtol=1e-12, atol=1e-15), (name, b, hq)
    zero = V.limits_of(c.seq_lens, c.q_lens) <= 0
    assert not ref[zero].any() and (name != "q_len = seq_len + 3" or zero.sum() == 3)


def test_split_choice_restated(lib):
    """fp8mi_attn_auto_splits_varlen through fp8mi_paged_attention_varlen_splits (without a device the library counts 256 compute units,
    with one its own count)"""
    info = L.DeviceInfo()
    cus = info.compute_units if lib.fp8mi_device_info(0, info) == 0 and info.compute_units > 0 else 256
    big = 1 << 40
    shapes = [(T, B, mq, g * Hkv, Hkv, D, ms) for g in (1, 4, 5, 16) for Hkv in (1, 8) for (T, B, mq) in ((8, 8, 1), (64, 8, 8), (40, 3, 33), (512, 1, 512), (7, 2, 100))
              for D in (64, 128) for ms in (300, 513, 1300, 8192, 1 << 17)]
    seen = set()
    for T, B, mq, Hq, Hkv, D, ms in shapes:
        for ws in (big, R.workspace_bytes(T, Hq, D, 2), R.workspace_bytes(T, Hq, D, 2) - 1, 0):
            want = V.auto_splits_varlen(T, B, min(mq, T), Hq, Hkv, D, ms, ws, cus)
            assert lib.fp8mi_paged_attention_varlen_splits(T, B, mq, Hq, Hkv, D, ms, ws) == want, (T, B, mq, Hq, Hkv, D, ms, ws)
            seen.add(want)
    assert {1, 2, 3, 64} <= seen
    # one token per sequence: the decode choice
    for B, Hq, Hkv, D, ms in ((8, 32, 8, 128, 8192), (1, 4, 1, 128, 1300), (64, 32, 8, 128, 32768), (3, 5, 1, 64, 100000)):
        assert V.auto_splits_varlen(B, B, 1, Hq, Hkv, D, ms, big, cus) == R.auto_splits(B, Hq, Hkv, D, ms, big, cus)
    assert V.auto_splits_varlen(8, 1, 8, 32, 8, 128, 8192, big, 256) == 16     # TQ = 4: 2 tiles x 8 KV heads = 16 workgroups -> min(32, 16 by steps)
    assert V.auto_splits_varlen(8, 1, 8, 4, 4, 128, 8192, big, 256) == 16      # G = 1: one tile holds the 8 tokens
    assert V.auto_splits_varlen(512, 1, 512, 32, 8, 128, 8192, big, 256) == 1  # 128 tiles x 8 heads
    assert lib.fp8mi_paged_attention_varlen_splits(8, 1, 8, 34, 2, 128, 8192, big) == 0 and lib.fp8mi_paged_attention_varlen_splits(-1, 1, 8, 4, 2, 128, 8192, big) == 0
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_attn.h")).read()
    assert int(re.search(r"kAttnMaxGroup = (\d+)", shared).group(1)) == V.MAX_GROUP == L.ATTN_MAX_GROUP


# ---- argument errors, before any HIP call ---------------------------------------------------------------------------------------------------

def varlen(lib, q=P, q_dtype=L.BF16, T=6, B=2, cu=P, max_q_len=4, Hq=8, Hkv=2, D=128, ld_q=None, kc=P, vc=P, nb=8, bs=16, bt=P, ld_bt=None, max_blocks=4,
           lens=P, max_seq_len=64, ks=P, vs=P, mode=L.KV_SCALE_TENSOR, scale=0.1, splits=1, ws=None, ws_bytes=0, out=P, out_dtype=L.BF16, ld_out=None):
    return lib.fp8mi_paged_attention_varlen(q, q_dtype, T, B, cu, max_q_len, Hq, Hkv, D, Hq * D if ld_q is None else ld_q, kc, vc, nb, bs, bt,
                                            max_blocks if ld_bt is None else ld_bt, max_blocks, lens, max_seq_len, ks, vs, mode, scale, splits, ws,
                                            ws_bytes, out, out_dtype, Hq * D if ld_out is None else ld_out, None)


def test_varlen_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("q", "cu", "kc", "vc", "bt", "lens", "ks", "vs", "out"):
        assert varlen(lib, **{name: None}) == E_NULL, name
    assert b"NULL" in err() and b"fp8mi_paged_attention_varlen" in err()
    assert varlen(lib, T=-1) == E_SHAPE and b"T=-1" in err()
    assert varlen(lib, max_q_len=-1) == E_SHAPE and b"max_q_len=-1" in err()
    assert varlen(lib, B=-1) == E_SHAPE and varlen(lib, max_blocks=-1) == E_SHAPE and varlen(lib, max_seq_len=-1) == E_SHAPE
    assert varlen(lib, ws_bytes=-1) == E_SHAPE and varlen(lib, nb=-1) == E_SHAPE
    assert varlen(lib, Hkv=0) == E_SHAPE
    assert varlen(lib, Hq=7) == E_SHAPE and b"Hq=7" in err()
    assert varlen(lib, Hq=0) == E_SHAPE
    assert varlen(lib, D=96) == E_SHAPE and varlen(lib, bs=48) == E_SHAPE
    assert varlen(lib, ld_q=1023) == E_SHAPE and b"ld_q=1023" in err()
    assert varlen(lib, ld_out=1023) == E_SHAPE and varlen(lib, ld_bt=3) == E_SHAPE
    assert varlen(lib, splits=-1) == E_SHAPE and b"num_splits" in err()
    assert varlen(lib, q_dtype=3) == E_ENUM and varlen(lib, out_dtype=-1) == E_ENUM and varlen(lib, mode=2) == E_ENUM
    assert varlen(lib, Hq=34, Hkv=2) == E_UNSUPPORTED and b"Hq / Hkv = 17" in err()
    assert varlen(lib, Hq=32, Hkv=2, out=None) == E_NULL                                  # 16 query heads to a KV head pass
    assert varlen(lib, splits=L.ATTN_MAX_SPLITS + 1, ws=P, ws_bytes=1 << 40) == E_UNSUPPORTED and b"MAX_SPLITS" in err()
    for bad in (float("inf"), float("nan")):
        assert varlen(lib, scale=bad) == E_UNSUPPORTED and b"softmax_scale" in err()
    # the workspace is per query ROW: T in place of B
    need = lib.fp8mi_paged_attention_workspace_bytes(6, 8, 128, 3)
    assert need == 6 * 8 * 3 * (128 + 2) * 4 and need > lib.fp8mi_paged_attention_workspace_bytes(2, 8, 128, 3)
    assert varlen(lib, splits=3) == E_UNSUPPORTED and b"workspace" in err()              # forced, none given
    assert varlen(lib, splits=3, ws=P, ws_bytes=need - 1) == E_UNSUPPORTED
    assert varlen(lib, splits=3, ws=P + 4, ws_bytes=need) == E_UNSUPPORTED
    assert varlen(lib, splits=3, ws=P, ws_bytes=need, out=None) == E_NULL                 # ... enough: the next check
    assert varlen(lib, q=P + 1) == E_UNSUPPORTED and b"aligned" in err()
    assert varlen(lib, cu=P + 2) == E_UNSUPPORTED and b"cu_seqlens_q" in err()
    assert varlen(lib, kc=P + 8) == E_UNSUPPORTED and varlen(lib, bt=P + 2) == E_UNSUPPORTED and varlen(lib, lens=P + 1) == E_UNSUPPORTED
    # sizes at or beyond 2^31: the query rows, the grid, the combine's grid
    assert varlen(lib, T=1 << 28, Hq=8) == E_UNSUPPORTED and b"query rows" in err()
    assert varlen(lib, T=1 << 20, B=1 << 29, max_q_len=1, Hq=4, Hkv=4, D=64) == E_UNSUPPORTED and b"workgroups" in err()
    assert varlen(lib, T=1 << 20, B=1 << 12, max_q_len=1 << 20, Hq=2, Hkv=2, D=64) == E_UNSUPPORTED   # B max_q_len Hq: the launcher's check, no HIP call yet
    none = dict(q=None, cu=None, kc=None, vc=None, bt=None, lens=None, ks=None, vs=None, out=None)
    assert varlen(lib, T=0, **none) == 0 and varlen(lib, B=0, **none) == 0 and varlen(lib, max_q_len=0, **none) == 0
    for empty in (dict(T=0), dict(B=0), dict(max_q_len=0)):
        assert varlen(lib, Hq=7, **empty, **none) == E_SHAPE and varlen(lib, q_dtype=5, **empty, **none) == E_ENUM
        assert varlen(lib, Hq=34, Hkv=2, **empty, **none) == E_UNSUPPORTED


def test_decode_return_codes_are_what_they_were(lib):
    """the two entries share one front end: the decode entry knows nothing of T, cu and max_q_len"""
    def decode(B=2, out=P, splits=1, ws=None, ws_bytes=0, Hq=8):
        return lib.fp8mi_paged_attention_decode(P, L.BF16, B, Hq, 2, 128, Hq * 128, P, P, 8, 16, P, 4, 4, P, 64, P, P, L.KV_SCALE_TENSOR, 0.1, splits, ws, ws_bytes,
                                                out, L.BF16, Hq * 128, None)
    assert decode(out=None) == E_NULL and b"fp8mi_paged_attention_decode" in lib.fp8mi_last_error()
    need = lib.fp8mi_paged_attention_workspace_bytes(2, 8, 128, 3)
    assert decode(splits=3, ws=P, ws_bytes=need - 1) == E_UNSUPPORTED and decode(splits=3, ws=P, ws_bytes=need, out=None) == E_NULL
    assert decode(B=0, out=None) == 0 and decode(B=-1) == E_SHAPE and decode(B=1 << 29, Hq=8, out=None) == E_NULL


def test_binding_and_op_layer_arguments(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, n in (("fp8mi_paged_attention_varlen", 30), ("fp8mi_paged_attention_varlen_splits", 8)):
        assert re.search(r"\b" + name + r"\s*\(", hdr)
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.fp8mi_version() == 0x000400   # new entry points only
    import fp8_mi355x_native as N
    params = inspect.signature(N.fp8_paged_attention).parameters
    assert list(params)[-2:] == ["cu_seqlens_q", "max_q_len"] and params["cu_seqlens_q"].default is None and params["max_q_len"].default is None
    assert list(params)[:12] == ["q", "k_cache", "v_cache", "block_table", "seq_lens", "k_scale", "v_scale", "softmax_scale", "max_seq_len", "num_splits",
                                 "out_dtype", "workspace"]
