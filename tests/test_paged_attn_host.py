"""The FP8 paged KV cache and decode attention on the host (no GPU): the reference's two forms (tests/paged_attn_ref.py) against each other -
which pins the constant E, and with it TOL, of every GPU comparison, and every E_<group> of the edge groups, whose shaped cases the model
with the softmax rescale left out must miss -, the library's split choice restated, the float64 reference against a plain dense softmax attention, the
slot arithmetic and both cache layouts for every block size, every argument error of fp8mi_kv_cache_append and
fp8mi_paged_attention_decode through the built library (each check runs before any HIP call), the bindings and the op layer's assertions."""
import os
import re

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import paged_attn_ref as R

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------

def test_model_stays_within_E_of_the_reference_on_every_gpu_case():
    """E of paged_attn_ref.py is the largest ratio of the model (b) against the reference (a) over all_cases(): no case exceeds it, one
    reaches it (the constant is the measurement, rounded up in its fourth digit - not a looser number), and TOL is twice it."""
    worst, names = 0.0, set()
    for name, c in R.all_cases():
        ref, vmax = R.attention_ref(c)
        r = R.ratio(R.attention_model(c), ref, vmax)
        assert r <= R.E, (name, r)
        worst = max(worst, r)
        assert name not in names
        names.add(name)
    assert R.E - 1e-5 <= worst <= R.E, worst
    assert R.TOL == 2 * R.E and R.E < 2.0 ** -4
    assert len(names) == len(R.GRID) + len(R.GROUPS) + 2 + len(R.SPLITS) + 4 + 1 + 9 + 1 + 4 + len(R.APPEND_AT)


@pytest.mark.parametrize("group", list(R.EDGE_NAMES))
def test_model_stays_within_each_edge_groups_E(group):
    """E_<group> is the measurement over the group, rounded up in its last digit, and TOL_<group> twice it"""
    worst = R.measure_edge_E(group)
    assert R.EDGE_E[group] - 1e-5 <= worst <= R.EDGE_E[group], worst
    assert R.EDGE_TOL[group] == 2 * R.EDGE_E[group] and R.EDGE_E[group] < R.E
    assert (R.E_long, R.E_scales, R.E_heads, R.E_tiny_q) == tuple(R.EDGE_E[g] for g in ("long", "scales", "heads", "tiny_q"))
    assert (R.TOL_long, R.TOL_scales, R.TOL_heads, R.TOL_tiny_q) == tuple(R.EDGE_TOL[g] for g in ("long", "scales", "heads", "tiny_q"))
    assert [n for n, _ in R.edge_groups()[group]] == R.EDGE_NAMES[group] and len(set(R.EDGE_NAMES[group])) == len(R.EDGE_NAMES[group])


def test_the_long_group_is_what_it_says():
    """every profile meets every length once, every (block size, head dimension) pair appears, every head is shaped, and the waves make
    the two and three passes the group exists for"""
    assert len(R.LONG) == 20 and {(L_, n, p) for L_, n, p, _, _ in R.LONG} == {(L_, n, p) for L_, n in R.LONG_LENS for p in R.PROFILES}
    assert {(bs, D) for *_, bs, D in R.LONG} == {(bs, D) for bs in (16, 64, 128) for D in (64, 128)}
    assert [R.most_passes(L_, n)[0] for L_, n in R.LONG_LENS] == [2, 2, 3, 3, 2]
    assert R.split_bounds(1300, 1300, 2) == [(0, 768), (768, 1300)] and [len(R.wave_steps(768, 1300, w)) for w in range(4)] == [2, 1, 1, 1]
    assert R.most_passes(513, 1) == (2, 512, 513) and R.most_passes(640, 1) == (2, 512, 640) and R.most_passes(1300, 2) == (2, 512, 640)
    assert R.most_passes(1025, 1) == (3, 1024, 1025) and R.most_passes(1153, 1) == (3, 1024, 1152)
    for i, (L_, n, prof, bs, D) in enumerate(R.LONG):
        _name, c, _ref, _vmax = R.edge_case("long", i)
        assert c.q.shape == (1, 2, D) and c.Hkv == 2 and c.block_size == bs and c.num_splits == n and tuple(c.seq_lens) == (L_,)
        if prof == "random":
            continue
        for h in range(2):   # the logits the reference sees: the target, moved by the cache's rounding of K only
            kb, _ = R.gather(c, 0, h)
            s = (R.LUT64[kb] * float(c.k_scale[0])) @ c.q[0, h].astype(np.float64) * c.softmax_scale
            step = np.arange(L_) // R.STEP
            if prof == "late_peak":
                peak = int(np.argmax(s))
                _passes, p0, end = R.most_passes(L_, n)
                assert peak == p0 + (end - p0) // 2 and s[peak] > 7 and np.delete(s, peak).max() < 1.5
            else:
                lift = s - (3.0 if prof == "rising" else -3.0) * step
                assert np.abs(lift).max() < 1.5, (prof, L_)


@pytest.mark.parametrize("mutate", ("o", "l"))
def test_long_cases_catch_a_missing_rescale(mutate):
    """The model with the rescale by alpha left out, on O or on l, is beyond TOL_long on every rising and late_peak case: a kernel with
    that bug cannot pass them.  (On all_cases() the mutated model equals the unmutated one: no wave makes a second pass there.)"""
    for i, (L_, n, prof, _bs, _D) in enumerate(R.LONG):
        if prof in ("rising", "late_peak"):
            _name, c, ref, vmax = R.edge_case("long", i)
            r = R.ratio(R.attention_model(c, mutate=mutate), ref, vmax)
            assert r > R.TOL_long, (L_, n, prof, r)
    c = R.split_case(1)
    assert np.array_equal(R.attention_model(c, mutate=mutate), R.attention_model(c))


def test_auto_splits_restates_the_librarys_choice(lib):
    assert R.auto_splits(1, 1, 1, 128, 1300, 1 << 40, 256) == 3             # 11 steps: ceil(11 / 4) splits keep a step per wave
    assert R.auto_splits(1, 1, 1, 128, 512, 1 << 40, 256) == 1              # steps <= 4: one split
    assert R.auto_splits(1, 1, 1, 128, 513, 1 << 40, 256) == 2
    assert R.auto_splits(1, 8, 1, 128, 1 << 20, 1 << 40, 256) == 64         # never more than 64
    assert R.auto_splits(8, 32, 8, 128, 8192, 1 << 40, 256) == 8            # ceil(2 * 256 / 64) workgroups' worth
    assert R.auto_splits(64, 32, 8, 128, 32768, 1 << 40, 256) == 1          # 512 workgroups already
    assert R.auto_splits(0, 8, 1, 128, 4096, 1 << 40, 256) == 1
    # the workspace cap: as many splits as it holds, one with none
    assert R.workspace_bytes(1, 4, 128, 3) == 3 * 4 * 130 * 4 and R.workspace_bytes(1, 4, 128, 1) == 0
    assert R.auto_splits(1, 4, 1, 128, 1300, R.workspace_bytes(1, 4, 128, 3), 256) == 3
    assert R.auto_splits(1, 4, 1, 128, 1300, R.workspace_bytes(1, 4, 128, 3) - 1, 256) == 2
    assert R.auto_splits(1, 4, 1, 128, 1300, R.workspace_bytes(1, 4, 128, 2) - 1, 256) == 1 and R.auto_splits(1, 4, 1, 128, 1300, 0, 256) == 1
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_attn.h")).read()
    assert int(re.search(r"kAttnAutoSplits = (\d+)", shared).group(1)) == R.AUTO_SPLITS_MAX
    for B, Hq, D, n in ((1, 4, 128, 3), (3, 6, 64, 2), (2, 8, 128, 64)):
        assert lib.fp8mi_paged_attention_workspace_bytes(B, Hq, D, n) == R.workspace_bytes(B, Hq, D, n)


@pytest.mark.parametrize("q_dtype", R.TINY_Q_DTYPES)
def test_model_is_finite_on_query_rows_too_small_for_448_over_amax(q_dtype):
    """448 / amax is +inf in fp32 for these rows; kernel and model multiply such a row by 2^64 first.  The result is the mean of V."""
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_attn.h")).read()
    assert float.fromhex(re.search(r"kAttnTinyQ = (0x1p-\d+)f", shared).group(1)) == R.TINY_Q
    assert float.fromhex(re.search(r"kAttnTinyQUp = (0x1p\d+)f", shared).group(1)) == R.TINY_Q_UP == 1.0 / R.TINY_Q
    c = R.tiny_q_case(q_dtype)
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(448.0) / np.abs(c.q[0, [1, 2, 3, 6]]).max(axis=-1)).all()
    out = R.attention_model(c)
    assert np.isfinite(out).all()
    ref, vmax = R.attention_ref(c)
    for hq in R.TINY_Q_ROWS:
        _kb, vb = R.gather(c, 0, hq // 4)
        mean = (R.LUT64[vb] * float(c.v_scale[0])).mean(axis=0)
        assert np.abs(out[0, hq] - mean).max() <= 1e-6 * vmax[0, hq] and np.abs(ref[0, hq] - mean).max() <= 1e-12 * vmax[0, hq], hq


def test_reference_equals_dense_attention_on_an_identity_table():
    rng = np.random.default_rng(5)
    for bs, D, L_ in ((16, 64, 50), (32, 128, 64), (64, 64, 65), (128, 128, 130)):
        Hkv, Hq, nb = 2, 4, (L_ + bs - 1) // bs
        kb = rng.integers(0, 0x7F, (nb, Hkv, bs, D), dtype=np.uint8) | (rng.integers(0, 2, (nb, Hkv, bs, D), dtype=np.uint8) << 7)
        vb = rng.integers(0, 0x7F, (nb, Hkv, D, bs), dtype=np.uint8) | (rng.integers(0, 2, (nb, Hkv, D, bs), dtype=np.uint8) << 7)
        q = rng.standard_normal((1, Hq, D)).astype(np.float32)
        c = R.Case(q=q, k_cache=kb, v_cache=vb, block_table=np.arange(nb, dtype=np.int32)[None], seq_lens=np.array([L_], np.int32),
                   k_scale=np.array([0.01], np.float32), v_scale=np.array([0.02, 0.03], np.float32), softmax_scale=0.3, block_size=bs, Hkv=Hkv, D=D)
        out, vmax = R.attention_ref(c)
        for hq in range(Hq):
            h = hq // 2
            K = R.LUT64[kb[:, h].reshape(nb * bs, D)[:L_]] * float(np.float32(0.01))                       # an identity table: the blocks in order
            V = R.LUT64[vb[:, h].transpose(0, 2, 1).reshape(nb * bs, D)[:L_]] * float(c.v_scale[h])
            assert np.allclose(out[0, hq], R.dense_attention(q[0, hq].astype(np.float64), K, V, 0.3), rtol=1e-12, atol=1e-15)
            assert vmax[0, hq] == np.abs(V).max()


@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_slot_arithmetic_and_both_layouts(bs):
    Hkv, D, nb = 3, 64, 5
    kc = np.zeros((nb, Hkv, bs, D), np.uint8)
    vc = np.zeros((nb, Hkv, D, bs), np.uint8)
    rng = np.random.default_rng(bs)
    slots = rng.permutation(nb * bs)[:2 * bs + 3]
    k = rng.standard_normal((len(slots), Hkv, D)).astype(np.float32)
    v = rng.standard_normal((len(slots), Hkv, D)).astype(np.float32)
    scale = np.array([0.01], np.float32)
    R.append_ref(kc, vc, k, v, np.concatenate([slots, [-1, nb * bs]]), scale, scale)   # the two extra slots are padding: k, v are never indexed for them
    for t, slot in enumerate(slots.tolist()):
        blk, off = R.slot_block_offset(slot, bs)
        assert (blk, off) == divmod(slot, bs) and blk * bs + off == slot and 0 <= off < bs
        want_k, want_v = R.quantise(k[t], scale), R.quantise(v[t], scale)
        for h in range(Hkv):
            for d in (0, 1, D - 1):
                assert kc.reshape(-1)[R.k_index(slot, h, d, Hkv, bs, D)] == want_k[h, d] == kc[blk, h, off, d]
                assert vc.reshape(-1)[R.v_index(slot, h, d, Hkv, bs, D)] == want_v[h, d] == vc[blk, h, d, off]
        # a channel's positions are contiguous in V, a position's channels in K
        assert R.v_index(slot, 1, 5, Hkv, bs, D) + 1 == R.v_index(slot + 1, 1, 5, Hkv, bs, D) or off == bs - 1
        assert R.k_index(slot, 1, 5, Hkv, bs, D) + 1 == R.k_index(slot, 1, 6, Hkv, bs, D)
    owned = np.zeros(nb * bs, bool)
    owned[slots] = True
    assert not kc.transpose(0, 2, 1, 3).reshape(nb * bs, -1)[~owned].any() and not vc.transpose(0, 3, 1, 2).reshape(nb * bs, -1)[~owned].any()
    assert R.quantise(np.float32(1.0), np.float32(3.0)) == R.quantise(np.float32(1.0) * (np.float32(1.0) / np.float32(3.0)), np.float32(1.0))


def test_model_restates_the_kernels_constants():
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_attn.h")).read()
    assert int(re.search(r"kAttnStep = (\d+)", shared).group(1)) == R.STEP
    assert int(re.search(r"kAttnWaves = (\d+)", shared).group(1)) == R.WAVES
    assert 2.0 ** int(re.search(r"kAttnPScaleLog2 = (\d+)", shared).group(1)) == R.P_SCALE
    assert R.chunk_of(300, 2) == 256 and R.chunk_of(300, 8) == 128 and R.chunk_of(1, 1) == 128


# ---- argument errors, before any HIP call ---------------------------------------------------------------------------------------------------

def append(lib, k=P, v=P, dtype=L.BF16, T=4, Hkv=2, D=128, ld_k=None, ld_v=None, kc=P, vc=P, nb=8, bs=16, slots=P, slot_bytes=4, ks=P, vs=P,
           mode=L.KV_SCALE_TENSOR, enc=L.ENC_RNE):
    return lib.fp8mi_kv_cache_append(k, v, dtype, T, Hkv, D, Hkv * D if ld_k is None else ld_k, Hkv * D if ld_v is None else ld_v, kc, vc, nb, bs, slots,
                                     slot_bytes, ks, vs, mode, enc, None)


def decode(lib, q=P, q_dtype=L.BF16, B=2, Hq=8, Hkv=2, D=128, ld_q=None, kc=P, vc=P, nb=8, bs=16, bt=P, ld_bt=None, max_blocks=4, lens=P,
           max_seq_len=64, ks=P, vs=P, mode=L.KV_SCALE_TENSOR, scale=0.1, splits=1, ws=None, ws_bytes=0, out=P, out_dtype=L.BF16, ld_out=None):
    return lib.fp8mi_paged_attention_decode(q, q_dtype, B, Hq, Hkv, D, Hq * D if ld_q is None else ld_q, kc, vc, nb, bs, bt,
                                            max_blocks if ld_bt is None else ld_bt, max_blocks, lens, max_seq_len, ks, vs, mode, scale, splits, ws,
                                            ws_bytes, out, out_dtype, Hq * D if ld_out is None else ld_out, None)


def test_append_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("k", "v", "kc", "vc", "slots", "ks", "vs"):
        assert append(lib, **{name: None}) == E_NULL, name
    assert b"NULL" in err()
    assert append(lib, T=-1) == E_SHAPE and b"T=-1" in err()
    assert append(lib, Hkv=0) == E_SHAPE and b"Hkv=0" in err()
    assert append(lib, nb=-1) == E_SHAPE
    for D in (0, 32, 96, 256):
        assert append(lib, D=D) == E_SHAPE and b"head dimension" in err()
    for bs in (0, 8, 24, 256):
        assert append(lib, bs=bs) == E_SHAPE and b"block_size" in err()
    assert append(lib, ld_k=255) == E_SHAPE and b"ld_k=255" in err()
    assert append(lib, ld_v=255) == E_SHAPE
    assert append(lib, dtype=3) == E_ENUM and b"dtype" in err()
    assert append(lib, mode=2) == E_ENUM and b"scale_mode" in err()
    assert append(lib, enc=2) == E_ENUM and b"encode_mode" in err()
    assert append(lib, slot_bytes=2) == E_ENUM and b"slot_bytes" in err()
    assert append(lib, k=P + 1) == E_UNSUPPORTED and b"aligned" in err()
    assert append(lib, kc=P + 4) == E_UNSUPPORTED and append(lib, vc=P + 8) == E_UNSUPPORTED
    assert append(lib, slots=P + 4, slot_bytes=8) == E_UNSUPPORTED and append(lib, ks=P + 2) == E_UNSUPPORTED
    assert append(lib, T=1 << 40) == E_UNSUPPORTED
    none = dict(k=None, v=None, kc=None, vc=None, slots=None, ks=None, vs=None)
    assert append(lib, T=0, **none) == 0
    assert append(lib, T=0, D=100, **none) == E_SHAPE and append(lib, T=0, dtype=9, **none) == E_ENUM


def test_decode_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    for name in ("q", "kc", "vc", "bt", "lens", "ks", "vs", "out"):
        assert decode(lib, **{name: None}) == E_NULL, name
    assert b"NULL" in err()
    assert decode(lib, B=-1) == E_SHAPE and decode(lib, max_blocks=-1) == E_SHAPE and decode(lib, max_seq_len=-1) == E_SHAPE
    assert decode(lib, ws_bytes=-1) == E_SHAPE
    assert decode(lib, Hkv=0) == E_SHAPE
    assert decode(lib, Hq=7) == E_SHAPE and b"Hq=7" in err()
    assert decode(lib, Hq=0) == E_SHAPE
    assert decode(lib, D=96) == E_SHAPE and decode(lib, bs=48) == E_SHAPE
    assert decode(lib, ld_q=1023) == E_SHAPE and b"ld_q=1023" in err()
    assert decode(lib, ld_out=1023) == E_SHAPE and decode(lib, ld_bt=3) == E_SHAPE
    assert decode(lib, splits=-1) == E_SHAPE and b"num_splits" in err()
    assert decode(lib, q_dtype=3) == E_ENUM and decode(lib, out_dtype=-1) == E_ENUM and decode(lib, mode=2) == E_ENUM
    assert decode(lib, Hq=34, Hkv=2) == E_UNSUPPORTED and b"Hq / Hkv = 17" in err()
    assert decode(lib, Hq=32, Hkv=2, out=None) == E_NULL                                  # 16 query heads to a KV head pass
    assert decode(lib, splits=L.ATTN_MAX_SPLITS + 1, ws=P, ws_bytes=1 << 40) == E_UNSUPPORTED and b"MAX_SPLITS" in err()
    for bad in (float("inf"), float("nan")):
        assert decode(lib, scale=bad) == E_UNSUPPORTED and b"softmax_scale" in err()
    need = lib.fp8mi_paged_attention_workspace_bytes(2, 8, 128, 3)
    assert need == 2 * 8 * 3 * (128 + 2) * 4
    assert decode(lib, splits=3) == E_UNSUPPORTED and b"workspace" in err()              # forced, none given
    assert decode(lib, splits=3, ws=P, ws_bytes=need - 1) == E_UNSUPPORTED
    assert decode(lib, splits=3, ws=P + 4, ws_bytes=need) == E_UNSUPPORTED
    assert decode(lib, splits=3, ws=P, ws_bytes=need, out=None) == E_NULL                 # ... enough: the next check
    assert decode(lib, q=P + 1) == E_UNSUPPORTED and b"aligned" in err()
    assert decode(lib, kc=P + 8) == E_UNSUPPORTED and decode(lib, bt=P + 2) == E_UNSUPPORTED and decode(lib, lens=P + 1) == E_UNSUPPORTED
    none = dict(q=None, kc=None, vc=None, bt=None, lens=None, ks=None, vs=None, out=None)
    assert decode(lib, B=0, **none) == 0
    assert decode(lib, B=0, Hq=7, **none) == E_SHAPE and decode(lib, B=0, q_dtype=5, **none) == E_ENUM
    # the workspace size: 0 unsplit, for the library's own choice never more than 64 splits and never less than what it may pick
    assert lib.fp8mi_paged_attention_workspace_bytes(4, 8, 128, 1) == 0 and lib.fp8mi_paged_attention_workspace_bytes(0, 8, 128, 4) == 0
    auto = lib.fp8mi_paged_attention_workspace_bytes(1, 32, 128, 0)
    assert 0 < auto <= 32 * 64 * 130 * 4 and auto % (32 * 130 * 4) == 0


# ---- bindings and ops -------------------------------------------------------------------------------------------------------------------------

def test_symbols_and_constants_match_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name in ("KV_SCALE_TENSOR", "KV_SCALE_HEAD", "ATTN_MAX_GROUP", "ATTN_MAX_SPLITS"):
        assert int(re.search(r"#define FP8MI_" + name + r"\s+(\d+)", hdr).group(1)) == getattr(L, name), name
    for name, n in (("fp8mi_kv_cache_append", 19), ("fp8mi_paged_attention_workspace_bytes", 4), ("fp8mi_paged_attention_decode", 27)):
        assert re.search(r"\b" + name + r"\s*\(", hdr)
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert L.KV_BLOCK_SIZES == R.BLOCK_SIZES and L.KV_HEAD_DIMS == R.HEAD_DIMS
    assert lib.fp8mi_version() == 0x000400   # new entry points only: the ABI version does not move


def test_op_layer_exposes_the_cache_and_the_attention_and_asserts_their_arguments():
    import fp8_mi355x_native as N
    import fp8_mps_native as alias
    for name in ("fp8_kv_cache_alloc", "fp8_kv_cache_append", "fp8_paged_attention"):
        assert callable(getattr(N, name)) and getattr(alias, name) is getattr(N, name), name
    kc, vc = N.fp8_kv_cache_alloc(3, 32, 2, 64, device="cpu")
    assert tuple(kc.shape) == (3, 2, 32, 64) and tuple(vc.shape) == (3, 2, 64, 32) and kc.dtype == vc.dtype == torch.uint8
    assert not kc.any() and not vc.any()
    with pytest.raises(AssertionError, match="block_size"):
        N.fp8_kv_cache_alloc(3, 48, 2, 64, device="cpu")
    with pytest.raises(AssertionError, match="block_size"):
        N.fp8_kv_cache_alloc(3, 32, 2, 96, device="cpu")
    x = torch.zeros(1, 2, 64)
    s = torch.ones(1)
    with pytest.raises(AssertionError, match="HIP device"):     # no CPU path
        N.fp8_kv_cache_append(x, x, kc, vc, torch.zeros(1, dtype=torch.int64), s, s)
    with pytest.raises(AssertionError, match="v_cache has shape"):
        N.fp8_kv_cache_append(x, x, kc, kc, torch.zeros(1, dtype=torch.int64), s, s)
    with pytest.raises(AssertionError, match="uint8"):
        N.fp8_paged_attention(x, kc.float(), vc, torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), s, s)
