"""The reference of the sparse (top-k indexed) MLA attention (fp8mi_mla_attention_sparse): numpy, CPU only.  A plain module: no fixtures, no tests.
  CASES         the table of tests/test_gpu_mla_sparse.py: an mla_varlen_ref case (cu, q_lens, the cache) plus `indices` (T, topk), a seeded
                list of logical positions per query token; `form` "decode" passes no cu_seqlens_q.
  compact       the mla_ref Case whose single sequence is token t's valid rows in list order (block i of the new cache is entries
                [i bs, (i + 1) bs) of them), seq_len = their count, max_seq_len = topk: what the decode entry must equal bit for bit when the
                list is valid up to n and -1 from there on (prefix_n), and what mla_ref.attention_ref (float64) is taken on.
  masked_model  mla_ref.attention_model restated on the LIST: holes stay in place inside their 128-entry steps (logit -inf, a zero row), a step
                of holes is no step, splits divide the list - the kernel's step composition.  On a hole-free list it is attention_model on the
                compaction, exactly.
  E_mla_sparse  the largest ratio of masked_model against the float64 reference over the table, measured on the CPU:
                    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import mla_sparse_ref as S; print(S.measure_E())"
                    -> 0.02228975572886433 (heads Hq=128), recorded below rounded up; TOL = 2 E, the project's convention.  tests/test_mla_sparse_host.py pins it."""
import math

import numpy as np

import fp8_oracle
import mla_ref as R
import mla_varlen_ref as V

CAPACITY = 1024   # the "splits" lists: this many entries, the first n valid


def _distinct(rng, limit, n):
    return rng.permutation(limit)[:n]


def _permuted(c, rng):
    return _distinct(rng, 300, 200)[None]


def _wrap(c, rng):
    return _distinct(rng, 1000, 520)[None]


def _heads(c, rng):
    return _distinct(rng, 200, 130)[None]


def _prefix(n):
    def lists(c, rng):
        out = np.full((1, CAPACITY), -1)
        out[0, :n] = _distinct(rng, 600, n)
        return out
    return lists


def _mtp(c, rng):
    """limits 139, 140 and 50: the first token's list names position 139, which only the second may see"""
    out = np.stack([_distinct(rng, 139, 64), _distinct(rng, 140, 64), np.r_[_distinct(rng, 50, 50), np.full(14, -1)]])
    out[0, [5, 40]] = 139
    return out


def _holes(c, rng):
    """token 0 (limit 300): -1, other negatives and positions at or beyond the limit scattered in steps 0 and 2, step 1 all three kinds;
    token 1 (limit 40): no valid entry"""
    out = np.stack([rng.integers(0, 300, 384), rng.integers(40, 4000, 384)])   # duplicates count
    kinds = np.array([-1, -7, -(1 << 31), 300, 301, (1 << 31) - 1])
    out[0, 128:256] = kinds[np.arange(128) % 6]
    at = np.concatenate([rng.permutation(128)[:37], 256 + rng.permutation(128)[:90], [0, 127, 256, 383]])
    out[0, at] = kinds[np.arange(len(at)) % 6]
    out[1, ::3] = kinds[np.arange(128) % 3]
    return out


# name, Hq, block_size, (seq_len, q_len) per sequence, form, lists, make_case keywords
_TABLE = [("permuted", 16, 16, [(300, 1)], "decode", _permuted, {}),
          ("wrap", 5, 64, [(1000, 1)], "decode", _wrap, {}),
          ("heads Hq=65", 65, 128, [(200, 1)], "decode", _heads, {}),
          ("heads Hq=128", 128, 128, [(200, 1)], "decode", _heads, {}),
          ("splits=2 n=530", 8, 32, [(600, 1)], "decode", _prefix(530), dict(num_splits=2)),
          ("splits=3 n=400", 8, 32, [(600, 1)], "decode", _prefix(400), dict(num_splits=3)),
          ("splits=8 n=300", 8, 32, [(600, 1)], "decode", _prefix(300), dict(num_splits=8)),
          ("mtp", 16, 16, [(140, 2), (50, 1)], "varlen", _mtp, {}),
          ("holes", 16, 16, [(300, 1), (40, 1)], "decode", _holes, {}),
          ("dtypes f16->f16", 16, 16, [(300, 1)], "decode", _permuted, dict(q_dtype="f16", out_dtype="f16")),
          ("dtypes bf16->bf16", 16, 16, [(300, 1)], "decode", _permuted, dict(q_dtype="bf16", out_dtype="bf16"))]
CASES = [n for n, *_ in _TABLE]
PREFIX_CASES = [n for n in CASES if n not in ("holes", "mtp")]   # every list valid up to n and -1 from there on
_cache = {}


def make_case(seed, Hq, bs, pairs, form, lists, **kw):
    c = V.make_case(seed, pairs, bs, Hq, **kw)
    c.form, c.indices = form, lists(c, np.random.default_rng(seed + 2)).astype(np.int32)
    c.topk = c.indices.shape[1]
    return c


def valid(c):
    """-> bool (T, topk): 0 <= index < the token's limit"""
    return (c.indices >= 0) & (c.indices < np.maximum(V.limits(c)[1], 0)[:, None])


def prefix_n(c, t):
    """-> n if token t's list is valid up to n and -1 from there on, else None"""
    ok = valid(c)[t]
    n = int(ok.sum())
    return n if ok[:n].all() and (c.indices[t, n:] == -1).all() else None


def rows_of(c, t):
    """-> the cache bytes (topk, 576) the list of token t names, zeros at invalid entries"""
    ok, idx, b = valid(c)[t], c.indices[t].astype(np.int64), V.limits(c)[0][t]
    out = np.zeros((c.topk, R.ROW), np.uint8)
    out[ok] = c.cache[c.block_table[b, idx[ok] // c.block_size].astype(np.int64), idx[ok] % c.block_size]
    return out


def compact(c, t):
    rows, bs = rows_of(c, t)[valid(c)[t]], c.block_size
    nb = max((c.topk + bs - 1) // bs, 1)
    cache = np.zeros((nb * bs, R.ROW), np.uint8)
    cache[:len(rows)] = rows
    return R.Case(q=c.q[t:t + 1], q_dtype=c.q_dtype, out_dtype=c.out_dtype, cache=cache.reshape(nb, bs, R.ROW), block_table=np.arange(nb, dtype=np.int32)[None],
                  seq_lens=np.array([len(rows)], np.int32), kv_scale=c.kv_scale, num_splits=c.num_splits, max_seq_len=c.topk, block_size=bs)


def attention_ref(c):
    """-> (out float64 (T, Hq, 512), vmax (T, Hq): max|dequantised latent| among the token's valid rows): mla_ref.attention_ref on the compactions"""
    per = [R.attention_ref(compact(c, t)) for t in range(c.q.shape[0])]
    return np.concatenate([o for o, _ in per]), np.concatenate([v for _, v in per])


def masked_model(c):
    T, Hq, _ = c.q.shape
    splits = max(c.num_splits, 1)
    chunk = R.chunk_of(c.topk, splits)
    out, ok = np.zeros((T, Hq, R.LATENT)), valid(c)
    for t in range(T):
        if not ok[t].any():
            continue
        K8 = R.LUT64[rows_of(c, t)]
        q = c.q[t].astype(np.float32)
        amax = np.abs(q).max(axis=1).astype(np.float32)
        tiny = (amax > 0) & (amax < R.TINY_Q)
        up = np.where(tiny, np.float32(R.TINY_Q_UP), np.float32(1.0))
        q, amax = q * up[:, None], amax * up
        safe = np.where(amax > 0, amax, np.float32(1.0))
        q_scale = np.where(amax > 0, safe / np.float32(448.0), np.float32(1.0))
        q_inv = np.where(amax > 0, np.float32(448.0) / safe, np.float32(1.0))
        q8 = R.LUT64[fp8_oracle.encode_torch_rne((q * q_inv[:, None]).astype(np.float32))]
        logit2 = (K8 @ q8.T) * (q_scale.astype(np.float64) / up * float(c.kv_scale[0]) * R.SOFTMAX_SCALE * math.log2(math.e))   # (topk, Hq)
        logit2[~ok[t]] = -np.inf
        M, Lsum, O = np.full(Hq, -np.inf), np.zeros(Hq), np.zeros((Hq, R.LATENT))
        for s in range(splits):
            m, l, o = np.full(Hq, -np.inf), np.zeros(Hq), np.zeros((Hq, R.LATENT))
            for p0 in range(s * chunk, min(s * chunk + chunk, c.topk), R.STEP):
                x = logit2[p0:min(p0 + R.STEP, c.topk)]
                if not ok[t, p0:p0 + R.STEP].any():
                    continue
                m_new = np.maximum(m, x.max(axis=0))
                alpha, p = 2.0 ** (m - m_new), 2.0 ** (x - m_new)
                p8 = R.LUT64[fp8_oracle.encode_torch_rne((p * R.P_SCALE).astype(np.float32))]
                l = l * alpha + p.sum(axis=0)
                o = o * alpha[:, None] + p8.T @ K8[p0:p0 + len(x), :R.LATENT]
                m = m_new
            if np.isfinite(m).all():   # the combine: a split without a valid entry weighs 0
                M_new = np.maximum(M, m)
                wa, wb = 2.0 ** (M - M_new), 2.0 ** (m - M_new)
                Lsum, O, M = Lsum * wa + l * wb, O * wa[:, None] + o * wb[:, None], M_new
        out[t] = O / (R.P_SCALE * Lsum[:, None]) * float(c.kv_scale[0])
    return R.round_to(out, c.out_dtype)


def case(name):
    """-> (Case, ref, vmax) of a named case: made once, shared, never written"""
    if name not in _cache:
        i = CASES.index(name)
        _, Hq, bs, pairs, form, lists, kw = _TABLE[i]
        c = make_case(1100 + i, Hq, bs, pairs, form, lists, **kw)
        _cache[name] = (c,) + attention_ref(c)
    return _cache[name]


def measure_E():
    return max(R.ratio(masked_model(case(n)[0]), *case(n)[1:]) for n in CASES)


E_mla_sparse = 0.02229
TOL = 2 * E_mla_sparse


def auto_splits(T, B, max_q_len, Hq, topk, ws_bytes, cus):
    """fp8mi_attn_auto_splits_mla_sparse: mla_ref.auto_splits with B max_q_len ceil(Hq / 64) workgroups, ceil(topk / 128) steps, partials for T rows"""
    steps, wgs = (topk + R.STEP - 1) // R.STEP, B * max_q_len * ((Hq + R.HEAD_TILE - 1) // R.HEAD_TILE)
    s = 1 if wgs <= 0 or steps <= R.MIN_STEPS else min((2 * cus + wgs - 1) // wgs, (steps + R.MIN_STEPS - 1) // R.MIN_STEPS, R.AUTO_SPLITS_MAX)
    while s > 1 and T * Hq * s * (R.LATENT + 2) * 4 > ws_bytes:
        s -= 1
    return s
