"""The reference of the multi-token (causal, variable-length) paged attention, fp8mi_paged_attention_varlen: numpy, CPU only, on top of
tests/paged_attn_ref.py.  A plain module: no fixtures, no tests.

A varlen case is a decode case of paged_attn_ref.make_case - caches filled to seq_lens, a shuffled table - with q (T, Hq, D) and
cu_seqlens_q in place of one query row per sequence.  The definition of the entry is its EXPANSION: expand(case) is the decode Case
with one sequence per query token - that token's q row, its sequence's table row, seq_len = max(limit, 0), limit = seq_len - q_len + j + 1 -
and the same caches, max_seq_len and num_splits.  The kernel is held to fp8mi_paged_attention_decode on expand(case) BIT FOR BIT; and
paged_attn_ref.attention_ref / attention_model apply to expand(case) as they are.

E_varlen is the largest ratio of attention_model(expand(c)) against attention_ref(expand(c)) over VARLEN_CASES, measured on the CPU with
the seeded generators here (the convention of DESIGN.md 5.18):
    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import paged_attn_varlen_ref as V; print(V.measure_E_varlen())"
    -> 0.025499785870037362 (the mixed batch, either split count; prefill q_len = seq_len = 17 gives 0.0252: rows with a handful of visible
       positions, where e4m3's step on Q shows most), recorded below rounded up to four digits; TOL_varlen = 2 E_varlen.  tests/test_paged_attn_varlen_host.py recomputes and pins it.
"""
import numpy as np

import paged_attn_ref as R

MAX_GROUP = 16   # csrc/fp8mi_attn.h: kAttnMaxGroup, the columns of a tile


def tile_tokens(Hq, Hkv):
    """TQ: the query tokens of one 16-column tile"""
    return MAX_GROUP // (Hq // Hkv)


def q_tiles(max_q_len, Hq, Hkv):
    tq = tile_tokens(Hq, Hkv)
    return (max_q_len + tq - 1) // tq


def auto_splits_varlen(T, B, max_q_len, Hq, Hkv, D, max_seq_len, ws_bytes, cus):
    """fp8mi_attn_auto_splits_varlen: paged_attn_ref.auto_splits with B Hkv ceil(max_q_len / TQ) workgroups and partials for T rows"""
    steps, wgs = (max_seq_len + R.STEP - 1) // R.STEP, B * Hkv * q_tiles(max_q_len, Hq, Hkv)
    if wgs <= 0 or steps <= R.WAVES:
        return 1
    s = min((2 * cus + wgs - 1) // wgs, (steps + R.WAVES - 1) // R.WAVES, R.AUTO_SPLITS_MAX)
    while s > 1 and R.workspace_bytes(T, Hq, D, s) > ws_bytes:
        s -= 1
    return max(s, 1)


def limits_of(seq_lens, q_lens):
    """the causal limit of every query token, in row order: token j of sequence b attends [0, seq_len - q_len + j + 1)"""
    return np.array([int(L) - int(n) + j + 1 for L, n in zip(seq_lens, q_lens) for j in range(int(n))], dtype=np.int64)


def make_varlen_case(seed, seq_lens, q_lens, block_size, D, Hq, Hkv, num_splits=1, max_seq_len=None, q_spread=None, **kw):
    """paged_attn_ref.make_case(seed, seq_lens, ...) with q (T, Hq, D), T = sum(q_lens), N(0, 1) rounded to q_dtype, and cu = the running sum
    of q_lens.  q_spread (with logits=): token rows are the base case's row of their sequence plus q_spread N(0, 1), so that the logit
    shape make_case gave K against that row holds, approximately, for every token."""
    c = R.make_case(seed, list(seq_lens), block_size, D, Hq, Hkv, num_splits=num_splits, **kw)
    rng = np.random.default_rng(seed + 77777)
    q_lens = np.array(q_lens, dtype=np.int64)
    T = int(q_lens.sum())
    q = rng.standard_normal((T, Hq, D))
    if q_spread is not None:
        q = np.repeat(c.q.astype(np.float64), q_lens, axis=0) + q_spread * q
    c.base_q = c.q
    c.q = R.round_to(q, c.q_dtype).astype(np.float32)
    c.q_lens = q_lens
    c.cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    c.max_q_len = int(max(q_lens.max(), 1))
    if max_seq_len is not None:
        assert max_seq_len >= max(seq_lens)
        c.max_seq_len = max_seq_len
    return c


def expand(c):
    """-> the decode Case with one sequence per query token, in row order (its row i is the varlen row i)"""
    seq_of = np.repeat(np.arange(len(c.q_lens)), c.q_lens)
    lim = np.maximum(limits_of(c.seq_lens, c.q_lens), 0)
    assert len(seq_of) == c.q.shape[0] and (lim <= c.seq_lens[seq_of]).all()
    d = dict(c.__dict__)
    d.update(seq_lens=lim.astype(np.int32), block_table=np.ascontiguousarray(c.block_table[seq_of]), seq_of=seq_of)
    return R.Case(**d)


def dense_causal(c, b, hq):
    """float64 causal attention of sequence b, query head hq, written directly: the q_len x seq_len score matrix, masked at the END of
    the context, a softmax per row -> (q_len, D); a row without a visible position is zero"""
    h = hq // (c.q.shape[1] // c.Hkv)
    kb, vb = R.gather(c, b, h)
    K, V = R.LUT64[kb] * R.head_scale(c.k_scale, h), R.LUT64[vb] * R.head_scale(c.v_scale, h)
    L, n = int(c.seq_lens[b]), int(c.q_lens[b])
    Q = c.q[c.cu[b]:c.cu[b + 1], hq].astype(np.float64)
    S = (Q @ K.T) * c.softmax_scale                                  # (n, L)
    visible = np.arange(L)[None, :] <= (L - n + np.arange(n))[:, None]   # position p <= the token's own position
    out = np.zeros((n, c.q.shape[2]))
    for j in range(n):
        if visible[j].any():
            s = np.where(visible[j], S[j], -np.inf)
            p = np.exp(s - s.max())
            out[j] = (p / p.sum()) @ V
    return out


# ---- the cases: tests/test_gpu_paged_attn_varlen.py runs every one -----------------------------------------------------------------------

GROUPS = (1, 2, 4, 5, 8, 16)
MAPPING = [(g, Hkv, i) for g in GROUPS for Hkv in (1, 2) for i in range(4)]   # i: q_len = TQ - 1, TQ, TQ + 1, 2 TQ + 1
STEP_EDGE = ((130, 4), (129, 2), (128, 1), (131, 8))          # (seq_len, q_len), G = 4: early columns own nothing of the second wave's step
PASS_EDGE = ((514, 4), (1026, 4))                             # a later pass of wave 0 is fully masked for columns whose m is finite
SPLIT_EDGE = ((2, 258, 4), (3, 386, 8), (8, 300, 5))          # (num_splits, seq_len, q_len) at max_seq_len = 512
BLOCK_EDGE = (16, 32, 128)                                    # q_len = 3 ending one past a block
PREFILL = (1, 17, 130)                                        # q_len = seq_len: into an empty cache
MIXED_Q, MIXED_SEQ = (1, 0, 7, 1, 33), (300, 12, 7, 1, 200)
LONG = [(prof, n) for prof in ("rising", "late_peak") for n in (1, 2)]
DTYPES = (("f16", "f16"), ("bf16", "bf16"), ("f32", "bf16"))


def mapping_q_len(g, i):
    tq = MAX_GROUP // g
    return (tq - 1, tq, tq + 1, 2 * tq + 1)[i]


def _makers():
    m = {}
    for k, (g, Hkv, i) in enumerate(MAPPING):
        n = mapping_q_len(g, i)
        # the sequence under test and a two-token companion: TQ - 1 is 0 at G = 16, and no case may compare nothing
        m[f"mapping G={g} Hkv={Hkv} q_len={n}"] = lambda g=g, Hkv=Hkv, n=n, k=k: make_varlen_case(
            20000 + k, [n + 40, 42], [n, 2], 16, (64, 128)[k % 2], g * Hkv, Hkv)
    for k, (L, n) in enumerate(STEP_EDGE):
        m[f"step edge L={L} q_len={n}"] = lambda L=L, n=n, k=k: make_varlen_case(21000 + k, [L], [n], 16, (128, 64)[k % 2], 8, 2)
    for k, (L, n) in enumerate(PASS_EDGE):
        m[f"pass edge L={L} q_len={n}"] = lambda L=L, n=n, k=k: make_varlen_case(22000 + k, [L], [n], 16, (64, 128)[k % 2], 4, 1)
    for k, (ns, L, n) in enumerate(SPLIT_EDGE):
        m[f"split edge splits={ns} L={L} q_len={n}"] = lambda ns=ns, L=L, n=n, k=k: make_varlen_case(
            23000 + k, [L], [n], 16, (128, 64)[k % 2], 8, 2, num_splits=ns, max_seq_len=512)
    for k, bs in enumerate(BLOCK_EDGE):
        m[f"block edge bs={bs}"] = lambda bs=bs, k=k: make_varlen_case(24000 + k, [2 * bs + 1], [3], bs, (64, 128)[k % 2], 4, 2)
    for k, L in enumerate(PREFILL):
        m[f"prefill q_len=seq_len={L}"] = lambda L=L, k=k: make_varlen_case(25000 + k, [L], [L], 16, (128, 64)[k % 2], 4, 2)
    m["q_len = seq_len + 3"] = lambda: make_varlen_case(25100, [5, 20], [8, 2], 16, 64, 8, 2)
    m["q_len = 0 and seq_len = 0 in a batch"] = lambda: make_varlen_case(25200, [50, 30, 0, 0, 19], [3, 0, 2, 0, 1], 16, 128, 8, 2)
    for ns in (1, 3):
        m[f"mixed batch splits={ns}"] = lambda ns=ns: make_varlen_case(26000, list(MIXED_SEQ), list(MIXED_Q), 16, 128, 8, 2, num_splits=ns)
    for prof, ns in LONG:
        m[f"long {prof} splits={ns}"] = lambda prof=prof, ns=ns: make_varlen_case(
            27000 + ns, [1300], [8], 16, 128, 4, 1, num_splits=ns, logits=R.PROFILES[prof](1300, ns), q_spread=0.25)
    for qd, od in DTYPES:
        m[f"dtypes {qd}->{od}"] = lambda qd=qd, od=od: make_varlen_case(28000, [45, 131], [5, 9], 16, 64, 4, 2, q_dtype=qd, out_dtype=od)
    m["per-head scales"] = lambda: make_varlen_case(28100, [90, 33], [6, 3], 64, 128, 8, 4, per_head=True)
    for ns in (1, 3):
        m[f"all q_len=1 splits={ns}"] = lambda ns=ns: make_varlen_case(29000, [300, 1, 77, 140], [1, 1, 1, 1], 16, 128, 8, 2, num_splits=ns)
    return m


_MAKERS = _makers()
VARLEN_CASES = list(_MAKERS)
_cache = {}


def varlen_case(name):
    """-> (Case, expand(Case), ref (a) of the expansion, vmax): made once, shared, never written"""
    if name not in _cache:
        c = _MAKERS[name]()
        e = expand(c)
        _cache[name] = (c, e) + R.attention_ref(e)
    return _cache[name]


def measure_E_varlen():
    """the largest ratio of the model (b) against the reference (a) over the expansions of VARLEN_CASES"""
    worst = 0.0
    for name in VARLEN_CASES:
        _c, e, ref, vmax = varlen_case(name)
        worst = max(worst, R.ratio(R.attention_model(e), ref, vmax))
    return worst


E_varlen = 0.02550          # measure_E_varlen(), rounded up
TOL_varlen = 2 * E_varlen   # 0.05100
