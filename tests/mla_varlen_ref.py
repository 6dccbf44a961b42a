"""The reference of the multi-token MLA attention (fp8mi_mla_attention_varlen): numpy, CPU only.  A plain module: no fixtures, no tests.
  expand        a varlen case as a tests/mla_ref.py Case with ONE sequence per query row - that row's q, its sequence's table row, seq_len =
                max(limit, 0), limit = seq_len_b - q_len_b + j + 1 - on which mla_ref.attention_ref (float64) and attention_model apply as they
                are, and on which the decode entry is what every row must equal bit for bit.
  CASES         the table of tests/test_gpu_mla_varlen.py, each the smallest that exercises its hazard; block_size rotates over 16 / 64 / 128.
  E_mla_varlen  the largest ratio of the model against the float64 reference over that table, measured on the CPU: measure_E() ->
                0.044693235362393544 (short-context: one or two keys, one e4m3 step of Q among few terms), recorded below rounded up; TOL = 2 E
                is the project's convention (tests/paged_attn_ref.py says what the factor covers).  tests/test_mla_varlen_host.py pins it."""
import numpy as np

import mla_ref as R

SPLIT_MAX_SEQ = 1024


def make_case(seed, pairs, block_size, Hq, **kw):
    """pairs: (seq_len, q_len) per sequence, seq_len counting the q_len tokens -> an mla_ref Case of the B sequences whose q is (T, Hq, 576),
    with cu (B + 1,) and q_lens"""
    c = R.make_case(seed, [L for L, _ in pairs], block_size, Hq, **kw)
    c.q_lens = np.array([n for _, n in pairs], dtype=np.int32)
    c.cu = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    c.q = R.round_to(np.random.default_rng(seed + 1).standard_normal((int(c.cu[-1]), Hq, R.ROW)), c.q_dtype).astype(np.float32)
    return c


def limits(c):
    """-> (the sequence of every query row, its limit: may be negative)"""
    seq = np.repeat(np.arange(len(c.q_lens)), c.q_lens)
    return seq, c.seq_lens[seq].astype(np.int64) - c.q_lens[seq] + (np.arange(len(seq)) - c.cu[seq]) + 1


def expand(c):
    seq, lim = limits(c)
    return R.Case(q=c.q, q_dtype=c.q_dtype, out_dtype=c.out_dtype, cache=c.cache, block_table=c.block_table[seq], seq_lens=np.maximum(lim, 0).astype(np.int32),
                  kv_scale=c.kv_scale, num_splits=c.num_splits, max_seq_len=c.max_seq_len, block_size=c.block_size)


_TABLE = [("mtp", 128, [(130, 2), (257, 2)], {}),            # two tiles per token, four per sequence
          ("packed", 16, [(130, 4)], {}),                    # four tokens in one tile; limits 127 .. 130 straddle a step
          ("straddle", 20, [(140, 3)], {}),                  # a token across two waves, two tokens in one wave
          ("odd", 5, [(40, 13)], {}),                        # 65 columns: a second tile with one live column
          ("one-head", 1, [(33, 17)], {}),                   # 16 tokens in one wave, a 17th in the next
          ("short-context", 16, [(2, 4), (0, 3)], {}),       # limit <= 0 beside live columns, all-empty tiles: zero rows
          ("mixed", 16, [(300, 1), (37, 0), (131, 5), (16, 16)], {}),   # decode rows, an absent sequence, a prompt of its own length
          ("chunk", 16, [(300, 140)], {}),                   # 35 tiles whose trimmed ends differ by whole steps
          ("splits=2", 8, [(514, 4)], dict(num_splits=2, max_seq_len=SPLIT_MAX_SEQ)),    # limits either side of a split boundary
          ("splits=3", 8, [(400, 6)], dict(num_splits=3, max_seq_len=SPLIT_MAX_SEQ)),
          ("splits=8", 8, [(300, 4)], dict(num_splits=8, max_seq_len=SPLIT_MAX_SEQ))]    # columns whose split owns nothing, splits that own nothing
_TABLE += [(f"dtypes {qd}->{od}", 8, [(45, 3), (131, 2)], dict(q_dtype=qd, out_dtype=od)) for qd in R.DTYPES for od in R.DTYPES]
CASES = [n for n, *_ in _TABLE]
_cache = {}


def case(name):
    """-> (varlen Case, its expansion, ref (a), vmax) of a named case: made once, shared, never written"""
    if name not in _cache:
        i = CASES.index(name)
        _, Hq, pairs, kw = _TABLE[i]
        bs = (16, 64, 128)[i % 3]
        e = expand(c := make_case(900 + i, pairs, bs, Hq, table_blocks=kw.get("max_seq_len", 0) // bs, **kw))
        _cache[name] = (c, e) + R.attention_ref(e)
    return _cache[name]


def measure_E():
    return max(R.ratio(R.attention_model(case(n)[1]), *case(n)[2:]) for n in CASES)


E_mla_varlen = 0.0447
TOL = 2 * E_mla_varlen


def auto_splits(T, B, max_q_len, Hq, max_seq_len, ws_bytes, cus):
    """fp8mi_attn_auto_splits_mla_varlen: mla_ref.auto_splits with B ceil(max_q_len Hq / 64) workgroups and partials for T rows"""
    steps, wgs = (max_seq_len + R.STEP - 1) // R.STEP, B * ((max_q_len * Hq + R.HEAD_TILE - 1) // R.HEAD_TILE)
    s = 1 if wgs <= 0 or steps <= R.MIN_STEPS else min((2 * cus + wgs - 1) // wgs, (steps + R.MIN_STEPS - 1) // R.MIN_STEPS, R.AUTO_SPLITS_MAX)
    while s > 1 and T * Hq * s * (R.LATENT + 2) * 4 > ws_bytes:
        s -= 1
    return s
