"""The reference of the lightning indexer (fp8mi_mla_index_cache_append, fp8mi_mla_index_logits, fp8mi_mla_index_topk): numpy, CPU only.  A plain
module: no fixtures, no tests.  The e4m3 table, the encoders and round_to are tests/paged_attn_ref.py's and the oracle's; limits() is
tests/mla_varlen_ref.py's.  The logits bound 2^-15 abs_sum is derived in tests/test_gpu_mla_indexer.py."""
import numpy as np

import fp8_oracle
import mla_varlen_ref as V
from paged_attn_ref import LUT64, TINY_Q, TINY_Q_UP, quantise, round_to

DIM, ROW = 128, 132
BOUND = 2.0 ** -15


def append_ref(k, rne=True):
    """k float32 (T, 128), finite -> (bytes (T, 128), scales float32 (T,))"""
    amax = np.abs(k).max(axis=1).astype(np.float32)
    d = (amax / np.float32(448.0)).astype(np.float32)
    m, e = np.frexp(d.astype(np.float64))                       # d = m 2^e, 0.5 <= m < 1
    up = np.where(d == 0, 0.0, np.where(m == 0.5, np.exp2(e - 1.0), np.exp2(1.0 * e)))
    scale = np.where(amax == 0, 1.0, np.maximum(up, 2.0 ** -126)).astype(np.float32)
    return np.stack([quantise(k[t], scale[t:t + 1], rne) for t in range(len(k))]), scale


def write_cache(cache, block_size, slots, data, scales):
    """cache uint8 (num_blocks, block_size 132), in place: rows and scales at `slots`"""
    blk, off = slots // block_size, slots % block_size
    for t in range(len(slots)):
        cache[blk[t], off[t] * DIM:(off[t] + 1) * DIM] = data[t]
        cache[blk[t], block_size * DIM + 4 * off[t]:block_size * DIM + 4 * off[t] + 4] = np.frombuffer(np.float32(scales[t]).tobytes(), np.uint8)


def make_case(seed, pairs, block_size, Hi, q_dtype="bf16", spare_blocks=2):
    """pairs: (seq_len, q_len) per sequence -> an mla_ref-style Case: N(0, 1) keys and queries, mixed-sign weights, a shuffled block table over
    blocks no two sequences share with spare blocks nobody owns, entries past the needed ones -1; the cache as append_ref fills it"""
    rng = np.random.default_rng(seed)
    lens = [L for L, _ in pairs]
    need = [(L + block_size - 1) // block_size for L in lens]
    num_blocks, max_blocks = sum(need) + spare_blocks, max(need) + 2
    perm = rng.permutation(num_blocks)
    table = np.full((len(pairs), max_blocks), -1, dtype=np.int32)
    cache = np.zeros((num_blocks, block_size * ROW), dtype=np.uint8)
    at = 0
    for b, L in enumerate(lens):
        table[b, :need[b]] = perm[at:at + need[b]]
        at += need[b]
        pos = np.arange(L)
        k = (rng.standard_normal((L, DIM)) * np.exp2(rng.integers(-3, 4, (L, 1)))).astype(np.float32)
        write_cache(cache, block_size, table[b, pos // block_size].astype(np.int64) * block_size + pos % block_size, *append_ref(k))
    c = V.R.Case(block_size=block_size, block_table=table, cache=cache, seq_lens=np.array(lens, np.int32), q_dtype=q_dtype,
                 q_lens=np.array([n for _, n in pairs], np.int32))
    c.cu = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    T = int(c.cu[-1])
    c.q = round_to(rng.standard_normal((T, Hi, DIM)), q_dtype).astype(np.float32)
    c.weights = (rng.standard_normal((T, Hi)) * Hi ** -0.5).astype(np.float32)
    c.max_seq_len = max_blocks * block_size
    return c


def keys_of(c, b, n):
    """-> (k8 values float64 (n, 128), scales float64 (n,)) of the first n positions of sequence b; a table entry out of range: zeros"""
    pos = np.arange(n)
    blk, off = c.block_table[b, pos // c.block_size].astype(np.int64), pos % c.block_size
    ok = (blk >= 0) & (blk < len(c.cache))
    blocks = c.cache[np.where(ok, blk, 0)]
    k8 = LUT64[blocks[pos[:, None], off[:, None] * DIM + np.arange(DIM)]]
    sc = np.ascontiguousarray(blocks[pos[:, None], c.block_size * DIM + 4 * off[:, None] + np.arange(4)]).view(np.float32)[:, 0].astype(np.float64)
    return np.where(ok[:, None], k8, 0.0), np.where(ok, sc, 0.0)


def quantise_q(q, weights):
    """q float32 (T, Hi, 128), weights float32 (T, Hi) -> (q8 float64, w' float32), every step in float32 as the kernel takes it"""
    amax = np.abs(q).max(axis=-1).astype(np.float32)
    tiny = (amax > 0) & (amax < TINY_Q)
    up = np.where(tiny, np.float32(TINY_Q_UP), np.float32(1.0))
    q, amax = q * up[..., None], amax * up
    safe = np.where(amax > 0, amax, np.float32(1.0))
    q_scale = np.where(amax > 0, safe / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    q_inv = np.where(amax > 0, np.float32(448.0) / safe, np.float32(1.0)).astype(np.float32)
    q8 = LUT64[fp8_oracle.encode_torch_rne((q * q_inv[..., None]).astype(np.float32))]
    qs = np.where(tiny, q_scale * np.float32(1.0 / TINY_Q_UP), q_scale).astype(np.float32)
    return q8, (weights * qs).astype(np.float32)


def logits_ref(c):
    """-> (per query row: logits float64 (limit,), abs_sum (limit,), the smallest head dot product), limits clamped to [0, max_seq_len]"""
    seq, lim = V.limits(c)
    q8, w = quantise_q(c.q, c.weights)
    rows = []
    for t in range(len(seq)):
        n = int(np.clip(lim[t], 0, c.max_seq_len))
        k8, sc = keys_of(c, seq[t], n)
        dots = k8 @ q8[t].T                                                    # (n, Hi)
        mags = np.abs(k8) @ np.abs(q8[t]).T
        rows.append((sc * (np.maximum(dots, 0.0) @ w[t].astype(np.float64)), np.abs(sc) * (mags @ np.abs(w[t]).astype(np.float64)), dots.min() if n else 0.0))
    return rows


def order_key(x):
    """float32 -> uint32 keys: IEEE totalOrder on the bits, every NaN below -inf"""
    u = np.asarray(x, np.float32).view(np.uint32)
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000))
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0, key).astype(np.uint32)


def topk_ref(row, limit, k):
    """-> int32 (k,): the min(k, limit) largest of row[:limit], ties to the lower position, ascending, then -1"""
    limit = int(np.clip(limit, 0, len(row)))
    order = np.argsort(~order_key(row[:limit]), kind="stable")   # descending keys, equal keys by rising position
    out = np.full(k, -1, np.int32)
    out[:min(k, limit)] = np.sort(order[:k])
    return out
