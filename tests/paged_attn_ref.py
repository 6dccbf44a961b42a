"""The reference of the FP8 paged KV cache and the single-query decode attention (fp8mi_kv_cache_append, fp8mi_paged_attention_decode):
numpy, CPU only.  A plain module: no fixtures, no tests.

  (a) attention_ref    float64 attention over the cache bytes decoded with the oracle's e4m3 table (OCP: 0x7F / 0xFF are NaN) times the
                       scales, with Q exact: the thing every GPU result is compared against.
  (b) attention_model  the kernel's documented roundings restated, float64 otherwise: Q rounded to e4m3 per (sequence, head) row with
                       the scale amax / 448 (a row with amax below 2^-64 through a factor 2^64, as the kernel does); the probabilities rounded to e4m3 as rne(p 2^8), p relative to the running maximum of the
                       wave that owns the 128-position step (waves take the steps of their split round-robin); the row sum from the
                       unrounded p; the output rounded to out_dtype.
  (c) TOL              every comparison is |out - ref(a)| <= TOL * max|dequantised V of that sequence and KV head| (the output is a
                       convex combination of V rows), no element left out.  E is the largest such ratio of (b) against (a) over
                       all_cases() - every case tests/test_gpu_paged_attn.py runs - and TOL = 2 E: the factor covers the places where
                       kernel and model may round a probability to different neighbours (hardware exp2, the summation order inside an
                       MFMA, the fp32 score scale), each bounded by the per-element step that produced E.

E was measured on the CPU with the seeded generator below:
    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import paged_attn_ref as R; print(R.measure_E())"
    -> 0.022931255127231685 (the "graph 1" case; the dominant-key case gives 0.0038), recorded below rounded up to four digits.  It is below
    2^-4 = 0.0625, one e4m3 half-step on a convex combination.  tests/test_paged_attn_host.py recomputes it and pins the constant.

  (d) the edge groups  what all_cases() leaves out, for tests/test_gpu_paged_attn_edges.py (the section at the end of this file): splits of
                       more than 512 positions with shaped logits, other softmax scales, Hkv = 3, query rows too small for 448 / amax - each
                       group with its own E_<group> and TOL_<group> = 2 E_<group>; attention_model(case, mutate=) leaves the online
                       softmax's rescale out, to prove that the shaped cases would catch it; auto_splits restates the library's split choice.
"""
import math

import numpy as np

import fp8_oracle

STEP, WAVES, P_SCALE = 128, 4, 256.0   # csrc/fp8mi_attn.h: positions per step, waves per workgroup, the scale of P before it is packed
BLOCK_SIZES, HEAD_DIMS = (16, 32, 64, 128), (64, 128)
LUT64 = fp8_oracle.decode_lut(nan_to_zero=False).astype(np.float64)   # OCP: the two NaN bytes are NaN


# ---- the cache: slots, layouts ----------------------------------------------------------------------------------------------------------

def slot_block_offset(slot, block_size):
    """slot = block * block_size + offset"""
    return slot // block_size, slot % block_size


def k_index(slot, h, d, Hkv, block_size, D):
    """flat index into the K cache uint8 [num_blocks, Hkv, block_size, D]"""
    blk, off = slot_block_offset(slot, block_size)
    return ((blk * Hkv + h) * block_size + off) * D + d


def v_index(slot, h, d, Hkv, block_size, D):
    """flat index into the V cache uint8 [num_blocks, Hkv, D, block_size]"""
    blk, off = slot_block_offset(slot, block_size)
    return ((blk * Hkv + h) * D + d) * block_size + off


def quantise(x, scale, rne=True):
    """the bytes fp8mi_encode gives x with prescale = 1.0f / scale (an IEEE fp32 division, an fp32 product)"""
    pre = np.float32(1.0) / np.asarray(scale, dtype=np.float32)
    y = (np.asarray(x, dtype=np.float32) * pre).astype(np.float32)
    return fp8_oracle.encode_torch_rne(y) if rne else fp8_oracle.encode(y)


def append_ref(k_cache, v_cache, k, v, slots, k_scale, v_scale, rne=True):
    """fp8mi_kv_cache_append on numpy caches, in place: k, v (T, Hkv, D) float32 values, scales [1] or [Hkv]"""
    nb, Hkv, bs, D = k_cache.shape
    ks = np.broadcast_to(np.asarray(k_scale, np.float32).reshape(-1, 1), (Hkv, 1)) if np.size(k_scale) == Hkv else np.float32(np.ravel(k_scale)[0])
    vs = np.broadcast_to(np.asarray(v_scale, np.float32).reshape(-1, 1), (Hkv, 1)) if np.size(v_scale) == Hkv else np.float32(np.ravel(v_scale)[0])
    for t, slot in enumerate(np.asarray(slots).tolist()):
        if slot < 0 or slot >= nb * bs:
            continue
        blk, off = slot_block_offset(slot, bs)
        k_cache[blk, :, off, :] = quantise(k[t], ks, rne)
        v_cache[blk, :, :, off] = quantise(v[t], vs, rne)


def gather(case, b, h):
    """-> (K bytes (L, D), V bytes (L, D)) of sequence b, KV head h, through the block table"""
    L, bs = int(case.seq_lens[b]), case.block_size
    pos = np.arange(L)
    blk = case.block_table[b, pos // bs].astype(np.int64)
    return case.k_cache[blk, h, pos % bs, :], case.v_cache[blk, h, :, pos % bs]


def head_scale(s, h):
    s = np.asarray(s, np.float32).reshape(-1)
    return float(s[h] if s.size > 1 else s[0])


def round_to(x, dtype):
    """float64 -> the nearest value of the output dtype (round to nearest even), as float64"""
    if dtype == "f32":
        return x.astype(np.float32).astype(np.float64)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float64)
    bits = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


# ---- (a) the float64 reference -----------------------------------------------------------------------------------------------------------

def attention_ref(case):
    """-> (out float64 (B, Hq, D), vmax float64 (B, Hq): max|dequantised V| of the row's sequence and KV head, 0 for an empty one)"""
    B, Hq, D = case.q.shape
    group = Hq // case.Hkv
    out, vmax = np.zeros((B, Hq, D)), np.zeros((B, Hq))
    for b in range(B):
        if case.seq_lens[b] == 0:
            continue
        for h in range(case.Hkv):
            kb, vb = gather(case, b, h)
            K, V = LUT64[kb] * head_scale(case.k_scale, h), LUT64[vb] * head_scale(case.v_scale, h)
            for hq in range(h * group, (h + 1) * group):
                s = (K @ case.q[b, hq].astype(np.float64)) * case.softmax_scale
                p = np.exp(s - s.max())
                out[b, hq] = (p / p.sum()) @ V
                vmax[b, hq] = np.abs(V).max()
    return out, vmax


def dense_attention(q, K, V, softmax_scale):
    """plain softmax attention of one query row over dense float64 K, V (L, D)"""
    s = (K @ q) * softmax_scale
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V


# ---- (b) the model of the kernel's roundings ---------------------------------------------------------------------------------------------

def chunk_of(max_seq_len, splits):
    steps = (max_seq_len + STEP - 1) // STEP
    return ((steps + splits - 1) // splits) * STEP


TINY_Q, TINY_Q_UP = 2.0 ** -64, 2.0 ** 64   # csrc/fp8mi_attn.h: a query row with 0 < amax < TINY_Q is quantised as the row times TINY_Q_UP


def attention_model(case, mutate=None):
    """-> out float64 (B, Hq, D), rounded to case.out_dtype.  mutate = "o" / "l": the rescale by alpha = exp2(m_old - m_new) left out on the
    output accumulator / on the row sum - the bug tests/test_paged_attn_host.py proves the `long` cases catch."""
    assert mutate in (None, "o", "l")
    B, Hq, D = case.q.shape
    group, splits = Hq // case.Hkv, max(case.num_splits, 1)
    chunk = chunk_of(case.max_seq_len, splits)
    out = np.zeros((B, Hq, D))
    for b in range(B):
        L = int(case.seq_lens[b])
        if L == 0:
            continue
        for h in range(case.Hkv):
            kb, vb = gather(case, b, h)
            K8, V8 = LUT64[kb], LUT64[vb]
            for hq in range(h * group, (h + 1) * group):
                q = case.q[b, hq].astype(np.float32)
                amax = np.float32(np.abs(q).max())
                fold = 1.0
                if 0 < amax < TINY_Q:   # 448 / amax would be +inf below 448 / FLT_MAX: an exact power of two first, folded back into the scale
                    q, amax, fold = q * np.float32(TINY_Q_UP), amax * np.float32(TINY_Q_UP), TINY_Q
                q_scale = amax / np.float32(448.0) if amax > 0 else np.float32(1.0)
                q_inv = np.float32(448.0) / amax if amax > 0 else np.float32(1.0)
                q8 = LUT64[fp8_oracle.encode_torch_rne((q * q_inv).astype(np.float32))]
                logit2 = (K8 @ q8) * (float(q_scale) * fold * head_scale(case.k_scale, h) * case.softmax_scale * math.log2(math.e))
                parts = []   # (m, l, O) of every wave of every split that owns a step
                for s in range(splits):
                    lo = s * chunk
                    hi = L if (s == splits - 1 or lo + chunk > L) else lo + chunk
                    for w in range(WAVES):
                        m, l, o = -np.inf, 0.0, np.zeros(D)
                        for p0 in range(lo + w * STEP, hi, WAVES * STEP):
                            x = logit2[p0:min(p0 + STEP, hi)]
                            m_new = max(m, x.max())
                            alpha = 2.0 ** (m - m_new)
                            p = 2.0 ** (x - m_new)
                            p8 = LUT64[fp8_oracle.encode_torch_rne((p * P_SCALE).astype(np.float32))]
                            l = l * (1.0 if mutate == "l" else alpha) + p.sum()
                            o = o * (1.0 if mutate == "o" else alpha) + p8 @ V8[p0:p0 + len(x)]
                            m = m_new
                        if m > -np.inf:
                            parts.append((m, l, o))
                M = max(m for m, _, _ in parts)
                Lsum = sum(2.0 ** (m - M) * l for m, l, _ in parts)
                O = sum(2.0 ** (m - M) * o for m, _, o in parts)
                out[b, hq] = O / (P_SCALE * Lsum) * head_scale(case.v_scale, h)
    return round_to(out, case.out_dtype)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------

class Case:
    """One call of fp8mi_paged_attention_decode on numpy data.  `k_owned` / `v_owned`: the bytes of the caches that hold a position below
    its sequence's length - every other byte must not influence the output."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def dominant_logits(pos, rng):
    """key 0 at 8, the others U(-1, 1)"""
    t = rng.uniform(-1.0, 1.0, len(pos))
    t[pos == 0] = 8.0
    return t


def make_case(seed, seq_lens, block_size, D, Hq, Hkv, num_splits=1, q_dtype="f32", out_dtype="f32", per_head=False, dominant=False,
              name_spares=False, spare_blocks=2, logits=None, softmax_scale=None):
    """N(0, 1) Q, K, V, softmax_scale = D^-1/2, scales such that the caches use the e4m3 range; a shuffled, non-monotonic block table over
    physical blocks no two sequences share, entries past the needed ones -1 (name_spares: the ids of unowned spare blocks instead);
    dominant: one key of every sequence scores 8 above the others in the scaled logits, the others within +-1 of each other;
    logits: the general form - a function (positions, rng) -> the target scaled logit of every position, set exactly (before the cache's
    rounding) for the first query head of every KV head by a rank-one correction of K (Hq == Hkv shapes every head); dominant is
    logits=dominant_logits;  softmax_scale: in place of D^-1/2."""
    if dominant:
        logits = dominant_logits
    rng = np.random.default_rng(seed)
    B = len(seq_lens)
    need = [(L + block_size - 1) // block_size for L in seq_lens]
    num_blocks = sum(need) + spare_blocks
    max_blocks = max(need) + 2
    perm = rng.permutation(num_blocks)
    table = np.full((B, max_blocks), -1, dtype=np.int32)
    at = 0
    for b in range(B):
        table[b, :need[b]] = perm[at:at + need[b]]
        at += need[b]
    spares = perm[at:]
    if name_spares:
        for b in range(B):
            table[b, need[b]:] = spares[rng.integers(0, len(spares), max_blocks - need[b])]
    q = round_to(rng.standard_normal((B, Hq, D)), q_dtype).astype(np.float32)
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    ks, vs = [], []
    for b in range(B):
        k = rng.standard_normal((seq_lens[b], Hkv, D))
        v = rng.standard_normal((seq_lens[b], Hkv, D))
        if logits is not None:   # every key's logit against query head h * group set exactly (dominant: 8 for key 0, U(-1, 1) for the others)
            group = Hq // Hkv
            for h in range(Hkv):
                qh = q[b, h * group].astype(np.float64)
                t = logits(np.arange(seq_lens[b]), rng)
                k[:, h, :] += np.outer((t / scale - k[:, h, :] @ qh) / (qh @ qh), qh)
        ks.append(k)
        vs.append(v)
    allk = np.concatenate(ks) if sum(seq_lens) else np.ones((1, Hkv, D))
    allv = np.concatenate(vs) if sum(seq_lens) else np.ones((1, Hkv, D))
    if per_head:
        k_scale = (np.abs(allk).max(axis=(0, 2)) / 448.0).astype(np.float32)
        v_scale = (np.abs(allv).max(axis=(0, 2)) / 448.0).astype(np.float32)
    else:
        k_scale = np.array([np.abs(allk).max() / 448.0], dtype=np.float32)
        v_scale = np.array([np.abs(allv).max() / 448.0], dtype=np.float32)
    k_cache = np.zeros((num_blocks, Hkv, block_size, D), dtype=np.uint8)
    v_cache = np.zeros((num_blocks, Hkv, D, block_size), dtype=np.uint8)
    k_owned, v_owned = np.zeros(k_cache.shape, dtype=bool), np.zeros(v_cache.shape, dtype=bool)
    slots = []
    for b in range(B):
        pos = np.arange(seq_lens[b])
        s = table[b, pos // block_size].astype(np.int64) * block_size + pos % block_size
        append_ref(k_cache, v_cache, ks[b], vs[b], s, k_scale, v_scale)
        k_owned[s // block_size, :, s % block_size, :] = True
        v_owned[s // block_size, :, :, s % block_size] = True
        slots.append(s)
    return Case(q=q, q_dtype=q_dtype, out_dtype=out_dtype, k_cache=k_cache, v_cache=v_cache, k_owned=k_owned, v_owned=v_owned, block_table=table,
                seq_lens=np.array(seq_lens, dtype=np.int32), k_scale=k_scale, v_scale=v_scale, softmax_scale=scale, num_splits=num_splits,
                max_seq_len=max(max(seq_lens), 1), block_size=block_size, Hkv=Hkv, D=D, k_values=ks, v_values=vs, slots=slots)


GRID_LENS = (1, 15, 16, 17, 127, 128, 129, 257)          # both sides of a block, of an S tile, of a 128-position step
GRID = [(L, bs, D) for L in GRID_LENS for bs in (16, 32, 128) for D in (64, 128)]
GROUPS = [(g, Hkv) for g in (1, 4, 5, 8, 16) for Hkv in (1, 2)]
MIXED_LENS = (0, 1, 300, 37)
SPLITS = (1, 2, 3, 8)
DTYPES = ("f32", "f16", "bf16")
APPEND_STEPS, APPEND_AT = 40, (1, 16, 17, 40)


def grid_case(L, bs, D):
    return make_case(1000 + 7 * L + bs + D, [L], bs, D, Hq=4, Hkv=2)


def group_case(g, Hkv):
    return make_case(2000 + 10 * g + Hkv, [70], 16, 128, Hq=g * Hkv, Hkv=Hkv)


def mixed_case(num_splits):
    return make_case(3000, list(MIXED_LENS), 16, 128, Hq=8, Hkv=2, num_splits=num_splits)


def split_case(num_splits):
    return make_case(4000, [300], 32, 128, Hq=4, Hkv=1, num_splits=num_splits)


def garbage_case(D, num_splits=1):
    return make_case(5000 + D, [37, 130], 32, D, Hq=4, Hkv=2, num_splits=num_splits, name_spares=True, spare_blocks=3)


def dominant_case():
    return make_case(6000, [256], 64, 128, Hq=2, Hkv=2, dominant=True)


def dtype_case(q_dtype, out_dtype):
    return make_case(7000, [45, 131], 16, 64, Hq=4, Hkv=2, q_dtype=q_dtype, out_dtype=out_dtype)


def per_head_case():
    return make_case(8000, [90], 64, 128, Hq=8, Hkv=4, per_head=True)


GRAPH_MAX_BLOCKS, GRAPH_MAX_SEQ = 12, 192   # the static table of the graph test and the bound it passes


def graph_cases(num_splits):
    """two cases of one geometry (16 physical blocks; the test pads both tables to GRAPH_MAX_BLOCKS entries): a graph captured on the first
    replays on the second"""
    cases = (make_case(9000, [33, 140], 16, 128, Hq=4, Hkv=2, num_splits=num_splits, spare_blocks=4),
             make_case(9001, [150, 9], 16, 128, Hq=4, Hkv=2, num_splits=num_splits, spare_blocks=5))
    for c in cases:
        assert c.k_cache.shape[0] == 16 and c.block_table.shape[1] <= GRAPH_MAX_BLOCKS
        c.max_seq_len = GRAPH_MAX_SEQ
    return cases


def append_case(steps):
    """the op-layer test's cache after `steps` tokens (one sequence, appended token by token): a prefix of one fixed sequence"""
    c = make_case(9500, [APPEND_STEPS], 16, 64, Hq=4, Hkv=2)
    c.seq_lens = np.array([steps], dtype=np.int32)
    c.max_seq_len = APPEND_STEPS   # the op layer's default bound is what the table can name; the test passes this one
    return c


def all_cases():
    """(name, Case) of every numeric configuration tests/test_gpu_paged_attn.py compares against (a)"""
    for L, bs, D in GRID:
        yield f"grid L={L} bs={bs} D={D}", grid_case(L, bs, D)
    for g, Hkv in GROUPS:
        yield f"group {g} Hkv={Hkv}", group_case(g, Hkv)
    for n in (1, 3):
        yield f"mixed splits={n}", mixed_case(n)
    for n in SPLITS:
        yield f"splits={n}", split_case(n)
    for D in HEAD_DIMS:
        for n in (1, 2):
            yield f"garbage D={D} splits={n}", garbage_case(D, n)
    yield "dominant", dominant_case()
    for qd in DTYPES:
        for od in DTYPES:
            yield f"dtypes {qd}->{od}", dtype_case(qd, od)
    yield "per-head scales", per_head_case()
    for n in (1, 2):
        for i, c in enumerate(graph_cases(n)):
            yield f"graph {i} splits={n}", c
    for n in APPEND_AT:
        yield f"append {n}", append_case(n)


def ratio(out, ref, vmax):
    """max over every element of |out - ref| / vmax of its row (rows of an empty sequence: |out - ref| must be 0)"""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref)
    if np.isnan(err).any():
        return np.inf
    live = vmax > 0
    assert np.all(err[~live] == 0), "a row of an empty sequence is not zero"
    return float((err[live] / vmax[live][:, None]).max()) if live.any() else 0.0


def measure_E():
    """the largest ratio of the model (b) against the reference (a) over all_cases()"""
    worst = 0.0
    for _name, c in all_cases():
        ref, vmax = attention_ref(c)
        worst = max(worst, ratio(attention_model(c), ref, vmax))
    return worst


E = 0.02294     # measure_E(), rounded up
TOL = 2 * E     # 0.04588


# ---- the library's split choice, restated ---------------------------------------------------------------------------------------------------

AUTO_SPLITS_MAX = 64   # csrc/fp8mi_attn.h: kAttnAutoSplits


def workspace_bytes(B, Hq, D, splits):
    """fp8mi_attn_workspace_bytes: m, l and O (D floats) per sequence, query head and split"""
    return 0 if splits <= 1 else B * Hq * splits * (D + 2) * 4


def auto_splits(B, Hq, Hkv, D, max_seq_len, ws_bytes, cus):
    """fp8mi_attn_auto_splits: two workgroups per compute unit, no split shorter than one step per wave, no more than the workspace holds"""
    steps, wgs = (max_seq_len + STEP - 1) // STEP, B * Hkv
    if wgs <= 0 or steps <= WAVES:
        return 1
    s = min((2 * cus + wgs - 1) // wgs, (steps + WAVES - 1) // WAVES, AUTO_SPLITS_MAX)
    while s > 1 and workspace_bytes(B, Hq, D, s) > ws_bytes:
        s -= 1
    return max(s, 1)


# ---- the edge groups: tests/test_gpu_paged_attn_edges.py ------------------------------------------------------------------------------------
# What all_cases() does not reach.  No wave of a case above makes a second pass of its loop (a split of more than WAVES * STEP = 512
# positions), so alpha = exp2(m_old - m_new) is exp2(-inf) = 0 there and the rescale of l and O never acts.  Each group below has its own
# E_<group> - the largest ratio of (b) against (a) over the group, measured on the CPU with the seeded generators here
# (measure_edge_E(group)), recorded rounded up as E is - and TOL_<group> = 2 E_<group>.

def split_bounds(L, max_seq_len, splits):
    """[(lo, hi)] of every split of a sequence of L positions, as the kernel cuts them"""
    chunk = chunk_of(max_seq_len, splits)
    return [(s * chunk, L if (s == splits - 1 or s * chunk + chunk > L) else s * chunk + chunk) for s in range(splits)]


def wave_steps(lo, hi, w):
    """the first positions of the steps wave w takes of the split [lo, hi)"""
    return list(range(lo + w * STEP, hi, WAVES * STEP))


def most_passes(L, splits):
    """-> (passes, first position, end) of the last step of the wave that makes the most passes (the first such wave)"""
    best = (0, 0, 0)
    for lo, hi in split_bounds(L, L, splits):
        for w in range(WAVES):
            st = wave_steps(lo, hi, w)
            if len(st) > best[0]:
                best = (len(st), st[-1], min(st[-1] + STEP, hi))
    return best


def rising(L, splits, sign=3.0):
    """every 128-position step 3 nats above the one before: every pass of every wave meets a new maximum, 12 nats above its last"""
    return lambda pos, rng: rng.uniform(-1.0, 1.0, len(pos)) + sign * (pos // STEP)


def falling(L, splits):
    """... 3 nats below: the maximum stays the first pass's, alpha is 1 and the later passes' probabilities are e^-12 and less"""
    return rising(L, splits, -3.0)


def late_peak(L, splits):
    """U(-1, 1), and one key at 8 in the middle of the last step of the wave that makes the most passes: what that wave accumulated
    before is worth e^-7 of it"""
    _n, p0, end = most_passes(L, splits)

    def f(pos, rng):
        t = rng.uniform(-1.0, 1.0, len(pos))
        t[pos == p0 + (end - p0) // 2] = 8.0
        return t
    return f


PROFILES = {"random": None, "rising": rising, "falling": falling, "late_peak": late_peak}
LONG_LENS = ((513, 1), (640, 1), (1025, 1), (1153, 1), (1300, 2))               # (L, splits): two passes from 513, three from 1025
LONG_SHAPES = [(bs, D) for bs in (16, 64, 128) for D in (64, 128)]              # bs = 64 with D = 64 among them
LONG = [(L, n, prof) + LONG_SHAPES[(4 * i + j) % 6] for i, (L, n) in enumerate(LONG_LENS) for j, prof in enumerate(PROFILES)]
SCALE_FACTORS = (0.0, -4.0, 32.0, 1.0 / 64)                                     # softmax_scale = factor D^-1/2
HEADS_LENS, HEADS_SPLITS = (130, 1, 300), 3
TINY_Q_DTYPES = ("f32", "bf16")
# scale 0: every probability is 1 and packs to 256 exactly, l = L exactly: what is left is the fp8 MFMA's in-instruction sum, which drops
# from an addend what lies 2^13 below its group's largest product (a mean of such terms is within 2^-13 max|V|), and
# at most L = 200 fp32 roundings of partial sums of at most L max|V| (L 2^-24 max|V| after the division by L).  The model has neither.
FLOOR_SCALE0 = 2.0 ** -13 + 200 * 2.0 ** -24


def long_case(L, splits, profile, bs, D):
    shape = PROFILES[profile]
    return make_case(10000 + 8 * L + list(PROFILES).index(profile), [L], bs, D, Hq=2, Hkv=2, num_splits=splits, logits=shape and shape(L, splits))


def scales_case(factor):
    """q on the e4m3 grid (every row's amax 448 2^-8, the other elements e4m3 values times 2^-8): the kernel's row quantisation is exact,
    and what separates (b) from (a) is the rounding of P alone.  With N(0, 1) q the 32x case tests nothing: e4m3's steps on Q are a nat of
    noise on logits of deviation 32, the softmax is one-hot, and the model itself is 0.36 max|V| from (a) (measured)."""
    c = make_case(10500, [200], 32, 128, Hq=4, Hkv=2, softmax_scale=factor * 128 ** -0.5)
    amax = np.abs(c.q).max(axis=-1, keepdims=True)
    c.q = (LUT64[fp8_oracle.encode_torch_rne((c.q * (np.float32(448.0) / amax)).astype(np.float32))] / 256.0).astype(np.float32)
    assert (np.abs(c.q).max(axis=-1) == 1.75).all()
    return c


def heads_case():
    """Hkv not a power of two in blockIdx -> (sequence, KV head, split)"""
    return make_case(10600, list(HEADS_LENS), 32, 64, Hq=6, Hkv=3, num_splits=HEADS_SPLITS)


TINY_Q_ROWS = {1: "amax 1e-37", 2: "subnormal amax", 3: "one element 1e-37", 4: "all zero", 6: "amax 1e-37, another row"}   # the others: N(0, 1)


def tiny_q_case(q_dtype):
    """Query rows whose amax is below 448 / FLT_MAX = 1.32e-36 (448 / amax is +inf in fp32) next to N(0, 1) rows in one launch: their
    logits are 0 to every precision here and their output is the mean of V.  Row 2: amax 2^-140, an fp32 subnormal (bf16: 2^-130, a
    bfloat16 subnormal)."""
    c = make_case(10700 + TINY_Q_DTYPES.index(q_dtype), [150], 16, 128 if q_dtype == "f32" else 64, Hq=8, Hkv=2, q_dtype=q_dtype)
    q = c.q.astype(np.float64)
    unit = q / np.abs(q).max(axis=-1, keepdims=True)
    q[0, 1] = unit[0, 1] * 1e-37
    q[0, 2] = np.rint(unit[0, 2] * 512) * 2.0 ** -149 if q_dtype == "f32" else unit[0, 2] * 2.0 ** -130
    q[0, 3] = 0.0
    q[0, 3, 7] = 1e-37
    q[0, 4] = 0.0
    q[0, 6] = -unit[0, 6] * 1e-37
    c.q = round_to(q, q_dtype).astype(np.float32)
    amax = np.abs(c.q[0]).max(axis=-1)
    assert all(0 < amax[r] < 448.0 / np.finfo(np.float32).max for r in (1, 2, 3, 6)) and amax[4] == 0 and amax[[0, 5, 7]].min() > 0.5
    assert amax[2] == (2.0 ** -140 if q_dtype == "f32" else 2.0 ** -130) and np.count_nonzero(c.q[0, 3]) == 1
    return c


EDGE_NAMES = {
    "long": [f"L={L} splits={n} {prof} bs={bs} D={D}" for L, n, prof, bs, D in LONG],
    "scales": [f"softmax_scale = {f:g} D^-1/2" for f in SCALE_FACTORS],
    "heads": ["Hkv=3 Hq=6 B=3 splits=3"],
    "tiny_q": [f"tiny q rows {d}" for d in TINY_Q_DTYPES],
}
_EDGE_MAKERS = {
    "long": [lambda s=s: long_case(*s) for s in LONG],
    "scales": [lambda f=f: scales_case(f) for f in SCALE_FACTORS],
    "heads": [heads_case],
    "tiny_q": [lambda d=d: tiny_q_case(d) for d in TINY_Q_DTYPES],
}
_edge_cache = {}


def edge_case(group, i):
    """-> (name, Case, ref (a), vmax) of case i of a group: made once, shared, never written"""
    if (group, i) not in _edge_cache:
        c = _EDGE_MAKERS[group][i]()
        _edge_cache[group, i] = (EDGE_NAMES[group][i], c) + attention_ref(c)
    return _edge_cache[group, i]


def edge_groups():
    """{group: [(name, Case)]}"""
    return {g: [edge_case(g, i)[:2] for i in range(len(names))] for g, names in EDGE_NAMES.items()}


def measure_edge_E(group):
    """the largest ratio of the model (b) against the reference (a) over a group"""
    worst = 0.0
    for i in range(len(EDGE_NAMES[group])):
        _name, c, ref, vmax = edge_case(group, i)
        worst = max(worst, ratio(attention_model(c), ref, vmax))
    return worst


# python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import paged_attn_ref as R; print({g: R.measure_edge_E(g) for g in R.EDGE_NAMES})"
# -> long 0.0088047 (L=1153 late_peak; the random cases 0.0018 at most), scales 0.0048156 (-4; 32x: 0.0011, 0: 2e-9), heads 0.0050353,
#    tiny_q 0.0030944 (its N(0, 1) rows; the tiny rows 1e-8)
EDGE_E = {"long": 0.00881, "scales": 0.00482, "heads": 0.00504, "tiny_q": 0.00310}   # measure_edge_E(group), rounded up
EDGE_TOL = {g: 2 * e for g, e in EDGE_E.items()}
E_long, E_scales, E_heads, E_tiny_q = (EDGE_E[g] for g in ("long", "scales", "heads", "tiny_q"))
TOL_long, TOL_scales, TOL_heads, TOL_tiny_q = (EDGE_TOL[g] for g in ("long", "scales", "heads", "tiny_q"))
