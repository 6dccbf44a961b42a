"""The reference of the FP8 MLA latent cache and its weight-absorbed decode attention (fp8mi_mla_cache_append, fp8mi_mla_attention_decode):
numpy, CPU only.  A plain module: no fixtures, no tests.  quantise, round_to, ratio and the e4m3 table are tests/paged_attn_ref.py's.

  (a) attention_ref    float64 attention over the decoded cache bytes (576 per position: latent then rope) times kv_scale, Q exact; the
                       output is softmax . latent.  rope=False drops the 64 rope channels from the scores: what a kernel that ignores its
                       fifth K-step would compute.
  (b) attention_model  the kernel's roundings restated, float64 otherwise: [q_lat | q_pe] rounded to e4m3 per (sequence, head) row with
                       one amax over the 576 channels; P = rne(p 2^8) relative to the running maximum of the ONE walk over a split's
                       128-position steps; the row sum from the unrounded p; the splits merged; the output rounded to out_dtype.
  (c) TOL_mla          every comparison is |out - ref(a)| <= TOL_mla * max|dequantised latent of that sequence|, no element left out.  E_mla
                       is the largest such ratio of (b) against (a) over all_cases() - every case tests/test_gpu_mla.py compares - and
                       TOL_mla = 2 E_mla, the project's convention (tests/paged_attn_ref.py says what the factor covers).

E_mla was measured on the CPU with the seeded generator below:
    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import mla_ref as R; print(R.measure_E())"
    -> 0.03722713125747339, recorded below rounded up; tests/test_mla_host.py recomputes it and pins the constant.
"""
import math

import numpy as np

import fp8_oracle
from paged_attn_ref import LUT64, P_SCALE, STEP, TINY_Q, TINY_Q_UP, chunk_of, quantise, ratio, round_to  # noqa: F401

LATENT, ROPE, ROW = 512, 64, 576
HEAD_TILE, MIN_STEPS, AUTO_SPLITS_MAX = 64, 4, 64   # csrc/fp8mi_attn.h: kMlaHeadTile, kAttnPrefillMinSteps, kAttnAutoSplits
SOFTMAX_SCALE = 192 ** -0.5                          # the un-absorbed head dimension of DeepSeek-V3: 128 nope + 64 rope


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def rising(pos, rng):
    """every 128-position step 3 nats above the one before: every step meets a new maximum and alpha acts; the peak is in the last step"""
    return rng.uniform(-1.0, 1.0, len(pos)) + 3.0 * (pos // STEP)


def make_case(seed, seq_lens, block_size, Hq, num_splits=1, q_dtype="f32", out_dtype="f32", logits=None, rope_gain=1.0, max_seq_len=None, spare_blocks=2, table_blocks=0):
    """N(0, 1) latents and queries, the rope parts times rope_gain; kv_scale such that the cache uses the e4m3 range; a shuffled block table
    over physical blocks no two sequences share, entries past the needed ones -1 (table_blocks: at least that many entries a row, so that the
    table can name max_seq_len positions).  logits: a function (positions, rng) -> the scaled logit
    of every position against head 0, set exactly before the cache's rounding by a rank-one correction of the rows."""
    rng = np.random.default_rng(seed)
    B = len(seq_lens)
    need = [(L + block_size - 1) // block_size for L in seq_lens]
    num_blocks, max_blocks = sum(need) + spare_blocks, max(max(need) + 2, table_blocks)
    perm = rng.permutation(num_blocks)
    table = np.full((B, max_blocks), -1, dtype=np.int32)
    at = 0
    for b in range(B):
        table[b, :need[b]] = perm[at:at + need[b]]
        at += need[b]
    gain = np.concatenate([np.ones(LATENT), np.full(ROPE, rope_gain)])
    q = round_to(rng.standard_normal((B, Hq, ROW)) * gain, q_dtype).astype(np.float32)
    rows = []
    for b in range(B):
        k = rng.standard_normal((seq_lens[b], ROW)) * gain
        if logits is not None:
            q0 = q[b, 0].astype(np.float64)
            k += np.outer((logits(np.arange(seq_lens[b]), rng) / SOFTMAX_SCALE - k @ q0) / (q0 @ q0), q0)
        rows.append(k)
    allk = np.concatenate(rows) if sum(seq_lens) else np.ones((1, ROW))
    kv_scale = np.array([np.abs(allk).max() / 448.0], dtype=np.float32)
    cache = np.zeros((num_blocks, block_size, ROW), dtype=np.uint8)
    slots = []
    for b in range(B):
        pos = np.arange(seq_lens[b])
        s = table[b, pos // block_size].astype(np.int64) * block_size + pos % block_size
        cache.reshape(-1, ROW)[s] = quantise(rows[b], kv_scale)
        slots.append(s)
    return Case(q=q, q_dtype=q_dtype, out_dtype=out_dtype, cache=cache, block_table=table, seq_lens=np.array(seq_lens, dtype=np.int32), kv_scale=kv_scale,
                num_splits=num_splits, max_seq_len=max(max(seq_lens), 1) if max_seq_len is None else max_seq_len, block_size=block_size, rows=rows, slots=slots)


def gather(case, b):
    """-> the cache bytes (L, 576) of sequence b through the block table"""
    pos = np.arange(int(case.seq_lens[b]))
    return case.cache[case.block_table[b, pos // case.block_size].astype(np.int64), pos % case.block_size]


def attention_ref(case, rope=True):
    """-> (out float64 (B, Hq, 512), vmax float64 (B, Hq): max|dequantised latent| of the row's sequence, 0 for an empty one)"""
    B, Hq, _ = case.q.shape
    out, vmax = np.zeros((B, Hq, LATENT)), np.zeros((B, Hq))
    for b in range(B):
        if case.seq_lens[b] == 0:
            continue
        K = LUT64[gather(case, b)] * float(case.kv_scale[0])
        n = ROW if rope else LATENT
        s = (K[:, :n] @ case.q[b, :, :n].astype(np.float64).T) * SOFTMAX_SCALE   # (L, Hq)
        p = np.exp(s - s.max(axis=0))
        out[b] = (p / p.sum(axis=0)).T @ K[:, :LATENT]
        vmax[b] = np.abs(K[:, :LATENT]).max()
    return out, vmax


def attention_model(case):
    """-> out float64 (B, Hq, 512), rounded to case.out_dtype"""
    B, Hq, _ = case.q.shape
    splits = max(case.num_splits, 1)
    chunk = chunk_of(case.max_seq_len, splits)
    out = np.zeros((B, Hq, LATENT))
    for b in range(B):
        L = int(case.seq_lens[b])
        if L == 0:
            continue
        K8 = LUT64[gather(case, b)]
        q = case.q[b].astype(np.float32)
        amax = np.abs(q).max(axis=1).astype(np.float32)
        tiny = (amax > 0) & (amax < TINY_Q)
        up = np.where(tiny, np.float32(TINY_Q_UP), np.float32(1.0))
        q, amax = q * up[:, None], amax * up
        safe = np.where(amax > 0, amax, np.float32(1.0))
        q_scale = np.where(amax > 0, safe / np.float32(448.0), np.float32(1.0))
        q_inv = np.where(amax > 0, np.float32(448.0) / safe, np.float32(1.0))
        q8 = LUT64[fp8_oracle.encode_torch_rne((q * q_inv[:, None]).astype(np.float32))]
        logit2 = (K8 @ q8.T) * (q_scale.astype(np.float64) / up * float(case.kv_scale[0]) * SOFTMAX_SCALE * math.log2(math.e))   # (L, Hq)
        M, Lsum, O = np.full(Hq, -np.inf), np.zeros(Hq), np.zeros((Hq, LATENT))
        for s in range(splits):
            lo = s * chunk
            hi = L if (s == splits - 1 or lo + chunk > L) else lo + chunk
            m, l, o = np.full(Hq, -np.inf), np.zeros(Hq), np.zeros((Hq, LATENT))
            for p0 in range(lo, hi, STEP):
                x = logit2[p0:min(p0 + STEP, hi)]
                m_new = np.maximum(m, x.max(axis=0))
                alpha = 2.0 ** (m - m_new)
                p = 2.0 ** (x - m_new)
                p8 = LUT64[fp8_oracle.encode_torch_rne((p * P_SCALE).astype(np.float32))]
                l = l * alpha + p.sum(axis=0)
                o = o * alpha[:, None] + p8.T @ K8[p0:p0 + len(x), :LATENT]
                m = m_new
            if hi > lo:   # the combine: a split that owns nothing weighs 0
                M_new = np.maximum(M, m)
                wa, wb = 2.0 ** (M - M_new), 2.0 ** (m - M_new)
                Lsum, O, M = Lsum * wa + l * wb, O * wa[:, None] + o * wb[:, None], M_new
        out[b] = O / (P_SCALE * Lsum[:, None]) * float(case.kv_scale[0])
    return round_to(out, case.out_dtype)


# ---- the cases of tests/test_gpu_mla.py ---------------------------------------------------------------------------------------------------

GRID_LENS = (0, 1, 15, 16, 17, 127, 128, 129, 257, 300, 520)   # both sides of a block, an S tile and a step; five steps: the stage ring wraps twice
GRID = [(L, (16, 64, 128)[i % 3], (16, 128, 5, 64, 80)[i % 5]) for i, L in enumerate(GRID_LENS)]
HEADS = (1, 5, 16, 17, 64, 65, 128)                            # dead columns, a dead wave, a second head tile
SPLITS = ((2, 530), (3, 400), (8, 300))                        # (num_splits, seq_len) at max_seq_len 1024; (8, 300): splits that own nothing
SPLIT_MAX_SEQ = 1024
RESCALE_LEN, RESCALE_SPLITS = 1300, (1, 2)
MIXED_LENS = (0, 1, 300, 37)
DTYPES = ("f32", "f16", "bf16")
GRAPH_MAX_BLOCKS, GRAPH_MAX_SEQ = 12, 192


def grid_case(L, bs, Hq):
    return make_case(100 + L, [L], bs, Hq)


def heads_case(Hq):
    return make_case(200 + Hq, [130], 32, Hq)


def split_case(n, L):
    return make_case(300 + n, [L], 32, 8, num_splits=n, max_seq_len=SPLIT_MAX_SEQ, table_blocks=SPLIT_MAX_SEQ // 32)


def rescale_case(n):
    return make_case(400, [RESCALE_LEN], 64, 4, num_splits=n, logits=rising)


def rope_case():
    """q_pe and k_pe eight times the latent's spread: the 64 rope channels decide the softmax.  q on the e4m3 grid (every row's amax 448 / 16),
    so the kernel's row quantisation is exact: with N(0, 1) q its steps are nats of noise on logits this large and the model itself is 0.2
    max|latent| from (a) (measured), which would be everybody's tolerance."""
    c = make_case(500, [200], 16, 8, rope_gain=8.0)
    amax = np.abs(c.q).max(axis=-1, keepdims=True)
    c.q = (LUT64[fp8_oracle.encode_torch_rne((c.q * (np.float32(448.0) / amax)).astype(np.float32))] / 16.0).astype(np.float32)
    return c


def mixed_case():
    return make_case(600, list(MIXED_LENS), 16, 20)


def dtype_case(qd, od):
    return make_case(700, [45, 131], 16, 8, q_dtype=qd, out_dtype=od)


def graph_cases():
    """two cases of one geometry (16 physical blocks): a graph captured on the first replays on the second"""
    cases = (make_case(800, [33, 140], 16, 20, spare_blocks=4), make_case(801, [150, 9], 16, 20, spare_blocks=5))
    for c in cases:
        assert c.cache.shape[0] == 16 and c.block_table.shape[1] <= GRAPH_MAX_BLOCKS
        c.max_seq_len = GRAPH_MAX_SEQ
    return cases


_MAKERS = ([(f"grid L={L} bs={bs} Hq={Hq}", lambda s=(L, bs, Hq): grid_case(*s)) for L, bs, Hq in GRID]
           + [(f"heads Hq={h}", lambda h=h: heads_case(h)) for h in HEADS]
           + [(f"splits={n} L={L}", lambda s=(n, L): split_case(*s)) for n, L in SPLITS]
           + [(f"rescale splits={n}", lambda n=n: rescale_case(n)) for n in RESCALE_SPLITS]
           + [("rope-dominant", rope_case), ("mixed", mixed_case)]
           + [(f"dtypes {qd}->{od}", lambda s=(qd, od): dtype_case(*s)) for qd in DTYPES for od in DTYPES]
           + [(f"graph {i}", lambda i=i: graph_cases()[i]) for i in (0, 1)])
NAMES = [n for n, _ in _MAKERS]
_cache = {}


def case(name):
    """-> (Case, ref (a), vmax) of a named case: made once, shared, never written"""
    if name not in _cache:
        c = dict(_MAKERS)[name]()
        _cache[name] = (c,) + attention_ref(c)
    return _cache[name]


def measure_E():
    """the largest ratio of the model (b) against the reference (a) over every case"""
    return max(ratio(attention_model(case(n)[0]), *case(n)[1:]) for n in NAMES)


E_mla = 0.03723   # measure_E() = 0.037227131 (grid L=16 Hq=64: sixteen keys, one e4m3 step of Q among few terms), rounded up
TOL_mla = 2 * E_mla


def auto_splits(B, Hq, max_seq_len, ws_bytes, cus):
    """fp8mi_attn_auto_splits_mla: two workgroups per compute unit from B ceil(Hq / 64), no split shorter than four steps, no more than
    the workspace (B Hq splits (512 + 2) floats) holds"""
    steps, wgs = (max_seq_len + STEP - 1) // STEP, B * ((Hq + HEAD_TILE - 1) // HEAD_TILE)
    if wgs <= 0 or steps <= MIN_STEPS:
        return 1
    s = min((2 * cus + wgs - 1) // wgs, (steps + MIN_STEPS - 1) // MIN_STEPS, AUTO_SPLITS_MAX)
    while s > 1 and B * Hq * s * (LATENT + 2) * 4 > ws_bytes:
        s -= 1
    return max(s, 1)
