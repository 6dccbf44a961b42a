"""The cases and the bound of the FP8 flash attention over contiguous K / V, fp8mi_attention_prefill: numpy, CPU only, on
top of tests/paged_attn_ref.py.  A plain module: no fixtures, no tests.

A flash case holds q (T, Hq, DQK), e4m3 bytes k (Tk, Hkv, 128), k_rope (Tk, Hr, 64) or None, v (Tk, Hkv, 128), cu_q, cu_k and `causal`.  Its
definition is its EXPANSION, expand(case): the decode Case of paged_attn_ref with one sequence per query token - seq_len = the token's limit -
over a cache of 128-position blocks that holds each sequence's rows in order.  attention_ref (float64) and attention_model (under WAVES = 1, as
paged_attn_prefill_ref.model) apply to it as they are, with ONE difference for DQK = 192 != DV = 128, stated here and nowhere else: the
expansion's K rows are [k | k_rope] (192 channels) and its V rows are v followed by 64 zero bytes, so both functions run at D = 192 and the
result is their [..., :128] (the zero channels give zero outputs and leave max|V| alone).

E_flash is the largest ratio of the model against the float64 reference over FLASH_CASES, measured on the CPU with the seeded generators here:
    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import flash_attn_ref as F; print(F.measure_E_flash())"
    -> 0.02774977517489215 ("q_len = k_len + 3": rows with a handful of visible positions, where e4m3's step on Q shows most), recorded below
       rounded up to four digits; TOL_flash = 2 E_flash (the convention of DESIGN.md 5.18).  tests/test_flash_attn_host.py recomputes and pins it."""
import numpy as np

import paged_attn_prefill_ref as P
import paged_attn_ref as R

COLS, DV, ROPE = 128, 128, 64   # csrc/fp8mi_attn.h: kAttnFlashCols, kAttnFlashDV, kAttnFlashRope


def tokens_per_workgroup(Hq, Hkv):
    """fp8mi_attn_flash_tokens: W"""
    return COLS // 16 * (16 // (Hq // Hkv))


def q_tiles(max_q_len, Hq, Hkv):
    W = tokens_per_workgroup(Hq, Hkv)
    return (max_q_len + W - 1) // W


def limits_of(c):
    """the limit of every query token, in row order"""
    return np.array([(int(L) - int(n) + j + 1) if c.causal else int(L) for L, n in zip(c.k_lens, c.q_lens) for j in range(int(n))], dtype=np.int64)


def make_flash_case(seed, k_lens, q_lens, Hq, Hkv, DQK=128, causal=True, Hr=1, q_dtype="f32", out_dtype="f32", per_head=False, logits=None, q_spread=None,
                    fused=False):
    """N(0, 1) q, k, v, softmax_scale = DQK^-1/2, scales such that the bytes use the e4m3 range (k_rope shares k_scale).  Hr = 1: one rotary key
    for all heads.  logits (DQK = 128 only): paged_attn_ref.make_case's rank-one shaping of K against the first query head of every KV head of a
    base row per sequence; q_spread: token rows are that base row plus q_spread N(0, 1).  fused: the GPU test lays q, k and v out as slices."""
    rng = np.random.default_rng(seed)
    k_lens, q_lens = np.array(k_lens, dtype=np.int64), np.array(q_lens, dtype=np.int64)
    T, Tk, group, scale = int(q_lens.sum()), int(k_lens.sum()), Hq // Hkv, DQK ** -0.5
    base = rng.standard_normal((len(k_lens), Hq, DQK))
    q = rng.standard_normal((T, Hq, DQK))
    if q_spread is not None:
        q = np.repeat(base, q_lens, axis=0) + q_spread * q
    k, v = rng.standard_normal((Tk, Hkv, DQK)), rng.standard_normal((Tk, Hkv, DV))
    if DQK > DV and Hr == 1:
        k[:, :, DV:] = k[:, :1, DV:]
    cu_q, cu_k = (np.concatenate([[0], np.cumsum(x)]).astype(np.int32) for x in (q_lens, k_lens))
    if logits is not None:
        assert DQK == DV
        for b, L in enumerate(k_lens):
            for h in range(Hkv):
                qh, rows = base[b, h * group], slice(cu_k[b], cu_k[b + 1])
                t = logits(np.arange(L), rng)
                k[rows, h, :] += np.outer((t / scale - k[rows, h, :] @ qh) / (qh @ qh), qh)
    axes = (0, 2) if per_head else None
    k_scale = np.atleast_1d(np.abs(k).max(axis=axes) / 448.0 if Tk else 1.0).astype(np.float32) * np.ones(Hkv if per_head else 1, np.float32)
    v_scale = np.atleast_1d(np.abs(v).max(axis=axes) / 448.0 if Tk else 1.0).astype(np.float32) * np.ones(Hkv if per_head else 1, np.float32)
    k8 = R.quantise(k, k_scale.reshape(-1, 1) if per_head else k_scale)
    v8 = R.quantise(v, v_scale.reshape(-1, 1) if per_head else v_scale)
    return R.Case(q=R.round_to(q, q_dtype).astype(np.float32), q_dtype=q_dtype, out_dtype=out_dtype, k=np.ascontiguousarray(k8[:, :, :DV]),
                  k_rope=np.ascontiguousarray(k8[:, :Hr, DV:]) if DQK > DV else None, v=v8, k_scale=k_scale, v_scale=v_scale, softmax_scale=scale, causal=causal,
                  k_lens=k_lens, q_lens=q_lens, cu_q=cu_q, cu_k=cu_k, max_q_len=int(max(q_lens.max(), 1)), max_k_len=int(max(k_lens.max(), 1)), Hkv=Hkv, Hr=Hr,
                  DQK=DQK, fused=fused)


def expand(c):
    """-> the decode Case with one sequence per query token, in row order, over 128-position blocks (see the module text for DQK = 192)"""
    T, Hq, DQK = c.q.shape
    need = [(int(L) + R.STEP - 1) // R.STEP for L in c.k_lens]
    first = np.concatenate([[0], np.cumsum(need)]).astype(np.int64)
    nb, width = max(int(first[-1]), 1), max(max(need), 1)
    k_cache, v_cache = np.zeros((nb, c.Hkv, R.STEP, DQK), np.uint8), np.zeros((nb, c.Hkv, DQK, R.STEP), np.uint8)
    table = np.full((len(c.k_lens), width), -1, np.int32)
    for b, L in enumerate(c.k_lens):
        table[b, :need[b]] = first[b] + np.arange(need[b])
        for p in range(int(L)):
            row, blk, off = c.cu_k[b] + p, first[b] + p // R.STEP, p % R.STEP
            k_cache[blk, :, off, :DV] = c.k[row]
            if c.k_rope is not None:
                k_cache[blk, :, off, DV:] = c.k_rope[row]   # Hr = 1 broadcasts over the heads
            v_cache[blk, :, :DV, off] = c.v[row]
    seq_of = np.repeat(np.arange(len(c.q_lens)), c.q_lens)
    lim = np.maximum(limits_of(c), 0)
    assert len(seq_of) == T and (lim <= c.k_lens[seq_of]).all()
    return R.Case(q=c.q, q_dtype=c.q_dtype, out_dtype=c.out_dtype, k_cache=k_cache, v_cache=v_cache, block_table=np.ascontiguousarray(table[seq_of]),
                  seq_lens=lim.astype(np.int32), k_scale=c.k_scale, v_scale=c.v_scale, softmax_scale=c.softmax_scale, num_splits=1,
                  max_seq_len=max(int(lim.max()) if T else 1, 1), block_size=R.STEP, Hkv=c.Hkv, D=DQK)


def reference(e):
    """-> (out float64 (T, Hq, 128), vmax (T, Hq)) of an expansion"""
    out, vmax = R.attention_ref(e)
    return out[..., :DV], vmax


def model(e):
    return P.model(e)[..., :DV]


GROUPS = (1, 4, 16)                        # W = 128, 32, 8
K_LENS = (1, 127, 128, 129, 257, 300)      # one to three steps, the stage ring wrapping
mk = make_flash_case


def _makers():
    m = {}
    for k, (g, i) in enumerate((g, i) for g in GROUPS for i in range(4)):
        W = COLS // 16 * (16 // g)
        n, L = (W - 1, W, W + 1, 2 * W + 1)[i], K_LENS[(5 * k + 3) % 6]
        m[f"tile edge G={g} q_len={n} k_len={L}"] = lambda g=g, n=n, L=L, k=k: mk(40000 + k, [L, 42], [n, 2], g * (1 + k % 2), 1 + k % 2, (128, 192)[k % 2],
                                                                                   causal=k % 4 < 2, Hr=(1, 1 + k % 2)[(k >> 1) % 2])
    for k, (L, causal) in enumerate((L, c) for L in K_LENS for c in (False, True)):
        m[f"steps k_len={L} causal={causal}"] = lambda L=L, causal=causal, k=k: mk(41000 + k, [L], [33], 8, 2, (192, 128)[(k >> 1) % 2], causal=causal, Hr=(2, 1)[k % 2])
    for k, DQK in enumerate((128, 192)):
        m[f"diagonal q_len=k_len=300 DQK={DQK}"] = lambda DQK=DQK, k=k: mk(42000 + k, [300], [300], 4, 1, DQK, causal=True)
    m["q_len = k_len + 3"] = lambda: mk(42100, [5, 20], [8, 2], 8, 2, 192, causal=True, Hr=2)
    for causal in (False, True):
        m[f"q_len = 0 and k_len = 0 in a batch causal={causal}"] = lambda causal=causal: mk(42200, [50, 30, 0, 0, 19], [3, 0, 2, 0, 1], 8, 2, 128, causal=causal)
    for qd, od in (("f16", "f16"), ("bf16", "bf16"), ("f32", "bf16")):
        m[f"dtypes {qd}->{od}"] = lambda qd=qd, od=od: mk(43000, [45, 131], [5, 9], 4, 2, 192, causal=True, q_dtype=qd, out_dtype=od)
    m["per-head scales"] = lambda: mk(43100, [90, 33], [6, 3], 8, 4, 128, causal=False, per_head=True)
    m["fused buffer"] = lambda: mk(43200, [150, 33], [40, 3], 8, 2, 192, causal=True, Hr=2, q_dtype="bf16", out_dtype="bf16", fused=True)
    m["long rising"] = lambda: mk(44000, [1300], [8], 4, 1, 128, causal=True, logits=R.PROFILES["rising"](1300, 1), q_spread=0.25)
    return m


_MAKERS, _cache = _makers(), {}
FLASH_CASES = list(_MAKERS)


def flash_case(name):
    """-> (case, expand(case), ref (a) of the expansion, vmax): made once, shared, never written"""
    if name not in _cache:
        c = _MAKERS[name]()
        e = expand(c)
        _cache[name] = (c, e) + reference(e)
    return _cache[name]


def measure_E_flash():
    return max(R.ratio(model(e), ref, vmax) for _c, e, ref, vmax in map(flash_case, FLASH_CASES))


E_flash = 0.02775          # measure_E_flash(), rounded up
TOL_flash = 2 * E_flash     # 0.05550
