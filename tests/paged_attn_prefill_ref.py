"""The cases and the bound of the LDS-tiled paged attention for prompt chunks, fp8mi_paged_attention_prefill: numpy, CPU
only, on top of tests/paged_attn_ref.py and tests/paged_attn_varlen_ref.py.  A plain module: no fixtures, no tests.

The contract is fp8mi_paged_attention_varlen's: the reference is attention_ref on expand(case).  ONE wave walks all the steps of a row's
split in order, so the model is paged_attn_ref.attention_model under WAVES = 1; E_prefill is its largest ratio against attention_ref:
    python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import paged_attn_prefill_ref as P; print(P.measure_E_prefill())"
    -> 0.027387500997112443 (prefill q_len = seq_len = 130: rows with a handful of visible positions, where e4m3's step on Q shows most),
       recorded below rounded up to four digits; TOL_prefill = 2 E_prefill (the convention of DESIGN.md 5.18).
tests/test_paged_attn_prefill_host.py recomputes and pins it."""
import paged_attn_ref as R
import paged_attn_varlen_ref as V

COLS = 128   # csrc/fp8mi_attn.h: kAttnPrefillCols, the MFMA columns of a workgroup


def model(e):
    """attention_model with one owner per split"""
    waves, R.WAVES = R.WAVES, 1
    try:
        return R.attention_model(e)
    finally:
        R.WAVES = waves


GROUPS = (1, 4, 5, 16)                                   # W = 128, 32, 24, 8
STEPS = (128, 129, 257, 300, 520)                        # seq_len at q_len = 33, G = 4: one, two, three and five steps, the stage ring wrapping twice
EMPTY_CACHE = (1, 17, 130, 300)                          # q_len = seq_len
SPLITS = ((2, 530, 40), (3, 400, 33), (8, 300, 50))      # (num_splits, seq_len, q_len) at max_seq_len = 1024: chunks 512, 384, 128, limits on both sides of an end
LONG = [(prof, n) for prof in ("rising", "late_peak") for n in (1, 2)]
mk = V.make_varlen_case


def _makers():
    m = {}
    for k, (g, i) in enumerate((g, i) for g in GROUPS for i in range(4)):
        W = COLS // 16 * (16 // g)
        n = (W - 1, W, W + 1, 2 * W + 1)[i]
        m[f"tile edge G={g} q_len={n}"] = lambda g=g, n=n, k=k: mk(30000 + k, [n + 40, 42], [n, 2], (16, 32, 128)[k % 3], (64, 128)[k % 2], g * (1 + k % 2), 1 + k % 2)
    for k, L in enumerate(STEPS):
        m[f"steps L={L}"] = lambda L=L, k=k: mk(31000 + k, [L], [33], (16, 32, 128)[k % 3], (128, 64)[k % 2], 8, 2)
    m["wave skips"] = lambda: mk(31100, [260], [32], 16, 128, 8, 2)   # limits 229 .. 260: the tiles of waves 0 .. 2 own nothing of the last step
    for k, L in enumerate(EMPTY_CACHE):
        m[f"prefill q_len=seq_len={L}"] = lambda L=L, k=k: mk(32000 + k, [L], [L], (16, 32, 128)[k % 3], (128, 64)[k % 2], 4, 2)
    m["q_len = seq_len + 3"] = lambda: mk(32100, [5, 20], [8, 2], 16, 64, 8, 2)
    m["q_len = 0 and seq_len = 0 in a batch"] = lambda: mk(32200, [50, 30, 0, 0, 19], [3, 0, 2, 0, 1], 16, 128, 8, 2)
    m["mixed batch"] = lambda: mk(33000, list(V.MIXED_SEQ), list(V.MIXED_Q), 16, 128, 8, 2)
    for k, (ns, L, n) in enumerate(SPLITS):
        m[f"splits={ns} L={L} q_len={n}"] = lambda ns=ns, L=L, n=n, k=k: mk(34000 + k, [L], [n], 16, (128, 64)[k % 2], 8, 2, num_splits=ns, max_seq_len=1024)
    for prof, ns in LONG:
        m[f"long {prof} splits={ns}"] = lambda prof=prof, ns=ns: mk(35000 + ns, [1300], [8], 16, 128, 4, 1, num_splits=ns,
                                                                    logits=R.PROFILES[prof](1300, ns), q_spread=0.25)
    for qd, od in V.DTYPES:
        m[f"dtypes {qd}->{od}"] = lambda qd=qd, od=od: mk(36000, [45, 131], [5, 9], 16, 64, 4, 2, q_dtype=qd, out_dtype=od)
    m["per-head scales"] = lambda: mk(36100, [90, 33], [6, 3], 64, 128, 8, 4, per_head=True)
    return m


_MAKERS, _cache = _makers(), {}
PREFILL_CASES = list(_MAKERS)


def prefill_case(name):
    """-> (Case, expand(Case), ref (a) of the expansion, vmax): made once, shared, never written"""
    if name not in _cache:
        c = _MAKERS[name]()
        e = V.expand(c)
        _cache[name] = (c, e) + R.attention_ref(e)
    return _cache[name]


def measure_E_prefill():
    return max(R.ratio(model(e), ref, vmax) for _c, e, ref, vmax in map(prefill_case, PREFILL_CASES))


E_prefill = 0.02739          # measure_E_prefill(), rounded up
TOL_prefill = 2 * E_prefill   # 0.05478
