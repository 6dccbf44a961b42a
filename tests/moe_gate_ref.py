"""Reference of fp8mi_moe_gate (include/fp8mi.h), written from its definition on the CPU in two independent forms, the inputs of the
scored-form tests (SCORED_CASES: tests/test_gpu_moe_gate.py; EDGE_CASES: tests/test_gpu_moe_gate_edges.py), and the two derived tolerances.
A plain module: no fixtures, no tests.

gate_ref    vectorised numpy.  Scores in float64 from the exactly converted logits; keys and group scores rounded to float32 where the
            definition rounds; the order through canonicalised float64 keys (NaN above +inf, -0 == +0) and stable sorts.
gate_brute  a per-token Python loop on the same keys that applies the order pairwise (`_before`) and selects by repeated scans.

Tolerance 1 - weights.  A device weight is compared with `weights_at` (the float64 scores at the ids the DEVICE returned, renormalised over
those ids, scaled) within  rel |ref| + 1e-37:
  sigmoid  rel = 1e-5: the exponential's argument product errs by |x| log2(e) 2^-24 <= 7.6e-6 for |x| <= 88, plus a few ulp (2^-24 each)
           for the exponential, the add and the reciprocal.
  softmax  rel = 1e-4: the same argument terms at |x - m| <= 104, taken twice (the subtraction and the product), about 1.5e-5; plus
           (G - 1) 2^-24 <= 6.1e-5, which bounds a positive sum of up to 1024 terms added in any order; plus (k - 1) 2^-24 for the
           renormalising sum; plus a few ulp.
Both hold for the hardware exponential as well as for expf.  Every token is checked, also one skipped under tolerance 2.

Tolerance 2 - ids of the scored form.  The device's key fl32(fl32(s) + b) differs from the reference's by at most
  err_e = rel s_e + 2^-23 |key_e|          (the score's error, and one rounding each of the score and of the sum)
and a group score by the sum of its terms' bounds + 2^-23 |score|.  A token is `close` when some selected and some unselected group, or
some selected and some unselected eligible expert, lie within the sum of their bounds: only then may the device select differently.
Ids are compared as sets per token, close tokens are left out of the id comparison only, and at most SKIP_CAP of a case's tokens may be
close (the host test asserts it on the very inputs the GPU test uses).  In the plain form nothing is left out."""
import math
from types import SimpleNamespace

import numpy as np

REL = {"sigmoid": 1e-5, "softmax": 1e-4}
ABS = 1e-37
SKIP_CAP = 0.02
T_SCORED = 2048
_NAN_RANK, _INF_RANK = np.inf, 1e300   # canonical float64 keys: a NaN above +inf, +inf above every finite float32


def scores_f64(x, scoring):
    """x: (T, G) float32 values -> float64 scores (T, G)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if scoring == "softmax":
            m = np.max(np.where(np.isnan(x), np.inf, x), axis=1, keepdims=True)
            m = np.where(np.isnan(x).any(axis=1, keepdims=True), np.nan, m)
            ex = np.exp(x - m)
            return ex / ex.sum(axis=1, keepdims=True)
        assert scoring == "sigmoid", scoring
        return 1.0 / (1.0 + np.exp(-x))


def keys_f32(x, scores, bias, n_group):
    """the keys of the definition's step 3, float32 (T, G)"""
    if bias is None and n_group == 1:
        return np.asarray(x, dtype=np.float32)
    b = np.zeros(scores.shape[1]) if bias is None else np.asarray(bias, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (scores + b[None, :]).astype(np.float32)


def _canon(key):
    c = np.asarray(key, dtype=np.float32).astype(np.float64)
    c = np.where(np.isposinf(c), _INF_RANK, c)
    return np.where(np.isnan(c), _NAN_RANK, c) + 0.0   # (+ 0.0: -0 becomes +0)


def _order(c, eligible=None):
    """indices (T, n) of every row in the order: eligible first, the larger canonical key first, the smaller index first"""
    idx = np.broadcast_to(np.arange(c.shape[1]), c.shape)
    first = np.zeros(c.shape, dtype=np.int8) if eligible is None else (~eligible).astype(np.int8)
    return np.lexsort((idx, -c, first), axis=1)


def weights_at(scores, ids, renormalize, scale):
    """float64 weights of the experts `ids` (T, k): tolerance 1's reference"""
    w = np.take_along_axis(scores, np.asarray(ids, dtype=np.int64), axis=1)
    with np.errstate(all="ignore"):
        if renormalize:
            w = w / (w.sum(axis=1, keepdims=True) + 1e-20)
        return w * float(scale)


def gate_ref(x, k, scoring="softmax", renormalize=False, scale=1.0, bias=None, n_group=1, topk_group=1, group_score="max"):
    """-> ids (T, k) int64, weights (T, k) float64, scores (T, G) float64, keys (T, G) float32, eligible (T, G) bool, close (T,) bool"""
    x = np.asarray(x, dtype=np.float32)
    T, G = x.shape
    s = scores_f64(x, scoring)
    key = keys_f32(x, s, bias, n_group)
    c = _canon(key)
    rel = REL[scoring]
    key64 = key.astype(np.float64)
    with np.errstate(all="ignore"):
        err = rel * s + 2.0 ** -23 * np.abs(key64)
    eligible = np.ones((T, G), dtype=bool)
    close = np.zeros(T, dtype=bool)
    if n_group > 1:
        gs = G // n_group
        cg = c.reshape(T * n_group, gs)
        og = _order(cg)
        top = np.take_along_axis(key64.reshape(T * n_group, gs), og[:, :2], axis=1)
        top_err = np.take_along_axis(err.reshape(T * n_group, gs), og[:, :2], axis=1)
        with np.errstate(all="ignore"):
            if group_score == "top2":
                score = (top[:, 0] + top[:, 1]).astype(np.float32)
                gerr = top_err[:, 0] + top_err[:, 1]
            else:
                assert group_score == "max", group_score
                score = top[:, 0].astype(np.float32)
                gerr = top_err[:, 0]
            score = score.reshape(T, n_group)
            gerr = gerr.reshape(T, n_group) + 2.0 ** -23 * np.abs(score.astype(np.float64))
        go = _order(_canon(score))
        kept = np.zeros((T, n_group), dtype=bool)
        np.put_along_axis(kept, go[:, :topk_group], True, axis=1)
        eligible = np.repeat(kept, gs, axis=1)
        if topk_group < n_group:
            with np.errstate(all="ignore"):
                sc64 = score.astype(np.float64)
                lo = np.where(kept, sc64 - gerr, np.inf).min(axis=1)
                hi = np.where(~kept, sc64 + gerr, -np.inf).max(axis=1)
                close |= lo <= hi
    order = _order(c, eligible)
    ids = order[:, :k]
    chosen = np.zeros((T, G), dtype=bool)
    np.put_along_axis(chosen, ids, True, axis=1)
    if not (bias is None and n_group == 1):
        with np.errstate(all="ignore"):
            lo = np.where(chosen, key64 - err, np.inf).min(axis=1)
            hi = np.where(eligible & ~chosen, key64 + err, -np.inf).max(axis=1)
            close |= lo <= hi
    return SimpleNamespace(ids=ids.astype(np.int64), weights=weights_at(s, ids, renormalize, scale), scores=s, keys=key, eligible=eligible, close=close)


# ---- the brute-force form -------------------------------------------------------------------------------------------------------------------

def _before(ka, ia, kb, ib):
    """does (key ka, index ia) come before (kb, ib) in the order of the definition?"""
    na, nb = math.isnan(ka), math.isnan(kb)
    if na or nb:
        return ia < ib if na and nb else na
    if ka == kb:   # (-0.0 == +0.0 here)
        return ia < ib
    return ka > kb


def _first(items):
    best = items[0]
    for it in items[1:]:
        if _before(it[0], it[1], best[0], best[1]):
            best = it
    return best


def gate_brute(x, k, scoring="softmax", renormalize=False, scale=1.0, bias=None, n_group=1, topk_group=1, group_score="max"):
    """-> ids as a list of T lists of k experts, by pairwise comparisons (the keys themselves are gate_ref's: scores_f64 / keys_f32)"""
    x = np.asarray(x, dtype=np.float32)
    T, G = x.shape
    key = keys_f32(x, scores_f64(x, scoring), bias, n_group)
    out = []
    for t in range(T):
        items = [(float(key[t, e]), e) for e in range(G)]
        if n_group > 1:
            gs = G // n_group
            groups = []
            for g in range(n_group):
                mine = items[g * gs:(g + 1) * gs]
                a = _first(mine)
                if group_score == "top2":
                    b = _first([it for it in mine if it[1] != a[1]])
                    with np.errstate(all="ignore"):
                        sc = float(np.float32(np.float32(a[0]) + np.float32(b[0])))
                else:
                    sc = a[0]
                groups.append((sc, g))
            kept = set()
            for _ in range(topk_group):
                w = _first(groups)
                kept.add(w[1])
                groups.remove(w)
            items = [it for it in items if it[1] // gs in kept]
        ids = []
        for _ in range(k):
            w = _first(items)
            ids.append(w[1])
            items.remove(w)
        out.append(ids)
    return out


# ---- the scored-form cases: the GPU test runs them, the host test holds the reference to the skip cap on the same inputs ------------------

# name -> (G, k, scoring, bias sigma, n_group, topk_group, group_score, renormalize, scale)
SCORED_CASES = {
    "sigmoid-bias-64": (64, 6, "sigmoid", 0.1, 1, 1, "max", False, 1.0),
    "softmax-bias-60": (60, 4, "softmax", 0.01, 1, 1, "max", True, 1.0),
    "v3-256-renorm": (256, 8, "sigmoid", 0.1, 8, 4, "top2", True, 2.5),
    "v3-256-raw": (256, 8, "sigmoid", 0.1, 8, 4, "top2", False, 1.0),
    "softmax-160-max": (160, 6, "softmax", 0.002, 8, 3, "max", True, 1.0),
    "sigmoid-96-top2": (96, 5, "sigmoid", 0.1, 4, 2, "top2", False, 2.5),
    "sigmoid-1024": (1024, 8, "sigmoid", 0.1, 16, 4, "top2", True, 1.0),
}


def scored_inputs(name, seed=0):
    """-> (logits (T_SCORED, G) float32 = 2 N(0, 1), bias (G,) float32 = sigma N(0, 1)) of a scored case"""
    G, sigma = SCORED_CASES[name][0], SCORED_CASES[name][3]
    rng = np.random.default_rng([seed, sorted(SCORED_CASES).index(name)])
    return (2.0 * rng.standard_normal((T_SCORED, G))).astype(np.float32), (sigma * rng.standard_normal(G)).astype(np.float32)


def scored_kwargs(name):
    _G, k, scoring, _sigma, n_group, topk_group, group_score, renormalize, scale = SCORED_CASES[name]
    return dict(k=k, scoring=scoring, renormalize=renormalize, scale=scale, n_group=n_group, topk_group=topk_group, group_score=group_score)


# ---- the edge cases of the scored and grouped forms (tests/test_gpu_moe_gate_edges.py; the host test holds them to the skip cap too) -------

# name -> (G, k, scoring, bias sigma or None for a NULL bias, n_group, topk_group, group_score, renormalize, scale).  With E the slots per
# lane, gs = G / n_group and L the lanes of a group's team.  Both scorings meet both values of renormalize and of scale.
EDGE_CASES = {
    "e8-320-5groups": (320, 8, "sigmoid", 0.1, 5, 2, "top2", True, 2.5),              # E = 8, L = 8, 24 lanes without a group
    "e8-512-64groups": (512, 8, "sigmoid", 0.1, 64, 8, "max", False, 1.0),            # E = 8, L = 1
    "e8-384-softmax-12groups": (384, 6, "softmax", 0.001, 12, 4, "top2", True, 1.0),  # E = 8, L = 4, 16 lanes without a group
    "e4-130-gs65": (130, 4, "sigmoid", 0.1, 2, 1, "top2", False, 2.5),                # a group boundary inside a lane, E = 4
    "e2-75-gs25": (75, 5, "sigmoid", 0.1, 3, 2, "max", True, 1.0),                    # the same, E = 2, L = 16
    "e8-264-gs33": (264, 8, "sigmoid", 0.1, 8, 3, "max", False, 2.5),                 # the same, E = 8
    "e16-1000-gs125": (1000, 8, "sigmoid", 0.1, 8, 3, "top2", False, 1.0),            # the same, E = 16
    "e16-1023-33groups": (1023, 8, "sigmoid", 0.1, 33, 5, "top2", True, 2.5),         # odd G: one element per load; gs = 31, L = 1
    "e16-1023-softmax-3groups": (1023, 8, "softmax", 0.0003, 3, 1, "max", False, 2.5),   # gs = 341, L = 16
    "e2-128-gs2": (128, 8, "sigmoid", 0.1, 64, 8, "top2", True, 1.0),                 # one group per lane, gs = E
    "e1-6-gs2": (6, 2, "sigmoid", 0.1, 3, 1, "top2", False, 1.0),                     # gs < L = 16
    "e1-2-gs1": (2, 1, "softmax", 0.1, 2, 1, "max", True, 2.5),                       # gs = 1, L = 32
    "e4-192-softmax-6groups": (192, 6, "softmax", 0.002, 6, 2, "max", False, 1.0),    # E = 4 with vector loads, L = 8, 16 lanes without a group
    "bias-33-softmax": (33, 3, "softmax", 0.01, 1, 1, "max", False, 1.0),             # bias only, E = 1
    "bias-100-sigmoid": (100, 7, "sigmoid", 0.1, 1, 1, "max", False, 2.5),            # bias only, E = 2
    "bias-200-softmax": (200, 8, "softmax", 0.002, 1, 1, "max", True, 2.5),           # bias only, E = 4
    "bias-512-softmax": (512, 8, "softmax", 0.0005, 1, 1, "max", False, 1.0),         # bias only, E = 8
    "bias-257-sigmoid": (257, 8, "sigmoid", 0.1, 1, 1, "max", True, 2.5),             # bias only, the odd E = 8 boundary
    "bias-1024-k64": (1024, 64, "softmax", 0.0002, 1, 1, "max", True, 1.0),           # bias only, the 64-term renormalising sum
    "nullbias-256": (256, 8, "sigmoid", None, 8, 4, "top2", False, 2.5),              # the key fl32(s + 0) through bias == NULL
    "nullbias-160-softmax": (160, 6, "softmax", None, 8, 3, "max", True, 1.0),
    "e16-1000-k64-one-group": (1000, 64, "sigmoid", 0.1, 8, 1, "top2", True, 1.0),    # k = 64 of one group's 125 experts
}
EDGE_DTYPES = ("f32", "f16", "bf16")
EDGE_SEED = 3   # (seeds 0 and 1 give expert 25 of "e2-75-gs25", the one expert behind its in-lane boundary, a bias under which it is never selected)


def edge_dtypes(name):
    """the logit types a case runs with: without a bias bfloat16 logits repeat, equal logits give equal keys and the reference flags every
    exact tie `close` (about 6 % of the tokens), so the NULL-bias cases leave bfloat16 to the exact tests"""
    return EDGE_DTYPES[:2] if EDGE_CASES[name][3] is None else EDGE_DTYPES


def edge_inputs(name, seed=EDGE_SEED):
    """-> (logits (T_SCORED, G) float32 = 2 N(0, 1), bias (G,) float32 = sigma N(0, 1) or None) of an edge case"""
    G, sigma = EDGE_CASES[name][0], EDGE_CASES[name][3]
    rng = np.random.default_rng([seed, 1000 + sorted(EDGE_CASES).index(name)])
    x = (2.0 * rng.standard_normal((T_SCORED, G))).astype(np.float32)
    return x, None if sigma is None else (sigma * rng.standard_normal(G)).astype(np.float32)


def edge_kwargs(name):
    _G, k, scoring, _sigma, n_group, topk_group, group_score, renormalize, scale = EDGE_CASES[name]
    return dict(k=k, scoring=scoring, renormalize=renormalize, scale=scale, n_group=n_group, topk_group=topk_group, group_score=group_score)


def as_logit_dtype(x, dtype):
    """float32 values (numpy) as a torch tensor of the logit type "f32", "f16" or "bf16": the device gets this tensor, the reference its
    `.float().numpy()`, the values after the conversion"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype])
