"""The scored and grouped forms of fp8mi_moe_gate on every kernel instance, against tests/moe_gate_ref.py (tests/test_gpu_moe_gate.py covers
the plain form on all of them and the scored forms at float32, E = 1, 2, 4, 16, power-of-two n_group and gs a multiple of E only).  With
E the slots per lane, gs = G / n_group the group size, L the lanes of one group's team (64 / n_group rounded down to a power of two):

1. EDGE_CASES x {f32, f16, bf16} logits x two row layouts.  Tolerances 1 and 2 of moe_gate_ref.py on the contiguous layout (ids as sets
   outside the `close` tokens, at most 2 % of a case - tests/test_moe_gate_host.py asserts that on the same inputs; weights for every
   token); the same values at ld = G + 3 from a base one element off must give the same id and weight bits.  A NULL bias runs with f32
   and f16 only (bfloat16 logits repeat, and without a bias equal logits are exact ties, which the reference flags `close`).
2. Special values: logits from {NaN, +inf, -inf, +0, -0} under the sigmoid (scores NaN, 1, 0, 1/2), softmax rows of 2^n zeros among -inf
   (scores 2^-n and 0), biases from {0, +-2, 4, +inf, -inf, NaN}, zero and NULL.  Every key is then the same float on any device and
   distinct keys are 0.5 apart, so ids are compared IN ORDER and nothing is skipped: NaN and inf - inf group scores, ties of groups and of
   experts, the score handed out from its owner lane.  Weights only have to be written (include/fp8mi.h leaves their values open there).
3. T on the four-tokens-per-workgroup edges in the grouped form (the waves past T run up to the barrier): prefixes of one case equal the
   full run's rows bit for bit and pass the reference check.

Which case reaches which instance <logit type, E, VEC (vector loads) or ELT (one element per load), scored or grouped>.  The second layout
is ELT everywhere except float32 at E = 1, whose 4-byte load IS one element (16-bit logits at E = 1 are always ELT).  Contiguous layout:
   e1-2-gs1, e1-6-gs2              E = 1   grouped  f32 VEC, f16 / bf16 ELT     gs = 1 with L = 32; gs = 2 < L = 16
   bias-33-softmax                 E = 1   scored   f32 VEC, f16 / bf16 ELT
   e2-75-gs25                      E = 2   grouped  ELT (odd G)                  n_group = 3, L = 16; a group boundary inside a lane
   e2-128-gs2                      E = 2   grouped  VEC                          L = 1: a lane's two keys are its group
   bias-100-sigmoid                E = 2   scored   VEC
   e4-130-gs65                     E = 4   grouped  ELT (G % 4 != 0)             boundary inside a lane
   e4-192-softmax-6groups          E = 4   grouped  VEC                          n_group = 6, L = 8, 16 lanes without a group
   nullbias-256, -160-softmax      E = 4   grouped  VEC (f32, f16)               bias == NULL: the key fl32(s + 0)
   bias-200-softmax                E = 4   scored   VEC
   e8-320-5groups                  E = 8   grouped  VEC                          n_group = 5, L = 8, 24 lanes without a group
   e8-512-64groups                 E = 8   grouped  VEC                          L = 1
   e8-384-softmax-12groups         E = 8   grouped  VEC                          n_group = 12, L = 4, 16 lanes without a group
   e8-264-gs33                     E = 8   grouped  VEC                          boundary inside a lane
   bias-512-softmax, bias-257-sigmoid   E = 8   scored   VEC, ELT (odd G)
   e16-1000-gs125, -k64-one-group  E = 16  grouped  VEC                          boundary inside a lane; k = 64 of one group's 125
   e16-1023-33groups               E = 16  grouped  ELT (odd G)                  n_group = 33, gs = 31, L = 1, 31 lanes without a group
   e16-1023-softmax-3groups        E = 16  grouped  ELT (odd G)                  n_group = 3, gs = 341, L = 16
   bias-1024-k64                   E = 16  scored   VEC                          the 64-term renormalising sum
Every test launches the kernel on valid arguments only (the argument errors are tests/test_moe_gate_host.py's)."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from moe_gate_gpu_util import check_weights, compare_scored, run_gate
from moe_gate_ref import EDGE_CASES, EDGE_SEED, as_logit_dtype, edge_dtypes, edge_inputs, edge_kwargs, gate_ref
from moe_route_gpu_util import DEV, bits

pytestmark = pytest.mark.gpu

ONE_GROUP = "e16-1000-k64-one-group"
EDGE_T = (1, 2, 3, 4, 5, 7, 257)   # four tokens per workgroup: one to three idle waves, none, and past one workgroup


@pytest.fixture(scope="module")
def lib():
    return L.load()


def off_by_one_rows(xd):
    """the same values with the row stride G + 3, from a base one element past an aligned one: no vector load is possible"""
    T, G = xd.shape
    buf = torch.zeros((T * (G + 3) + 9,), dtype=xd.dtype, device=DEV)
    view = buf[1:1 + T * (G + 3)].view(T, G + 3)[:, :G]
    view.copy_(xd)
    assert view.data_ptr() == buf.data_ptr() + buf.element_size() and view.stride(0) == G + 3
    return view


def run_edge_case(lib, name, dtype):
    """Part 1's check of one (case, logit type) -> (device ids, device weights, the reference, the logits and the bias on the device, the
    gate's arguments)"""
    x, bias = edge_inputs(name, EDGE_SEED)
    kw = edge_kwargs(name)
    xt = as_logit_dtype(x, dtype)
    r = gate_ref(xt.float().numpy(), bias=bias, **kw)
    xd = xt.to(DEV)
    bd = None if bias is None else torch.from_numpy(bias).to(DEV)
    ids, w = run_gate(lib, xd, bias=bd, **kw)
    compare_scored(ids, w, r, kw, f"{name} {dtype}")
    ids2, w2 = run_gate(lib, off_by_one_rows(xd), bias=bd, **kw)
    assert torch.equal(ids2, ids) and torch.equal(bits(w2), bits(w)), (name, dtype, "one element per load")
    return ids, w, r, xd, bd, kw


# ---- 1. the instance matrix ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", [(n, d) for n in sorted(EDGE_CASES) if n != ONE_GROUP for d in edge_dtypes(n)])
def test_edge_cases(lib, name, dtype):
    run_edge_case(lib, name, dtype)


@pytest.mark.parametrize("dtype", edge_dtypes(ONE_GROUP))
def test_k_64_of_the_one_kept_group_at_sixteen_slots(lib, dtype):
    """G = 1000 in 8 groups of 125, one kept, k = 64: every token's ids lie in ONE group, for every token, and that group is the
    reference's outside the `close` tokens."""
    ids, _w, r, _xd, _bd, _kw = run_edge_case(lib, ONE_GROUP, dtype)
    groups = ids.numpy() // 125
    assert bool((groups == groups[:, :1]).all())
    keep = ~r.close
    assert bool((groups[:, 0] == r.ids[:, 0] // 125)[keep].all())
    assert bool(np.take_along_axis(r.eligible, ids.numpy().astype(np.int64), axis=1)[keep].all())


# ---- 2. special values and exact ties ------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
# G, n_group, topk_group, group_score, k
SPECIAL_SHAPES = ((96, 4, 2, "top2", 9), (130, 2, 1, "top2", 6), (75, 3, 2, "max", 7), (320, 5, 2, "top2", 12),
                  (128, 64, 8, "top2", 16),   # every TOP2 sum is two keys of one lane; k = every eligible expert
                  (64, 1, 1, "max", 8))


def special_logits(G, rng):
    """236 rows drawn from {NaN, +inf, -inf, +0, -0} with their own (skewed) frequencies, 16 rows of one value with one to three others put
    in (a single NaN group next to groups of numbers, a single winner), and the four constant rows, on which a pad slot or an excluded
    expert must never win"""
    vals = np.array([NAN, INF, -INF, 0.0, -0.0], dtype=np.float32)
    p = rng.random((236, 5)) ** 6
    edges = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)
    pick = np.minimum((rng.random((236, G))[:, :, None] > edges[:, None, :]).sum(axis=2), 4)
    sparse = np.repeat(np.array([0.0, -INF, -0.0, INF], dtype=np.float32), 4)[:, None] * np.ones((1, G), dtype=np.float32)
    for n, row in enumerate(sparse):
        at = rng.permutation(G)[:1 + n % 3]
        row[at] = vals[rng.integers(0, 5, size=len(at))] if n % 2 else NAN
    fixed = np.stack([np.full(G, v, dtype=np.float32) for v in (NAN, -INF, INF, 0.0)])
    return np.concatenate([vals[pick], sparse, fixed])


def softmax_rows(G, rng):
    """2^n logits of +-0 among -inf: the scores are exactly 2^-n and 0"""
    rows = np.full((3, G), -INF, dtype=np.float32)
    n_max = 1
    while 4 * n_max <= G:
        n_max *= 2
    for row, n in zip(rows, (2, 4, n_max)):
        at = rng.permutation(G)[:n]
        row[at] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    return rows


def special_bias(G, gs, rng):
    """from {0, +-2, 4} with a NaN, a +inf, a -inf and G / 32 more of them: distinct finite keys are at least 0.5 apart.  With groups, the
    last one holds one +inf and -inf otherwise: its two largest keys are +inf and -inf wherever its logits hold no NaN"""
    b = rng.choice(np.array([0.0, 2.0, -2.0, 4.0], dtype=np.float32), size=G)
    at = rng.permutation(G)[:min(G, 3 + G // 32)]
    b[at] = np.concatenate([[NAN, INF, -INF], rng.choice([NAN, INF, -INF], size=len(at))])[:len(at)].astype(np.float32)
    if 1 < gs < G:
        b[G - gs:] = -INF
        b[G - gs + int(rng.integers(0, gs))] = INF
    return b


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("G,n_group,topk_group,group_score,k", SPECIAL_SHAPES)
def test_special_values_select_as_the_reference_in_order(lib, G, n_group, topk_group, group_score, k, dtype):
    rng = np.random.default_rng([7, G])
    biases = {"special": special_bias(G, G // n_group, rng), "zero": np.zeros(G, dtype=np.float32)}
    if n_group > 1:
        biases["NULL"] = None
    for scoring, x in (("sigmoid", special_logits(G, rng)), ("softmax", softmax_rows(G, rng))):
        xt = as_logit_dtype(x, dtype)
        back = xt.float().numpy()   # every value is exact in bfloat16 too (a NaN stays one, whatever its bits)
        assert np.array_equal(back, x, equal_nan=True) and np.array_equal(np.signbit(back) | np.isnan(back), np.signbit(x) | np.isnan(x))
        xd = xt.to(DEV)
        for n, (which, bias) in enumerate(biases.items()):
            kw = dict(k=k, scoring=scoring, renormalize=n % 2 == 0, scale=(1.0, 2.5)[n % 2], n_group=n_group, topk_group=topk_group, group_score=group_score)
            r = gate_ref(x, bias=bias, **kw)
            ids, _w = run_gate(lib, xd, bias=None if bias is None else torch.from_numpy(bias).to(DEV), **kw)
            want = torch.from_numpy(r.ids).to(torch.int32)
            bad = (ids != want).any(dim=1).nonzero().flatten()
            assert bad.numel() == 0, (G, dtype, scoring, which, bad[:8].tolist(), ids[bad[:1]].tolist(), want[bad[:1]].tolist())


# ---- 3. the tokens-per-workgroup edges in the grouped form --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", edge_dtypes("e8-320-5groups"))
def test_grouped_prefixes_equal_the_full_run_and_the_reference(lib, dtype):
    ids, w, r, xd, bd, kw = run_edge_case(lib, "e8-320-5groups", dtype)
    want = np.sort(r.ids, axis=1)
    for t in EDGE_T:
        ids_t, w_t = run_gate(lib, xd[:t], bias=bd, **kw)
        assert torch.equal(ids_t, ids[:t]) and torch.equal(bits(w_t), bits(w[:t])), (dtype, t)
        differ = (np.sort(ids_t.numpy().astype(np.int64), axis=1) != want[:t]).any(axis=1)
        assert not bool((differ & ~r.close[:t]).any()), (dtype, t)
        check_weights(w_t, r.scores[:t], ids_t, kw["scoring"], kw["renormalize"], kw["scale"], (dtype, t))
