"""fp8mi_moe_gate / fp8_moe_gate / fp8_moe_layer on the GPU against tests/moe_gate_ref.py, at the smallest shapes at which the kernel can go
wrong (none is a workload size).

Plain form (no bias, no groups): ids bit-equal with the reference, order included; nothing is skipped.  Scored form: ids as sets, the
tokens the reference flags `close` left out of the id comparison only (tolerance 2 of moe_gate_ref.py, at most 2 % of a case).  Weights,
always and for every token: within rel |ref| + 1e-37 of the float64 scores at the ids the device returned (tolerance 1).  Every run has
its ids and weights between guard elements prefilled with a sentinel, and every token's ids are k distinct values in [0, G)."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from moe_gate_gpu_util import check_scored, check_weights, run_gate
from moe_gate_ref import SCORED_CASES, gate_ref, scored_inputs, scored_kwargs, scores_f64
from moe_route_gpu_util import DEV, SINGLE, TILE, bits

pytestmark = pytest.mark.gpu

PLAIN_G = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024)   # every slots-per-lane instance, both sides of each boundary
PLAIN_K = (1, 2, 8, 63, 64)                                               # and k = G
PLAIN_T = (1, 3, 4, 5, 257)                                               # four tokens per workgroup
# scoring, renormalize, scale: both scorings with and without renormalisation at both scales; every (G, dtype) case walks through all eight
CONFIGS = (("softmax", True, 1.0), ("sigmoid", False, 2.5), ("softmax", False, 2.5), ("sigmoid", True, 1.0),
           ("softmax", True, 2.5), ("sigmoid", False, 1.0), ("softmax", False, 1.0), ("sigmoid", True, 2.5))


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


@pytest.fixture(scope="module")
def lib():
    return L.load()


def random_logits(gen, T, G, dtype):
    return (2.0 * torch.randn((T, G), generator=gen)).to(dtype)


# ---- plain form ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("G", PLAIN_G)
def test_plain_ids_equal_the_reference_in_order(lib, G, dtype):
    """Every k and T of the lists; the row layouts ld = G, G + 3, G + 16 and a base one element off (the one-element-per-load form) against the
    aligned form of the same values.  16-bit logits hold many equal values at the larger G: the tie rule is part of every comparison."""
    gen = torch.Generator().manual_seed(1000 + G)
    T = max(PLAIN_T)
    x = random_logits(gen, T, G, dtype)
    xd = x.to(DEV)
    ks = sorted({k for k in PLAIN_K + (G,) if k <= min(G, L.MOE_GATE_MAX_K)})
    ref = gate_ref(x.float().numpy(), max(ks))            # the order once: the ids of a smaller k are its prefix
    scores = {s: scores_f64(x.float().numpy(), s) for s in ("softmax", "sigmoid")}
    want = torch.from_numpy(ref.ids).to(torch.int32)
    for n, k in enumerate(ks):
        scoring, renorm, scale = CONFIGS[n % len(CONFIGS)]
        ids, w = run_gate(lib, xd, k, scoring, renorm, scale)
        assert torch.equal(ids, want[:, :k]), (G, dtype, k)
        check_weights(w, scores[scoring], ids, scoring, renorm, scale, (G, dtype, k, scoring))
    # the tokens-per-workgroup edges, every configuration
    k = min(G, 8)
    for n, t in enumerate(PLAIN_T):
        scoring, renorm, scale = CONFIGS[(n + 4) % len(CONFIGS)]
        ids, w = run_gate(lib, xd[:t], k, scoring, renorm, scale)
        assert torch.equal(ids, want[:t, :k]), (G, dtype, t)
        check_weights(w, scores[scoring][:t], ids, scoring, renorm, scale, (G, dtype, t, scoring))
    # layouts: the same values through other strides and another base give the same bits
    for n, (pad, off) in enumerate(((0, 0), (3, 0), (16, 0), (0, 1), (3, 1))):
        scoring, renorm, scale = CONFIGS[(n + 3) % len(CONFIGS)]
        base_ids, base_w = run_gate(lib, xd, k, scoring, renorm, scale)
        buf = torch.zeros((T * (G + pad) + 8 + off,), dtype=dtype, device=DEV)
        view = buf[off:off + T * (G + pad)].view(T, G + pad)[:, :G]
        view.copy_(xd)
        assert view.data_ptr() == buf.data_ptr() + off * buf.element_size()
        ids, w = run_gate(lib, view, k, scoring, renorm, scale)
        assert torch.equal(ids, base_ids) and torch.equal(bits(w), bits(base_w)), (G, dtype, pad, off)


@pytest.mark.parametrize("G", [65, 256, 1000])
def test_ties_and_special_values(lib, G):
    """For these rows only the ids are compared (and that the weights were written: run_gate)."""
    nan, inf = float("nan"), float("inf")
    E = 1
    while 64 * E < G:
        E *= 2
    rows = []
    rows.append(torch.full((G,), 0.75))                                   # all equal -> 0 .. k-1
    rows.append(torch.full((G,), -inf))                                   # all -inf -> 0 .. k-1: a pad slot never wins
    r = torch.arange(G, dtype=torch.float32) * -0.01                      # duplicates straddling lane and slot boundaries
    for e in (E - 1, E, 2 * E - 1, 2 * E, 63, 64, G - 2, G - 1):
        r[e] = 5.0
    rows.append(r)
    r = torch.full((G,), -1.0)                                            # -0.0 against +0.0: equal, the index decides
    r[[3, G - 1, E]] = torch.tensor([-0.0, 0.0, -0.0])
    r[1] = 0.0
    rows.append(r)
    for where in ([0], [G - 1], [G - 1, 7]):                              # NaNs come first, in index order
        r = torch.linspace(-2, 2, G)
        r[where] = nan
        rows.append(r)
    r = torch.linspace(-2, 2, G)                                          # +inf next to the largest finite value, -inf last
    r[5], r[6], r[G - 1] = torch.finfo(torch.float32).max, inf, -inf
    rows.append(r)
    x = torch.stack(rows)
    k = min(G, 12)
    want = torch.from_numpy(gate_ref(x.numpy(), k).ids).to(torch.int32)
    assert want[0].tolist() == list(range(k)) and want[1].tolist() == list(range(k))
    dup = sorted({E - 1, E, 2 * E - 1, 2 * E, 63, 64, G - 2, G - 1})
    assert want[2, :len(dup)].tolist() == dup
    assert want[3, :4].tolist() == sorted([1, 3, E, G - 1]) and want[4, 0] == 0 and want[5, 0] == G - 1 and want[6, :2].tolist() == [7, G - 1]
    assert want[7, :2].tolist() == [6, 5]
    for dtype in (torch.float32, torch.bfloat16):
        if dtype is torch.bfloat16:
            xs = x.to(dtype)
            wanted = torch.from_numpy(gate_ref(xs.float().numpy(), k).ids).to(torch.int32)   # (bfloat16 merges neighbouring values: its own order)
            assert torch.equal(wanted[:2], want[:2]) and wanted[7, :2].tolist() == [5, 6]      # (the largest float32 rounds to +inf: a tie)
        else:
            xs, wanted = x, want
        for scoring, renorm in (("softmax", True), ("sigmoid", False)):
            ids, _w = run_gate(lib, xs.to(DEV), k, scoring, renorm, 1.0)
            assert torch.equal(ids, wanted), (G, dtype, scoring)


# ---- scored form -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCORED_CASES))
def test_scored_cases(lib, name):
    x, bias = scored_inputs(name, 0)
    check_scored(lib, x, bias, scored_kwargs(name), name)


def test_groups_that_exclude_nothing_select_as_the_ungrouped_scored_form(lib):
    x, bias = scored_inputs("sigmoid-bias-64", 0)
    xd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(bias).to(DEV)
    for scoring in ("sigmoid", "softmax"):
        base_ids, base_w = run_gate(lib, xd, 6, scoring, True, 2.5, bias=bd)
        for n_group, group_score in ((64, "max"), (8, "max"), (8, "top2"), (2, "top2")):   # groups of one; every group kept
            ids, w = run_gate(lib, xd, 6, scoring, True, 2.5, bias=bd, n_group=n_group, topk_group=n_group, group_score=group_score)
            assert torch.equal(ids, base_ids) and torch.equal(bits(w), bits(base_w)), (scoring, n_group, group_score)
    # groups of one with some excluded: the kept groups ARE the top experts
    ids, _w = run_gate(lib, xd, 6, "sigmoid", False, 1.0, bias=bd, n_group=64, topk_group=6)
    base_ids, _w = run_gate(lib, xd, 6, "sigmoid", False, 1.0, bias=bd)
    assert torch.equal(ids, base_ids)


def test_k_takes_every_eligible_expert(lib):
    """G = 96 in 4 groups of 24, 2 kept, k = 48: a token's ids are exactly two whole groups - none from an excluded one, for EVERY token."""
    x, bias = scored_inputs("sigmoid-96-top2", 0)
    kw = dict(scored_kwargs("sigmoid-96-top2"), k=48)
    ids, r = check_scored(lib, x, bias, kw, "k = topk_group gs")
    groups = np.sort(ids.numpy() // 24, axis=1)
    assert bool((groups[:, :24] == groups[:, :1]).all()) and bool((groups[:, 24:] == groups[:, 47:]).all()) and bool((groups[:, 0] != groups[:, 47]).all())
    keep = ~r.close
    assert bool(np.take_along_axis(r.eligible, ids.numpy().astype(np.int64), axis=1)[keep].all())


def test_groups_whose_scores_tie_exactly(lib):
    """bf16 logits from a few well separated levels, a zero bias, GROUP_MAX: four or more of the eight groups hold the same largest logit, so
    their scores are the same float on any device and the three LOWEST of them win; equal levels in different groups tie on the expert
    level too.  Exact: ids compared in order, nothing skipped."""
    gen = torch.Generator().manual_seed(99)
    T, n_group, gs = 2048, 8, 8
    levels = torch.arange(-3.0, 1.5, 0.5)   # nine levels below 1.5
    x = torch.empty((T, n_group, gs))
    for g in range(n_group):
        pick = torch.argsort(torch.rand((T, levels.numel()), generator=gen), dim=1)[:, :gs]
        x[:, g] = levels[pick]
    tied = torch.rand((T, n_group), generator=gen) < 0.6
    tied[:, 7] = tied[:, 5] = tied[:, 2] = tied[:, 6] = True   # at least four
    top = torch.where(tied, torch.tensor(2.0), torch.tensor(1.5))
    x.scatter_(2, torch.randint(0, gs, (T, n_group, 1), generator=gen), top.unsqueeze(2))
    x = x.reshape(T, n_group * gs).to(torch.bfloat16)
    kw = dict(k=5, scoring="sigmoid", renormalize=True, scale=1.0, n_group=n_group, topk_group=3, group_score="max")
    r = gate_ref(x.float().numpy(), bias=np.zeros(64, dtype=np.float32), **kw)
    first_three = torch.from_numpy(np.argsort(~tied.numpy(), axis=1, kind="stable")[:, :3])
    assert torch.equal(torch.from_numpy(r.ids[:, :3] // gs), first_three)   # the reference keeps the three lowest tied groups
    ids, w = run_gate(lib, x.to(DEV), bias=torch.zeros(64, device=DEV), **kw)
    assert torch.equal(ids, torch.from_numpy(r.ids).to(torch.int32))
    check_weights(w, r.scores, ids, "sigmoid", True, 1.0, "tied groups")


def test_bias_selects_and_does_not_weight(lib):
    """A bias that reverses the selection: the ids follow the keys, the weights stay the scores (and are far from the keys)."""
    gen = torch.Generator().manual_seed(5)
    G, k = 64, 4
    x = random_logits(gen, 257, G, torch.float32)
    bias = torch.zeros(G)
    bias[G - k:] = 8.0   # the last k experts always win
    for scoring in ("sigmoid", "softmax"):
        ids, w = run_gate(lib, x.to(DEV), k, scoring, False, 1.0, bias=bias.to(DEV))
        assert bool((ids.sort(dim=1).values == torch.arange(G - k, G, dtype=torch.int32)).all())
        check_weights(w, scores_f64(x.numpy(), scoring), ids, scoring, False, 1.0, scoring)
        assert bool((w <= 1.0).all())


# ---- containment -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,k", [(64, 8), (8, 8), (5, 3), (1, 1), (257, 7), (129, 64)])
def test_exactly_the_ids_and_weights_are_written(lib, T, k):
    """T k a multiple of 64 and not (run_gate checks the sentinels on both sides of both outputs), plain and grouped."""
    gen = torch.Generator().manual_seed(T * 100 + k)
    x = random_logits(gen, T, 128, torch.bfloat16).to(DEV)
    run_gate(lib, x, k, "softmax", True, 1.0)
    run_gate(lib, x, k, "sigmoid", True, 1.0, bias=torch.zeros(128, device=DEV), n_group=2, topk_group=1, group_score="top2")


# ---- the op layer --------------------------------------------------------------------------------------------------------------------------

def test_gate_op(N_, lib):
    gen = torch.Generator().manual_seed(17)
    x = random_logits(gen, 130, 256, torch.bfloat16).to(DEV)
    bias = (0.1 * torch.randn(256, generator=gen)).to(DEV)
    kw = dict(scoring="sigmoid", renormalize=True, scale=2.5, n_group=8, topk_group=4, group_score="top2")
    want_ids, want_w = run_gate(lib, x, 8, bias=bias, **kw)
    ids, w = N_.fp8_moe_gate(x, 8, bias=bias, **kw)
    assert ids.dtype is torch.int32 and w.dtype is torch.float32 and tuple(ids.shape) == (130, 8) == tuple(w.shape)
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(bits(w.cpu()), bits(want_w))
    # a row-strided view is read in place, a column-strided one and another dtype are copied: the same result
    wide = torch.zeros((130, 300), dtype=torch.bfloat16, device=DEV)
    wide[:, 8:264] = x
    ids2, w2 = N_.fp8_moe_gate(wide[:, 8:264], 8, bias=bias, **kw)
    ids3, w3 = N_.fp8_moe_gate(x.t().contiguous().t(), 8, bias=bias.double(), **kw)
    ids4, w4 = N_.fp8_moe_gate(x.double(), 8, bias=bias, **kw)
    for i, ww in ((ids2, w2), (ids3, w3), (ids4, w4)):
        assert torch.equal(i, ids) and torch.equal(bits(ww), bits(w))
    empty_ids, empty_w = N_.fp8_moe_gate(x[:0], 8)
    assert tuple(empty_ids.shape) == (0, 8) == tuple(empty_w.shape)
    with pytest.raises(L.Fp8miError, match="k=40"):   # one group of 32 experts holds fewer
        N_.fp8_moe_gate(x, 40, n_group=8, topk_group=1)


class Layer:
    """One small MoE layer's weights in the four recipes"""

    def __init__(self, N_, G, K=256, H=256, N=128):
        gen = torch.Generator().manual_seed(G)
        W1 = (torch.randn((G, 2 * H, K), generator=gen) * K ** -0.5).to(DEV)
        W2 = (torch.randn((G, N, H), generator=gen) * H ** -0.5).to(DEV)
        self.G, self.K, self.N = G, K, N
        q1, s1 = N_.fp8_quantize_rowwise(W1.reshape(G * 2 * H, K), encode_mode=L.ENC_RNE)
        q2, s2 = N_.fp8_quantize_rowwise(W2.reshape(G * N, H), encode_mode=L.ENC_RNE)
        self.w = {"rowwise": (q1.reshape(G, 2 * H, K), s1.reshape(G, 2 * H), q2.reshape(G, N, H), s2.reshape(G, N))}
        b1 = [N_.fp8_quantize_blockwise(W1[g], 128) for g in range(G)]
        b2 = [N_.fp8_quantize_blockwise(W2[g], 128) for g in range(G)]
        self.w["blockwise"] = (torch.stack([q for q, _ in b1]), torch.stack([s for _, s in b1]), torch.stack([q for q, _ in b2]),
                               torch.stack([s for _, s in b2]))
        for fmt, quant in (("mxfp8", N_.fp8_quantize_mxfp8), ("mxfp4", N_.fp8_quantize_mxfp4)):
            (q1, s1), (q2, s2) = quant(W1.reshape(G * 2 * H, K)), quant(W2.reshape(G * N, H))
            self.w[fmt] = (q1.view(torch.uint8).reshape(G, 2 * H, -1), s1.view(torch.uint8).reshape(G, 2 * H, -1),
                           q2.view(torch.uint8).reshape(G, N, -1), s2.view(torch.uint8).reshape(G, N, -1))


@pytest.fixture(scope="module")
def layers(N_):
    return {G: Layer(N_, G) for G in (4, 16)}


GATE_KW = dict(scoring="sigmoid", renormalize=True, scale=2.5, n_group=2, topk_group=1, group_score="top2")


@pytest.mark.parametrize("T,k,G", [(5, 2, 4), (130, 8, 16)])
@pytest.mark.parametrize("recipe", ["rowwise", "blockwise", "mxfp8", "mxfp4"])
def test_layer_equals_gate_then_forward_bit_for_bit(N_, layers, recipe, T, k, G):
    """Seven launches with the one-launch route; T k = 1040 is past MOE_ROUTE_SINGLE_MAX: the three-launch route, nine."""
    gen = torch.Generator().manual_seed(T)
    layer = layers[G]
    forward = getattr(N_, "fp8_moe_forward_" + recipe)
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    logits = random_logits(gen, T, G, torch.bfloat16).to(DEV)
    bias = (0.1 * torch.randn(G, generator=gen)).to(DEV)
    N_.fp8_moe_layer(x, logits, k, *layer.w[recipe], recipe, bias=bias, kernel=TILE, **GATE_KW)   # (the route's workspace, outside the count)
    with L.kernel_timer(16) as kt:
        got = N_.fp8_moe_layer(x, logits, k, *layer.w[recipe], recipe, bias=bias, kernel=TILE, **GATE_KW)
    torch.cuda.synchronize()
    assert len(kt.ms) == (7 if T * k <= SINGLE else 9)
    ids, w = N_.fp8_moe_gate(logits, k, bias=bias, **GATE_KW)
    want = forward(x, ids, w, *layer.w[recipe], kernel=TILE)
    assert tuple(got.shape) == (T, layer.N) and got.dtype is torch.bfloat16
    assert torch.equal(bits(got), bits(want))
    assert bool(got.float().abs().sum() > 0)


def test_layer_captured_into_a_graph_follows_new_logits_on_replay(N_, layers):
    gen = torch.Generator().manual_seed(3)
    layer, T, k, G = layers[4], 5, 2, 4
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    first = (torch.argsort(torch.rand((T, G), generator=gen), dim=1).float() / 4).to(torch.bfloat16)   # distinct in every row
    logits = first.to(DEV)
    run = lambda: N_.fp8_moe_layer(x, logits, k, *layer.w["rowwise"], "rowwise", scoring="softmax", renormalize=True, kernel=TILE)   # noqa: E731
    eager1 = run()
    ids1, _w = N_.fp8_moe_gate(logits, k, "softmax", True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):   # (a host sync or a read of the routing inside the capture would fail it)
        out = run()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager1))
    logits.copy_((-first).to(DEV))   # in place: the two best experts of every token become its two worst
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    ids2, _w = N_.fp8_moe_gate(logits, k, "softmax", True)
    assert not bool((ids1.sort(dim=1).values == ids2.sort(dim=1).values).any())   # a replay that ignored the new logits fails below
    assert torch.equal(bits(replayed), bits(run()))
    assert not torch.equal(bits(replayed), bits(eager1))
