"""The lightning indexer (fp8_mla_index_*, fp8_mla_indexer) on the GPU against tests/mla_indexer_ref.py.  The logits bound is derived, not measured: a logit is k_scale sum_h w' relu(dot_h); a 128-term fp32 dot product of exact e4m3 products takes at
most 128 roundings, the Hi-term weighted sum Hi more, w' = weights qs and the final product one each: at most 128 + Hi + 2 <= 194 roundings of
relative size u = 2^-23 (truncating accumulation included), each applied to a partial sum no larger than abs_sum: 194 2^-23 < 2^-15."""
import functools

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import fp8_mi355x_native as N
import mla_indexer_ref as I
import mla_varlen_ref as V
from moe_route_gpu_util import DEV, SENT_F, bits
from test_gpu_mla import TORCH, run as run_dense

pytestmark = pytest.mark.gpu
DECODE = [(1, 1), (16, 1), (17, 1), (129, 1), (300, 1)]   # one position, a full tile, one past it, one past a 128 step, several blocks
VARLEN = [(40, 3), (150, 1), (9, 0), (2, 5)]              # the last sequence's context is shorter than its q_len: rows with limit <= 0
FORMS = {"decode": DECODE, "varlen": VARLEN}


@functools.lru_cache(maxsize=None)
def case(form, Hi, bs):
    c = I.make_case(1300 + Hi + bs, FORMS[form], bs, Hi)
    return c, I.logits_ref(c)


def run_logits(c, form, cache=None, table=None, max_q_len=None, extra_rows=0):
    """-> logits (T + extra_rows, max_seq_len + 3) on the CPU, prefilled with the sentinel"""
    T = len(c.q)
    out = torch.full((T + extra_rows, c.max_seq_len + 3), SENT_F, device=DEV)
    q, w = torch.zeros((T + extra_rows,) + c.q.shape[1:], dtype=TORCH[c.q_dtype], device=DEV), torch.zeros((T + extra_rows, c.q.shape[1]), device=DEV)
    q[:T], w[:T] = torch.from_numpy(c.q), torch.from_numpy(c.weights)
    kw = dict(cu_seqlens_q=torch.from_numpy(c.cu).to(DEV), max_q_len=int(c.q_lens.max()) if max_q_len is None else max_q_len) if form == "varlen" else {}
    N.fp8_mla_index_logits(q, w, torch.from_numpy(c.cache if cache is None else cache).to(DEV), torch.from_numpy(c.block_table if table is None else table).to(DEV),
                           torch.from_numpy(c.seq_lens).to(DEV), max_seq_len=c.max_seq_len, out=out, **kw)
    return out.cpu()


@pytest.mark.parametrize("dtype", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("bs", (16, 128))
def test_append_bytes_and_scales(dtype, bs):
    """k a strided slice of a wider tensor; a zero row, a row whose amax / 448 is a power of two; slots -1 and num_blocks bs leave the sentinel"""
    T, nb = 70, 3 if bs == 128 else 6
    rng = np.random.default_rng(21)
    wide = rng.standard_normal((T, 160)) * np.exp2(rng.integers(-10, 10, (T, 1)))
    wide[5], wide[6, 8:136] = 0.0, 0.25
    wide[6, 50] = -448.0 * 2.0 ** -5
    wide = torch.from_numpy(wide).to(TORCH[dtype])
    k = wide[:, 8:136].float().numpy()
    slots = rng.permutation(nb * bs)[:T].astype(np.int64)
    slots[[3, 40]] = -1, nb * bs
    keep = (slots >= 0) & (slots < nb * bs)
    data, scales = I.append_ref(k)
    assert scales[5] == 1.0 and scales[6] == 2.0 ** -5
    want = np.full((nb, bs * I.ROW), 0xA5, np.uint8)
    I.write_cache(want, bs, slots[keep], data[keep], scales[keep])
    cache = torch.full((nb, bs * I.ROW), 0xA5, dtype=torch.uint8, device=DEV)
    N.fp8_mla_index_cache_append(wide.to(DEV)[:, 8:136], cache, torch.from_numpy(slots).to(DEV), encode_mode=L.ENC_RNE)
    bad = np.argwhere(cache.cpu().numpy() != want)
    assert tuple(N.fp8_mla_index_cache_alloc(nb, bs, device=DEV).shape) == (nb, bs * I.ROW) and len(bad) == 0, (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("form", ("decode", "varlen"))
@pytest.mark.parametrize("bs", (16, 64))
@pytest.mark.parametrize("Hi", (16, 32, 64))
def test_logits_within_the_derived_bound_and_nothing_else_written(form, Hi, bs):
    c, ref = case(form, Hi, bs)
    assert min(r[2] for r in ref) < 0, "no negative head dot product: the ReLU would not be seen"
    out = run_logits(c, form, extra_rows=2 if form == "varlen" else 0).double().numpy()   # two rows behind cu[B]: nobody's
    worst = 0.0
    for t, (want, abs_sum, _) in enumerate(ref):
        n = len(want)
        assert (out[t, n:] == SENT_F).all(), (t, "a column at or beyond the limit was written")
        if n:
            worst = max(worst, float((np.abs(out[t, :n] - want) / abs_sum).max()))
    print(f"{form} Hi={Hi} bs={bs}: max |got - ref| / abs_sum = {worst:.3e} (bound {I.BOUND:.3e})")
    assert worst <= I.BOUND and (out[len(ref):] == SENT_F).all() and any(len(r[0]) == 0 for r in ref) == (form == "varlen")
    if form == "varlen":   # max_q_len = 2: the third token of the first sequence and the later tokens of the last keep the sentinel
        short, j = run_logits(c, form, max_q_len=2), np.arange(len(c.q)) - c.cu[V.limits(c)[0]]
        assert (short[j >= 2] == SENT_F).all() and torch.equal(bits(short[j < 2]), bits(run_logits(c, form)[j < 2]))


@pytest.mark.parametrize("form", ("decode", "varlen"))
def test_logits_isolation(form):
    """per token: 0x7F key bytes and NaN scales at or beyond its limit and in every block it does not need, 1 << 30 in every table entry beyond
    its need - the bits stay; a needed table entry out of range gives exactly 0.0 there and nothing else moves"""
    c, ref = case(form, 32, 16)
    clean, (seq, _) = run_logits(c, form), V.limits(c)
    bs = c.block_size
    for t, (want, _, _) in enumerate(ref):
        n, need = len(want), (len(want) + bs - 1) // bs
        cache, table = np.full_like(c.cache, 0x7F), np.full_like(c.block_table, 1 << 30)
        cache[:, bs * I.DIM:] = 0xFF   # NaN scales
        for i, blk in enumerate(c.block_table[seq[t], :need]):
            rows = min(bs, n - i * bs)
            cache[blk, :rows * I.DIM] = c.cache[blk, :rows * I.DIM]
            cache[blk, bs * I.DIM:bs * I.DIM + 4 * rows] = c.cache[blk, bs * I.DIM:bs * I.DIM + 4 * rows]
        table[seq[t], :need] = c.block_table[seq[t], :need]
        assert torch.equal(bits(run_logits(c, form, cache=cache)[t]), bits(clean[t])) and torch.equal(bits(run_logits(c, form, table=table)[t]), bits(clean[t])), t
    t = int(np.argmax([len(r[0]) for r in ref]))
    table = c.block_table.copy()
    table[seq[t], 1] = len(c.cache)
    out = run_logits(c, form, table=table)
    hit = np.zeros(clean.shape, bool)
    for u in np.flatnonzero(seq == seq[t]):
        hit[u, bs:min(2 * bs, len(ref[u][0]))] = True
    assert hit[t].sum() == bs and bool((bits(out)[torch.from_numpy(hit)] == 0).all()) and torch.equal(bits(out)[torch.from_numpy(~hit)], bits(clean)[torch.from_numpy(~hit)])


def _rows(k):
    """synthetic (name, row, limit) for topk = k"""
    rng = np.random.default_rng(k)
    n = 9000 + 1009
    special = rng.standard_normal(max(3 * k, 64)).astype(np.float32)
    special[rng.permutation(len(special))[:10]] = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, np.inf, np.nan]
    rows = [(f"limit={k + d}", rng.standard_normal(k + 40).astype(np.float32), k + d) for d in (-1, 0, 1) if k + d > 0]
    rows += [("small integers", rng.integers(-3, 4, 4 * k + 100).astype(np.float32), 4 * k + 100), ("all equal", np.full(2 * k + 7, 1.5, np.float32), 2 * k + 7),
             ("last digit", (1.0 + rng.permutation(2 * k + 50) * 2.0 ** -23).astype(np.float32), 2 * k + 50), ("special values", special, len(special)),
             ("long", rng.standard_normal(n).astype(np.float32), n)]
    return rows


@pytest.mark.parametrize("k", (1, 64, 2048))
def test_topk_is_the_reference_selection(k):
    """one decode-form call over all the rows, ld_logits > n_cols; then a varlen batch whose middle row nobody owns"""
    rows = _rows(k)
    n_cols = max(len(r) for _, r, _ in rows)
    x = torch.full((len(rows), n_cols + 5), float("nan"))
    for i, (_, r, _) in enumerate(rows):
        x[i, :len(r)] = torch.from_numpy(r)
    lens = torch.tensor([limit for *_, limit in rows], dtype=torch.int32)
    got = N.fp8_mla_index_topk(x.to(DEV)[:, :n_cols], lens.to(DEV), k).cpu().numpy()
    for i, (name, r, limit) in enumerate(rows):
        assert np.array_equal(got[i], I.topk_ref(x[i, :n_cols].numpy(), limit, k)), (name, k)
    # rows 0 and 1 are sequence 0's two tokens (limits seq - 1 and seq), row 2 is sequence 1's, row 3 lies behind cu[B]: nobody's
    ints = [name for name, *_ in rows].index("small integers")
    seq, out = [len(rows[-1][1]), rows[ints][2]], torch.full((4, k), -7777, dtype=torch.int32, device=DEV)
    y = x[[len(rows) - 1, len(rows) - 1, ints, 0]].to(DEV)[:, :n_cols]
    N.fp8_mla_index_topk(y, torch.tensor(seq, dtype=torch.int32), k, cu_seqlens_q=torch.tensor([0, 2, 3]), max_q_len=2, out=out)
    for t, limit in ((0, seq[0] - 1), (1, seq[0]), (2, seq[1])):
        assert np.array_equal(out[t].cpu().numpy(), I.topk_ref(y[t].cpu().numpy(), limit, k)), t
    assert bool((out[3] == -7777).all())


def _indexer_inputs(c, seed, Hi=64):
    """an index-key cache, q and weights for the sequences of an mla_varlen_ref case, over ITS block table"""
    rng = np.random.default_rng(seed)
    cache = N.fp8_mla_index_cache_alloc(c.cache.shape[0], c.block_size, device=DEV)
    for b, L in enumerate(c.seq_lens):
        pos = np.arange(int(L))
        slots = c.block_table[b, pos // c.block_size].astype(np.int64) * c.block_size + pos % c.block_size
        N.fp8_mla_index_cache_append(torch.from_numpy(rng.standard_normal((int(L), I.DIM)).astype(np.float32)), cache, torch.from_numpy(slots))
    T = len(c.q)
    return torch.from_numpy(rng.standard_normal((T, Hi, I.DIM)).astype(np.float32)).to(DEV), torch.from_numpy(rng.standard_normal((T, Hi)).astype(np.float32)).to(DEV), cache


@pytest.mark.parametrize("num_splits", (1, 2))
def test_sparse_attention_on_the_indexers_output_is_the_dense_call(num_splits):
    """topk >= every limit: the indexer gives 0 .. limit - 1 then -1, and the sparse attention on it equals, bit for bit, the dense call with
    max_seq_len = topk and the same num_splits"""
    c, e = V.case("mixed")[:2]
    topk = 384
    _, lim = V.limits(c)
    assert lim.max() <= topk
    q, w, icache = _indexer_inputs(c, 77)
    tensors = [torch.from_numpy(x).to(DEV) for x in (c.block_table, c.seq_lens, c.cu)]
    idx = N.fp8_mla_indexer(q, w, icache, tensors[0], tensors[1], topk, cu_seqlens_q=tensors[2], max_q_len=int(c.q_lens.max()))
    want = np.where(np.arange(topk) < np.maximum(lim, 0)[:, None], np.arange(topk), -1)
    assert np.array_equal(idx.cpu().numpy(), want)
    ql = torch.from_numpy(c.q).to(DEV)
    sparse = N.fp8_mla_paged_attention(ql[..., :V.R.LATENT], ql[..., V.R.LATENT:], torch.from_numpy(c.cache).to(DEV), tensors[0], tensors[1], torch.from_numpy(c.kv_scale).to(DEV),
                                       V.R.SOFTMAX_SCALE, num_splits=num_splits, indices=idx, cu_seqlens_q=tensors[2], max_q_len=int(c.q_lens.max())).cpu()
    assert torch.equal(bits(sparse), bits(run_dense(e, max_seq_len=topk, num_splits=num_splits)))


def test_graph_replay_after_every_input_changed_in_place():
    first, second = I.make_case(1400, [(33, 1), (140, 1)], 16, 64, spare_blocks=4), I.make_case(1401, [(150, 1), (9, 1)], 16, 64, spare_blocks=5)

    def tensors(c):
        table = np.full((2, 12), -1, np.int32)
        table[:, :c.block_table.shape[1]] = c.block_table
        return [torch.from_numpy(x) for x in (c.q, c.weights, c.cache, table, c.seq_lens)]

    assert first.cache.shape == second.cache.shape
    q, w, cache, table, lens = held = [x.to(DEV) for x in tensors(first)]
    logits = torch.empty((2, 192), device=DEV)   # the capture runs on a stream of its own, which holds no workspace yet
    call = lambda: N.fp8_mla_indexer(q, w, cache, table, lens, 64, logits=logits)   # noqa: E731
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().clone()
    assert torch.equal(got, call().cpu())
    for dst, src in zip(held, tensors(second)):
        dst.copy_(src)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), call().cpu())
    assert not torch.equal(out.cpu(), got)
