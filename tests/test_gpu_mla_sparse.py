"""fp8_mla_paged_attention(indices=) / fp8mi_mla_attention_sparse on the GPU against tests/mla_sparse_ref.py: every token within TOL max|latent|
of the float64 reference on its valid rows and - where its list is valid up to n and -1 from there on - bit for bit the decode entry on the
compacted cache; isolation from everything no valid entry names, the split choice, rows nobody owns, graph replay."""
import functools

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import fp8_mi355x_native as N
import mla_ref as R
import mla_sparse_ref as S
import mla_varlen_ref as V
from moe_route_gpu_util import CODE, DEV, SENT_F, bits, stream
from test_gpu_mla import TORCH, run as run_decode

pytestmark = pytest.mark.gpu
BIG = 1 << 62


def run(c, **kw):
    """one sparse fp8_mla_paged_attention of the case -> out (T, Hq, 512) on the CPU"""
    q = torch.from_numpy(c.q).to(DEV, TORCH[c.q_dtype])
    args = dict(num_splits=c.num_splits, out_dtype=TORCH[c.out_dtype])
    if c.form == "varlen":
        args.update(cu_seqlens_q=torch.from_numpy(c.cu).to(DEV), max_q_len=int(c.q_lens.max()))
    args.update(kw)
    cache, table, indices = (torch.from_numpy(x).to(DEV) for x in (args.pop("cache", c.cache), args.pop("table", c.block_table), args.pop("indices", c.indices)))
    return N.fp8_mla_paged_attention(q[..., :R.LATENT], q[..., R.LATENT:], cache, table, torch.from_numpy(c.seq_lens).to(DEV), torch.from_numpy(c.kv_scale).to(DEV),
                                     R.SOFTMAX_SCALE, indices=indices, **args).cpu()


@functools.lru_cache(maxsize=None)
def out_of(name):
    return run(S.case(name)[0])


@pytest.mark.parametrize("name", S.CASES)
def test_within_tol_of_the_float64_reference_and_bit_for_bit_the_decode_entry_on_the_compacted_cache(name):
    (c, ref, vmax), out = S.case(name), out_of(name)
    got = out.double().numpy()
    assert got.shape == ref.shape and not np.isnan(got).any(), name
    r = R.ratio(got, ref, vmax)   # asserts a zero row for a token without a valid entry
    print(f"{name}: max |out - ref| / max|latent| = {r:.5f} (TOL {S.TOL})")
    assert r <= S.TOL, (name, r)
    prefix = [t for t in range(len(got)) if S.prefix_n(c, t) is not None]
    assert len(prefix) == len(got) or name in ("holes", "mtp")
    for t in prefix:
        assert torch.equal(bits(out[t:t + 1]), bits(run_decode(S.compact(c, t)))), (name, t)


@pytest.mark.parametrize("name", ("holes", "mtp"))
def test_nothing_but_the_rows_its_valid_entries_name_moves_a_token(name):
    """(a) every kind of invalid entry rewritten as every other; per token (b) NaN bytes in every cache row no valid entry of it names,
    (c) an out-of-range value in every table entry no valid entry of it needs: the bits stay"""
    c, clean, ok = S.case(name)[0], out_of(name), S.valid(S.case(name)[0])
    seq, lim = V.limits(c)
    for kind in (np.full(len(lim), -1), np.full(len(lim), -9), lim, np.full(len(lim), (1 << 31) - 1)):
        assert torch.equal(bits(run(c, indices=np.where(ok, c.indices, kind[:, None].astype(np.int32)))), bits(clean)), kind[0]
    assert name != "mtp" or (c.indices[0] == lim[0]).any(), "the first mtp token names a position between the two limits"
    for t in range(len(lim)):
        idx = c.indices[t, ok[t]].astype(np.int64)
        blocks = c.block_table[seq[t], idx // c.block_size].astype(np.int64)
        cache, table = np.full_like(c.cache, 0x7F), np.full_like(c.block_table, 1 << 30)
        cache[blocks, idx % c.block_size] = c.cache[blocks, idx % c.block_size]
        table[seq[t], idx // c.block_size] = blocks
        assert torch.equal(bits(run(c, cache=cache)[t]), bits(clean[t])) and torch.equal(bits(run(c, table=table)[t]), bits(clean[t])), t


def test_the_librarys_split_choice_is_the_forced_count_bit_for_bit():
    c = S.case("splits=3 n=400")[0]
    Hq = c.q.shape[1]
    n = L.load().fp8mi_mla_attention_sparse_splits(1, 1, 1, Hq, c.topk, BIG)
    assert n == S.auto_splits(1, 1, 1, Hq, c.topk, BIG, torch.cuda.get_device_properties(0).multi_processor_count) and n > 1
    with L.kernel_timer(4) as kt:
        auto = run(c, num_splits=0)
    assert len(kt.ms) == 2 and torch.equal(bits(auto), bits(run(c, num_splits=n)))


@pytest.mark.parametrize("num_splits", (1, 3))
def test_rows_nobody_owns_are_not_written(num_splits):
    """the C entry on an output prefilled with a sentinel: T = cu[B] + 3 and max_q_len = 1 below the 2 tokens of the first sequence - the padding
    rows and that sequence's second token keep the sentinel, the others are the full call's"""
    c, lib = S.case("mtp")[0], L.load()
    T, Hq = c.q.shape[:2]
    q, idx = torch.zeros((T + 3, Hq, R.ROW), device=DEV), torch.full((T + 3, c.topk + 5), 7, dtype=torch.int32, device=DEV)   # ld_idx > topk
    q[:T], idx[:T, :c.topk] = torch.from_numpy(c.q), torch.from_numpy(c.indices)
    ql, qp = q[..., :R.LATENT].contiguous(), q[..., R.LATENT:].contiguous()
    cache, table, lens, kvs, cu = (torch.from_numpy(x).to(DEV) for x in (c.cache, c.block_table, c.seq_lens, c.kv_scale, c.cu))
    ws = torch.empty(max(lib.fp8mi_mla_attention_workspace_bytes(T + 3, Hq, num_splits), 16), dtype=torch.uint8, device=DEV)

    def call(max_q_len):
        out = torch.full((T + 3, Hq, R.LATENT), SENT_F, device=DEV)
        with L.kernel_timer(4) as kt:
            rc = lib.fp8mi_mla_attention_sparse(ql.data_ptr(), qp.data_ptr(), CODE[torch.float32], T + 3, len(c.q_lens), cu.data_ptr(), max_q_len, Hq, Hq * R.LATENT,
                                                Hq * R.ROPE, idx.data_ptr(), c.topk, idx.stride(0), cache.data_ptr(), cache.shape[0], c.block_size, table.data_ptr(),
                                                table.stride(0), table.shape[1], lens.data_ptr(), kvs.data_ptr(), R.SOFTMAX_SCALE, num_splits, ws.data_ptr(), ws.numel(),
                                                out.data_ptr(), CODE[torch.float32], Hq * R.LATENT, stream())
        assert rc == 0 and len(kt.ms) == (1 if num_splits == 1 else 2)
        return out.cpu()

    full, out = call(T + 3), call(1)
    owned = torch.tensor([True, False, True, False, False, False])
    assert bool((out[~owned] == SENT_F).all()), "a row no sequence owns, or one at or beyond max_q_len, was written"
    assert bool((full[T:] == SENT_F).all()) and torch.equal(bits(out[owned]), bits(full[:T][owned[:T]]))
    assert num_splits != 1 or torch.equal(bits(full[:T]), bits(out_of("mtp")))


@pytest.mark.parametrize("num_splits", (1, 2))
def test_graph_replay_on_new_indices_table_and_cache(num_splits):
    """captured on one batch, replayed after every input changed in place: the rows equal the eager call's bits on every replay"""
    lists = lambda c, rng: rng.integers(-3, 170, (2, 160))   # noqa: E731  two steps; holes: negatives, positions beyond the shorter limits
    first, second = S.make_case(1180, 20, 16, [(33, 1), (140, 1)], "decode", lists, spare_blocks=4), S.make_case(1181, 20, 16, [(150, 1), (9, 1)], "decode", lists, spare_blocks=5)

    def tensors(c):
        table = np.full((2, R.GRAPH_MAX_BLOCKS), -1, np.int32)
        table[:, :c.block_table.shape[1]] = c.block_table
        return [torch.from_numpy(x) for x in (c.q[..., :R.LATENT].copy(), c.q[..., R.LATENT:].copy(), c.indices, c.cache, table, c.seq_lens, c.kv_scale)]

    ql, qp, idx, cache, table, lens, scale = held = [x.to(DEV) for x in tensors(first)]
    ws = torch.empty(max(L.load().fp8mi_mla_attention_workspace_bytes(2, 20, num_splits), 16), dtype=torch.uint8, device=DEV)
    call = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, scale, R.SOFTMAX_SCALE, num_splits=num_splits, workspace=ws, indices=idx)   # noqa: E731
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().clone()
    assert torch.equal(bits(got), bits(call().cpu())) and torch.equal(bits(got), bits(run(first, num_splits=num_splits)))
    for dst, src in zip(held, tensors(second)):
        dst.copy_(src)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().clone()
        assert torch.equal(bits(replayed), bits(call().cpu()))
    assert not torch.equal(bits(replayed), bits(got)) and torch.equal(bits(replayed), bits(run(second, num_splits=num_splits)))
