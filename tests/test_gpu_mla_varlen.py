"""fp8_mla_paged_attention(cu_seqlens_q=) / fp8mi_mla_attention_varlen on the GPU: every owned row bit for bit the decode entry on the
one-sequence-per-token expansion and within TOL max|latent| of the float64 reference (tests/mla_varlen_ref.py); rows nobody owns, bytes
beyond a limit and graph replay."""
import functools

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import fp8_mi355x_native as N
import mla_ref as R
import mla_varlen_ref as V
from moe_route_gpu_util import CODE, DEV, SENT_F, bits, stream
from test_gpu_mla import TORCH, run as run_decode

pytestmark = pytest.mark.gpu
BIG = 1 << 62


def run(c, **kw):
    """one multi-token fp8_mla_paged_attention of the case -> out (T, Hq, 512) on the device"""
    q = torch.from_numpy(c.q).to(DEV, TORCH[c.q_dtype])
    args = dict(max_seq_len=c.max_seq_len, num_splits=c.num_splits, out_dtype=TORCH[c.out_dtype])
    if "cu_seqlens_q" not in kw:
        args.update(cu_seqlens_q=torch.from_numpy(c.cu).to(DEV), max_q_len=int(c.q_lens.max()))
    args.update(kw)
    cache, table = (torch.from_numpy(x).to(DEV) for x in (args.pop("cache", c.cache), args.pop("table", c.block_table)))
    return N.fp8_mla_paged_attention(q[..., :R.LATENT], q[..., R.LATENT:], cache, table, torch.from_numpy(c.seq_lens).to(DEV), torch.from_numpy(c.kv_scale).to(DEV),
                                     R.SOFTMAX_SCALE, **args)


@functools.lru_cache(maxsize=None)
def out_of(name):
    return run(V.case(name)[0]).cpu()


def within_tol(out, name):
    ref, vmax = V.case(name)[2:]
    got = out.double().numpy()
    assert got.shape == ref.shape and not np.isnan(got).any(), name
    r = R.ratio(got, ref, vmax)
    print(f"{name}: max |out - ref| / max|latent| = {r:.5f} (TOL {V.TOL})")
    assert r <= V.TOL, (name, r)


@pytest.mark.parametrize("name", V.CASES)
def test_every_row_is_the_decode_entry_on_the_expansion_bit_for_bit_and_within_tol_of_the_float64_reference(name):
    e, out = V.case(name)[1], out_of(name)
    assert out.numel() > 0 and torch.equal(bits(out), bits(run_decode(e)))
    assert not out[torch.from_numpy(e.seq_lens == 0)].any(), "limit <= 0 gives a zero row"
    within_tol(out, name)


@pytest.mark.parametrize("name", ("mixed", "splits=3 L=400"))
def test_one_token_per_sequence_is_the_decode_entry(name):
    c = R.case(name)[0]
    B, Hq = c.q.shape[:2]
    out = run(c, cu_seqlens_q=torch.arange(B + 1, dtype=torch.int32, device=DEV), max_q_len=1)
    assert torch.equal(bits(out.cpu()), bits(run_decode(c)))
    for ms in (300, 1024, 8192, 1 << 17):
        assert L.load().fp8mi_mla_attention_varlen_splits(B, B, 1, Hq, ms, BIG) == L.load().fp8mi_mla_attention_splits(B, Hq, ms, BIG)


def test_the_librarys_split_choice_is_the_forced_count_bit_for_bit():
    c = V.case("splits=3")[0]
    T, Hq = c.q.shape[:2]
    n = L.load().fp8mi_mla_attention_varlen_splits(T, 1, T, Hq, V.SPLIT_MAX_SEQ, BIG)
    assert n == V.auto_splits(T, 1, T, Hq, V.SPLIT_MAX_SEQ, BIG, torch.cuda.get_device_properties(0).multi_processor_count) and n > 1
    with L.kernel_timer(4) as kt:
        auto = run(c, num_splits=0, max_q_len=None)   # max_q_len defaults to T
    assert len(kt.ms) == 2 and torch.equal(bits(auto), bits(run(c, num_splits=n)))


@pytest.mark.parametrize("num_splits", (1, 3))
def test_rows_nobody_owns_are_not_written(num_splits):
    """the C entry on an output prefilled with a sentinel: T = cu[B] + 3 and max_q_len = 3 below the 5 and 16 tokens of two sequences - the
    padding rows and the tokens from the fourth on keep the sentinel, the others are the full call's"""
    c, lib = V.case("mixed")[0], L.load()
    T, Hq = c.q.shape[:2]
    q = torch.zeros((T + 3, Hq, R.ROW), device=DEV)
    q[:T] = torch.from_numpy(c.q)
    ql, qp = q[..., :R.LATENT].contiguous(), q[..., R.LATENT:].contiguous()
    cache, table, lens, kvs, cu = (torch.from_numpy(x).to(DEV) for x in (c.cache, c.block_table, c.seq_lens, c.kv_scale, c.cu))
    ws = torch.empty(max(lib.fp8mi_mla_attention_workspace_bytes(T + 3, Hq, num_splits), 16), dtype=torch.uint8, device=DEV)

    def call(max_q_len):
        out = torch.full((T + 3, Hq, R.LATENT), SENT_F, device=DEV)
        with L.kernel_timer(4) as kt:
            rc = lib.fp8mi_mla_attention_varlen(ql.data_ptr(), qp.data_ptr(), CODE[torch.float32], T + 3, len(c.q_lens), cu.data_ptr(), max_q_len, Hq, Hq * R.LATENT,
                                                Hq * R.ROPE, cache.data_ptr(), cache.shape[0], c.block_size, table.data_ptr(), table.stride(0), table.shape[1],
                                                lens.data_ptr(), c.max_seq_len, kvs.data_ptr(), R.SOFTMAX_SCALE, num_splits, ws.data_ptr(), ws.numel(),
                                                out.data_ptr(), CODE[torch.float32], Hq * R.LATENT, stream())
        assert rc == 0 and len(kt.ms) == (1 if num_splits == 1 else 2)
        return out.cpu()

    full, out = call(T + 3), call(3)
    owned = torch.zeros(T + 3, dtype=torch.bool)
    for b, n in enumerate(c.q_lens):
        owned[c.cu[b]:c.cu[b] + min(int(n), 3)] = True
    assert int(owned.sum()) == 7 and bool((out[~owned] == SENT_F).all()), "a row no sequence owns, or one at or beyond max_q_len, was written"
    assert bool((full[T:] == SENT_F).all()) and torch.equal(bits(out[owned]), bits(full[owned]))
    within_tol(full[:T], "mixed")


@pytest.mark.parametrize("name", ("packed", "chunk"))
def test_nothing_at_or_beyond_a_rows_limit_moves_it(name):
    """one sequence, Hq = 16: workgroup tile i holds the tokens 4 i .. 4 i + 3.  (a) NaN bytes at and beyond the tile's largest limit, table
    entries beyond its need -1: the tile's rows keep their bits.  (b) finite garbage in [limit_j, the largest limit of j's tile): row j does."""
    c = V.case(name)[0]
    clean, lim, bs, n = out_of(name), V.limits(c)[1], c.block_size, int(c.q_lens[0])
    assert c.q.shape[1] == 16 and len(c.q_lens) == 1
    slots, rng, flat = c.slots[0], np.random.default_rng(5), c.cache.reshape(-1, R.ROW)
    for j0 in range(0, n, 4):
        top = int(lim[min(j0 + 3, n - 1)])
        cache, table = np.full_like(c.cache, 0x7F), c.block_table.copy()
        cache.reshape(-1, R.ROW)[slots[:top]] = flat[slots[:top]]
        table[0, (top + bs - 1) // bs:] = -1
        assert torch.equal(bits(run(c, cache=cache, table=table)[j0:j0 + 4].cpu()), bits(clean[j0:j0 + 4])), (j0, top)
    for j in range(n):
        lo, top = int(lim[j]), int(lim[min(j // 4 * 4 + 3, n - 1)])
        cache = c.cache.copy()
        cache.reshape(-1, R.ROW)[slots[lo:top]] = rng.integers(0, 0x7F, (top - lo, R.ROW), dtype=np.uint8) | (rng.integers(0, 2, (top - lo, R.ROW), dtype=np.uint8) << 7)
        assert top == lo or torch.equal(bits(run(c, cache=cache)[j].cpu()), bits(clean[j])), j


@pytest.mark.parametrize("num_splits", (1, 2))
def test_graph_replay_on_new_cu_lengths_table_and_cache(num_splits):
    """captured on one batch, replayed after every input changed in place: owned rows equal the eager call's bits on every replay, the row the
    second batch does not own is not written"""
    T, Hq = 8, 20
    first, second = V.make_case(980, [(33, 3), (140, 5)], 16, Hq, spare_blocks=4), V.make_case(981, [(150, 6), (9, 1)], 16, Hq, spare_blocks=5)

    def tensors(c):
        table, q = np.full((2, R.GRAPH_MAX_BLOCKS), -1, np.int32), np.zeros((T, Hq, R.ROW), np.float32)
        table[:, :c.block_table.shape[1]], q[:c.q.shape[0]] = c.block_table, c.q
        return [torch.from_numpy(x) for x in (q[..., :R.LATENT].copy(), q[..., R.LATENT:].copy(), c.cu, c.cache, table, c.seq_lens, c.kv_scale)]

    ql, qp, cu, cache, table, lens, scale = held = [x.to(DEV) for x in tensors(first)]
    ws = torch.empty(max(L.load().fp8mi_mla_attention_workspace_bytes(T, Hq, num_splits), 16), dtype=torch.uint8, device=DEV)
    call = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, scale, R.SOFTMAX_SCALE, max_seq_len=R.GRAPH_MAX_SEQ, num_splits=num_splits,   # noqa: E731
                                             workspace=ws, cu_seqlens_q=cu, max_q_len=T)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().clone()
    assert torch.equal(bits(got), bits(call().cpu()))
    for dst, src in zip(held, tensors(second)):
        dst.copy_(src)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        replayed, n = out.cpu().clone(), second.q.shape[0]
        assert n == 7 and torch.equal(bits(replayed[:n]), bits(call().cpu()[:n])) and torch.equal(bits(replayed[n:]), bits(got[n:]))
    assert not torch.equal(bits(replayed[:n]), bits(got[:n]))
