"""fp8_mla_cache_append / fp8_mla_paged_attention (fp8mi_mla_cache_append, fp8mi_mla_attention_decode) on the GPU: the append byte for byte
against quantise(), every attention element within TOL_mla max|latent| of the float64 reference (a) of tests/mla_ref.py."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import fp8_mi355x_native as N
import mla_ref as R
from moe_route_gpu_util import DEV, bits

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def run(c, **kw):
    """one fp8_mla_paged_attention of the case -> out on the CPU"""
    q = torch.from_numpy(c.q).to(DEV, TORCH[c.q_dtype])
    args = dict(max_seq_len=c.max_seq_len, num_splits=c.num_splits, out_dtype=TORCH[c.out_dtype])
    args.update(kw)
    cache, table = (torch.from_numpy(x).to(DEV) for x in (args.pop("cache", c.cache), args.pop("table", c.block_table)))
    return N.fp8_mla_paged_attention(q[..., :R.LATENT], q[..., R.LATENT:], cache, table, torch.from_numpy(c.seq_lens).to(DEV),
                                     torch.from_numpy(c.kv_scale).to(DEV), R.SOFTMAX_SCALE, **args).cpu()


def within_tol(out, name):
    c, ref, vmax = R.case(name)
    got = out.double().numpy()
    assert got.shape == ref.shape and not np.isnan(got).any(), name
    r = R.ratio(got, ref, vmax)
    print(f"{name}: max |out - ref| / max|latent| = {r:.5f} (TOL_mla {R.TOL_mla})")
    assert r <= R.TOL_mla, (name, r)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("slot_dtype", (torch.int32, torch.int64))
def test_append_bytes(dtype, slot_dtype):
    """kv_c and k_pe as slices of one fused (T, 600) tensor; slots -1 and beyond the cache leave the 0xA5 the cache was filled with; int32 slots
    run the round-to-nearest-even encoder, int64 slots the reference one"""
    rne = slot_dtype is torch.int32
    T, bs, nb = 70, 16, 6
    rng = np.random.default_rng(11)
    fused = torch.from_numpy(rng.standard_normal((T, 600)).astype(np.float32)).to(TORCH[dtype])
    scale = np.array([fused.float().abs().max().item() / 448.0], np.float32)
    slots = rng.permutation(nb * bs)[:T].astype(np.int64)
    slots[[3, 40]] = -1, nb * bs
    want = np.full((nb * bs, R.ROW), 0xA5, np.uint8)
    keep = (slots >= 0) & (slots < nb * bs)
    want[slots[keep]] = R.quantise(np.concatenate([fused[:, 8:520].float().numpy(), fused[:, 530:594].float().numpy()], axis=1), scale, rne)[keep]
    cache = torch.full((nb, bs, R.ROW), 0xA5, dtype=torch.uint8, device=DEV)
    dev = fused.to(DEV)
    N.fp8_mla_cache_append(dev[:, 8:520], dev[:, 530:594], cache, torch.from_numpy(slots).to(DEV, slot_dtype), torch.from_numpy(scale).to(DEV),
                           L.ENC_RNE if rne else L.ENC_REFERENCE)
    assert np.array_equal(cache.cpu().numpy().reshape(-1, R.ROW), want)
    assert tuple(N.fp8_mla_cache_alloc(3, 32, device=DEV).shape) == (3, 32, R.ROW)


@pytest.mark.parametrize("name", [n for n in R.NAMES if not n.startswith("graph")])
def test_within_tol_of_the_float64_reference(name):
    c = R.case(name)[0]
    out = run(c)
    within_tol(out, name)
    assert not out[torch.from_numpy(c.seq_lens == 0)].any(), "seq_len == 0 gives a zero row"


def test_the_librarys_split_choice_is_the_forced_count_bit_for_bit():
    c = R.case("splits=3 L=400")[0]
    lib, B, Hq = L.load(), 1, c.q.shape[1]
    n = lib.fp8mi_mla_attention_splits(B, Hq, R.SPLIT_MAX_SEQ, 1 << 62)
    assert n == R.auto_splits(B, Hq, R.SPLIT_MAX_SEQ, 1 << 62, torch.cuda.get_device_properties(0).multi_processor_count) and n > 1
    assert lib.fp8mi_mla_attention_workspace_bytes(B, Hq, n) == B * Hq * n * (R.LATENT + 2) * 4
    with L.kernel_timer(4) as kt:
        auto = run(c, num_splits=0)
    assert len(kt.ms) == 2 and torch.equal(bits(auto), bits(run(c, num_splits=n)))


def test_nothing_at_or_beyond_seq_len_moves_the_output():
    c = R.case("mixed")[0]
    clean = run(c)
    bs = c.block_size
    cache, table = np.full_like(c.cache, 0x7F), c.block_table.copy()   # NaN bytes everywhere: unreferenced blocks, the tails of last blocks
    for b, s in enumerate(c.slots):
        cache.reshape(-1, R.ROW)[s] = c.cache.reshape(-1, R.ROW)[s]
        table[b, (int(c.seq_lens[b]) + bs - 1) // bs:] = -1
    assert (cache == 0x7F).sum() > 2 * bs * R.ROW   # the two spare blocks whole, and the tails of the last blocks
    assert torch.equal(bits(clean), bits(run(c, cache=cache, table=table)))


def test_graph_replay_on_new_lengths_table_and_cache():
    first, second = R.graph_cases()

    def tensors(c):
        table = np.full((2, R.GRAPH_MAX_BLOCKS), -1, np.int32)
        table[:, :c.block_table.shape[1]] = c.block_table
        return [torch.from_numpy(x) for x in (c.q[..., :R.LATENT].copy(), c.q[..., R.LATENT:].copy(), c.cache, table, c.seq_lens, c.kv_scale)]

    ql, qp, cache, table, lens, scale = held = [x.to(DEV) for x in tensors(first)]
    call = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, scale, R.SOFTMAX_SCALE, max_seq_len=R.GRAPH_MAX_SEQ, num_splits=1)   # noqa: E731
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    within_tol(out.cpu(), "graph 0")
    for dst, src in zip(held, tensors(second)):
        dst.copy_(src)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().clone()
        assert torch.equal(bits(replayed), bits(call().cpu()))
    within_tol(replayed, "graph 1")
