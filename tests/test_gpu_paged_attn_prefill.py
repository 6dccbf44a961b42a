"""fp8mi_paged_attention_prefill / fp8_paged_attention(kernel="tile") on the GPU: every element within TOL_prefill max|V| of the float64
reference of the expansion; guards, sentinel padding and launch counts through the helpers of tests/test_gpu_paged_attn_varlen.py."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import paged_attn_prefill_ref as P
import paged_attn_ref as R
import paged_attn_varlen_ref as V
import test_gpu_paged_attn_varlen as TV
from moe_route_gpu_util import DEV, SENT_F, bits, stream
from test_gpu_paged_attn_varlen import lib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def run_tile(lib, c, dev=None, num_splits=None, max_q_len=None):
    """one fp8mi_paged_attention_prefill of the case -> out (dev.T, Hq, D): rows the call did not write hold the sentinel"""
    dev = TV.Device(c) if dev is None else dev
    ns = c.num_splits if num_splits is None else num_splits
    _T, Hq, D = c.q.shape
    out, launches = TV.launch(lib, c, dev, dev.T, ns, lambda ws, ws_bytes, out, ld_out: lib.fp8mi_paged_attention_prefill(
        dev.q_buf.data_ptr(), TV.CODE[c.q_dtype], dev.T, len(c.q_lens), dev.cu.data_ptr(), c.max_q_len if max_q_len is None else max_q_len, Hq, c.Hkv, D,
        dev.q_buf.stride(0), *TV.cache_args(c, dev, dev.table, dev.lens, ns), ws, ws_bytes, out, TV.CODE[c.out_dtype], ld_out, stream()))
    assert launches == (1 if ns == 1 else 2), (launches, ns)
    return out


def within_tol(out, ref, vmax, what):
    got = out.double().numpy()
    assert not np.isnan(got).any(), what
    r = R.ratio(got, ref, vmax)
    print(f"{what}: max |out - ref| / max|V| = {r:.5f} (TOL_prefill {P.TOL_prefill})")
    assert r <= P.TOL_prefill, (what, r)


@pytest.mark.parametrize("name", P.PREFILL_CASES)
def test_within_tol_of_the_float64_reference(lib, name):
    c, e, ref, vmax = P.prefill_case(name)
    out = run_tile(lib, c)
    within_tol(out, ref, vmax, name)
    assert out.numel() > 0 and tuple(out.shape) == c.q.shape and not out[torch.from_numpy(e.seq_lens == 0)].any(), "a row without a visible position is zero"


def test_the_librarys_own_split_choice_at_a_prompt_sized_T_through_the_op_layer(lib):
    """T = 512 over 640 positions, G = 4: 16 tiles, five steps -> two splits, for which the op layer sizes its own workspace (the decode bound is 0
    bytes); q is a strided slice of a fused qkv; the bits are the forced count's on a contiguous q"""
    import fp8_mi355x_native as N
    c = V.make_varlen_case(37000, [640], [512], 16, 64, 4, 1, q_dtype="bf16", out_dtype="bf16")
    T, Hq, D = c.q.shape
    assert lib.fp8mi_paged_attention_workspace_bytes(T, Hq, D, 0) == 0 and lib.fp8mi_paged_attention_prefill_splits(T, 1, T, Hq, 1, D, 640, 1 << 62) == 2
    dev = TV.Device(c, q_pad=2 * D)   # q, k, v of a token side by side
    forced = run_tile(lib, c, dev, num_splits=2)
    assert dev.q_buf.stride(0) == (Hq + 2) * D and torch.equal(bits(forced), bits(run_tile(lib, c, num_splits=2)))
    with L.kernel_timer(4) as kt:
        out = N.fp8_paged_attention(dev.q_buf[:, :Hq * D].unflatten(1, (Hq, D)), dev.kc, dev.vc, dev.table, dev.lens, dev.ks, dev.vs, max_seq_len=640, kernel="tile",
                                    cu_seqlens_q=dev.cu, max_q_len=T)
    assert len(kt.ms) == 2 and torch.equal(bits(out.cpu()), bits(forced))
    within_tol(forced, *R.attention_ref(V.expand(c)), "T = 512, the library's two splits")


@pytest.mark.parametrize("num_splits", (1, 3))
def test_rows_nobody_owns_are_not_written(lib, num_splits):
    """T = cu[B] + 3, max_q_len = 7 below the last sequence's 33 tokens: padding rows and tokens 7 .. 32 keep the sentinel, the others are the full call's"""
    c = P.prefill_case("mixed batch")[0]
    full = run_tile(lib, c, num_splits=num_splits)
    out = run_tile(lib, c, TV.Device(c, extra_rows=3), num_splits=num_splits, max_q_len=7)
    T = c.q.shape[0]
    owned = np.zeros(T + 3, bool)
    for b, n in enumerate(c.q_lens):
        owned[c.cu[b]:c.cu[b] + min(int(n), 7)] = True
    owned = torch.from_numpy(owned)
    assert int(owned.sum()) == 16 and bool((out[~owned] == SENT_F).all()), "a row no sequence owns, or one at or beyond max_q_len, was written"
    assert torch.equal(bits(out[owned]), bits(full[owned[:T]])) and not bool((full == SENT_F).any())


@pytest.mark.parametrize("num_splits", (1, 2))
def test_nan_bytes_beyond_a_rows_limit_on_a_dirty_cache(lib, num_splits):
    """40 tokens ending at 200, G = 4: workgroup tile 0 = tokens 0 .. 31 (limits 161 .. 192), tile 1 = tokens 32 .. 39 (193 .. 200); the table names dirty
    spare blocks past the need.  V NaN at 195 (KV head 0, channel 9) and at every position >= 200: only tokens 32 .. 34 of tile 1, the documented
    exception, are left out.  Then K NaN at 195 and at every position >= 200: rows with a limit above 195 are NaN, the others keep their bits."""
    c = V.make_varlen_case(37100, [200, 60], [40, 3], 16, 128, 8, 2, num_splits=num_splits, spare_blocks=3, name_spares=True)
    rng = np.random.default_rng(2)
    for cache, owned in ((c.k_cache, c.k_owned), (c.v_cache, c.v_owned)):
        junk = rng.integers(0, 256, cache.shape, dtype=np.uint8)
        junk.reshape(-1)[::7] = 0xFF
        cache[~owned] = junk[~owned]
    dev = TV.Device(c)
    clean = run_tile(lib, c, dev)
    within_tol(clean, *R.attention_ref(V.expand(c)), "dirty cache")
    blk = int(c.block_table[0, 12])   # positions 192 .. 207
    dev.vc[blk, 0, 9, 3] = 0x7F
    dev.vc[blk, :, :, 8:] = 0x7F
    out = run_tile(lib, c, dev)
    same = torch.ones(out.shape[:2], dtype=torch.bool)
    same[32:40, :4] = False   # tile 1, the heads of KV head 0
    assert torch.equal(bits(out[same]), bits(clean[same])) and bool(out[35:40, :4, 9].isnan().all())
    lanes = [d for d in range(128) if d != 9]
    assert torch.equal(bits(out[35:40, :4][:, :, lanes]), bits(clean[35:40, :4][:, :, lanes]))
    dev.kc[blk, :, 3, 5] = 0x7F
    dev.kc[blk, :, 8:, :] = 0xFF
    out = run_tile(lib, c, dev)
    same[35:40] = False
    assert torch.equal(bits(out[same]), bits(clean[same])) and bool(out[35:40].isnan().all())


@pytest.mark.parametrize("num_splits", (1, 2))
def test_graph_replay_on_new_cu_lengths_table_and_cache(lib, num_splits):
    """captured on one batch, replayed once after every input changed in place: owned rows equal the eager call's bits, the unowned row is not written"""
    import fp8_mi355x_native as N
    T = 8
    first = V.make_varlen_case(29800, [33, 140], [3, 5], 16, 128, 4, 2, spare_blocks=4)
    second = V.make_varlen_case(29801, [150, 9], [6, 1], 16, 128, 4, 2, spare_blocks=5)

    def tensors(c):
        table = np.full((2, R.GRAPH_MAX_BLOCKS), -1, np.int32)
        table[:, :c.block_table.shape[1]] = c.block_table
        q = np.zeros((T,) + c.q.shape[1:], np.float32)
        q[:c.q.shape[0]] = c.q
        return [torch.from_numpy(x) for x in (q, c.cu, c.k_cache, c.v_cache, table, c.seq_lens, c.k_scale, c.v_scale)]

    q, cu, kc, vc, table, lens, ks, vs = held = [x.to(DEV) for x in tensors(first)]
    ws = torch.empty(max(lib.fp8mi_paged_attention_workspace_bytes(T, 4, 128, num_splits), 16), dtype=torch.uint8, device=DEV)
    call = lambda: N.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=R.GRAPH_MAX_SEQ, num_splits=num_splits, workspace=ws,   # noqa: E731
                                         kernel="tile", cu_seqlens_q=cu, max_q_len=T)
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
    g.replay()
    torch.cuda.synchronize()
    replayed, n = out.cpu().clone(), second.q.shape[0]
    assert n == 7 and torch.equal(bits(replayed[:n]), bits(call().cpu()[:n])) and torch.equal(bits(replayed[n:]), bits(got[n:]))
    within_tol(replayed[:n], *R.attention_ref(V.expand(second)), "graph replay")
