"""fp8mi_paged_attention_varlen / fp8_paged_attention(cu_seqlens_q=) on the GPU.  The main comparison needs no tolerance: out[t] equals
fp8mi_paged_attention_decode on the expansion of tests/paged_attn_varlen_ref.py - one sequence per query token, seq_len = its causal limit -
BIT FOR BIT (NaNs as NaNs), with the same max_seq_len and the same forced num_splits, on every case of VARLEN_CASES and nothing left out.
Every output is also within TOL_varlen max|V| of the float64 reference of the expansion, over every element.  Outputs lie between guards, in
rows with sentinel padding behind them, pre-filled with the sentinel; the launch count (1 unsplit, 2 split) is checked on every run."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import paged_attn_ref as R
import paged_attn_varlen_ref as V
from moe_route_gpu_util import DEV, SENT_B, SENT_F, bits, equal_bits_or_both_nan, guarded, guards_intact, stream

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}
PAD = 32   # sentinel elements behind every output row


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


class Device:
    """a varlen case's tensors on the device; extra_rows: q rows behind cu[B] that no sequence owns; q_pad: a strided q"""

    def __init__(self, c, extra_rows=0, q_pad=0):
        T, Hq, D = c.q.shape
        self.T = T + extra_rows
        self.q_buf = torch.full((self.T, Hq * D + q_pad), 77.0, dtype=TORCH[c.q_dtype], device=DEV)
        self.q_buf[:T, :Hq * D] = torch.from_numpy(c.q).reshape(T, Hq * D).to(TORCH[c.q_dtype])
        self.kc, self.vc = torch.from_numpy(c.k_cache).to(DEV), torch.from_numpy(c.v_cache).to(DEV)
        self.table = torch.from_numpy(c.block_table).to(DEV)
        self.lens = torch.from_numpy(c.seq_lens).to(DEV)
        self.cu = torch.from_numpy(c.cu).to(DEV)
        self.ks, self.vs = torch.from_numpy(c.k_scale).to(DEV), torch.from_numpy(c.v_scale).to(DEV)


def launch(lib, c, dev, rows, num_splits, call):
    """`call(ws, ws_bytes, out, ld_out)` -> rc, with a guarded workspace and a guarded, sentinel-filled out of `rows` query rows ->
    (rows, Hq, D) on the CPU in the case's out_dtype; guards, padding and the launch count checked"""
    _T, Hq, D = c.q.shape
    ld_out = Hq * D + PAD
    out_buf, out = guarded(rows * ld_out, TORCH[c.out_dtype], SENT_F)
    need = lib.fp8mi_paged_attention_workspace_bytes(rows, Hq, D, num_splits)
    assert (need == 0) == (num_splits == 1)
    ws_buf, ws = guarded(max(need, 16), torch.uint8, SENT_B)
    with L.kernel_timer(4) as kt:
        rc = call(ws.data_ptr() if need else None, need, out.data_ptr(), ld_out)
    assert rc == 0, lib.fp8mi_last_error()
    torch.cuda.synchronize()
    assert guards_intact(out_buf, rows * ld_out, SENT_F) and guards_intact(ws_buf, max(need, 16), SENT_B)
    got = out.reshape(rows, ld_out).cpu()
    assert bool((got[:, Hq * D:] == SENT_F).all()), "the padding behind an output row was written"
    return got[:, :Hq * D].reshape(rows, Hq, D), len(kt.ms)


def cache_args(c, dev, table, lens, num_splits):
    nb, _Hkv, bs, _ = c.k_cache.shape
    return (dev.kc.data_ptr(), dev.vc.data_ptr(), nb, bs, table.data_ptr(), table.stride(0), table.shape[1], lens.data_ptr(), c.max_seq_len,
            dev.ks.data_ptr(), dev.vs.data_ptr(), L.KV_SCALE_HEAD if c.k_scale.size > 1 else L.KV_SCALE_TENSOR, c.softmax_scale, num_splits)


def run_varlen(lib, c, dev=None, num_splits=None, max_q_len=None):
    """one fp8mi_paged_attention_varlen of the case -> out (dev.T, Hq, D): rows the call did not write hold the sentinel"""
    dev = Device(c) if dev is None else dev
    ns = c.num_splits if num_splits is None else num_splits
    _T, Hq, D = c.q.shape
    out, launches = launch(lib, c, dev, dev.T, ns, lambda ws, ws_bytes, out, ld_out: lib.fp8mi_paged_attention_varlen(
        dev.q_buf.data_ptr(), CODE[c.q_dtype], dev.T, len(c.q_lens), dev.cu.data_ptr(), c.max_q_len if max_q_len is None else max_q_len, Hq, c.Hkv, D,
        dev.q_buf.stride(0), *cache_args(c, dev, dev.table, dev.lens, ns), ws, ws_bytes, out, CODE[c.out_dtype], ld_out, stream()))
    assert ns == 0 or launches == (1 if ns == 1 else 2), (launches, ns)
    return out


def run_expanded(lib, c, e, dev, num_splits=None):
    """fp8mi_paged_attention_decode on the expansion, over the SAME device caches and q rows -> (T, Hq, D)"""
    ns = c.num_splits if num_splits is None else num_splits
    T, Hq, D = c.q.shape
    table, lens = torch.from_numpy(e.block_table).to(DEV), torch.from_numpy(e.seq_lens).to(DEV)
    out, launches = launch(lib, c, dev, T, ns, lambda ws, ws_bytes, out, ld_out: lib.fp8mi_paged_attention_decode(
        dev.q_buf.data_ptr(), CODE[c.q_dtype], T, Hq, c.Hkv, D, dev.q_buf.stride(0), *cache_args(c, dev, table, lens, ns), ws, ws_bytes, out, CODE[c.out_dtype],
        ld_out, stream()))
    assert launches == (1 if ns == 1 else 2)
    return out


def within_tol(out, ref, vmax, what):
    got = out.double().numpy()
    assert not np.isnan(got).any(), what
    r = R.ratio(got, ref, vmax)
    print(f"{what}: max |out - ref| / max|V| = {r:.5f} (TOL_varlen {V.TOL_varlen})")
    assert r <= V.TOL_varlen, (what, r)


@pytest.mark.parametrize("name", V.VARLEN_CASES)
def test_equals_decode_on_the_expansion_bit_for_bit(lib, name):
    """mapping (every G, TQ - 1 .. 2 TQ + 1 tokens), step / pass / split / block edges, prefill into an empty cache, zero rows, q_len = 0
    and seq_len = 0 in a batch, the mixed batch, the long shaped cases, dtypes, per-head scales, all q_len = 1"""
    c, e, ref, vmax = V.varlen_case(name)
    dev = Device(c)
    out = run_varlen(lib, c, dev)
    want = run_expanded(lib, c, e, dev)
    assert out.numel() > 0 and tuple(out.shape) == tuple(want.shape) == c.q.shape
    assert equal_bits_or_both_nan(out, want), (name, int((bits(out) != bits(want)).sum()))
    within_tol(out, ref, vmax, name)
    assert not out[torch.from_numpy(e.seq_lens == 0)].any(), "a row without a visible position is zero"


def test_q_as_a_strided_slice_of_a_fused_qkv(lib):
    c, e, ref, vmax = V.varlen_case("dtypes bf16->bf16")
    plain = run_varlen(lib, c)
    dev = Device(c, q_pad=2 * c.Hkv * c.D)   # q, k, v of a token side by side: ld_q = (Hq + 2 Hkv) D
    strided = run_varlen(lib, c, dev)
    assert dev.q_buf.stride(0) == (c.q.shape[1] + 2 * c.Hkv) * c.D and torch.equal(bits(plain), bits(strided))
    assert equal_bits_or_both_nan(strided, run_expanded(lib, c, e, dev))
    within_tol(strided, ref, vmax, "strided q")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("num_splits", (0, 1, 3))
def test_one_token_per_sequence_is_the_decode_entry(lib, num_splits):
    """cu = 0 .. B: the same inputs through both entries, the same bits; at num_splits = 0 the two split choices coincide (3, here)"""
    c = V.make_varlen_case(29500, [1300, 700, 1], [1, 1, 1], 16, 128, 8, 2, num_splits=num_splits)
    assert tuple(c.cu) == (0, 1, 2, 3) and c.max_q_len == 1
    T, Hq, D = c.q.shape
    full = lib.fp8mi_paged_attention_workspace_bytes(T, Hq, D, 0)
    if num_splits == 0:
        assert lib.fp8mi_paged_attention_varlen_splits(T, T, 1, Hq, c.Hkv, D, c.max_seq_len, full) == R.auto_splits(T, Hq, c.Hkv, D, c.max_seq_len, full, cus()) == 3
    dev = Device(c)
    out = run_varlen(lib, c, dev)
    want = run_expanded(lib, c, c, dev)   # its own expansion: the decode entry on the very same table and seq_lens
    assert equal_bits_or_both_nan(out, want) and not np.isnan(out.double().numpy()).any()


@pytest.mark.parametrize("name", ("mixed batch splits=1", "long rising splits=1"))
def test_the_librarys_split_choice_is_the_restated_one(lib, name):
    c, _e, _ref, _vmax = V.varlen_case(name)
    T, Hq, D = c.q.shape
    full = lib.fp8mi_paged_attention_workspace_bytes(T, Hq, D, 0)
    chosen = V.auto_splits_varlen(T, len(c.q_lens), c.max_q_len, Hq, c.Hkv, D, c.max_seq_len, full, cus())
    assert chosen == lib.fp8mi_paged_attention_varlen_splits(T, len(c.q_lens), c.max_q_len, Hq, c.Hkv, D, c.max_seq_len, full)
    assert chosen == (1 if name.startswith("mixed") else 3)   # 300 positions: three steps, no split; 1300: 11 steps, a step per wave
    dev = Device(c)
    assert torch.equal(bits(run_varlen(lib, c, dev, num_splits=0)), bits(run_varlen(lib, c, dev, num_splits=chosen)))


@pytest.mark.parametrize("num_splits", (1, 3))
def test_rows_nobody_owns_are_not_written(lib, num_splits):
    """T = cu[B] + 3 (the padding of a captured shape) and max_q_len = 7 below the last sequence's 33 tokens: the padding rows and that
    sequence's tokens 7 .. 32 keep the sentinel, every other row is the full call's, in the one-launch form and through the combine"""
    c, _e, _ref, _vmax = V.varlen_case(f"mixed batch splits={num_splits}")
    assert tuple(c.q_lens) == V.MIXED_Q and c.num_splits == num_splits
    full = run_varlen(lib, c)
    dev = Device(c, extra_rows=3)
    out = run_varlen(lib, c, dev, max_q_len=7)
    T = c.q.shape[0]
    owned = np.zeros(T + 3, bool)
    for b, n in enumerate(c.q_lens):
        owned[c.cu[b]:c.cu[b] + min(int(n), 7)] = True
    assert owned.sum() == 1 + 0 + 7 + 1 + 7 and not owned[T:].any()
    owned = torch.from_numpy(owned)
    assert bool((out[~owned] == SENT_F).all()), "a row no sequence owns, or one at or beyond max_q_len, was written"
    assert torch.equal(bits(out[owned]), bits(full[owned[:T]])) and not bool((full == SENT_F).any())
    # and a max_q_len above T is T
    assert torch.equal(bits(run_varlen(lib, c, max_q_len=10 ** 6)), bits(full))


GARBAGE_SEQ, GARBAGE_Q, NAN_POS = (100, 60), (10, 3), 95   # G = 4: tiles of 4 tokens; limits of sequence 0: 91 .. 100


def garbage_case(num_splits):
    """every byte outside [0, seq_len) random, the NaN patterns among them; table entries past the need stay -1"""
    c = V.make_varlen_case(29700, list(GARBAGE_SEQ), list(GARBAGE_Q), 16, 128, 8, 2, num_splits=num_splits, spare_blocks=3)
    rng = np.random.default_rng(2)
    for cache, owned in ((c.k_cache, c.k_owned), (c.v_cache, c.v_owned)):
        junk = rng.integers(0, 256, cache.shape, dtype=np.uint8)
        junk.reshape(-1)[::7] = 0xFF
        junk.reshape(-1)[3::11] = 0x7F
        cache[~owned] = junk[~owned]
    need = (c.seq_lens + 15) // 16
    assert all((c.block_table[b, need[b]:] == -1).all() for b in range(2)) and (c.seq_lens % 16 != 0).all() and not c.k_owned.all()
    return c


@pytest.mark.parametrize("num_splits", (1, 2))
def test_garbage_and_k_nan_beyond_a_rows_limit(lib, num_splits):
    """On the dirty cache the output is the expansion's and NaN-free.  Then NaN bytes of K at position 95 of sequence 0, inside
    [limit_0, seq_len) = [91, 100): tokens 0 .. 4 (limits 91 .. 95) stay finite and equal - token 4 shares its tile with tokens whose
    scores are NaN there -, tokens 5 .. 9 are NaN, as in the expansion on the same cache; sequence 1 does not move."""
    c = garbage_case(num_splits)
    e = V.expand(c)
    dev = Device(c)
    clean = run_varlen(lib, c, dev)
    assert equal_bits_or_both_nan(clean, run_expanded(lib, c, e, dev)) and not np.isnan(clean.double().numpy()).any()
    ref, vmax = R.attention_ref(e)
    assert R.ratio(clean.double().numpy(), ref, vmax) <= V.TOL_varlen   # N(0, 1) data of the table's kind; the bound is the table's
    blk, off = int(c.block_table[0, NAN_POS // 16]), NAN_POS % 16
    dev.kc[blk, :, off, 5] = 0x7F
    dev.kc[blk, :, off, 70] = 0xFF
    out, want = run_varlen(lib, c, dev), run_expanded(lib, c, e, dev)
    assert equal_bits_or_both_nan(out, want)
    nan_rows = out.isnan().all(dim=2).all(dim=1)
    assert nan_rows.tolist() == [False] * 5 + [True] * 5 + [False] * 3 and not out[~nan_rows].isnan().any()
    assert torch.equal(bits(out[~nan_rows]), bits(clean[~nan_rows]))


@pytest.mark.parametrize("num_splits", (1, 2))
def test_one_v_nan_byte_beyond_a_rows_limit(lib, num_splits):
    """One NaN byte of V at position 95, KV head 0, channel 9.  Rows with limit above 95 (tokens 5 .. 9, the heads of KV head 0) are NaN in
    that channel, as in the expansion.  Token 4 (limit 95) sits in the tile of tokens 4 .. 7, whose columns share one V operand: its four
    heads of KV head 0 are the documented exception and the ONLY rows left out.  Tile 0 (limits up to 94) never reads the byte; KV head 1
    and sequence 1 do not see it: all equal to the expansion."""
    c = garbage_case(num_splits)
    e = V.expand(c)
    dev = Device(c)
    blk, off = int(c.block_table[0, NAN_POS // 16]), NAN_POS % 16
    dev.vc[blk, 0, 9, off] = 0x7F
    out, want = run_varlen(lib, c, dev), run_expanded(lib, c, e, dev)
    compared = torch.ones(out.shape[:2], dtype=torch.bool)
    compared[4, :4] = False
    assert int((~compared).sum()) == 4
    assert equal_bits_or_both_nan(out[compared], want[compared])
    nan = out.isnan()
    assert bool(nan[5:10, :4, 9].all()) and int(nan[compared].sum()) == 5 * 4, "exactly the rows with limit above the byte, in its channel"
    assert not want[4].isnan().any()   # the definition leaves token 4 clean; the kernel may not (0 x NaN in the shared operand)


@pytest.mark.parametrize("num_splits", (1, 2))
def test_graph_replay_on_new_cu_lengths_table_and_cache(lib, N_, num_splits):
    """fp8_paged_attention(cu_seqlens_q=) captured at one (T, B, max_q_len, max_seq_len) and replayed after cu, seq_lens, q, the table and
    both caches changed in place - the second batch owns 7 of the 8 rows -: the owned rows are bit-equal to the eager call on the same
    data and to the decode call on the expansion; nothing was read on the host."""
    T, B, MAXQ = 8, 2, 8
    first = V.make_varlen_case(29800, [33, 140], [3, 5], 16, 128, 4, 2, num_splits=num_splits, spare_blocks=4)
    second = V.make_varlen_case(29801, [150, 9], [6, 1], 16, 128, 4, 2, num_splits=num_splits, spare_blocks=5)
    for c in (first, second):
        assert c.k_cache.shape[0] == 16 and c.block_table.shape[1] <= R.GRAPH_MAX_BLOCKS

    def padded(table):
        t = np.full((table.shape[0], R.GRAPH_MAX_BLOCKS), -1, np.int32)
        t[:, :table.shape[1]] = table
        return torch.from_numpy(t)

    def q_rows(c):
        q = torch.zeros((T,) + c.q.shape[1:])
        q[:c.q.shape[0]] = torch.from_numpy(c.q)
        return q

    q, cu = q_rows(first).to(DEV), torch.from_numpy(first.cu).to(DEV)
    kc, vc = torch.from_numpy(first.k_cache).to(DEV), torch.from_numpy(first.v_cache).to(DEV)
    table, lens = padded(first.block_table).to(DEV), torch.from_numpy(first.seq_lens).to(DEV)
    ks, vs = torch.from_numpy(first.k_scale).to(DEV), torch.from_numpy(first.v_scale).to(DEV)
    ws = torch.empty(max(lib.fp8mi_paged_attention_workspace_bytes(T, 4, 128, num_splits), 16), dtype=torch.uint8, device=DEV)
    call = lambda: N_.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=R.GRAPH_MAX_SEQ, num_splits=num_splits, workspace=ws,   # noqa: E731
                                          cu_seqlens_q=cu, max_q_len=MAXQ)

    def expanded(c):
        e = V.expand(c)
        n = e.q.shape[0]
        return N_.fp8_paged_attention(q[:n], kc, vc, padded(e.block_table).to(DEV), torch.from_numpy(e.seq_lens).to(DEV), ks, vs,
                                      max_seq_len=R.GRAPH_MAX_SEQ, num_splits=num_splits, workspace=ws).cpu()

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().clone()
    assert tuple(got.shape) == (T, 4, 128) and torch.equal(bits(got), bits(call().cpu())) and torch.equal(bits(got), bits(expanded(first)))
    q.copy_(q_rows(second))
    cu.copy_(torch.from_numpy(second.cu))
    kc.copy_(torch.from_numpy(second.k_cache))
    vc.copy_(torch.from_numpy(second.v_cache))
    table.copy_(padded(second.block_table))
    lens.copy_(torch.from_numpy(second.seq_lens))
    ks.copy_(torch.from_numpy(second.k_scale))
    vs.copy_(torch.from_numpy(second.v_scale))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().clone()
    n = second.q.shape[0]
    assert n == 7 and torch.equal(bits(replayed[:n]), bits(call().cpu()[:n])) and torch.equal(bits(replayed[:n]), bits(expanded(second)))
    assert torch.equal(bits(replayed[n:]), bits(got[n:])), "the row the second batch does not own was written"
    ref, vmax = R.attention_ref(V.expand(second))
    assert not replayed[:n].isnan().any() and R.ratio(replayed[:n].double().numpy(), ref, vmax) <= V.TOL_varlen
