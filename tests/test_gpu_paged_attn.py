"""fp8mi_paged_attention_decode / fp8_paged_attention on the GPU against the float64 reference (a) of tests/paged_attn_ref.py.  Every
comparison is |out - ref| <= TOL * max|dequantised V of that sequence and KV head| over every element (TOL = 2 E, E measured on the CPU
and pinned by tests/test_paged_attn_host.py); each test prints the ratio it reached before it asserts.  Every output lies between guard
elements, in rows with sentinel padding behind them; the launch count (1 unsplit, 2 split) is checked on every run.  The cases are
paged_attn_ref.all_cases(): milliseconds each, the smallest lengths on both sides of a block, of an S tile and of a 128-position step."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import paged_attn_ref as R
from moe_route_gpu_util import DEV, SENT_B, SENT_F, bits, guarded, guards_intact, stream

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}
PAD = 32   # sentinel elements behind every (sequence's) output row


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


class Device:
    """a case's tensors on the device"""

    def __init__(self, c, q_pad=0):
        B, Hq, D = c.q.shape
        self.q_buf = torch.full((B, Hq * D + q_pad), 77.0, dtype=TORCH[c.q_dtype], device=DEV)   # q_pad: a strided q
        self.q_buf[:, :Hq * D] = torch.from_numpy(c.q).reshape(B, Hq * D).to(TORCH[c.q_dtype])
        self.kc, self.vc = torch.from_numpy(c.k_cache).to(DEV), torch.from_numpy(c.v_cache).to(DEV)
        self.table = torch.from_numpy(c.block_table).to(DEV)
        self.lens = torch.from_numpy(c.seq_lens).to(DEV)
        self.ks, self.vs = torch.from_numpy(c.k_scale).to(DEV), torch.from_numpy(c.v_scale).to(DEV)


def run_decode(lib, c, dev=None, q_pad=0):
    """one fp8mi_paged_attention_decode of the case -> out (B, Hq, D) on the CPU in the case's out_dtype; guards, padding and launches checked"""
    dev = Device(c, q_pad) if dev is None else dev
    B, Hq, D = c.q.shape
    nb, Hkv, bs, _ = c.k_cache.shape
    ld_out = Hq * D + PAD
    out_buf, out = guarded(B * ld_out, TORCH[c.out_dtype], SENT_F)
    need = lib.fp8mi_paged_attention_workspace_bytes(B, Hq, D, c.num_splits)
    assert (need == 0) == (c.num_splits == 1)
    ws_buf, ws = guarded(max(need, 16), torch.uint8, SENT_B)
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_paged_attention_decode(dev.q_buf.data_ptr(), CODE[c.q_dtype], B, Hq, Hkv, D, dev.q_buf.stride(0), dev.kc.data_ptr(), dev.vc.data_ptr(), nb,
                                              bs, dev.table.data_ptr(), dev.table.stride(0), dev.table.shape[1], dev.lens.data_ptr(), c.max_seq_len,
                                              dev.ks.data_ptr(), dev.vs.data_ptr(), L.KV_SCALE_HEAD if c.k_scale.size > 1 else L.KV_SCALE_TENSOR,
                                              c.softmax_scale, c.num_splits, ws.data_ptr() if need else None, need, out.data_ptr(), CODE[c.out_dtype],
                                              ld_out, stream())
    L.check(rc, "fp8mi_paged_attention_decode")
    torch.cuda.synchronize()
    assert len(kt.ms) == (1 if c.num_splits == 1 else 2), (len(kt.ms), c.num_splits)
    assert guards_intact(out_buf, B * ld_out, SENT_F) and guards_intact(ws_buf, max(need, 16), SENT_B)
    rows = out.reshape(B, ld_out).cpu()
    assert bool((rows[:, Hq * D:] == SENT_F).all()), "the padding behind an output row was written"
    return rows[:, :Hq * D].reshape(B, Hq, D)


def check(out, c, what):
    """every element against the float64 reference (a); rows of an empty sequence are exactly zero"""
    ref, vmax = R.attention_ref(c)
    got = out.double().numpy()
    assert not np.isnan(got).any(), what
    r = R.ratio(got, ref, vmax)
    print(f"{what}: max |out - ref| / max|V| = {r:.5f} (TOL {R.TOL})")
    assert r <= R.TOL, (what, r)
    empty = c.seq_lens == 0
    assert not out[torch.from_numpy(empty)].any()


@pytest.mark.parametrize("L_,bs,D", R.GRID)
def test_lengths_block_sizes_and_head_dims(lib, L_, bs, D):
    c = R.grid_case(L_, bs, D)
    check(run_decode(lib, c), c, f"L={L_} bs={bs} D={D}")


@pytest.mark.parametrize("g,Hkv", R.GROUPS)
def test_query_groups_and_padded_columns(lib, g, Hkv):
    """Hq / Hkv query heads fill g of the tile's 16 columns: the others' results are never stored (guards, padding, and every element of
    the neighbouring heads against the reference)"""
    c = R.group_case(g, Hkv)
    check(run_decode(lib, c), c, f"group={g} Hkv={Hkv}")


@pytest.mark.parametrize("splits", (1, 3))
def test_mixed_lengths_zero_row_and_splits_that_own_nothing(lib, splits):
    c = R.mixed_case(splits)
    assert tuple(c.seq_lens) == R.MIXED_LENS and R.chunk_of(c.max_seq_len, 3) == 128   # split 1 and 2 own nothing of the lengths 1 and 37
    out = run_decode(lib, c)
    check(out, c, f"mixed lengths, splits={splits}")
    assert not bits(out[0]).any(), "seq_len == 0 is a row of +0.0"


@pytest.mark.parametrize("splits", R.SPLITS)
def test_forced_splits(lib, splits):
    c = R.split_case(splits)
    check(run_decode(lib, c), c, f"L=300 splits={splits}")


def test_shuffled_table_with_minus_one_past_the_need(lib):
    c = R.mixed_case(1)
    t = c.block_table
    used = np.concatenate([t[b][t[b] >= 0] for b in range(len(t))])
    assert len(set(used.tolist())) == len(used), "a physical block is shared"
    assert (np.diff(t[2][t[2] >= 0]) < 0).any() and (np.diff(t[2][t[2] >= 0]) > 0).any(), "the table is monotonic"
    for b, n in enumerate(c.seq_lens):
        assert (t[b, (n + 15) // 16:] == -1).all() and (t[b, :(n + 15) // 16] >= 0).all()
    check(run_decode(lib, c), c, "shuffled table")


@pytest.mark.parametrize("splits", (1, 2))
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_garbage_immunity(lib, D, splits):
    """Every byte of both caches that holds no position below its sequence's length - the tail of the last block, unreferenced blocks,
    blocks the table names beyond the need - filled with the NaN pattern 0x7F, then with random bytes (0xFF and 0x7F among them): the two
    outputs are bit-identical, NaN-free and within TOL of the reference."""
    c = R.garbage_case(D, splits)
    need = (c.seq_lens + c.block_size - 1) // c.block_size
    assert all((c.block_table[b, need[b]:] >= 0).all() for b in range(2)) and not c.k_owned.all() and (c.seq_lens % c.block_size != 0).all()
    rng = np.random.default_rng(1)
    outs = []
    for fill in ("nan", "random"):
        for cache, owned in ((c.k_cache, c.k_owned), (c.v_cache, c.v_owned)):
            junk = np.full(cache.shape, 0x7F, np.uint8) if fill == "nan" else rng.integers(0, 256, cache.shape, dtype=np.uint8)
            if fill == "random":
                junk.reshape(-1)[::7] = 0xFF
            cache[~owned] = junk[~owned]
        outs.append(run_decode(lib, c))
        check(outs[-1], c, f"garbage ({fill}) D={D} splits={splits}")
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_dominant_key_keeps_the_small_probabilities(lib):
    """One key 7 to 9 above 255 others in the scaled logits: their probabilities (e^-8 each, a twelfth of the mass together) are below
    e4m3's subnormals relative to the dominant one and survive only through the 2^8 scale of P."""
    c = R.dominant_case()
    ref_logits = []
    for h in range(c.Hkv):
        kb, _ = R.gather(c, 0, h)
        ref_logits.append((R.LUT64[kb] * float(c.k_scale[0])) @ c.q[0, h].astype(np.float64) * c.softmax_scale)
    for s in ref_logits:
        gap = s[0] - s[1:]
        assert 6.5 < gap.min() and gap.max() < 9.5, (gap.min(), gap.max())
    check(run_decode(lib, c), c, "dominant key")


@pytest.mark.parametrize("od", R.DTYPES)
@pytest.mark.parametrize("qd", R.DTYPES)
def test_every_q_and_output_dtype(lib, qd, od):
    c = R.dtype_case(qd, od)
    check(run_decode(lib, c), c, f"{qd} -> {od}")


def test_strided_q(lib):
    c = R.dtype_case("bf16", "f32")
    plain = run_decode(lib, c)
    strided = run_decode(lib, c, q_pad=24)
    assert torch.equal(bits(plain), bits(strided))
    check(strided, c, "strided q")


def test_per_head_scales(lib):
    c = R.per_head_case()
    assert c.k_scale.size == c.Hkv and len(set(c.v_scale.tolist())) == c.Hkv
    check(run_decode(lib, c), c, "per-head scales")


@pytest.mark.parametrize("splits", (1, 2))
def test_graph_replay_on_new_lengths_table_and_cache(lib, N_, splits):
    """fp8_paged_attention captured into a torch.cuda.graph on one case, replayed after seq_lens, the table, q and both caches changed in
    place: bit-equal to the eager call on the same data (and within TOL of the reference); nothing was read on the host."""
    first, second = R.graph_cases(splits)

    def padded(table):
        t = np.full((2, R.GRAPH_MAX_BLOCKS), -1, np.int32)
        t[:, :table.shape[1]] = table
        return torch.from_numpy(t)

    q = torch.from_numpy(first.q).to(DEV)
    kc, vc = torch.from_numpy(first.k_cache).to(DEV), torch.from_numpy(first.v_cache).to(DEV)
    table, lens = padded(first.block_table).to(DEV), torch.from_numpy(first.seq_lens).to(DEV)
    ks, vs = torch.from_numpy(first.k_scale).to(DEV), torch.from_numpy(first.v_scale).to(DEV)
    # the split workspace is the caller's here: the op layer keeps its own per stream, and the capture runs on a stream of its own
    ws = torch.empty(max(lib.fp8mi_paged_attention_workspace_bytes(2, 4, 128, splits), 16), dtype=torch.uint8, device=DEV)
    call = lambda: N_.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=R.GRAPH_MAX_SEQ, num_splits=splits, workspace=ws)   # noqa: E731
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    check(out.cpu(), first, f"graph, first data, splits={splits}")
    assert torch.equal(bits(out.cpu()), bits(call().cpu()))
    q.copy_(torch.from_numpy(second.q))
    kc.copy_(torch.from_numpy(second.k_cache))
    vc.copy_(torch.from_numpy(second.v_cache))
    table.copy_(padded(second.block_table))
    lens.copy_(torch.from_numpy(second.seq_lens))
    ks.copy_(torch.from_numpy(second.k_scale))
    vs.copy_(torch.from_numpy(second.v_scale))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().clone()
    check(replayed, second, f"graph, replayed on new data, splits={splits}")
    assert torch.equal(bits(replayed), bits(call().cpu()))


def test_op_layer_append_token_by_token_then_attend(lib, N_):
    """fp8_kv_cache_append for 40 steps, one token each, with fp8_paged_attention on the cache so far at steps 1, 16, 17 and 40"""
    full = R.append_case(R.APPEND_STEPS)
    nb, Hkv, bs, D = full.k_cache.shape
    kc, vc = N_.fp8_kv_cache_alloc(nb, bs, Hkv, D, device=DEV)
    k, v = torch.from_numpy(full.k_values[0]).float().to(DEV), torch.from_numpy(full.v_values[0]).float().to(DEV)
    slots = torch.from_numpy(full.slots[0]).to(DEV)
    q, table = torch.from_numpy(full.q).to(DEV), torch.from_numpy(full.block_table).to(DEV)
    ks, vs = torch.from_numpy(full.k_scale).to(DEV), torch.from_numpy(full.v_scale).to(DEV)
    for t in range(R.APPEND_STEPS):
        N_.fp8_kv_cache_append(k[t:t + 1], v[t:t + 1], kc, vc, slots[t:t + 1], ks, vs, encode_mode=L.ENC_RNE)
        if t + 1 in R.APPEND_AT:
            c = R.append_case(t + 1)
            lens = torch.tensor([t + 1], dtype=torch.int32, device=DEV)
            out = N_.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=R.APPEND_STEPS, num_splits=1)
            assert out.dtype == torch.float32 and tuple(out.shape) == (1, 4, D)
            check(out.cpu(), c, f"append, step {t + 1}")
    assert torch.equal(kc.cpu(), torch.from_numpy(full.k_cache)) and torch.equal(vc.cpu(), torch.from_numpy(full.v_cache))
    # the defaults: the bound is what the table can name, the library chooses the splits (one, at this length) - the same bits
    lens = torch.tensor([R.APPEND_STEPS], dtype=torch.int32, device=DEV)
    assert torch.equal(bits(N_.fp8_paged_attention(q, kc, vc, table, lens, ks, vs).cpu()), bits(out.cpu()))
