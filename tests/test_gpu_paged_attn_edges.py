"""fp8mi_paged_attention_decode and fp8mi_kv_cache_append at the edges tests/test_gpu_paged_attn.py does not reach: splits of more than 512
positions (a wave makes a second and a third pass of its loop and the online-softmax rescale acts), softmax scales other than D^-1/2, an
Hkv that is no power of two, the library's own split choice, the clamp of seq_lens, needed table entries out of range, NaN bytes inside a
sequence, query rows scaled by powers of two and rows too small for 448 / amax, cache offsets past 4 GiB.  Numeric comparisons are against
the float64 reference (a) of tests/paged_attn_ref.py, |out - ref| <= TOL_<group> max|dequantised V| over every element with the group's
own TOL (2 E_<group>, pinned by tests/test_paged_attn_host.py); each prints the ratio it reached before it asserts.  Every output lies
between guard elements in rows with sentinel padding behind them, and the launch count is checked on every run."""
import copy

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
INT32_MAX = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    return L.load()


def run_decode(lib, c, num_splits=None, ws_bytes=None, launches=None):
    """one fp8mi_paged_attention_decode of the case -> out (B, Hq, D) on the CPU in the case's out_dtype; guards, padding and launches
    checked.  num_splits: in place of the case's (0: the library chooses); ws_bytes: the workspace handed over, in place of exactly what
    num_splits needs (0: none); launches: the count expected, where num_splits does not say it"""
    num_splits = c.num_splits if num_splits is None else num_splits
    B, Hq, D = c.q.shape
    nb, Hkv, bs, _ = c.k_cache.shape
    q = torch.from_numpy(c.q).reshape(B, Hq * D).to(TORCH[c.q_dtype]).to(DEV)
    kc, vc = torch.from_numpy(c.k_cache).to(DEV), torch.from_numpy(c.v_cache).to(DEV)
    table, lens = torch.from_numpy(c.block_table).contiguous().to(DEV), torch.from_numpy(c.seq_lens).to(DEV)
    ks, vs = torch.from_numpy(c.k_scale).to(DEV), torch.from_numpy(c.v_scale).to(DEV)
    ld_out = Hq * D + PAD
    out_buf, out = guarded(B * ld_out, TORCH[c.out_dtype], SENT_F)
    if ws_bytes is None:
        ws_bytes = lib.fp8mi_paged_attention_workspace_bytes(B, Hq, D, num_splits)
        assert ws_bytes == R.workspace_bytes(B, Hq, D, num_splits) or num_splits == 0
    ws_buf, ws = guarded(max(ws_bytes, 16), torch.uint8, SENT_B)
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_paged_attention_decode(q.data_ptr(), CODE[c.q_dtype], B, Hq, Hkv, D, q.stride(0), kc.data_ptr(), vc.data_ptr(), nb, bs, table.data_ptr(),
                                              table.stride(0), table.shape[1], lens.data_ptr(), c.max_seq_len, ks.data_ptr(), vs.data_ptr(),
                                              L.KV_SCALE_HEAD if c.k_scale.size > 1 else L.KV_SCALE_TENSOR, c.softmax_scale, num_splits,
                                              ws.data_ptr() if ws_bytes else None, ws_bytes, out.data_ptr(), CODE[c.out_dtype], ld_out, stream())
    L.check(rc, "fp8mi_paged_attention_decode")
    torch.cuda.synchronize()
    if launches is None:
        assert num_splits > 0
        launches = 1 if num_splits == 1 else 2
    assert len(kt.ms) == launches, (len(kt.ms), num_splits, ws_bytes)
    assert guards_intact(out_buf, B * ld_out, SENT_F) and guards_intact(ws_buf, max(ws_bytes, 16), SENT_B)
    rows = out.reshape(B, ld_out).cpu()
    assert bool((rows[:, Hq * D:] == SENT_F).all()), "the padding behind an output row was written"
    return rows[:, :Hq * D].reshape(B, Hq, D)


def check(out, c, what, tol, ref=None):
    """every element against the float64 reference (a) within tol max|V|; rows of an empty sequence are exactly zero -> the ratio"""
    ref, vmax = R.attention_ref(c) if ref is None else ref
    got = out.double().numpy()
    assert np.isfinite(got).all(), what
    r = R.ratio(got, ref, vmax)
    print(f"{what}: max |out - ref| / max|V| = {r:.5f} (TOL {tol:.5f})")
    assert r <= tol, (what, r)
    assert not out[torch.from_numpy(np.asarray(c.seq_lens) <= 0)].any()
    return r


def variant(c, **changed):
    """a shallow copy of a shared case with some members replaced: the shared one is never written"""
    v = copy.copy(c)
    v.__dict__.update(changed)
    return v


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- 1. the groups against reference (a) ----------------------------------------------------------------------------------------------------

EDGE = [(g, i) for g, names in R.EDGE_NAMES.items() for i in range(len(names))]


@pytest.mark.parametrize("group,i", EDGE, ids=[f"{g}: {R.EDGE_NAMES[g][i]}" for g, i in EDGE])
def test_edge_groups_against_the_reference(lib, group, i):
    name, c, ref, vmax = R.edge_case(group, i)
    out = run_decode(lib, c)
    check(out, c, f"{group}: {name}", R.EDGE_TOL[group], (ref, vmax))
    if group == "long":
        passes = max(len(R.wave_steps(lo, hi, w)) for lo, hi in R.split_bounds(int(c.seq_lens[0]), c.max_seq_len, c.num_splits) for w in range(R.WAVES))
        assert passes == (3 if c.seq_lens[0] in (1025, 1153) else 2)
    if group == "scales" and c.softmax_scale == 0:   # the mean of V, to the floor derived at R.FLOOR_SCALE0
        assert R.ratio(out.double().numpy(), ref, vmax) <= R.FLOOR_SCALE0
    if group == "tiny_q":   # the rows 448 / amax overflows for, and the all-zero row: every logit is 0, as at scale 0 - the mean of V to that floor
        g = c.q.shape[1] // c.Hkv
        for hq, what in R.TINY_Q_ROWS.items():
            _kb, vb = R.gather(c, 0, hq // g)
            mean = (R.LUT64[vb] * R.head_scale(c.v_scale, hq // g)).mean(axis=0)
            assert np.abs(out[0, hq].double().numpy() - mean).max() <= R.FLOOR_SCALE0 * vmax[0, hq], (hq, what)


# ---- 2. the library's own split choice ------------------------------------------------------------------------------------------------------

def test_auto_split_follows_the_workspace(lib):
    """num_splits = 0 at B = 1, Hkv = 1, max_seq_len = 1300: three splits with the workspace the library asks for, two with a workspace
    that holds two, one launch with none - each bit-equal to the forced call"""
    c = R.make_case(12000, [1300], 64, 128, Hq=4, Hkv=1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = lib.fp8mi_paged_attention_workspace_bytes(1, 4, 128, 0)
    assert full >= R.workspace_bytes(1, 4, 128, 3) and R.auto_splits(1, 4, 1, 128, 1300, full, cus) == 3
    forced = {n: run_decode(lib, c, num_splits=n) for n in (1, 2, 3)}
    assert not same_bits(forced[2], forced[3]) and not same_bits(forced[1], forced[2]), "the split count does not show in the bits: the equalities below prove nothing"
    two = R.workspace_bytes(1, 4, 128, 2)
    assert R.auto_splits(1, 4, 1, 128, 1300, two, cus) == 2 and R.auto_splits(1, 4, 1, 128, 1300, two + 16, cus) == 2
    assert same_bits(run_decode(lib, c, num_splits=0, ws_bytes=full, launches=2), forced[3])
    assert same_bits(run_decode(lib, c, num_splits=0, ws_bytes=two, launches=2), forced[2])
    assert same_bits(run_decode(lib, c, num_splits=0, ws_bytes=0, launches=1), forced[1])


# ---- 3. the clamp of seq_lens ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (1, 2))
def test_seq_lens_are_clamped_to_what_the_table_holds(lib, splits):
    """A length beyond max_blocks block_size reads max_blocks block_size positions, a negative one none (a row of +0.0)"""
    full = 9 * 32
    c = R.make_case(12100, [full, full, 0, 0], 32, 64, Hq=4, Hkv=2, num_splits=splits)
    c.block_table = np.ascontiguousarray(c.block_table[:, :9])   # max_blocks = 9: sequences 0 and 1 fill their rows, every entry valid
    assert (c.block_table[:2] >= 0).all() and c.max_seq_len == full
    want = run_decode(lib, c)
    check(want, c, f"the table's full length, splits={splits}", R.TOL)
    got = run_decode(lib, variant(c, seq_lens=np.array([full + 5, INT32_MAX, -1, -(1 << 31)], dtype=np.int32)))
    assert same_bits(got, want)
    assert not bits(got[2:]).any(), "a negative seq_len is a row of +0.0"


# ---- 4. needed table entries out of range ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (1, 2))
def test_needed_table_entries_out_of_range_read_as_zeros(lib, splits):
    """-1, num_blocks and 2^31 - 1 in entries below ceil(seq_len / block_size) (the kernel tests 0 <= entry < num_blocks before the K row
    and both V runs): the same as those entries naming a block of zero bytes"""
    c = R.make_case(12200, [200, 70], 16, 128, Hq=4, Hkv=2, num_splits=splits)
    nb = c.k_cache.shape[0]
    zero = next(i for i in range(nb) if not c.k_owned[i].any())
    assert not c.k_cache[zero].any() and not c.v_cache[zero].any()
    holes = {(0, 0): -1, (0, 5): nb, (0, 12): INT32_MAX, (1, 2): nb + 7, (1, 4): -(1 << 31)}   # (0, 12) is the partial last block
    bad, good = c.block_table.copy(), c.block_table.copy()
    for (b, i), entry in holes.items():
        assert c.block_table[b, i] >= 0 and i * 16 < c.seq_lens[b]
        bad[b, i], good[b, i] = entry, zero
    ref_case = variant(c, block_table=good)
    want = run_decode(lib, ref_case)
    got = run_decode(lib, variant(c, block_table=bad))
    check(got, ref_case, f"table entries out of range, splits={splits}", R.TOL)
    assert same_bits(got, want)
    assert not same_bits(got, run_decode(lib, c)), "the holes do not show in the output"


# ---- 5. NaN bytes inside a sequence ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (1, 2))
def test_nan_bytes_inside_a_sequence_poison_their_rows_only(lib, splits):
    c = R.make_case(12300, [200, 1, 70], 16, 64, Hq=4, Hkv=2, num_splits=splits)
    clean = run_decode(lib, c)
    check(clean, c, f"before the NaN bytes, splits={splits}", R.TOL)

    def at(b, pos):
        slot = int(c.slots[b][pos])
        return slot // 16, slot % 16

    # (what, cache, [(b, h, pos, d)], the (b, h) hit, the channels that must be NaN)
    plants = [("a K byte", "k", [(0, 1, 37, 5)], (0, 1), slice(None)),
              ("a V byte", "v", [(2, 0, 10, 21)], (2, 0), slice(21, 22)),
              ("the only position", "k", [(1, 0, 0, 63)], (1, 0), slice(None)),
              ("the only position's V", "v", [(1, 1, 0, 0)], (1, 1), slice(0, 1)),
              ("a whole step", "k", [(0, 0, p, d) for p in range(128, 200) for d in range(64)], (0, 0), slice(None))]
    for byte in (0x7F, 0xFF):
        for what, which, where, (hb, hh), channels in plants:
            kc, vc = c.k_cache.copy(), c.v_cache.copy()
            for b, h, pos, d in where:
                blk, off = at(b, pos)
                if which == "k":
                    assert c.k_owned[blk, h, off, d]
                    kc[blk, h, off, d] = byte
                else:
                    assert c.v_owned[blk, h, d, off]
                    vc[blk, h, d, off] = byte
            out = run_decode(lib, variant(c, k_cache=kc, v_cache=vc))
            hit = torch.zeros(3, 4, dtype=torch.bool)
            hit[hb, 2 * hh:2 * hh + 2] = True
            assert bool(out[hit][:, channels].isnan().all()), (what, hex(byte), splits)
            assert same_bits(out[~hit], clean[~hit]), (what, hex(byte), splits)


# ---- 6. powers of two between q and softmax_scale -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (1, 2))
def test_a_power_of_two_moves_between_q_and_softmax_scale_without_a_bit(lib, splits):
    """(q 2^15, scale 2^-15) and (q 2^-100, scale 2^100): the same Q bytes (amax and every element move by the same exact power), the
    same logit factor (q_scale k_scale softmax_scale log2 e: each product an exact power of two away from the unscaled one, nowhere near
    the ends of the fp32 range) - bit-equal outputs.  2^-100 takes the small-amax path of the row quantisation."""
    c = R.make_case(12400, [200, 45], 32, 128, Hq=4, Hkv=2, num_splits=splits, q_dtype="f32")
    want = run_decode(lib, c)
    check(want, c, f"unscaled, splits={splits}", R.TOL)
    for e in (15, -100):
        f = np.float32(2.0 ** e)
        assert np.abs(c.q * f).max() < R.TINY_Q or e > 0
        got = run_decode(lib, variant(c, q=c.q * f, softmax_scale=float(np.float32(c.softmax_scale) / f)))
        assert same_bits(got, want), e


# ---- 7. query rows too small for 448 / amax: the tiny_q group of 1. --------------------------------------------------------------------------

# ---- 8. cache offsets past 4 GiB ------------------------------------------------------------------------------------------------------------

def test_cache_offsets_past_4_gib(lib):
    """block_size 128, Hkv 8, D 128: 128 KiB a block, so block 32768 starts at byte 2^32 of either cache.  386 tokens appended through int64
    slots - 128 into block 3, 128 into block 20000 (between 2 and 4 GiB: a signed 32-bit offset is negative there), 130 into blocks 32775
    and 32769 - read back byte for byte against fp8mi_encode, then attended over; the reference is the small numpy cache of the same
    tokens.  Both caches are uninitialised device memory: whatever they hold beyond the 386 positions is the garbage the kernel ignores."""
    bs, Hkv, D, nb = 128, 8, 128, 32768 + 8
    c = R.make_case(12500, [386], bs, D, Hq=8, Hkv=Hkv)
    big_of = dict(zip(c.block_table[0, :4].tolist(), (3, 20000, 32775, 32769)))
    kc = vc = None
    try:
        try:
            kc = torch.empty((nb, Hkv, bs, D), dtype=torch.uint8, device=DEV)
            vc = torch.empty((nb, Hkv, D, bs), dtype=torch.uint8, device=DEV)
        except torch.cuda.OutOfMemoryError:
            pytest.skip("no room for two 4.3 GB caches on this device")
        assert kc.numel() > 1 << 32 and (32769 * Hkv * bs * D) >= 1 << 32
        small = c.slots[0]
        slots = torch.tensor([big_of[int(s) // bs] * bs + int(s) % bs for s in small], dtype=torch.int64, device=DEV)
        k, v = torch.from_numpy(c.k_values[0]).float().to(DEV), torch.from_numpy(c.v_values[0]).float().to(DEV)
        ks, vs = torch.from_numpy(c.k_scale).to(DEV), torch.from_numpy(c.v_scale).to(DEV)
        with L.kernel_timer(4) as kt:
            rc = lib.fp8mi_kv_cache_append(k.data_ptr(), v.data_ptr(), L.F32, 386, Hkv, D, Hkv * D, Hkv * D, kc.data_ptr(), vc.data_ptr(), nb, bs, slots.data_ptr(), 8,
                                           ks.data_ptr(), vs.data_ptr(), L.KV_SCALE_TENSOR, L.ENC_RNE, stream())
        L.check(rc, "fp8mi_kv_cache_append")
        torch.cuda.synchronize()
        assert len(kt.ms) == 1
        # the appended bytes: fp8mi_encode of the same values with prescale = 1.0f / scale, at the positions of the big blocks
        enc = []
        for x, s in ((k, c.k_scale), (v, c.v_scale)):
            e = torch.empty(x.shape, dtype=torch.uint8, device=DEV)
            pre = (torch.ones(1) / torch.from_numpy(s)).to(DEV)
            L.check(lib.fp8mi_encode(x.data_ptr(), L.F32, e.data_ptr(), pre.data_ptr(), x.numel(), L.ENC_RNE, stream()), "fp8mi_encode")
            enc.append(e.cpu())
        for i, blk in enumerate((3, 20000, 32775, 32769)):
            n = min(bs, 386 - i * bs)
            assert torch.equal(kc[blk, :, :n, :].cpu(), enc[0][i * bs:i * bs + n].permute(1, 0, 2)), blk
            assert torch.equal(vc[blk, :, :, :n].cpu(), enc[1][i * bs:i * bs + n].permute(1, 2, 0)), blk
        assert np.array_equal(enc[0][:bs].permute(1, 0, 2).numpy(), c.k_cache[c.block_table[0, 0]])   # ... and the numpy cache's
        # attention through a table that names the big blocks
        table = torch.tensor([[3, 20000, 32775, 32769, -1]], dtype=torch.int32, device=DEV)
        lens = torch.tensor([386], dtype=torch.int32, device=DEV)
        q = torch.from_numpy(c.q).reshape(1, 8 * D).to(DEV)
        for splits in (1, 2):
            need = lib.fp8mi_paged_attention_workspace_bytes(1, 8, D, splits)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
            out_buf, out = guarded(8 * D, torch.float32, SENT_F)
            rc = lib.fp8mi_paged_attention_decode(q.data_ptr(), L.F32, 1, 8, Hkv, D, 8 * D, kc.data_ptr(), vc.data_ptr(), nb, bs, table.data_ptr(), 5, 5, lens.data_ptr(),
                                                  386, ks.data_ptr(), vs.data_ptr(), L.KV_SCALE_TENSOR, c.softmax_scale, splits, ws.data_ptr() if need else None, need,
                                                  out.data_ptr(), L.F32, 8 * D, stream())
            L.check(rc, "fp8mi_paged_attention_decode")
            torch.cuda.synchronize()
            assert guards_intact(out_buf, 8 * D, SENT_F)
            check(out.reshape(1, 8, D).cpu(), c, f"blocks past 4 GiB, splits={splits}", R.TOL)
    finally:
        del kc, vc
        torch.cuda.empty_cache()
