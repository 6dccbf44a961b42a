"""GPU (MI355X): the MoE routing ops past one pass of each of their loops, at their rung and form boundaries, and on rows nobody owns.

tests/test_gpu_moe_route.py is exact about values; this file runs the code paths it leaves out:
  route            the per-expert scan's segment boundaries (1024 and 1025 chunks, 1024 experts), a full last workgroup, id runs that line
                   up with waves and workgroups, outputs REUSED without a refill while the number of valid ids shrinks and grows;
  scatter-quantise the second and third trip of the 64-at-a-time destination loop, k = 0, fewer tokens than a workgroup holds, the
                   column counts on either side of every rung, rows whose amax sits at the ends of the float range;
  combine          the same loop and its batch-of-four remainder, NaN in every row and weight that no valid assignment names, inf, NaN,
                   -0.0 and subnormal terms that ARE named, the edges of the vector form's alignment condition;
  forward          NaN bytes and non-finite scales BEHIND offs[-1] through both grouped GEMMs, the eight-launch form eagerly and from a
                   graph, a skewed gate, every id dropped, T = 1 and T = 0.
References: tests/moe_route_ref.py on the CPU and the existing quantisers, as in the first file; helpers in tests/moe_route_gpu_util.py."""
import pytest
import torch

import fp8_mi355x_lib as L
from moe_route_gpu_util import (CHUNK, CODE, DEV, GUARD, INT32_MAX, SENT_B, SENT_F, SENT_I, SINGLE, TILE, Layer, bits, check_combine, check_route,
                                check_scatter, forward_pair, forward_reference, gate, guarded, guards_intact, random_ids, run_route, stream)
from moe_route_ref import combine_ref, route_ref

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def N_(native):
    return native


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- route -----------------------------------------------------------------------------------------------------------------------------

def test_route_scan_where_every_thread_owns_one_chunk(lib):
    """1024 chunks: per = 1, every thread of the per-expert scan owns exactly one count, the last workgroup is full"""
    n = 1024 * CHUNK
    check_route(lib, random_ids(torch.Generator().manual_seed(31), n, 1, 3), 3, torch.int32)


def test_route_scan_with_segments_of_two_and_1024_experts(lib):
    """1025 chunks and 3 ids over 1024 experts: per = 2, the threads from 513 on own nothing, thread 512 one count; workspace rows of 1025
    ints for 1024 experts.  At this, the largest case, also the properties that hold without the reference."""
    n, G = 1025 * CHUNK + 3, 1024
    ids = random_ids(torch.Generator().manual_seed(32), n, 1, G, dropped=0.1).reshape(-1)
    assert 4_100_000 < lib.fp8mi_moe_route_workspace_bytes(n, G) < 4_300_000
    offs, row_of, src = run_route(lib, ids.to(DEV), G)
    w_offs, w_row_of, w_src = route_ref(ids, G)
    assert torch.equal(offs, w_offs) and torch.equal(row_of, w_row_of) and torch.equal(src, w_src)
    used = int(offs[-1])
    assert 0 < used < n
    own = src[:used].long()
    assert bool((own >= 0).all()) and torch.equal(row_of[own], torch.arange(used, dtype=torch.int32))   # row_of[src_of_row[r]] == r
    expert = ids[own]
    assert bool((expert[1:] >= expert[:-1]).all())                                  # ids[src_of_row[r]] is non-decreasing in r
    assert bool(((own[1:] > own[:-1]) | (expert[1:] != expert[:-1])).all())         # strictly increasing inside an expert's segment
    assert bool((src[used:] == -1).all())


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_route_with_a_full_last_workgroup(lib, dtype):
    for chunks in (2, 3):
        check_route(lib, random_ids(torch.Generator().manual_seed(chunks), chunks * CHUNK, 1, 9), 9, dtype)


def lone_assignment(n, at, main, other):
    ids = torch.full((n,), main, dtype=torch.int64)
    ids[at] = other
    return ids


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_route_id_runs_that_line_up_with_waves_and_workgroups(lib, dtype):
    n = 3 * CHUNK + 70
    i = torch.arange(n)
    for m in (n, 1000):   # three launches; the one-launch form
        ids = random_ids(torch.Generator().manual_seed(m), m, 1, 9).reshape(-1)   # (the dropped ids sort to both ends)
        check_route(lib, torch.sort(ids).values, 9, dtype)
        check_route(lib, torch.sort(ids, descending=True).values, 9, dtype)
    check_route(lib, i // 64, 64, dtype)            # one id per wave
    check_route(lib, i // CHUNK, 8, dtype)          # one id per workgroup: base[g][.] is one-hot
    check_route(lib, (i + 1) // 64, 64, dtype)      # a wave holds the last element of one run and the first of the next
    check_route(lib, (i + 1) // CHUNK, 8, dtype)    # a workgroup does
    # one expert owns everything but a single assignment: in the first lane and the last lane of a wave inside the second workgroup, and
    # in the last valid lane of the last, partial wave; the lone expert before and behind the other in the row order
    assert (n - 1) % 64 not in (0, 63)
    for at in (CHUNK + 5 * 64, CHUNK + 5 * 64 + 63, n - 1):
        for other in (0, 7):
            check_route(lib, lone_assignment(n, at, 5, other), 8, dtype)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("n", [700, 2 * CHUNK + 452], ids=["one-launch", "three-launches"])
def test_route_into_reused_outputs_while_the_valid_ids_shrink_and_grow(lib, n, dtype):
    """ONE set of offs / row_of / src_of_row / workspace buffers, never refilled: after every call all three outputs are the reference's.
    src_of_row[i] = -1 for i >= offs[-1] is what makes the second call right, whose rows end where the first one's were in use."""
    G = 9
    gen = torch.Generator().manual_seed(n)
    offs_buf, offs = guarded(G, torch.int32, SENT_I)
    row_buf, row_of = guarded(n, torch.int32, SENT_I)
    src_buf, src = guarded(n, torch.int32, SENT_I)
    need = lib.fp8mi_moe_route_workspace_bytes(n, G)
    ws_buf, ws = guarded(need, torch.uint8, SENT_B)
    used = []
    for dropped in (0.0, 0.6, 0.0):
        ids = random_ids(gen, n, 1, G, dropped=dropped).reshape(-1)
        dev_ids = ids.to(dtype).to(DEV)
        rc = lib.fp8mi_moe_route(dev_ids.data_ptr(), dev_ids.element_size(), n, G, offs.data_ptr(), row_of.data_ptr(), src.data_ptr(),
                                 ws.data_ptr() if need else None, need, stream())
        L.check(rc, "fp8mi_moe_route")
        torch.cuda.synchronize()
        w_offs, w_row_of, w_src = route_ref(ids, G)
        assert torch.equal(offs.cpu(), w_offs) and torch.equal(row_of.cpu(), w_row_of) and torch.equal(src.cpu(), w_src), dropped
        assert guards_intact(offs_buf, G, SENT_I) and guards_intact(row_buf, n, SENT_I) and guards_intact(src_buf, n, SENT_I)
        assert guards_intact(ws_buf, need, SENT_B)
        used.append(int(w_offs[-1]))
    assert used[0] == n == used[2] and 0 < used[1] < n // 2


# ---- scatter-quantise ------------------------------------------------------------------------------------------------------------------

def tokens(dtype, T, cols, seed):
    """(T, cols) on the device: magnitudes from 1e-3 to 1e3 over the tokens"""
    x = torch.randn((T, cols), generator=torch.Generator().manual_seed(seed)) * torch.logspace(-3, 3, T)[:, None]
    return x.to(dtype).to(DEV)


def scatter_plan(gen, T, k, gone):
    """(T, k) int32: a random permutation of range(T k) with 15 % of the entries replaced by -1, rows_out or INT32_MAX; token `gone` loses all"""
    row_of = torch.randperm(T * k, generator=gen).reshape(T, k).to(torch.int32)
    drop = torch.tensor([-1, T * k, INT32_MAX], dtype=torch.int32)[torch.randint(0, 3, (T, k), generator=gen)]
    row_of = torch.where(torch.rand((T, k), generator=gen) < 0.15, drop, row_of)
    if gone is not None:
        row_of[gone] = -1
    return row_of


@pytest.mark.parametrize("k", [63, 64, 65, 130])
def test_scatter_quantize_with_more_destinations_than_one_pass_reads(lib, N_, k):
    """The destinations are read 64 at a time: one pass short of full, exactly full, a second pass of one, a third pass of two.  Token 2 has
    no destination at all: check_scatter's sentinel comparison shows that nothing of it was stored."""
    T = 5
    row_of = scatter_plan(torch.Generator().manual_seed(k), T, k, gone=2)
    for dtype, cols in ((torch.bfloat16, 128), (torch.bfloat16, 4112), (torch.float32, 2064)):
        x = tokens(dtype, T, cols, cols + k)
        for group in (False, True):
            check_scatter(lib, N_, x, row_of, group, L.ENC_RNE)


def test_scatter_quantize_without_destinations_writes_nothing(lib):
    T, cols, rows_out = 5, 128, 8
    x = tokens(torch.bfloat16, T, cols, 1)
    row_of = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for group in (False, True):
        out_buf, out = guarded(rows_out * cols, torch.uint8, SENT_B)
        sc_buf, sc = guarded(rows_out, torch.float32, SENT_F)
        with L.kernel_timer(4) as kt:
            rc = lib.fp8mi_moe_scatter_quantize(x.data_ptr(), CODE[x.dtype], T, cols, cols, row_of.data_ptr(), 0, out.data_ptr(), rows_out, cols, sc.data_ptr(),
                                                1, 1, L.QSCALE_GROUP128 if group else L.QSCALE_ROW, L.FMT_E4M3, L.ENC_RNE, stream())
        torch.cuda.synchronize()
        assert rc == 0 and len(kt.ms) == 0
        assert bool((out_buf == SENT_B).all()) and bool((sc_buf == SENT_F).all())


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_scatter_quantize_of_fewer_tokens_than_a_workgroup_holds(lib, N_, T):
    """128 columns: one wave per token, four tokens per workgroup - one workgroup with one, two and three idle waves, and a second one"""
    row_of = torch.randperm(T * 3, generator=torch.Generator().manual_seed(T)).reshape(T, 3).to(torch.int32)
    row_of[T - 1, 1] = -1
    x = tokens(torch.bfloat16, T, 128, T)
    for group in (False, True):
        check_scatter(lib, N_, x, row_of, group, L.ENC_RNE)


def extreme_rows(dtype, cols):
    """rows whose amax is the smallest normal, a subnormal, 3e38 (inf in float16) and - bfloat16 and float32 - the largest finite value"""
    info = torch.finfo(dtype)
    amax = [info.tiny, info.tiny / 8, 3e38] + ([info.max] if dtype is not torch.float16 else [])
    pattern = torch.tensor([1.0, -1.0, 0.5, -0.75], dtype=torch.float64).repeat(cols // 4)
    return torch.stack([(a * pattern).to(dtype) for a in amax])


# the last column count of a rung and the first of the next (fp32: one wave up to 2048, four up to 8192, then eight; 16-bit: one wave up to
# 4096, four up to 16384)
SQ_EDGE_SHAPES = [(torch.float32, 2048), (torch.float32, 8192), (torch.float32, 8208), (torch.float16, 16384), (torch.float16, 4096)]


@pytest.mark.parametrize("dtype,cols", SQ_EDGE_SHAPES + [(torch.bfloat16, 144), (torch.float32, 144), (torch.float16, 144)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_scatter_quantize_at_rung_boundaries_with_rows_at_the_ends_of_the_range(lib, N_, dtype, cols):
    """The contract is bit equality with fp8_quantize_rowwise / fp8_act_quantize, whatever those give for such a row: this test does not
    judge the recipe."""
    x = torch.cat([tokens(dtype, 4, cols, cols), extreme_rows(dtype, cols).to(DEV)])
    T = x.shape[0]
    assert float(x[4:].float().abs().max(dim=1).values.min()) > 0.0   # (the subnormal row did not vanish in the conversion)
    row_of = scatter_plan(torch.Generator().manual_seed(cols), T, 3, gone=1)
    assert bool(((row_of[4:] >= 0) & (row_of[4:] < T * 3)).any(dim=1).all())   # every extreme row is stored somewhere
    for enc in (L.ENC_REFERENCE, L.ENC_RNE):
        check_scatter(lib, N_, x, row_of, False, enc)
    check_scatter(lib, N_, x, row_of, True, L.ENC_RNE)


# ---- combine ---------------------------------------------------------------------------------------------------------------------------

CB_T, CB_GONE = 5, 1


def combine_plan(gen, k, rows, T=CB_T, gone=CB_GONE):
    """(T, k) rows: distinct owned rows in a random order; a fifth of the assignments dropped (-1, rows, INT32_MAX); token `gone` loses all"""
    row_of = torch.randperm(rows, generator=gen)[:T * k].reshape(T, k).to(torch.int32)
    drop = torch.tensor([-1, rows, INT32_MAX], dtype=torch.int32)[torch.randint(0, 3, (T, k), generator=gen)]
    row_of = torch.where(torch.rand((T, k), generator=gen) < 0.2, drop, row_of)
    if gone is not None:
        row_of[gone] = -1
    return row_of


# 2, 3, 5, 7: every remainder of the batch of four, below and above one batch; 63 .. 67: the first pass short of full (its last batch
# clamped), full, and a second pass of 1, 3 (the clamp at a remainder of 3 with j0 = 64); 130: a third pass
CB_KS = [2, 3, 5, 7, 63, 64, 65, 67, 130]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["to-f32", "to-bf16"])
@pytest.mark.parametrize("y_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_combine_past_one_pass_and_at_every_batch_remainder(lib, y_dtype, out_dtype):
    gen = torch.Generator().manual_seed(91)
    for k in CB_KS:
        rows = CB_T * k + 3
        for N in (8, 264, 7):   # the vector form in one and in two kinds of lanes (264 = 33 pieces of 8: live and idle); the scalar form
            y = torch.randn((rows, N), generator=gen).to(y_dtype).to(DEV)
            w = torch.softmax(torch.randn((CB_T, k), generator=gen), dim=1) * 1.7
            row_of = combine_plan(gen, k, rows)
            check_combine(lib, y, row_of, w, out_dtype, gone_tokens=(CB_GONE,))
            if k == 65:
                check_combine(lib, y, row_of, None, out_dtype, gone_tokens=(CB_GONE,))


@pytest.mark.parametrize("y_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_combine_never_touches_a_row_or_a_weight_that_no_valid_assignment_names(lib, y_dtype):
    """NaN in every row of y that is not referenced and NaN / inf in every weight of a dropped assignment: the result is the one with those
    zeroed, and finite.  (A kernel that loads a dropped assignment's row or weight and multiplies by 0 gives NaN.)"""
    gen = torch.Generator().manual_seed(92)
    for k in (3, 65):
        rows = CB_T * k + 3
        for N in (264, 7):
            row_of = combine_plan(gen, k, rows)
            valid = (row_of >= 0) & (row_of < rows)
            unused = torch.ones(rows, dtype=torch.bool)
            unused[row_of[valid].long()] = False
            assert bool(unused.any()) and bool((~valid).any()) and bool(valid.any())
            clean_y = torch.randn((rows, N), generator=gen).to(y_dtype)
            clean_y[unused] = 0.0
            clean_w = torch.rand((CB_T, k), generator=gen)
            clean_w[~valid] = 0.0
            y, w = clean_y.clone(), clean_w.clone()
            y[unused] = NAN
            w[~valid] = torch.tensor([NAN, INF, -INF])[torch.arange(int((~valid).sum())) % 3]
            for out_dtype in (torch.float32, torch.bfloat16):
                got = check_combine(lib, y.to(DEV), row_of, w, out_dtype, gone_tokens=(CB_GONE,))
                assert bool(torch.isfinite(got).all())
                assert torch.equal(bits(got), bits(combine_ref(clean_y, row_of, clean_w, out_dtype)))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["to-f32", "to-f16", "to-bf16"])
def test_combine_of_non_finite_terms_that_are_named(lib, out_dtype):
    """inf, NaN and -0.0 that valid assignments reference go through the float32 loop like any number: NaN where the reference is NaN,
    the same bits everywhere else."""
    gen = torch.Generator().manual_seed(93)
    T, k = 6, 4
    rows = T * k
    row_of = torch.arange(rows, dtype=torch.int32).reshape(T, k)
    for N in (8, 7):
        y = torch.randn((rows, N), generator=gen)
        y[:, 2] = 0.0                                      # (a zero column: inf * 0)
        w = torch.rand((T, k), generator=gen) + 0.5
        y[row_of[0, 1], ::2], y[row_of[0, 3], ::2] = INF, -INF     # +inf, later -inf: NaN from there on; the other columns stay finite
        y[row_of[1, 2]], w[1, 2] = INF, 0.0                # a weight of 0 on an inf row: NaN
        w[2, 1] = INF                                      # a weight of inf: +-inf by the sign of y, NaN in the zero column
        row_of[3, 1:] = -1                                 # a single term -0.0 with weight 1: 0 + (-0) = +0
        y[row_of[3, 0]], w[3, 0] = -0.0, 1.0
        y[row_of[4, 0]:row_of[4, 0] + k] = 40000.0         # four terms of weight 1: beyond float16's 65504 from the second on
        y[row_of[4, 0]:row_of[4, 0] + k, 1] = -40000.0
        w[4] = 1.0
        want = combine_ref(y, row_of, w, out_dtype)
        assert bool(want[0, ::2].isnan().all()) and bool(torch.isfinite(want[0, 1::2]).all()) and bool(want[1].isnan().all())
        assert bool(want[2, 2].isnan()) and bool(want[2, [0, 1, 3]].isinf().all())
        assert bool((bits(want[3]) == 0).all())
        if out_dtype is torch.float16:
            assert want[4, 0] == INF and want[4, 1] == -INF
        for y_dtype in (torch.float32, torch.bfloat16):
            got = check_combine(lib, y.to(y_dtype).to(DEV), row_of, w, out_dtype, exact_only_tokens=(0, 1, 2, 3, 4))
            assert bool((bits(got[3]) == 0).all())


def test_combine_keeps_subnormal_products_and_sums(lib):
    """Weights around 1e-30 on values around 1e-10: every product and every sum is a float32 subnormal, which the sequential loop on the
    CPU keeps - and so must the kernel (bit equality; the derived bound has no term for underflow and is not taken)."""
    gen = torch.Generator().manual_seed(94)
    k = 3
    rows = CB_T * k + 3
    for N in (8, 7):
        y = (torch.randn((rows, N), generator=gen) * 1e-10).to(DEV)
        w = (torch.rand((CB_T, k), generator=gen) + 0.5) * 1e-30
        row_of = combine_plan(gen, k, rows)
        want = combine_ref(y, row_of, w, torch.float32)
        tiny = torch.finfo(torch.float32).tiny
        assert bool((want != 0).any()) and float(want.abs().max()) < tiny
        got = check_combine(lib, y, row_of, w, torch.float32, gone_tokens=(CB_GONE,), exact_only_tokens=range(CB_T))
        assert bool((got != 0).any())


def test_combine_at_the_edges_of_the_vector_forms_condition(lib):
    gen = torch.Generator().manual_seed(95)
    k, N = 5, 264
    # T = 1: ld_out is never used, an odd one keeps the vector form
    rows = k + 3
    y = torch.randn((rows, N), generator=gen).to(torch.bfloat16).to(DEV)
    row_of = combine_plan(gen, k, rows, T=1, gone=None)
    w = torch.rand((1, k), generator=gen)
    check_combine(lib, y, row_of, w, torch.bfloat16, ld_out=N + 3)
    check_combine(lib, y, row_of, w, torch.float32, ld_out=N + 1)
    # rows = 1: ld_y is never used, one that is no multiple of 16 bytes keeps the vector form
    row_of = torch.where(torch.rand((CB_T, k), generator=gen) < 0.4, -1, 0).to(torch.int32)
    row_of[0, 0], row_of[CB_GONE] = 0, -1
    w = torch.rand((CB_T, k), generator=gen)
    for dtype in (torch.bfloat16, torch.float32):
        check_combine(lib, y[:1].to(dtype), row_of, w, dtype, gone_tokens=(CB_GONE,), ld_y=N + 3)
    # N a multiple of the piece but an output base aligned to 4 bytes only: the scalar form
    rows = CB_T * k + 3
    row_of = combine_plan(gen, k, rows)
    for dtype, offset in ((torch.bfloat16, 2), (torch.float32, 1)):
        y = torch.randn((rows, N), generator=gen).to(dtype).to(DEV)
        check_combine(lib, y, row_of, w, dtype, gone_tokens=(CB_GONE,), out_offset=offset)
        check_combine(lib, y, row_of, w, dtype, gone_tokens=(CB_GONE,), out_offset=offset, ld_out=N + 8)


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def layers(N_):
    return {4: Layer(N_, 4, 256, 128, 256, 1), 64: Layer(N_, 64, 256, 128, 256, 2)}


def weights_of(layer, recipe):
    return layer.row if recipe == "row" else layer.block


def grouped_mm(N_, recipe, a, a_scales, w, w_scales, offs, **kw):
    if recipe == "row":
        return N_.fp8_scaled_mm_grouped(a, w, a_scales, w_scales, offs, **kw)
    return N_.fp8_scaled_mm_grouped_blockwise(a, w, a_scales, w_scales, offs, block_b=128, **kw)


PO_T, PO_K = 33, 2


def poisoned_case():
    """The first seed whose gate (about 40 % of the ids dropped) leaves 0 < offs[-1] < T k rows in use, and no multiple of a tile height"""
    for seed in range(100):
        gen = torch.Generator().manual_seed(seed)
        ids, wts = gate(gen, PO_T, PO_K, 4, dropped=0.4)
        used = int(route_ref(ids, 4)[0][-1])
        if 0 < used < PO_T * PO_K and all(used % bm for bm in (32, 64, 128)):
            return gen, ids, wts, used
    raise AssertionError("no seed gives the case")


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64], ids=["32x64", "64x64", "128x64"])
@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_chain_over_poisoned_rows_that_no_expert_owns(N_, layers, recipe, tile):
    """fp8_moe_scatter_quantize leaves the rows from offs[-1] on unwritten and the grouped GEMMs do not write them, so in the forward h and
    y carry whatever the allocator gave through fp8_act_quantize into the down GEMM, whose last tile straddles offs[-1].  Here those rows
    hold the worst (P: NaN bytes, NaN / inf scales, NaN in h and y) and the most harmless (Z: zeros, scales 1) content: the rows in use,
    and the layer's output, are the same bits, under either NaN mode - also where a NaN byte in the tile sends it down the scrubbed path."""
    layer = layers[4]
    gen, ids, wts, used = poisoned_case()
    rows = PO_T * PO_K
    assert 0 < used < rows and all(used % bm for bm in (32, 64, 128))
    x = torch.randn((PO_T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    w1, s1, w2, s2 = weights_of(layer, recipe)
    scale = recipe
    offs, row_of, _src = N_.fp8_moe_route(ids.to(DEV), 4)
    assert int(offs[-1]) == used
    q0, sc0 = N_.fp8_moe_scatter_quantize(x, row_of, scale)
    wts_dev = wts.to(DEV)
    results = {}
    for nan_mode in (L.NAN_ZERO, L.NAN_PROPAGATE):
        for variant in "PZ":
            q, sc = q0.clone(), sc0.clone()
            if variant == "P":
                q[used:] = torch.tensor([0x7F, 0xFF], dtype=torch.uint8, device=DEV).repeat(q.shape[1] // 2)
                tail = sc[used:]
                tail.copy_(torch.tensor([NAN, INF], device=DEV).repeat(tail.numel() // 2 + 1)[:tail.numel()].reshape(tail.shape))
            else:
                q[used:], sc[used:] = 0, 1.0
            fill = NAN if variant == "P" else 0.0
            h_buf, h = guarded(rows * 2 * layer.H, torch.bfloat16, fill)
            y_buf, y = guarded(rows * layer.N, torch.bfloat16, fill)
            h_before, y_before = bits(h_buf).clone(), bits(y_buf).clone()
            h, y = h.view(rows, 2 * layer.H), y.view(rows, layer.N)
            grouped_mm(N_, recipe, q, sc, w1, s1, offs, out_dtype=torch.bfloat16, nan_mode=nan_mode, kernel=tile, out=h)
            hq, hs = N_.fp8_act_quantize(h, "silu", True, scale)
            grouped_mm(N_, recipe, hq, hs, w2, s2, offs, out_dtype=torch.bfloat16, nan_mode=nan_mode, kernel=tile, out=y)
            out = N_.fp8_moe_combine(y, row_of, wts_dev)
            torch.cuda.synchronize()
            for buf, before, width in ((h_buf, h_before, 2 * layer.H), (y_buf, y_before, layer.N)):
                now = bits(buf)
                assert torch.equal(now[:GUARD], before[:GUARD]) and torch.equal(now[GUARD + rows * width:], before[GUARD + rows * width:])   # the guards
                assert torch.equal(now[GUARD + used * width:], before[GUARD + used * width:]), (variant, nan_mode)   # the tail keeps its prefill
            assert not bool(h[:used].isnan().any()) and not bool(y[:used].isnan().any()), (variant, nan_mode)
            results[nan_mode, variant] = (h[:used].clone(), y[:used].clone(), out)
    for nan_mode in (L.NAN_ZERO, L.NAN_PROPAGATE):
        (h_p, y_p, out_p), (h_z, y_z, out_z) = results[nan_mode, "P"], results[nan_mode, "Z"]
        assert torch.equal(bits(h_p), bits(h_z)), nan_mode
        assert torch.equal(bits(y_p), bits(y_z)), nan_mode
        assert torch.equal(bits(out_p), bits(out_z)) and bool(torch.isfinite(out_p).all()), nan_mode
    fwd, _mlp = forward_pair(N_, recipe)
    whole = fwd(x, ids.to(DEV), wts_dev, w1, s1, w2, s2, kernel=tile)   # (under the module's NAN_MODE)
    assert whole.shape == (PO_T, layer.N) and whole.dtype == torch.bfloat16
    assert torch.equal(bits(whole), bits(results[N_.NAN_MODE, "P"][2]))


def run_forward(N_, recipe, layer, x, ids, wts, launches):
    fwd, _mlp = forward_pair(N_, recipe)
    with L.kernel_timer(16) as kt:
        got = fwd(x, ids.to(DEV), wts.to(DEV) if wts is not None else None, *weights_of(layer, recipe), kernel=TILE)
    torch.cuda.synchronize()
    assert len(kt.ms) == launches
    assert got.shape == (x.shape[0], layer.N) and got.dtype == x.dtype
    return got


@pytest.mark.parametrize("recipe", ["row", "block128"])
@pytest.mark.parametrize("T,k,G", [(130, 8, 64), (520, 2, 4)])
def test_forward_on_the_three_launch_route(N_, layers, T, k, G, recipe):
    """n = 1040 > MOE_ROUTE_SINGLE_MAX: count, scan, rank, then the five launches of the one-launch form's layer"""
    assert T * k > SINGLE
    gen = torch.Generator().manual_seed(T)
    layer = layers[G]
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids, wts = gate(gen, T, k, G)
    got = run_forward(N_, recipe, layer, x, ids, wts, launches=8)
    assert torch.equal(bits(got.cpu()), bits(forward_reference(N_, recipe, layer, x, ids, wts)))


def test_forward_on_the_three_launch_route_captured_into_a_graph(N_, layers):
    """The capture needs the route's workspace to exist: one eager call at this size on the capturing stream first, then
    torch.cuda.graph(g, stream=side).  The replay follows a second routing and second gate weights."""
    gen = torch.Generator().manual_seed(41)
    layer, recipe, T, k, G = layers[64], "row", 130, 8, 64
    fwd, _mlp = forward_pair(N_, recipe)
    weights = weights_of(layer, recipe)
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids1, wts1 = gate(gen, T, k, G)
    ids2, wts2 = gate(gen, T, k, G)
    assert not torch.equal(ids1, ids2)
    ids, wts = ids1.to(DEV), wts1.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager1 = fwd(x, ids, wts, *weights, kernel=TILE)   # the warm-up on the capture's stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = fwd(x, ids, wts, *weights, kernel=TILE)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager1))
    ids.copy_(ids2.to(DEV))
    wts.copy_(wts2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager2 = fwd(x, ids, wts, *weights, kernel=TILE)
    assert torch.equal(bits(replayed), bits(eager2)) and not torch.equal(bits(eager2), bits(eager1))
    assert torch.equal(bits(replayed.cpu()), bits(forward_reference(N_, recipe, layer, x, ids2, wts2)))


@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_with_a_skewed_gate(N_, layers, recipe):
    """Every token names expert 0 first and one of experts 1 .. 3 second: one group of 520 rows, three of about 173, sixty empty ones"""
    gen = torch.Generator().manual_seed(42)
    layer, T = layers[64], 520
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids = torch.stack([torch.zeros(T, dtype=torch.int64), torch.randint(1, 4, (T,), generator=gen)], dim=1)
    wts = torch.softmax(torch.randn((T, 2), generator=gen), dim=1)
    offs = route_ref(ids, 64)[0]
    assert int(offs[0]) == T >= 130 and int(offs[-1]) == 2 * T and int((offs[1:] == offs[:-1]).sum()) == 60
    got = run_forward(N_, recipe, layer, x, ids, wts, launches=8)
    assert torch.equal(bits(got.cpu()), bits(forward_reference(N_, recipe, layer, x, ids, wts)))


@pytest.mark.parametrize("recipe", ["row", "block128"])
@pytest.mark.parametrize("T,k,launches", [(33, 2, 6), (520, 2, 8)], ids=["one-launch-route", "three-launch-route"])
def test_forward_with_every_id_dropped_is_zero(N_, layers, T, k, launches, recipe):
    gen = torch.Generator().manual_seed(43)
    layer = layers[4]
    for x_dtype in (torch.bfloat16, torch.float32):
        x = torch.randn((T, layer.K), generator=gen).to(x_dtype).to(DEV)
        ids = torch.tensor([-1, 4, INT32_MAX])[torch.randint(0, 3, (T, k), generator=gen)]
        got = run_forward(N_, recipe, layer, x, ids, torch.rand((T, k), generator=gen), launches)
        assert bool((bits(got) == 0).all())   # +0, not -0


@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_of_one_token_with_one_expert(N_, layers, recipe):
    gen = torch.Generator().manual_seed(44)
    layer = layers[4]
    x = torch.randn((1, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids, wts = torch.tensor([[2]]), torch.tensor([[0.75]])
    got = run_forward(N_, recipe, layer, x, ids, wts, launches=6)
    assert torch.equal(bits(got.cpu()), bits(forward_reference(N_, recipe, layer, x, ids, wts)))


@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_of_no_tokens(N_, layers, recipe):
    layer = layers[4]
    fwd, _mlp = forward_pair(N_, recipe)
    for x_dtype, out_dtype, want in ((torch.bfloat16, None, torch.bfloat16), (torch.float32, None, torch.float32), (torch.bfloat16, torch.float32, torch.float32)):
        x = torch.empty((0, layer.K), dtype=x_dtype, device=DEV)
        ids = torch.empty((0, 2), dtype=torch.int64, device=DEV)
        got = fwd(x, ids, torch.empty((0, 2), device=DEV), *weights_of(layer, recipe), out_dtype=out_dtype, kernel=TILE)
        assert got.shape == (0, layer.N) and got.dtype == want and got.device.type == "cuda"
