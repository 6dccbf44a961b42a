"""GPU (MI355X): MoE routing on the device - fp8mi_moe_route, fp8mi_moe_scatter_quantize, fp8mi_moe_combine and the fp8_moe_forward_* ops.

The contracts under test (include/fp8mi.h):
  route            offs, row_of, src_of_row EQUAL the stable-sort reference (tests/moe_route_ref.py), in the one-launch and the three-launch form;
  scatter-quantise row r of the output is, bit for bit, row src_of_row[r] // k of the existing quantiser's output, bytes and scales;
  combine          bit-equal to the sequential float32 loop on the CPU, and inside the derived bound around the float64 sum;
  forward          bit-equal to reference route -> fp8_moe_mlp_* on the gathered rows -> the float32 combine, eagerly and from a replayed graph.
Every output of the three C entry points sits between guard elements, prefilled with a sentinel: guards and unowned rows must keep it."""
import pytest
import torch

import fp8_mi355x_lib as L
from moe_route_gpu_util import (CHUNK, DEV, INT32_MAX, INT32_MIN, SENT_B, SINGLE, TILE, Layer, bits, check_route, check_scatter, forward_pair,
                                forward_reference, gate, random_ids, run_combine, run_route)
from moe_route_gpu_util import check_combine as check_combine_with
from moe_route_ref import combine_ref, route_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N_(native):
    return native


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- route -----------------------------------------------------------------------------------------------------------------------------

# (T, k): n = 1; the small example's size; the one-launch bound, one below and one above it; 3 chunks + 5; k in {1, 6, 8} in both forms
ROUTE_SIZES = [(1, 1), (5, 2), (SINGLE - 1, 1), (SINGLE // 8, 8), (SINGLE + 1, 1), (171, 6), (3 * CHUNK + 5, 1), (385, 8), (120, 6)]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("G", [1, 8, 9, 64, 65, 1024])
def test_route_equals_the_stable_sort_reference(lib, G, dtype):
    gen = torch.Generator().manual_seed(1000 + G)
    for T, k in ROUTE_SIZES:
        check_route(lib, random_ids(gen, T, k, G), G, dtype)


def test_route_small_example(lib):
    """T = 5, k = 2, G = 3: a token that names expert 1 twice owns two rows; ids 5 and -1 are dropped"""
    ids = torch.tensor([[1, 0], [1, 1], [2, 5], [0, -1], [1, 2]])
    for dtype in (torch.int32, torch.int64):
        offs, row_of, src = run_route(lib, ids.to(dtype).to(DEV), 3)
        assert offs.tolist() == [2, 6, 8] and row_of.tolist() == [2, 0, 3, 4, 6, -1, 1, -1, 5, 7] and src.tolist() == [1, 6, 0, 2, 3, 8, 4, 9, -1, -1]


@pytest.mark.parametrize("n", [700, 2 * CHUNK + 452], ids=["one-launch", "three-launches"])
def test_route_special_id_patterns(lib, n):
    for dtype in (torch.int32, torch.int64):
        # every id equal: one expert owns all rows, the match loop runs once per step
        check_route(lib, torch.full((n,), 5, dtype=torch.int64), 8, dtype)
        check_route(lib, torch.zeros((n,), dtype=torch.int64), 1, dtype)
        # all ids of a wave distinct: 64 passes of the match loop
        check_route(lib, torch.arange(n) % 64, 64, dtype)
        check_route(lib, (torch.arange(n) * 7) % 1024, 1024, dtype)
        # every id dropped: offs all 0, row_of and src_of_row all -1
        for bad in (-1, 8, INT32_MIN, INT32_MAX):
            offs, row_of, src = run_route(lib, torch.full((n,), bad, dtype=dtype, device=DEV), 8)
            assert bool((offs == 0).all()) and bool((row_of == -1).all()) and bool((src == -1).all()), bad
        # src_of_row is optional
        check_route(lib, random_ids(torch.Generator().manual_seed(n), n, 1, 9), 9, dtype, with_src=False)
    # int64 ids beyond 2^32 whose low words look like valid experts
    ids = random_ids(torch.Generator().manual_seed(7), n, 1, 8).reshape(-1)
    ids[::5] = (1 << 32) + 3
    ids[1::7] = -(1 << 32) + 2
    ids[2::11] = (1 << 40)
    check_route(lib, ids, 8, torch.int64)


def test_route_with_more_chunks_than_the_scan_has_threads(lib):
    """2500 chunks and a bit: a thread of the per-expert scan owns a segment of three counts (the smallest size at which it owns more than one),
    the last threads none"""
    n = 2500 * CHUNK + 7
    check_route(lib, random_ids(torch.Generator().manual_seed(5), n, 1, 3), 3, torch.int32)


def test_route_op(N_):
    """fp8_moe_route: torch.topk's int64 ids as they are; the three-launch form through the cached workspace; T = 0"""
    gen = torch.Generator().manual_seed(3)
    for T, k, G in ((64, 8, 256), (300, 6, 40)):
        ids = torch.topk(torch.rand((T, G), generator=gen), k, dim=1).indices
        offs, row_of, src = N_.fp8_moe_route(ids.to(DEV), G)
        w_offs, w_row_of, w_src = route_ref(ids, G)
        assert offs.dtype == row_of.dtype == src.dtype == torch.int32 and row_of.shape == (T, k)
        assert torch.equal(offs.cpu(), w_offs) and torch.equal(row_of.cpu().reshape(-1), w_row_of) and torch.equal(src.cpu(), w_src)
    offs, row_of, src = N_.fp8_moe_route(torch.empty((0, 8), dtype=torch.int64, device=DEV), 4)
    assert offs.tolist() == [0, 0, 0, 0] and row_of.shape == (0, 8) and src.numel() == 0


def test_a_captured_three_launch_route_outlives_its_workspace_being_superseded(N_):
    """The three-launch form writes through a cached workspace.  A graph captured at one size keeps that workspace's pointer, so a later,
    larger call on the same stream must leave it alive and untouched by the allocator: the replay is right, and tensors allocated in
    between (which would have been handed the workspace's memory had it been released) keep their content."""
    gen = torch.Generator().manual_seed(21)
    G, T, k = 16, 200, 8   # n = 1600: three launches
    ids1, ids2 = random_ids(gen, T, k, G), random_ids(gen, T, k, G)
    ids = ids1.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N_.fp8_moe_route(ids, G)   # the warm-up on the capture's stream: the workspace exists before the capture
    side.synchronize()
    held = N_._route_workspaces[(ids.device.index, side.cuda_stream)]
    first = held[-1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        offs, row_of, src = N_.fp8_moe_route(ids, G)
    assert held[-1] is first, "the capture used the workspace of the warm-up"
    with torch.cuda.stream(side):
        big = random_ids(gen, 6000, k, 64).to(DEV)
        b_offs, b_row_of, b_src = N_.fp8_moe_route(big, 64)   # needs more: a new workspace serves from here on
    side.synchronize()
    assert held[-1] is not first and held[-1].numel() > first.numel() and any(w is first for w in held)
    w_offs, w_row_of, w_src = route_ref(big.cpu(), 64)
    assert torch.equal(b_offs.cpu(), w_offs) and torch.equal(b_row_of.cpu().reshape(-1), w_row_of) and torch.equal(b_src.cpu(), w_src)
    junk = [torch.full((first.numel(),), SENT_B, dtype=torch.uint8, device=DEV) for _ in range(16)]
    for routing in (ids2, ids1):
        ids.copy_(routing.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        w_offs, w_row_of, w_src = route_ref(routing, G)
        assert torch.equal(offs.cpu(), w_offs) and torch.equal(row_of.cpu().reshape(-1), w_row_of) and torch.equal(src.cpu(), w_src)
        assert all(bool((j == SENT_B).all()) for j in junk)


# ---- scatter-quantise ------------------------------------------------------------------------------------------------------------------

SQ_T, SQ_K, SQ_G = 37, 3, 5


@pytest.fixture(scope="module")
def plan():
    """T = 37, k = 3 with a few dropped ids: (row_of (T, k) int32 on the CPU, src_of_row)"""
    ids = random_ids(torch.Generator().manual_seed(11), SQ_T, SQ_K, SQ_G, dropped=0.12)
    ids[4] = torch.tensor([1, 3, 1])   # token 4 is stored three times, twice for one expert
    offs, row_of, src = route_ref(ids, SQ_G)
    assert 0 < int(offs[-1]) < SQ_T * SQ_K
    return row_of.reshape(SQ_T, SQ_K), src


def make_x(dtype, cols, seed, ld_in=None):
    """(T, cols) on the device (a view of a wider allocation when ld_in is given); token 4 holds a NaN and an inf, token 7 is all zero"""
    x = torch.randn((SQ_T, cols), generator=torch.Generator().manual_seed(seed)) * torch.logspace(-3, 3, SQ_T)[:, None]
    x[4, 1], x[4, cols - 2] = float("nan"), float("inf")
    x[7] = 0.0
    x = x.to(dtype)
    if ld_in is None:
        return x.to(DEV)
    wide = torch.zeros((SQ_T, ld_in), dtype=dtype, device=DEV)
    wide[:, :cols] = x
    return wide[:, :cols]


# every rung of the ladder: one wave per token (16-bit: up to 4096 columns, fp32: 2048), four waves, eight waves (fp32 beyond 8192)
SQ_SHAPES = [(torch.bfloat16, 16), (torch.bfloat16, 128), (torch.bfloat16, 1040), (torch.bfloat16, 4096), (torch.bfloat16, 4112), (torch.bfloat16, 16384),
             (torch.float16, 128), (torch.float16, 4112), (torch.float32, 16), (torch.float32, 1040), (torch.float32, 2064), (torch.float32, 16384)]


@pytest.mark.parametrize("dtype,cols", SQ_SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_scatter_quantize_row_equals_the_rowwise_quantiser(lib, N_, plan, dtype, cols):
    row_of, _src = plan
    x = make_x(dtype, cols, cols)
    for enc in (L.ENC_REFERENCE, L.ENC_RNE):
        check_scatter(lib, N_, x, row_of, False, enc)


@pytest.mark.parametrize("dtype,cols", SQ_SHAPES + [(torch.bfloat16, 144), (torch.float32, 144)], ids=lambda v: str(v).replace("torch.", ""))
def test_scatter_quantize_block128_equals_the_group_quantiser(lib, N_, plan, dtype, cols):
    row_of, _src = plan
    check_scatter(lib, N_, make_x(dtype, cols, cols + 1), row_of, True, L.ENC_RNE)


def test_scatter_quantize_padded_rows_and_strided_scales(lib, N_, plan):
    row_of, _src = plan
    for dtype, cols, pad in ((torch.bfloat16, 1040, 8), (torch.float32, 272, 4), (torch.float16, 4112, 24)):
        x = make_x(dtype, cols, 5, ld_in=cols + pad)
        assert x.stride(0) == cols + pad
        ncb = (cols + 127) // 128
        check_scatter(lib, N_, x, row_of, False, L.ENC_RNE, ld_out=cols + 8, s_sr=3)
        check_scatter(lib, N_, x, row_of, True, L.ENC_RNE, ld_out=cols + 16, s_sr=2 * ncb + 3, s_sk=2)


def test_scatter_quantize_skips_destinations_outside_the_output(lib, N_, plan):
    """row_of entries rows_out, 2^31 - 1 and negative ones: skipped, like -1; and an output of fewer rows than the plan has: rows at or beyond
    rows_out are skipped too.  Guards intact (checked in run_scatter)."""
    row_of, _src = plan
    bad = row_of.clone()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[4, 0] = SQ_T * SQ_K, INT32_MAX, INT32_MIN, -5
    x = make_x(torch.bfloat16, 1040, 9)
    for group in (False, True):
        check_scatter(lib, N_, x, bad, group, L.ENC_RNE)
        check_scatter(lib, N_, x, bad, group, L.ENC_RNE, rows_out=50)


def test_scatter_quantize_op(N_, plan):
    row_of, src = plan
    x = make_x(torch.bfloat16, 256, 2)
    tok = (src.clamp(min=0) // SQ_K).long()
    own = src >= 0
    for scale, ref in (("row", lambda: N_.fp8_quantize_rowwise(x)), ("block128", lambda: N_.fp8_act_quantize(x, "none", False, "block128"))):
        q, s = N_.fp8_moe_scatter_quantize(x, row_of.to(DEV), scale)
        wq, ws = ref()
        assert q.shape == (SQ_T * SQ_K, 256) and s.shape == (SQ_T * SQ_K, ws.shape[1])
        assert torch.equal(q.cpu()[own], wq.cpu()[tok][own]) and torch.equal(bits(s.cpu()[own]), bits(ws.cpu()[tok][own])), scale


# ---- combine ---------------------------------------------------------------------------------------------------------------------------

CB_T = 9
def check_combine(lib, y, row_of, weights, out_dtype, ld_out=None):
    check_combine_with(lib, y, row_of, weights, out_dtype, ld_out, gone_tokens=(3,))   # combine_plan: token 3 loses every assignment


def combine_plan(gen, k, rows):
    """(T, k) rows: distinct owned rows in a random order; some assignments dropped (-1, rows, INT32_MAX); token 3 loses all of them"""
    row_of = torch.randperm(rows, generator=gen)[:CB_T * k].reshape(CB_T, k).to(torch.int32)
    drop = torch.tensor([-1, rows, INT32_MAX], dtype=torch.int32)[torch.randint(0, 3, (CB_T, k), generator=gen)]
    row_of = torch.where(torch.rand((CB_T, k), generator=gen) < 0.2, drop, row_of)
    row_of[3] = -1
    return row_of


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["to-f32", "to-f16", "to-bf16"])
@pytest.mark.parametrize("y_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_combine_equals_the_sequential_float32_loop(lib, y_dtype, out_dtype):
    gen = torch.Generator().manual_seed(77)
    for N in (1, 7, 8, 4096, 4100):
        for k in (1, 6, 8):
            rows = CB_T * k + 3
            y = torch.randn((rows, N), generator=gen).to(y_dtype).to(DEV)
            w = torch.softmax(torch.randn((CB_T, k), generator=gen), dim=1) * 1.7
            row_of = combine_plan(gen, k, rows)
            check_combine(lib, y, row_of, w, out_dtype)
            if k == 6:
                check_combine(lib, y, row_of, None, out_dtype)


def test_combine_padded_rows_misaligned_bases_and_empty_inputs(lib):
    gen = torch.Generator().manual_seed(78)
    k, N = 6, 264
    rows = CB_T * k + 3
    row_of = combine_plan(gen, k, rows)
    w = torch.rand((CB_T, k), generator=gen)
    for dtype in (torch.bfloat16, torch.float32):
        wide = torch.randn((rows, N + 24), generator=gen).to(dtype).to(DEV)
        check_combine(lib, wide[:, :N], row_of, w, dtype, ld_out=N + 8)        # 16-byte pieces through padded leading dimensions
        check_combine(lib, wide[:, 1:N + 1], row_of, w, dtype, ld_out=N + 3)   # a base and an ld_out that allow no vector access
    # k = 0 and rows = 0: every output row is written with zeros
    y = torch.randn((rows, N), generator=gen).to(torch.bfloat16).to(DEV)
    assert bool((run_combine(lib, y, torch.empty((CB_T, 0), dtype=torch.int32), None, torch.bfloat16) == 0).all())
    assert bool((run_combine(lib, y[:0], row_of, w, torch.float32) == 0).all())


def test_combine_op(N_):
    gen = torch.Generator().manual_seed(79)
    k, N = 8, 512
    rows = CB_T * k
    y = torch.randn((rows, N), generator=gen).to(torch.bfloat16).to(DEV)
    row_of, w = combine_plan(gen, k, rows), torch.rand((CB_T, k), generator=gen)
    got = N_.fp8_moe_combine(y, row_of.to(DEV), w.to(DEV))
    assert got.dtype == torch.bfloat16 and torch.equal(bits(got.cpu()), bits(combine_ref(y, row_of, w, torch.bfloat16)))
    got = N_.fp8_moe_combine(y, row_of.to(DEV), None, out_dtype=torch.float32)
    assert torch.equal(got.cpu(), combine_ref(y, row_of, None, torch.float32))


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def layers(N_):
    return {4: Layer(N_, 4, 256, 128, 256, 1), 64: Layer(N_, 64, 256, 128, 256, 2)}


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("recipe", ["row", "block128"])
@pytest.mark.parametrize("T,k,G", [(33, 2, 4), (3, 8, 64)])
def test_forward_equals_route_mlp_combine(N_, layers, T, k, G, recipe, x_dtype):
    gen = torch.Generator().manual_seed(T * 100 + k)
    layer = layers[G]
    fwd, _mlp = forward_pair(N_, recipe)
    weights = layer.row if recipe == "row" else layer.block
    x = torch.randn((T, layer.K), generator=gen).to(x_dtype).to(DEV)
    ids, wts = gate(gen, T, k, G)
    with L.kernel_timer(16) as kt:
        got = fwd(x, ids.to(DEV), wts.to(DEV), *weights, kernel=TILE)
    torch.cuda.synchronize()
    assert len(kt.ms) == 6   # route, scatter-quantise, gate_up GEMM, act + quantise, down GEMM, combine
    assert got.shape == (T, layer.N) and got.dtype == x_dtype
    assert torch.equal(bits(got.cpu()), bits(forward_reference(N_, recipe, layer, x, ids, wts)))


@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_with_dropped_ids_biases_and_an_out_dtype(N_, layers, recipe):
    gen = torch.Generator().manual_seed(5)
    layer = layers[4]
    fwd, _mlp = forward_pair(N_, recipe)
    weights = layer.row if recipe == "row" else layer.block
    x = torch.randn((33, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids, wts = gate(gen, 33, 2, 4, dropped=0.25)
    ids[6] = -1   # a token without any expert: zeros
    got = fwd(x, ids.to(torch.int32).to(DEV), wts.to(DEV), *weights, bias1=layer.bias1, bias2=layer.bias2, out_dtype=torch.float32, kernel=TILE)
    want = forward_reference(N_, recipe, layer, x, ids, wts, torch.float32, bias=True)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want) and bool((got[6] == 0).all())
    got = fwd(x, ids.to(DEV), None, *weights, kernel=TILE)   # no weights: the plain sum
    assert torch.equal(bits(got.cpu()), bits(forward_reference(N_, recipe, layer, x, ids, None)))


@pytest.mark.parametrize("recipe", ["row", "block128"])
def test_forward_captured_into_a_graph_follows_a_new_routing_on_replay(N_, layers, recipe):
    gen = torch.Generator().manual_seed(6)
    layer = layers[64]
    fwd, _mlp = forward_pair(N_, recipe)
    weights = layer.row if recipe == "row" else layer.block
    T, k = 3, 8
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids1, wts1 = gate(gen, T, k, 64)
    ids2, wts2 = gate(gen, T, k, 64)
    assert not torch.equal(ids1, ids2)
    ids, wts = ids1.to(DEV), wts1.to(DEV)
    eager1 = fwd(x, ids, wts, *weights, kernel=TILE)   # (also the warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a host sync or a read of the routing inside the capture would fail it)
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
