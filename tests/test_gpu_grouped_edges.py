"""GPU (MI355X): the edges of the grouped (MoE) FP8 GEMM that tests/test_gpu_grouped.py leaves out.  That file runs one shape (G = 6,
M_total = 240, N = 200, K = 400); at it the K loop of the five two-step tiles never refills a ring slot, the L2 prefetch plan is off
(K is no multiple of a stage), the offsets walk stays inside its first batch of eight and the surplus cut sees few residues.  Here:

 1. deep K - every ring wraps, the prefetch live (K = 1536) and off behind a partial last step (K = 1296); groups of five m-tiles (a full
    set of four plus a short one), two, one row, none;
 2. shallow K - 16 (one masked step), 128 (half a stage), 144, 256 (exactly one two-step stage, prefetch plan live with one stage);
 3. G across the batch-of-eight boundary of fp8mi_group_slot / fp8mi_group_tiles on the DEVICE (8, 9, 16, 17, 64) and the API maximum 1024;
 4. every residue mod 8 of the real tile count in the surplus-workgroup cut, the all-empty launch included;
 5. degenerate splits (G = 1, M_total = 1, M_total below every BM, one group owning everything);
 6. float16 output, bf16 / f16 bias;  7. strided blockwise scales;  8. NaN bytes in one expert's B and on both sides of a group boundary;
 9. offs written by a kernel right before the launch, no synchronisation;  10. the launch counts the fp8_moe_* docstrings promise.

Every case uses the three checks of tests/test_gpu_grouped.py (tests/grouped_ref.py): each group's rows BIT-equal to the single-problem
call on the same tile with split_k=1; the sentinel around C, in the rows no group owns and in the columns behind N; and, once per shape, an
independent reference - oracle.scaled_mm(accumulate="f64") within MFMA_TOL * oracle.abs_dot_bound (include/fp8mi.h), np.array_equal on
exact data, and for the blockwise forms mm_ref of tests/blockwise_ref.py at the bar of tests/test_gpu_blockwise_edges.py,
(1e-3 + nkb 2^-23) * bound.  Cases that name no tile run KERNEL_AUTO as well; its per-group reference runs the tile
fp8mi_choose_kernel_grouped names."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from blockwise_ref import mm_ref
from grouped_ref import (DEV, EXACT_VALS, GUARD, MFMA_TOL, SENTINEL, TILE_DIMS, TILES, Case, assert_untouched, blockwise_scales, clamped_groups,
                         exact_problem, guarded, reference_rows, resolved_tile, run_and_compare, run_and_compare_blockwise, t)

pytestmark = pytest.mark.gpu

AUTO_AND_TILES = [L.KERNEL_AUTO] + TILES
E_UNSUPPORTED = -4   # include/fp8mi.h
BASE_SIZES = [0, 1, 130, 64, 33, 0]
BASE_OFFS = np.cumsum(BASE_SIZES).astype(np.int32)
BASE_M, BASE_N, BASE_K = 240, 200, 400
ROW = L.SCALE_ROW


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


_CASES = {}


def case_of(offs, m_total, n, k, seed=1):
    """the device tensors of one shape, built once per module run"""
    key = (tuple(int(o) for o in offs), m_total, n, k, seed)
    if key not in _CASES:
        _CASES[key] = Case(offs, m_total, n, k, seed)
    return _CASES[key]


_BW = {}


def bw_of(c, block_b):
    """(scale_a, scale_b) numpy and device, once per (case, block_b)"""
    key = (id(c), block_b)
    if key not in _BW:
        sa, sb = blockwise_scales(np.random.default_rng([5, block_b, c.k]), c.m_total, c.G, c.n, c.k, block_b)
        _BW[key] = (sa, sb, t(sa), t(sb))
    return _BW[key]


def check_oracle(oracle, c, got, what, groups=None):
    """got: (m_total, n) float64 of a tensorwise run with row scales on both sides, no epilogue"""
    for g, (s, e) in enumerate(c.groups if groups is None else groups):
        if e > s:
            exact = oracle.scaled_mm(c.A_np[s:e], c.B_np[g], c.sa_np[s:e], c.sb_np[g], accumulate="f64")
            bound = oracle.abs_dot_bound(c.A_np[s:e], c.B_np[g], c.sa_np[s:e], c.sb_np[g])
            err = np.abs(got[s:e] - exact)
            assert np.all(err <= MFMA_TOL * bound + 1e-30), (what, g, float(np.max(err / (bound + 1e-300))))


_BW_REFS = {}


def check_mm_ref(c, block_b, got, what):
    """got: (m_total, n) float64 of a blockwise run on bw_of(c, block_b), no epilogue"""
    sa, sb, _, _ = bw_of(c, block_b)
    bar = MFMA_TOL + -(-c.k // 128) * 2.0 ** -23
    for g, (s, e) in enumerate(c.groups):
        if e > s:
            key = (id(c), block_b, g)
            if key not in _BW_REFS:
                _BW_REFS[key] = mm_ref(c.A_np[s:e], c.B_np[g], sa[s:e], sb[g], 1, block_b)
            exact, bound = _BW_REFS[key]
            err = np.abs(got[s:e] - exact)
            assert np.all(err <= bar * bound + 1e-30), (what, g, float(np.max(err / (bound + 1e-300))), bar)


def f64(x):
    return x.float().cpu().numpy().astype(np.float64)


# ---- 1. deep K: ring wrap and live prefetch --------------------------------------------------------------------------------------
DEEP_SIZES = [513, 0, 130, 1, 37]     # BM = 128: 5 m-tiles (4 + a short set of 1), none, 2 m-tiles, one row, one partial tile; 19 rows unowned
DEEP_M, DEEP_N = 700, 200
DEEP_KS = [1536, 1296]                # 6 x 256: 6 / 12 stages, prefetch live on 128x64;  5 x 256 + 16: a partial last step, prefetch off


def deep_case(K):
    return case_of(np.cumsum(DEEP_SIZES), DEEP_M, DEEP_N, K, seed=11)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", DEEP_KS)
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_deep_k_every_group_equals_the_single_problem_call(N_, tile, K, out_dtype):
    c = deep_case(K)
    assert sum(DEEP_SIZES) == DEEP_M - 19
    for epi in (False, True):
        run_and_compare(N_, c, tile, out_dtype, ROW, ROW, epi, ldc=None if epi else DEEP_N + 8)


@pytest.mark.parametrize("K", DEEP_KS)
def test_deep_k_against_the_oracle(N_, oracle, K):
    c = deep_case(K)
    for tile in AUTO_AND_TILES:
        buf, C = guarded(torch.float32, c.m_total, c.n)
        N_.fp8_scaled_mm_grouped(c.A, c.B, c.sa[ROW], c.sb[ROW], c.offs, kernel=tile, out=C)
        check_oracle(oracle, c, f64(C), (tile, K))
        assert_untouched(buf, c.n, c.groups)


@pytest.mark.parametrize("block_b", [1, 128])
@pytest.mark.parametrize("K", DEEP_KS)
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_deep_k_blockwise(N_, tile, K, block_b):
    """K = 1296: 11 scale blocks, the last one of 16 k"""
    c = deep_case(K)
    _, _, sa, sb = bw_of(c, block_b)
    assert sa.shape[1] == (12 if K == 1536 else 11)
    buf, C = run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, torch.float32, False)
    check_mm_ref(c, block_b, f64(C), (tile, K, block_b))
    run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, torch.bfloat16, True, ldc=DEEP_N + 8)


# ---- 2. shallow K ----------------------------------------------------------------------------------------------------------------
SHALLOW_KS = [16, 128, 144, 256]


@pytest.mark.parametrize("K", SHALLOW_KS)
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_shallow_k_tensorwise(N_, oracle, tile, K):
    c = case_of(BASE_OFFS, BASE_M, BASE_N, K, seed=12)
    buf, C = run_and_compare(N_, c, tile, torch.float32, ROW, ROW, False, ldc=BASE_N + 8)
    check_oracle(oracle, c, f64(C), (tile, K))
    run_and_compare(N_, c, tile, torch.bfloat16, ROW, ROW, True)
    run_and_compare(N_, c, tile, torch.float32, L.SCALE_TENSOR, L.SCALE_TENSOR, True)


@pytest.mark.parametrize("K", SHALLOW_KS)
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_shallow_k_blockwise(N_, tile, K):
    c = case_of(BASE_OFFS, BASE_M, BASE_N, K, seed=12)
    for block_b in (128, 1):
        _, _, sa, sb = bw_of(c, block_b)
        buf, C = run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, torch.float32, False, ldc=BASE_N + 8)
        check_mm_ref(c, block_b, f64(C), (tile, K, block_b))
        run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, torch.bfloat16, True)


# ---- 3. more than eight groups -----------------------------------------------------------------------------------------------------
MANY_GS = [8, 9, 16, 17, 64]
MANY_N, MANY_K = 72, 144


def many_sizes(G, BM):
    """seeded: about a third of the groups empty, the others 1 .. 2 BM + 1 rows; a group behind the first batch of eight is never the
    only non-empty one (G > 8), so a walk that loses the later batches loses rows"""
    rng = np.random.default_rng([3, G, BM])
    sizes = np.where(rng.random(G) < 1.0 / 3.0, 0, rng.integers(1, 2 * BM + 2, G))
    sizes[G - 1] = BM + 1                    # the last group of the last batch is real: two m-tiles behind every other group
    if G > 8:
        sizes[8] = max(int(sizes[8]), 1)     # and so is the first group of the second batch
    return [int(x) for x in sizes]


def many_case(G, BM):
    sizes = many_sizes(G, BM)
    return case_of(np.cumsum(sizes), sum(sizes) + 5, MANY_N, MANY_K, seed=13)


@pytest.mark.parametrize("G", MANY_GS)
@pytest.mark.parametrize("tile", TILES)
def test_more_than_eight_groups_bit_equality(N_, tile, G):
    c = many_case(G, TILE_DIMS[tile][0])
    empty = sum(1 for s, e in c.groups if e == s)
    assert c.G == G and (G < 16 or G // 6 <= empty <= G // 2)
    run_and_compare(N_, c, tile, torch.float32, ROW, ROW, False, ldc=MANY_N + 8)
    run_and_compare(N_, c, tile, torch.bfloat16, ROW, ROW, True)


@pytest.mark.parametrize("G", MANY_GS)
def test_more_than_eight_groups_auto_and_blockwise(N_, G):
    c = many_case(G, 64)
    run_and_compare(N_, c, L.KERNEL_AUTO, torch.float32, ROW, ROW, True)
    _, _, sa, sb = bw_of(c, 128)
    for tile in (L.KERNEL_AUTO, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64):
        buf, C = run_and_compare_blockwise(N_, c, sa, sb, 128, tile, torch.float32, False)
    check_mm_ref(c, 128, f64(C), G)


@pytest.mark.parametrize("G", MANY_GS)
def test_more_than_eight_groups_exact_data_equals_the_numpy_product(N_, oracle, G):
    for BM in (128, 64, 32):
        sizes = many_sizes(G, BM)
        offs, m_total = np.cumsum(sizes).astype(np.int32), sum(sizes) + 5
        A, B, sa, sb, exact = exact_problem(oracle, offs, m_total, MANY_N, MANY_K, seed=G + BM)
        dev = [t(x) for x in (A, B, sa, sb, offs)]
        for tile in [k for k in TILES if TILE_DIMS[k][0] == BM] + ([L.KERNEL_AUTO] if BM == 64 else []):
            buf, C = guarded(torch.float32, m_total, MANY_N)
            N_.fp8_scaled_mm_grouped(*dev, kernel=tile, out=C)
            assert np.array_equal(C.cpu().numpy(), exact), (tile, G)
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + m_total:] == SENTINEL).all())


BIG_G, BIG_N, BIG_K = 1024, 40, 32


def big_sizes():
    """G = 1024, the API maximum: most groups hold 0 .. 2 rows, one holds 200, the last five none"""
    rng = np.random.default_rng(1024)
    sizes = rng.integers(0, 3, BIG_G)
    sizes[517] = 200
    sizes[-5:] = 0
    return [int(x) for x in sizes]


def test_1024_groups_exact_data_every_tile_equals_one_numpy_product(N_, oracle):
    sizes = big_sizes()
    m_total = 1500
    assert 1100 <= sum(sizes) <= m_total - 7
    offs = np.cumsum(sizes).astype(np.int32)
    rng = np.random.default_rng(8)
    A = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (m_total, BIG_K))]
    sa = np.exp2(rng.integers(-2, 3, m_total)).astype(np.float32)
    B = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (BIG_G, BIG_N, BIG_K))]
    sb = np.exp2(rng.integers(-2, 3, (BIG_G, BIG_N))).astype(np.float32)
    owner = np.repeat(np.arange(BIG_G), sizes)                         # the expert of every owned row
    owned = len(owner)
    a64, b64 = oracle.decode(A).astype(np.float64), oracle.decode(B).astype(np.float64)
    exact = np.full((m_total, BIG_N), SENTINEL, dtype=np.float32)
    exact[:owned] = np.einsum("mk,mnk->mn", a64[:owned], b64[owner]) * sa[:owned, None] * sb[owner]
    dev = [t(x) for x in (A, B, sa, sb, offs)]
    for tile in AUTO_AND_TILES:
        buf, C = guarded(torch.float32, m_total, BIG_N, BIG_N + 8)
        N_.fp8_scaled_mm_grouped(*dev, kernel=tile, out=C)
        assert np.array_equal(C.cpu().numpy(), exact), tile
        assert_untouched(buf, BIG_N, [(0, owned)])


def test_1025_groups_are_refused(N_):
    G = BIG_G + 1
    A, B = torch.zeros((64, BIG_K), dtype=torch.uint8, device=DEV), torch.zeros((G, BIG_N, BIG_K), dtype=torch.uint8, device=DEV)
    sa, sb = torch.ones(64, device=DEV), torch.ones((G, BIG_N), device=DEV)
    offs = torch.zeros(G, dtype=torch.int32, device=DEV)
    buf, C = guarded(torch.float32, 64, BIG_N)
    with pytest.raises(L.Fp8miError, match=f"code {E_UNSUPPORTED}"):
        N_.fp8_scaled_mm_grouped(A, B, sa, sb, offs, out=C)
    with pytest.raises(L.Fp8miError, match=f"code {E_UNSUPPORTED}"):
        N_.fp8_scaled_mm_grouped_blockwise(A, B, torch.ones((64, 1), device=DEV), torch.ones((G, 1, 1), device=DEV), offs, out=C)
    assert bool((buf == SENTINEL).all())


# ---- 4. the surplus cut at every residue -------------------------------------------------------------------------------------------
CUT_G, CUT_K = 8, 144


def cut_case(tile):
    BM, BN = TILE_DIMS[tile]
    return case_of([0] * CUT_G, CUT_G * (BM + 1) + 3, 3 * BN - 8, CUT_K, seed=14)   # (offs are passed per run)


@pytest.mark.parametrize("rows", ["1", "BM+1"])
@pytest.mark.parametrize("tile", TILES)
def test_surplus_cut_at_every_residue(N_, oracle, tile, rows):
    """tn = 3 (the last n-tile partial); the first r of 8 groups hold `rows` rows: real = 3 r (one m-tile each) or 6 r (two) tiles, and
    3 r mod 8 takes every value 0 .. 7 over r = 0 .. 8.  The launch holds M_total / BM + 8 slots whatever r is."""
    BM, BN = TILE_DIMS[tile]
    per = 1 if rows == "1" else BM + 1
    c = cut_case(tile)
    assert -(-c.n // BN) == 3 and c.n % BN != 0
    seen = set()
    for r in range(CUT_G + 1):
        offs = [per * min(g + 1, r) for g in range(CUT_G)]
        groups = clamped_groups(offs, c.m_total)
        seen.add((sum(-(-(e - s) // BM) for s, e in groups) * 3) & 7)
        buf, C = run_and_compare(N_, c, tile, torch.float32, ROW, ROW, r % 2 == 1, ldc=c.n + 8, offs=t(np.array(offs, dtype=np.int32)),
                                 groups=groups)
        if r == CUT_G:
            check_oracle(oracle, c, f64(C), (tile, rows), groups)
    assert seen == (set(range(8)) if per == 1 else {0, 2, 4, 6})


def test_all_groups_empty_writes_nothing_and_completes(N_):
    """real = 0: every workgroup of every tile is surplus.  One sentinel buffer for all launches, one synchronisation."""
    wide = max(3 * bn - 8 for _, bn in TILE_DIMS.values())
    m_max = max(cut_case(tile).m_total for tile in TILES)
    buf = torch.full((GUARD + m_max + GUARD, wide + 8), SENTINEL, dtype=torch.float32, device=DEV)
    for offs in ([0] * CUT_G, [-3] * CUT_G):
        offs_d = t(np.array(offs, dtype=np.int32))
        for tile in TILES:
            c = cut_case(tile)
            C = buf[GUARD:GUARD + c.m_total, :c.n]
            N_.fp8_scaled_mm_grouped(c.A, c.B, c.sa[ROW], c.sb[ROW], offs_d, bias=c.bias, kernel=tile, out=C)
            _, _, sa, sb = bw_of(c, 128)
            N_.fp8_scaled_mm_grouped_blockwise(c.A, c.B, sa, sb, offs_d, kernel=tile, out=C)
        c = cut_case(L.KERNEL_GEMM_64x64)
        N_.fp8_scaled_mm_grouped(c.A, c.B, c.sa[ROW], c.sb[ROW], offs_d, out=buf[GUARD:GUARD + c.m_total, :c.n])
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- 5. degenerate splits ----------------------------------------------------------------------------------------------------------
DEGENERATE = {
    "G=1 owns all": ([BASE_M], BASE_M),
    "G=1 empty": ([0], BASE_M),
    "M_total=1": ([0, 1, 1], 1),
    "M_total=31": ([7, 7, 30, 31], 31),
    "last owns all": ([0, 0, 0, BASE_M], BASE_M),
    "first owns all": ([BASE_M] * 4, BASE_M),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_degenerate_splits(N_, oracle, tile, name):
    offs, m_total = DEGENERATE[name]
    c = case_of(offs, m_total, BASE_N, BASE_K, seed=15)
    buf, C = run_and_compare(N_, c, tile, torch.float32, ROW, ROW, False, ldc=BASE_N + 8)
    check_oracle(oracle, c, f64(C), (tile, name))
    run_and_compare(N_, c, tile, torch.bfloat16, ROW, ROW, True)
    if name == "G=1 owns all":      # the whole call IS the single-problem call
        whole = N_.fp8_scaled_mm(c.A, c.B[0], c.sa[ROW], c.sb[ROW][0], kernel=resolved_tile(c, tile, torch.float32, BASE_N + 8), split_k=1)
        assert torch.equal(C, whole)
    _, _, sa, sb = bw_of(c, 128)
    run_and_compare_blockwise(N_, c, sa, sb, 128, tile, torch.bfloat16, True)


# ---- 6. output and bias dtypes -----------------------------------------------------------------------------------------------------
def base_case():
    return case_of(BASE_OFFS, BASE_M, BASE_N, BASE_K, seed=1)


@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_f16_output_and_half_precision_bias(N_, oracle, tile):
    """the bias of expert g starts g N elements of ITS type behind expert 0's: 2 bytes each for bf16 / f16"""
    c = base_case()
    for epi in (False, True):
        run_and_compare(N_, c, tile, torch.float16, L.SCALE_TENSOR, ROW, epi, ldc=None if epi else BASE_N + 8)
    run_and_compare(N_, c, tile, torch.float16, ROW, ROW, True)
    for bias_dtype in (torch.bfloat16, torch.float16):
        bias = c.bias.to(bias_dtype)
        for out_dtype in (torch.float32, torch.bfloat16):
            run_and_compare(N_, c, tile, out_dtype, ROW, ROW, True, bias=bias)
        # independently: the fp32 result with the bias alone, against the oracle's product plus that expert's bias
        buf, C = guarded(torch.float32, c.m_total, c.n)
        N_.fp8_scaled_mm_grouped(c.A, c.B, c.sa[ROW], c.sb[ROW], c.offs, bias=bias, kernel=tile, out=C)
        got, b64 = f64(C), f64(bias)
        for g, (s, e) in enumerate(c.groups):
            if e > s:
                exact = oracle.scaled_mm(c.A_np[s:e], c.B_np[g], c.sa_np[s:e], c.sb_np[g], accumulate="f64") + b64[g][None, :]
                bound = oracle.abs_dot_bound(c.A_np[s:e], c.B_np[g], c.sa_np[s:e], c.sb_np[g]) + np.abs(b64[g])[None, :]
                assert np.all(np.abs(got[s:e] - exact) <= MFMA_TOL * bound + 1e-30), (tile, bias_dtype, g)


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64])
def test_f16_output_and_half_precision_bias_blockwise(N_, tile):
    c = base_case()
    for block_b in (128, 1):
        _, _, sa, sb = bw_of(c, block_b)
        for epi in (False, True):
            run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, torch.float16, epi, ldc=BASE_N + 8)
        for bias_dtype in (torch.bfloat16, torch.float16):
            for out_dtype in (torch.float32, torch.bfloat16):
                run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, out_dtype, True, bias=c.bias.to(bias_dtype))


# ---- 7. strided scales on the blockwise form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_b", [128, 1])
@pytest.mark.parametrize("tile", AUTO_AND_TILES)
def test_blockwise_strided_scales_are_read_in_place(N_, tile, block_b):
    """scale_b: sliced out of a wider (G + 1, nkb + 2, nrb + 3) tensor, then transposed in its last two dimensions - an expert stride, a row
    stride of 1 and a K stride of nrb + 3; scale_a: a column slice of a wider tensor.  Every float around them is NaN."""
    c = base_case()
    sa_np, sb_np, sa_c, sb_c = bw_of(c, block_b)
    G, nrb, nkb = sb_np.shape
    wide_b = torch.full((G + 1, nkb + 2, nrb + 3), float("nan"), device=DEV)
    wide_b[1:, 1:1 + nkb, 2:2 + nrb] = sb_c.transpose(1, 2)
    sb_v = wide_b[1:, 1:1 + nkb, 2:2 + nrb].transpose(1, 2)
    wide_a = torch.full((c.m_total, nkb + 3), float("nan"), device=DEV)
    wide_a[:, 1:1 + nkb] = sa_c
    sa_v = wide_a[:, 1:1 + nkb]
    assert sb_v.shape == sb_c.shape and sb_v.stride() == ((nkb + 2) * (nrb + 3), 1, nrb + 3) and not sb_v.is_contiguous()
    assert sa_v.stride() == (nkb + 3, 1) and not sa_v.is_contiguous() and torch.equal(sb_v, sb_c) and torch.equal(sa_v, sa_c)
    for out_dtype, epi in ((torch.float32, False), (torch.bfloat16, True)):
        kw = dict(block_b=block_b, bias=c.bias if epi else None, scale_result=c.sr if epi else None, out_dtype=out_dtype, kernel=tile)
        buf_c, C_c = guarded(out_dtype, c.m_total, c.n)
        N_.fp8_scaled_mm_grouped_blockwise(c.A, c.B, sa_c, sb_c, c.offs, out=C_c, **kw)
        buf_v, C_v = guarded(out_dtype, c.m_total, c.n)
        N_.fp8_scaled_mm_grouped_blockwise(c.A, c.B, sa_v, sb_v, c.offs, out=C_v, **kw)
        assert not bool(torch.isnan(buf_v).any()) and torch.equal(buf_v, buf_c), (tile, block_b, out_dtype)
        assert_untouched(buf_v, c.n, c.groups)
        if not epi:
            check_mm_ref(c, block_b, f64(C_c), (tile, block_b))
    # the views against the per-group calls on the contiguous scales
    run_and_compare_blockwise(N_, c, sa_v, sb_v, block_b, tile, torch.float32, True, sa_ref=sa_c, sb_ref=sb_c)


# ---- 8. NaN bytes at group edges -----------------------------------------------------------------------------------------------------
NAN_TILES = [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64]
NAN_MODES = [L.NAN_ZERO, L.NAN_PROPAGATE]


def nan_rows(C, groups):
    """the owned part of C as a bool (rows, n) NaN map on the host, unowned rows False"""
    m = torch.zeros(C.shape, dtype=torch.bool)
    for s, e in groups:
        m[s:e] = torch.isnan(C[s:e]).cpu()
    return m


@pytest.mark.parametrize("blockwise", [False, True], ids=["tensorwise", "blockwise"])
@pytest.mark.parametrize("nan_mode", NAN_MODES)
def test_a_nan_byte_in_one_experts_b(N_, nan_mode, blockwise):
    """B[3][77, 261] = NaN: under PROPAGATE exactly column 77 of group 3's rows (131 .. 194) is NaN; under ZERO nothing is"""
    c = base_case()
    B = c.B.clone()
    B[3, 77, 261] = 0xFF
    want = torch.zeros((c.m_total, c.n), dtype=torch.bool)
    if nan_mode == L.NAN_PROPAGATE:
        want[131:195, 77] = True
    assert c.groups[3] == (131, 195)
    for tile in NAN_TILES:
        if blockwise:
            _, _, sa, sb = bw_of(c, 128)
            buf, C = run_and_compare_blockwise(N_, c, sa, sb, 128, tile, torch.float32, False, B=B, nan_mode=nan_mode, bits=True)
        else:
            buf, C = run_and_compare(N_, c, tile, torch.float32, ROW, ROW, False, B=B, nan_mode=nan_mode, bits=True)
        assert torch.equal(nan_rows(C, c.groups), want), tile


@pytest.mark.parametrize("blockwise", [False, True], ids=["tensorwise", "blockwise"])
@pytest.mark.parametrize("nan_mode", NAN_MODES)
def test_nan_bytes_on_both_sides_of_a_group_boundary(N_, nan_mode, blockwise):
    """row 130 is the last of group 2, row 131 the first of group 3: under PROPAGATE those two rows are NaN and no other"""
    c = base_case()
    A = c.A.clone()
    A[130, 399] = 0x7F
    A[131, 0] = 0xFF
    assert c.groups[2][1] == 131 and c.groups[3][0] == 131
    want = torch.zeros((c.m_total, c.n), dtype=torch.bool)
    if nan_mode == L.NAN_PROPAGATE:
        want[130:132] = True
    for tile in NAN_TILES:
        if blockwise:
            _, _, sa, sb = bw_of(c, 1)
            buf, C = run_and_compare_blockwise(N_, c, sa, sb, 1, tile, torch.float32, False, A=A, nan_mode=nan_mode, bits=True)
        else:
            buf, C = run_and_compare(N_, c, tile, torch.float32, ROW, ROW, True, A=A, nan_mode=nan_mode, bits=True)
        assert torch.equal(nan_rows(C, c.groups), want), tile


# ---- 9. offs written on the device, no synchronisation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64])
def test_offs_written_by_a_kernel_right_before_the_launch(N_, tile):
    """Eager mode: the expert counts, their cumulative sum and its copy into ONE int32 buffer are device work queued right in front of the
    grouped launch; the next routing overwrites the buffer behind it.  Each launch must see its own routing's offs (the scalar cache is
    invalidated at kernel start: fp8mi_group_slot.h).  The counts are a one-hot sum: torch.bincount reads its result size back."""
    c = base_case()
    rng = np.random.default_rng(9)
    routed = [220, 240, 3]                                                     # tokens routed; the rows behind them stay unowned
    ids_np = [np.sort(rng.integers(0, c.G, r)) for r in routed]
    ids_np[1][:] = np.sort(rng.choice([1, 4, 5], routed[1]))                   # experts 0, 2, 3 empty
    ids = [t(x.astype(np.int64)) for x in ids_np]
    experts = torch.arange(c.G, device=DEV)
    offs = torch.zeros(c.G, dtype=torch.int32, device=DEV)
    outs = [guarded(torch.float32, c.m_total, c.n, c.n + 8) for _ in routed]
    torch.cuda.synchronize()
    for i, (buf, C) in zip(ids, outs):
        counts = (i[:, None] == experts[None, :]).sum(0)
        offs.copy_(torch.cumsum(counts, 0))
        N_.fp8_scaled_mm_grouped(c.A, c.B, c.sa[ROW], c.sb[ROW], offs, kernel=tile, out=C)
    torch.cuda.synchronize()
    assert len({tuple(np.bincount(x, minlength=c.G)) for x in ids_np}) == 3
    for x, (buf, C) in zip(ids_np, outs):
        groups = clamped_groups(np.cumsum(np.bincount(x, minlength=c.G)), c.m_total)
        for g, (s, e) in enumerate(groups):
            if e > s:
                assert torch.equal(C[s:e], reference_rows(N_, c, g, s, e, ROW, ROW, False, torch.float32, tile)), (len(x), g)
        assert_untouched(buf, c.n, groups)


# ---- 10. launch counts -------------------------------------------------------------------------------------------------------------
def test_moe_ops_make_the_launches_their_docstrings_promise(N_):
    H = 128
    c = base_case()
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(c.m_total, c.k, generator=g) * 2.0).to(torch.bfloat16).to(DEV)
    w1 = torch.randn(c.G, 2 * H, c.k, generator=g).to(DEV)
    w2 = torch.randn(c.G, c.n, H, generator=g).to(DEV)
    row = [[N_.fp8_quantize_rowwise(w[i]) for i in range(c.G)] for w in (w1, w2)]
    blk = [[N_.fp8_quantize_blockwise(w[i], 128) for i in range(c.G)] for w in (w1, w2)]
    (r1, rs1), (r2, rs2) = [(torch.stack([q for q, _ in qs]), torch.stack([s.reshape(-1) for _, s in qs])) for qs in row]
    (b1, bs1), (b2, bs2) = [(torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs])) for qs in blk]
    torch.cuda.synchronize()

    def launches(fn):
        with L.kernel_timer(16) as kt:
            fn()
        torch.cuda.synchronize()
        return len(kt.ms)

    assert launches(lambda: N_.fp8_moe_linear_rowwise(x, c.offs, r1, rs1)) == 2
    assert launches(lambda: N_.fp8_moe_linear_blockwise(x, c.offs, b1, bs1)) == 2
    assert launches(lambda: N_.fp8_moe_mlp_rowwise(x, c.offs, r1, rs1, r2, rs2, "silu", True)) == 4
    assert launches(lambda: N_.fp8_moe_mlp_blockwise(x, c.offs, b1, bs1, b2, bs2, "silu", True)) == 4
