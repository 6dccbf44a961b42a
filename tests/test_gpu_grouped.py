"""GPU (MI355X): the grouped (MoE) FP8 GEMM - fp8mi_scaled_mm_grouped / _grouped_blockwise, the fp8_moe_* ops and the patched
torch._scaled_grouped_mm.

The contract under test (include/fp8mi.h): one launch over rows sorted by expert; every group's rows equal, BIT FOR BIT, the
single-problem call on those rows with the same ring tile and split_k=1; rows no group owns, and everything around C, stay untouched.

Base case: G = 6 groups of [0, 1, 130, 64, 33, 0] rows inside M_total = 240 (12 unowned tail rows), N = 200, K = 400: the groups start at
rows 0, 0, 1, 131, 195, 228 - no start after row 1 is tile-aligned - with full and partial tiles in both directions, a partial K-step
and surplus slots on every tile size.  C sits between guard rows, prefilled with a sentinel."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import grouped_ref
from grouped_ref import (DEV, MFMA_TOL, SENTINEL, TILES, assert_untouched, clamped_groups, guarded, reference_rows, run_and_compare, t)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 130, 64, 33, 0]
G, M_TOTAL, N, K = len(SIZES), 240, 200, 400
OFFS = np.cumsum(SIZES).astype(np.int32)


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


def Case(n=N, seed=1):
    """One problem on the device, made once per (N, seed) and never modified."""
    return grouped_ref.Case(OFFS, M_TOTAL, n, K, seed)


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module")
def case202():
    return Case(202, 2)


# ---- bit equality with the per-group calls -------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tile", TILES)
def test_every_group_equals_the_single_problem_call_bit_for_bit(N_, case, tile, out_dtype):
    for sa_mode in (L.SCALE_TENSOR, L.SCALE_ROW):
        for sb_mode in (L.SCALE_TENSOR, L.SCALE_ROW):
            for epi in (False, True):
                run_and_compare(N_, case, tile, out_dtype, sa_mode, sb_mode, epi)


@pytest.mark.parametrize("tile", TILES)
def test_rows_that_do_not_allow_vector_stores(N_, case202, tile):
    """N = 202 bf16: rows of 404 bytes, no 16-byte aligned stores anywhere"""
    run_and_compare(N_, case202, tile, torch.bfloat16, L.SCALE_ROW, L.SCALE_ROW, True)


@pytest.mark.parametrize("tile", TILES)
def test_padded_lda_and_ldc(N_, case, tile):
    wide = torch.zeros((M_TOTAL, 448), dtype=torch.uint8, device=DEV)
    wide[:, :K] = case.A
    A = wide[:, :K]
    assert A.stride(0) == 448 and A.data_ptr() == wide.data_ptr()
    for out_dtype in (torch.float32, torch.bfloat16):
        run_and_compare(N_, case, tile, out_dtype, L.SCALE_ROW, L.SCALE_ROW, True, A=A, ldc=256)


def test_padded_expert_and_row_strides_of_b_are_read_in_place(N_, case):
    wide = torch.zeros((G, case.n + 8, 416), dtype=torch.uint8, device=DEV)
    wide[:, :case.n, :K] = case.B
    Bv = wide[:, :case.n, :K]
    a, b, *_ = N_._grouped_operands(case.A, Bv, case.offs)
    assert b.data_ptr() == wide.data_ptr() and Bv.stride() == ((case.n + 8) * 416, 416, 1)
    want = N_.fp8_scaled_mm_grouped(case.A, case.B, case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW], case.offs, kernel=L.KERNEL_GEMM_64x64)
    got = N_.fp8_scaled_mm_grouped(case.A, Bv, case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW], case.offs, kernel=L.KERNEL_GEMM_64x64)
    owned = int(OFFS[-1])
    assert torch.equal(got[:owned], want[:owned])


# ---- an independent reference ------------------------------------------------------------------------------------------------

def test_exact_data_every_tile_equals_the_numpy_product(N_, oracle):
    rng = np.random.default_rng(17)
    vals = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=np.uint8)   # 0, +-1, +-2, +-3, +-4
    A, B = vals[rng.integers(0, len(vals), (M_TOTAL, K))], vals[rng.integers(0, len(vals), (G, N, K))]
    sa = np.exp2(rng.integers(-2, 3, M_TOTAL)).astype(np.float32)
    sb = np.exp2(rng.integers(-2, 3, (G, N))).astype(np.float32)
    groups = clamped_groups(OFFS, M_TOTAL)
    exact = np.full((M_TOTAL, N), SENTINEL, dtype=np.float32)
    for g, (s, e) in enumerate(groups):
        exact[s:e] = (oracle.decode(A[s:e]).astype(np.float64) @ oracle.decode(B[g]).astype(np.float64).T) * sa[s:e, None] * sb[g][None, :]
    for tile in TILES:
        buf, C = guarded(torch.float32, M_TOTAL, N)
        N_.fp8_scaled_mm_grouped(t(A), t(B), t(sa), t(sb), t(OFFS), kernel=tile, out=C)
        assert np.array_equal(C.cpu().numpy(), exact), tile


@pytest.mark.parametrize("tile", [L.KERNEL_AUTO] + TILES)
def test_random_bytes_against_the_oracle(N_, case, oracle, tile):
    buf, C = guarded(torch.float32, M_TOTAL, N)
    N_.fp8_scaled_mm_grouped(case.A, case.B, case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW], case.offs, kernel=tile, out=C)
    got = C.cpu().numpy().astype(np.float64)
    for g, (s, e) in enumerate(clamped_groups(OFFS, M_TOTAL)):
        if e > s:
            exact = oracle.scaled_mm(case.A_np[s:e], case.B_np[g], case.sa_np[s:e], case.sb_np[g], accumulate="f64")
            bound = oracle.abs_dot_bound(case.A_np[s:e], case.B_np[g], case.sa_np[s:e], case.sb_np[g])
            err = np.abs(got[s:e] - exact)
            assert np.all(err <= MFMA_TOL * bound + 1e-30), (tile, g, float(np.max(err / (bound + 1e-300))))
    assert_untouched(buf, N, clamped_groups(OFFS, M_TOTAL))


# ---- NaN bytes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
def test_a_nan_byte_in_group_2(N_, case, nan_mode):
    A = case.A.clone()
    A[40, 133] = 0x7F     # row 40 is in group 2 (rows 1 .. 130)
    for tile in (L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64):
        groups = clamped_groups(OFFS, M_TOTAL)
        buf, C = guarded(torch.float32, M_TOTAL, N)
        N_.fp8_scaled_mm_grouped(A, case.B, case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW], case.offs, kernel=tile, out=C, nan_mode=nan_mode)
        for g, (s, e) in enumerate(groups):
            if e > s:
                want = reference_rows(N_, case, g, s, e, L.SCALE_ROW, L.SCALE_ROW, False, torch.float32, tile, A, nan_mode)
                assert torch.equal(C[s:e].view(torch.int32), want.view(torch.int32)), (tile, g)   # (bits: NaN != NaN)
        assert bool(torch.isnan(C[40]).all()) == (nan_mode == L.NAN_PROPAGATE)
        assert not bool(torch.isnan(C[41:131]).any()) and not bool(torch.isnan(C[1:40]).any())
        assert_untouched(buf, N, groups)


# ---- defined clamping (tests/test_grouped_host.py checks the same vectors' slot resolution on the CPU) ---------------------------------

@pytest.mark.parametrize("offs", [[100, 50, 200, 10, 240, 240], [100, 300, 500, 500, 500, 500], [-5, 40, -1, 90, 90, -2 ** 31]],
                         ids=["decreasing", "beyond M_total", "negative"])
def test_offs_outside_the_contract_follow_the_clamps(N_, case, offs):
    groups = clamped_groups(offs, M_TOTAL)
    assert all(0 <= s <= e <= M_TOTAL for s, e in groups)
    run_and_compare(N_, case, L.KERNEL_GEMM_64x64, torch.float32, L.SCALE_ROW, L.SCALE_ROW, True, offs=t(np.array(offs, dtype=np.int32)), groups=groups)


# ---- blockwise ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_b", [128, 1])
@pytest.mark.parametrize("tile", TILES)
def test_blockwise_groups_equal_the_single_problem_call(N_, case, tile, block_b):
    rng = np.random.default_rng(5 + block_b)
    nkb, nrb = -(-K // 128), -(-N // block_b)
    sa = t((np.exp2(rng.uniform(-6, 6, (M_TOTAL, nkb))) * rng.choice([-1.0, 1.0], (M_TOTAL, nkb))).astype(np.float32))
    sb = t((np.exp2(rng.uniform(-6, 6, (G, nrb, nkb))) * rng.choice([-1.0, 1.0], (G, nrb, nkb))).astype(np.float32))
    groups = clamped_groups(OFFS, M_TOTAL)
    for out_dtype, epi in ((torch.float32, False), (torch.bfloat16, True)):
        buf, C = guarded(out_dtype, M_TOTAL, N)
        N_.fp8_scaled_mm_grouped_blockwise(case.A, case.B, sa, sb, case.offs, block_b=block_b, bias=case.bias if epi else None,
                                           scale_result=case.sr if epi else None, out_dtype=out_dtype, kernel=tile, out=C)
        for g, (s, e) in enumerate(groups):
            if e > s:
                want = N_.fp8_scaled_mm_blockwise(case.A[s:e], case.B[g], sa[s:e], sb[g], block_a=1, block_b=block_b, bias=case.bias[g] if epi else None,
                                                  scale_result=case.sr if epi else None, out_dtype=out_dtype, kernel=tile, split_k=1)
                assert torch.equal(C[s:e], want), (tile, block_b, out_dtype, g)
        assert_untouched(buf, N, groups)


# ---- no host sync --------------------------------------------------------------------------------------------------------------

def test_one_launch_captured_into_a_graph_follows_offs_on_replay(N_, case):
    tile = L.KERNEL_GEMM_64x64
    sa, sb = case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW]
    offs = case.offs.clone()
    buf, C = guarded(torch.float32, M_TOTAL, N)
    with L.kernel_timer(4) as kt:   # eager: the call is ONE kernel launch of the library
        N_.fp8_scaled_mm_grouped(case.A, case.B, sa, sb, offs, kernel=tile, out=C)
    torch.cuda.synchronize()
    assert len(kt.ms) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a host sync or a read of offs inside the capture would fail it)
        N_.fp8_scaled_mm_grouped(case.A, case.B, sa, sb, offs, kernel=tile, out=C)
    other = [30, 30, 31, 100, 240, 240]
    for split in (other, list(OFFS)):
        offs.copy_(t(np.array(split, dtype=np.int32)))
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        groups = clamped_groups(split, M_TOTAL)
        for g, (s, e) in enumerate(groups):
            if e > s:
                assert torch.equal(C[s:e], reference_rows(N_, case, g, s, e, L.SCALE_ROW, L.SCALE_ROW, False, torch.float32, tile)), (split, g)
        assert_untouched(buf, N, groups)


# ---- op layer and patch ----------------------------------------------------------------------------------------------------------

H = 128   # hidden features of the MLPs: w1 (G, 2H, K) [gate | up], w2 (G, N, H)


@pytest.fixture(scope="module")
def moe(N_):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M_TOTAL, K, generator=g) * 2.0).to(torch.bfloat16).to(DEV)
    w1 = torch.randn(G, 2 * H, K, generator=g).to(DEV)
    w2 = torch.randn(G, N, H, generator=g).to(DEV)
    b1 = torch.randn(G, 2 * H, generator=g).to(torch.bfloat16).to(DEV)
    b2 = torch.randn(G, N, generator=g).to(torch.bfloat16).to(DEV)
    row = [[N_.fp8_quantize_rowwise(w[i]) for i in range(G)] for w in (w1, w2)]
    blk = [[N_.fp8_quantize_blockwise(w[i], 128) for i in range(G)] for w in (w1, w2)]
    pack_row = lambda qs: (torch.stack([q for q, _ in qs]), torch.stack([s.reshape(-1) for _, s in qs]))   # noqa: E731  (G, N, K), (G, N)
    pack_blk = lambda qs: (torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs]))               # noqa: E731  (G, N, K), (G, N/128, K/128)
    return dict(x=x, b1=b1, b2=b2, row=[pack_row(r) for r in row], blk=[pack_blk(b) for b in blk], offs=t(OFFS))


def force_tile(monkeypatch, N_, name, tile):
    """the single-problem ops run AUTO; the per-expert reference loop needs the grouped call's tile, unsplit"""
    real = getattr(N_, name)
    monkeypatch.setattr(N_, name, lambda *a, **kw: real(*a, **{**kw, "kernel": tile, "split_k": 1}))


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64])
def test_moe_linear_and_mlp_rowwise_equal_the_per_expert_loop(N_, moe, monkeypatch, tile):
    (w1, s1), (w2, s2) = moe["row"]
    x, offs = moe["x"], moe["offs"]
    y_lin = N_.fp8_moe_linear_rowwise(x, offs, w1, s1, moe["b1"], kernel=tile)
    y_mlp = N_.fp8_moe_mlp_rowwise(x, offs, w1, s1, w2, s2, "silu", True, moe["b1"], moe["b2"], kernel=tile)
    assert y_lin.shape == (M_TOTAL, 2 * H) and y_mlp.shape == (M_TOTAL, N) and y_mlp.dtype == torch.bfloat16
    force_tile(monkeypatch, N_, "fp8_scaled_mm", tile)
    for g, (s, e) in enumerate(clamped_groups(OFFS, M_TOTAL)):
        if e > s:
            assert torch.equal(y_lin[s:e], N_.fp8_linear_rowwise(x[s:e], w1[g], s1[g], moe["b1"][g])), g
            assert torch.equal(y_mlp[s:e], N_.fp8_mlp_rowwise(x[s:e], w1[g], s1[g], w2[g], s2[g], "silu", True, moe["b1"][g], moe["b2"][g])), g


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64])
def test_moe_linear_and_mlp_blockwise_equal_the_per_expert_loop(N_, moe, monkeypatch, tile):
    (w1, s1), (w2, s2) = moe["blk"]
    x, offs = moe["x"], moe["offs"]
    y_lin = N_.fp8_moe_linear_blockwise(x, offs, w1, s1, moe["b1"], kernel=tile)
    y_mlp = N_.fp8_moe_mlp_blockwise(x, offs, w1, s1, w2, s2, "silu", True, moe["b1"], moe["b2"], kernel=tile)
    force_tile(monkeypatch, N_, "fp8_scaled_mm_blockwise", tile)
    for g, (s, e) in enumerate(clamped_groups(OFFS, M_TOTAL)):
        if e > s:
            assert torch.equal(y_lin[s:e], N_.fp8_linear_blockwise(x[s:e], w1[g], s1[g], moe["b1"][g])), g
            assert torch.equal(y_mlp[s:e], N_.fp8_mlp_blockwise(x[s:e], w1[g], s1[g], w2[g], s2[g], "silu", True, moe["b1"][g], moe["b2"][g])), g


def test_patched_scaled_grouped_mm_equals_the_op(N_, case, patch, monkeypatch):
    routed = []
    real = N_.scaled_grouped_mm_colmajor
    monkeypatch.setattr(N_, "scaled_grouped_mm_colmajor", lambda *a, **kw: routed.append(1) or real(*a, **kw))
    e4 = torch.float8_e4m3fn
    a = case.A.view(e4)
    mat2 = case.B.view(e4).transpose(1, 2)          # (G, K, N), every expert column-major: torch's layout
    sa, sb = case.sa[L.SCALE_ROW], case.sb[L.SCALE_ROW]
    got = torch._scaled_grouped_mm(a, mat2, sa, sb, case.offs, out_dtype=torch.bfloat16)
    got_default = torch._scaled_grouped_mm(a, mat2, sa, sb, offs=case.offs)
    assert len(routed) == 2 and got.dtype == torch.bfloat16 and got_default.dtype == torch.bfloat16 and got.shape == (M_TOTAL, N)
    want = N_.fp8_scaled_mm_grouped(case.A, case.B, sa, sb, case.offs, out_dtype=torch.bfloat16)
    owned = int(OFFS[-1])
    assert torch.equal(got[:owned], want[:owned]) and torch.equal(got_default[:owned], want[:owned])
