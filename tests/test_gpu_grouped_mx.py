"""GPU (MI355X): the grouped MXFP8 / MXFP4 / MXW4A8 GEMM - fp8mi_scaled_mm_grouped_mxfp8 / _mxfp4 / _mxw4a8 through the ops of the same names.

Three checks per case (include/fp8mi.h): (a) every group's rows equal, bit for bit, the single-problem MX call on those rows
with the same ring tile and split_k=1 (a NaN matches a NaN); (b) the sentinel rows around C and the rows at or past offs[-1] are untouched;
(c) an independent reference - the float64 per-group product of the dequantised operands under the single-problem tests' bar
(|gpu - exact| <= 1e-3 sum |a 2^sa| |b 2^sb|), and exact data where equality is required.

Shapes: K in bytes 32 (one block row: a single partial K-step), 160 (five scale bytes in rows of 8; MXFP4: ten in 12), 1312 (the ring wraps,
then a partial last step; MXFP4: scale rows of 84 = 4 mod 8 bytes), 1536 (every ring wraps on the KS = 1 and KS = 2 tiles); N = 200 (no BN
divides it); group sizes from {0, 1, BM-1, BM, BM+1, 2 BM+3}; G in {1, 3, 9, 17}, across the batch of eight of the offsets walk.
MXW4A8 (A in e4m3 bytes, B in e2m1 pairs; its K-step is 256 k: 128 bytes of B against two 128-byte sub-steps of A), K in elements = bytes of A:
32 (one block), 160 (sub-step 0 full and one block of sub-step 1; five scale bytes in rows of 8), 320, 2624 (scale rows of 84 bytes, a partial
last step), 3072 (every ring wraps)."""
import numpy as np
import pytest
import torch

from grouped_ref import MFMA_TOL, TILES, guarded
from grouped_mx_ref import (DEV, FORMATS, SENTINEL, TILE_DIMS, L, MxCase, chosen_tile, group_sizes, grouped_op, owned_rows, reference_f64,
                            run_and_compare, same_bits, single_op)

pytestmark = pytest.mark.gpu

N = 200
KBYTES = (32, 160, 1312, 1536)
# bytes of K in a row of A per format (MxCase's kb); the ids of the MXFP8 / MXFP4 cases are those of a plain fmt x tile x kb product
KB_OF = {"mxfp8": KBYTES, "mxfp4": KBYTES, "mxw4a8": (32, 160, 320, 2624, 3072)}
KB_LONG = {"mxfp8": 1312, "mxfp4": 1312, "mxw4a8": 2624}   # the ring wraps, then a partial last step
KB_FIVE_BLOCKS = {"mxfp8": 160, "mxfp4": 80, "mxw4a8": 160}   # K = 160: scale rows of five bytes in eight
GROUPS = (1, 3, 9, 17)
SMALL = L.KERNEL_GEMM_32x64   # the tile of the cases that are not about the tile


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


def make(fmt, tile, G, kb, seed=None, **kw):
    bm = TILE_DIMS[tile][0]
    seed = 1000 * tile + 10 * G + kb if seed is None else seed
    return MxCase(fmt, group_sizes(np.random.default_rng(seed), G, bm), N, kb, seed, **kw)


def padded_views(c):
    """-> (A, B, sa, sb) of MxCase c on device buffers with lda, ldb, stride_b, ld_sa, ld_sb and stride_sb larger than dense (multiples of 16 /
    4); the bytes between the scale rows are 0xFF, the operands' zero"""
    A = torch.zeros((c.m_total, c.kb_a + 32), dtype=torch.uint8, device=DEV)[:, :c.kb_a]
    A.copy_(c.A)
    B = torch.zeros((c.G, c.n + 3, c.kb_b + 16), dtype=torch.uint8, device=DEV)[:, :c.n, :c.kb_b]
    B.copy_(c.B)
    sb = torch.full((c.G, c.n + 5, c.ld_s + 4), 0xFF, dtype=torch.uint8, device=DEV)[:, :c.n, :c.ld_s]
    sb.copy_(c.sb)
    sa = torch.full((c.m_total, c.ld_s + 8), 0xFF, dtype=torch.uint8, device=DEV)[:, :c.ld_s]
    sa.copy_(c.sa)
    assert A.stride(0) == c.kb_a + 32 and B.stride(0) == (c.n + 3) * (c.kb_b + 16) and sb.stride(0) == (c.n + 5) * (c.ld_s + 4)
    return A, B, sa, sb


def check_f64(c, C, nan_zero=True):
    exact, bound = reference_f64(c, nan_zero)
    own = owned_rows(c)
    got = C.float().cpu().numpy().astype(np.float64)[own]
    err = np.abs(got - exact[own])
    assert np.all(err <= MFMA_TOL * bound[own] + 1e-30), f"max err / bound {np.max(err / (bound[own] + 1e-300)):.3e}"


@pytest.mark.parametrize("fmt,tile,kb", [pytest.param(f, tile, kb, id=f"{f}-{tile}-{kb}") for kb in sorted({k for f in FORMATS for k in KB_OF[f]})
                                         for tile in TILES for f in FORMATS if kb in KB_OF[f]])
def test_groups_equal_the_single_problem_call_and_the_float64_product(N_, fmt, tile, kb):
    for G in GROUPS:
        c = make(fmt, tile, G, kb)
        _buf, C = run_and_compare(N_, c, tile)
        check_f64(c, C)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_data_gives_the_exact_sum(N_, fmt, tile):
    """0, +-1 .. +-4 and scales 2^-1 .. 2^1: every partial sum is a multiple of 2^-2 below 2^22, so the fp32 result is the exact one
    (MXFP4, MXW4A8: K = 2624 elements <= 4096; MXW4A8 draws A from the e4m3 bytes of these integers and B from their e2m1 codes)"""
    c = make(fmt, tile, 9, KB_LONG[fmt], exact=True)
    assert c.K * 16 * 4 * 4 < 2 ** 24
    _buf, C = run_and_compare(N_, c, tile)
    exact, _bound = reference_f64(c)
    own = owned_rows(c)
    assert np.array_equal(C.cpu().numpy()[own], exact[own].astype(np.float32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_epilogue_out_dtypes_and_rows_without_vector_stores(N_, fmt):
    """bias [G, N] in f32 and bf16 with scale_result; f32, bf16 and f16 out; ldc = 202 bf16 (rows of 404 bytes: no 16-byte stores)"""
    c = make(fmt, SMALL, 9, 160)
    for out_dtype in (torch.float32, torch.bfloat16, torch.float16):
        run_and_compare(N_, c, SMALL, out_dtype, epi=True)
    run_and_compare(N_, c, SMALL, torch.float32, epi=True, bias=c.bias.to(torch.bfloat16))
    run_and_compare(N_, c, L.KERNEL_GEMM_128x64, torch.bfloat16, epi=True, ldc=202)
    _buf, C = run_and_compare(N_, c, SMALL, torch.float32, epi=True)
    exact, bound = reference_f64(c)
    own = owned_rows(c)
    rows = np.repeat(np.arange(c.G), [e - s for s, e in c.groups])
    want = (exact[own] + c.bias_np[rows].astype(np.float64)) * np.float64(np.float32(0.37))
    assert np.all(np.abs(C.cpu().numpy().astype(np.float64)[own] - want) <= MFMA_TOL * bound[own] * 0.37 + 2.0 ** -22 * np.abs(want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_padded_operand_and_scale_strides(N_, fmt):
    """lda, ldb, stride_b and stride_sb larger than dense (multiples of 16 / 4), read in place"""
    c = make(fmt, SMALL, 3, 160)
    A, B, sa, sb = padded_views(c)
    _buf, C = run_and_compare(N_, c, SMALL, A=A, B=B, sa=sa, sb=sb)
    check_f64(c, C)


@pytest.mark.parametrize("fmt", FORMATS)
def test_poisoned_pad_bytes_inside_the_scale_rows(N_, fmt):
    """K / 32 = 5 in scale rows of 8 bytes, on the padded layouts of the test above: the three pad bytes INSIDE each scale row hold the E8M0 NaN
    0xFF instead of 0x7F.  They lie in the last K-step's 4-byte scale read next to a real block, and their operand bytes are zero: only the
    kernels' guard (blocks past K read as 2^0) keeps 0 x NaN out of the sums - in the grouped kernel and in the single-problem call that a
    group's rows must equal.  The result is finite and has the bits of the run on 0x7F pads, which is held to the float64 product."""
    for tile in (SMALL, L.KERNEL_GEMM_128):
        c = make(fmt, tile, 3, KB_FIVE_BLOCKS[fmt])
        assert c.K == 160 and c.nb == 5 and c.ld_s == 8
        A, B, sa, sb = padded_views(c)
        _buf, want = run_and_compare(N_, c, tile, A=A, B=B, sa=sa, sb=sb)
        check_f64(c, want)
        sa[:, c.nb:] = 0xFF
        sb[:, :, c.nb:] = 0xFF
        _buf, C = run_and_compare(N_, c, tile, A=A, B=B, sa=sa, sb=sb)
        own = torch.from_numpy(owned_rows(c)).to(DEV)
        assert bool(torch.isfinite(C[own]).all()) and same_bits(C[own], want[own]), (fmt, tile)


@pytest.mark.parametrize("fmt", FORMATS)
def test_all_groups_empty_and_one_row(N_, fmt):
    c = MxCase(fmt, [0, 0, 0, 0, 0], N, 160, 5, tail=7)
    run_and_compare(N_, c, SMALL)                                   # nothing is written
    run_and_compare(N_, c, L.KERNEL_GEMM_128)
    one = MxCase(fmt, [1], N, 160, 6, tail=0)                       # G = 1, M_total = 1
    for tile in (SMALL, L.KERNEL_GEMM_128x64):
        _buf, C = run_and_compare(N_, one, tile)
        check_f64(one, C)
    auto = make(fmt, SMALL, 9, KB_LONG[fmt])                        # AUTO: the tile fp8mi_choose_kernel_grouped_mx / _mxw4a8 names
    tile = chosen_tile(auto)
    assert tile in TILES
    run_and_compare(N_, auto, L.KERNEL_AUTO, ref_tile=tile)


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_nan_scales_stay_in_their_rows_and_columns(N_, fmt, tile):
    """0xFF in one block of expert 1's scales (column 7) and on the last row of group 1 and the first row of group 2: NaN in exactly those
    rows, and in column 7 of group 1 - a scale read that crossed into the neighbouring group or expert would spread it"""
    bm = TILE_DIMS[tile][0]
    c = MxCase(fmt, [bm + 1, bm - 1, 2 * bm + 3, 1], N, 160, 77)
    (s1, e1), (s2, _e2) = c.groups[1], c.groups[2]
    sa, sb = c.sa.clone(), c.sb.clone()
    sa[e1 - 1, 2] = 0xFF
    sa[s2, c.nb - 1] = 0xFF
    sb[1, 7, 1] = 0xFF
    _buf, C = run_and_compare(N_, c, tile, sa=sa, sb=sb)
    want = torch.zeros((c.m_total, N), dtype=torch.bool, device=DEV)
    want[e1 - 1] = True
    want[s2] = True
    want[s1:e1, 7] = True
    own = torch.from_numpy(owned_rows(c)).to(DEV)
    assert torch.equal(torch.isnan(C)[own], want[own])


def nan_bytes_on_both_sides_of_a_group_boundary(N_, fmt, tile, nan_mode):
    """bytes 0x7F / 0xFF in the last row of group 0, the first row of group 1 and row 9 of expert 1's B; MXW4A8: B's byte is the finite pair
    6.0 | 1.5, and its column holds no NaN under either mode"""
    bm = TILE_DIMS[tile][0]
    c = MxCase(fmt, [bm - 1, bm + 1, 1], N, 160, 78)
    (_s0, e0), (s1, _e1) = c.groups[0], c.groups[1]
    A, B = c.A.clone(), c.B.clone()
    A[e0 - 1, 5] = 0x7F
    A[s1, 130] = 0xFF
    B[1, 9, 40] = 0x7F
    _buf, C = run_and_compare(N_, c, tile, A=A, B=B, nan_mode=nan_mode)
    nan = torch.isnan(C)
    if nan_mode == L.NAN_ZERO:
        assert not bool(nan[:int(c.offs_np[-1])].any())
    else:
        want = torch.zeros_like(nan)
        want[e0 - 1] = True
        want[s1] = True
        if not c.w4a8:
            want[c.groups[1][0]:c.groups[1][1], 9] = True
        assert torch.equal(nan[:int(c.offs_np[-1])], want[:int(c.offs_np[-1])])
    if c.w4a8:                                                      # B's byte is a value: the float64 product of the changed operands
        c.A_np, c.B_np = A.cpu().numpy(), B.cpu().numpy()           # (this case is the test's own)
        exact, bound = reference_f64(c, nan_zero=True)
        fin = owned_rows(c) & ~np.isnan(C.cpu().numpy()).any(axis=1)
        err = np.abs(C.cpu().numpy().astype(np.float64)[fin] - exact[fin])
        assert np.all(err <= MFMA_TOL * bound[fin] + 1e-30)


@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128D])
def test_mxfp8_nan_bytes_on_both_sides_of_a_group_boundary(N_, tile, nan_mode):
    nan_bytes_on_both_sides_of_a_group_boundary(N_, "mxfp8", tile, nan_mode)


@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128D])
def test_mxw4a8_nan_bytes_on_both_sides_of_a_group_boundary(N_, tile, nan_mode):
    nan_bytes_on_both_sides_of_a_group_boundary(N_, "mxw4a8", tile, nan_mode)


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replays_after_offs_and_operands_changed(N_, fmt):
    """captured once on one stream; replayed after offs, A, B and the scales were overwritten in place"""
    tile = SMALL
    c1 = MxCase(fmt, [33, 0, 70, 1, 31, 64, 5, 0, 9], N, 160, 91, tail=4)
    c2 = MxCase(fmt, [1, 60, 0, 0, 90, 2, 32, 12, 20], N, 160, 92, tail=0)
    assert c1.m_total == c2.m_total
    A, B, sa, sb, offs = c1.A.clone(), c1.B.clone(), c1.sa.clone(), c1.sb.clone(), c1.offs.clone()
    buf, C = guarded(torch.bfloat16, c1.m_total, N)
    op = grouped_op(N_, fmt)
    call = lambda: op(A, B, sa[:, :c1.nb], sb[:, :, :c1.nb], offs, bias=c1.bias, out_dtype=torch.bfloat16, kernel=tile, out=C)   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    for c in (c2, c1):
        A.copy_(c.A), B.copy_(c.B), sa.copy_(c.sa), sb.copy_(c.sb), offs.copy_(c.offs)
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        for g, (s, e) in enumerate(c.groups):
            if e > s:
                want = single_op(N_, fmt)(c.A[s:e], c.B[g], c.sa[s:e, :c.nb], c.sb[g][:, :c.nb], bias=c1.bias[g], out_dtype=torch.bfloat16,
                                          kernel=tile, split_k=1)
                assert same_bits(C[s:e], want), (fmt, g)
        assert bool((C[int(c.offs_np[-1]):] == SENTINEL).all()) and bool((buf[:8] == SENTINEL).all()) and bool((buf[-8:] == SENTINEL).all())
