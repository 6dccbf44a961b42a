"""GPU (MI355X): the MXW4A8 GEMM - e4m3 activations against e2m1 weights, E8M0 scales per 32 k on both sides (include/fp8mi.h,
DESIGN.md 5.16) - through fp8_scaled_mm_mxw4a8, and fp8_linear_mxw4a8.

Bars, the project's own (tests/test_gpu_mxfp4.py): |gpu - exact| <= 1e-3 sum_k |a 2^sa| |b 2^sb| on the matrix-core tiles against the
float64 product of the decoded operands (tests/mxw4a8_ref.py), 4e-6 on the generic kernel (IEEE fp32 sums).  Exact data - A from the e4m3
bytes that are multiples of 1/8 up to 16, any e2m1 code in B, unit scales, K <= 4096: every product is a multiple of 1/16 up to 96 and
every partial sum an fp32 value - must give the float64 sum bit for bit."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from mxw4a8_ref import mm_ref, rand_exact_a, w_as_e4m3

pytestmark = pytest.mark.gpu

MFMA_TOL = 1.0e-3
FP32_TOL = 4e-6
TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
         L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
DEV = "cuda"


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


def rand_a(rng, rows, K):
    b = rng.integers(0, 256, size=(rows, K), dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def rand_fp4(rng, rows, K):
    return rng.integers(0, 256, size=(rows, K // 2), dtype=np.uint8)


def rand_scales(rng, rows, nb, lo=117, hi=137):
    return rng.integers(lo, hi + 1, size=(rows, nb), dtype=np.uint8)


def ones(rows, K):
    return np.full((rows, K // 32), 127, np.uint8)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(N_, A, B, sa, sb, **kw):
    out = N_.fp8_scaled_mm_mxw4a8(t(A), t(B), t(sa), t(sb), **kw)
    torch.cuda.synchronize()
    return out.float().cpu().numpy().astype(np.float64)


def tol_of(kernel):
    return FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL


def check(got, A, B, sa, sb, tol, nan_zero=True):
    exact, bound = mm_ref(A, B, sa, sb, nan_zero)
    err = np.abs(got - exact)
    assert np.all(err <= tol * bound + 1e-30), f"max err / bound {np.max(err / (bound + 1e-300)):.3e}"


@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC])
def test_scale_and_operand_map_every_kernel(N_, kernel):
    """Each (row, block) of both operands gets its own scale, one power of two apart from its neighbours along K, M and N, on asymmetric
    data; then one (row, block) of each operand at 2^1 / 2^2 on exact data, which must be bit-equal to float64.  A kernel that swaps the
    operands' scales or formats, pairs X's second K-step with W's first half, or reads W's high registers fails one of the two."""
    rng = np.random.default_rng(kernel)
    M, Nn, K = 96, 80, 512
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    nb = K // 32
    sa = (112 + (np.arange(M)[:, None] * 3 + np.arange(nb)[None, :] * 2) % 31).astype(np.uint8)
    sb = (100 + (np.arange(Nn)[:, None] * 5 + np.arange(nb)[None, :] * 7) % 29).astype(np.uint8)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, tol_of(kernel))
    A = rand_exact_a(rng, M, K)
    one, oneb = ones(M, K), ones(Nn, K)
    one[17, 5] = 128
    oneb[3, 9] = 129
    got = run(N_, A, B, one, oneb, kernel=kernel, split_k=1)
    exact, _ = mm_ref(A, B, one, oneb)
    assert np.array_equal(got, exact)


# one block; inside X's first K-step; exactly it; just into the second; one full stage; a stage plus one block; 12 blocks (scale rows with
# ld = 4 mod 8); eight stages (every ring refills a slot: NSTAGE <= 6); the same plus a partial stage
K_EDGES = [32, 96, 128, 160, 256, 288, 384, 2048, 2080]


@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128x64])
@pytest.mark.parametrize("K", K_EDGES)
def test_k_edges(N_, K, kernel):
    for Nn in (72, 200):
        rng = np.random.default_rng(K * 7 + Nn)
        B, sb = rand_fp4(rng, Nn, K), rand_scales(rng, Nn, K // 32)
        for M in (1, 7, 33, 64, 130):
            A, sa = rand_a(rng, M, K), rand_scales(rng, M, K // 32)
            check(run(N_, A, B, sa, sb, kernel=kernel, split_k=1), A, B, sa, sb, MFMA_TOL)


@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO])
@pytest.mark.parametrize("K", [256, 4096])
def test_unit_scales_are_exact_on_exact_data(N_, kernel, K):
    rng = np.random.default_rng(K + kernel)
    M, Nn = 70, 96
    A, B = rand_exact_a(rng, M, K), rand_fp4(rng, Nn, K)
    A[:3] = 0x58                        # rows of 16.0 x 6.0 products: |sum| up to 96 K
    B[:2] = 0x77
    got = run(N_, A, B, ones(M, K), ones(Nn, K), kernel=kernel, split_k=1)
    exact, _ = mm_ref(A, B, ones(M, K), ones(Nn, K))
    assert np.array_equal(got, exact)


def test_every_unsplit_tile_gives_the_same_bits(N_):
    rng = np.random.default_rng(11)
    M, Nn, K = 130, 200, 1024
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    outs = [run(N_, A, B, sa, sb, kernel=k, split_k=1) for k in TILES]
    check(outs[0], A, B, sa, sb, MFMA_TOL)
    for k, o in zip(TILES[1:], outs[1:]):
        assert np.array_equal(o, outs[0]), k


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D])
def test_same_values_through_mxfp8(N_, kernel):
    """W's codes re-encoded as e4m3 bytes (tests/mxw4a8_ref.py): the MXFP8 kernel on the same tile gives equal bits on exact data with
    unit scales, and a result within 2e-3 x bound under random scales"""
    rng = np.random.default_rng(41)
    M, Nn, K = 100, 144, 1024
    A, B = rand_exact_a(rng, M, K), rand_fp4(rng, Nn, K)
    b8 = w_as_e4m3(B)
    mixed = run(N_, A, B, ones(M, K), ones(Nn, K), kernel=kernel, split_k=1)
    fp8 = N_.fp8_scaled_mm_mxfp8(t(A), t(b8), t(ones(M, K)), t(ones(Nn, K)), kernel=kernel, split_k=1).double().cpu().numpy()
    assert np.array_equal(mixed, fp8)
    A = rand_a(rng, M, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    mixed = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    fp8 = N_.fp8_scaled_mm_mxfp8(t(A), t(b8), t(sa), t(sb), kernel=kernel, split_k=1).double().cpu().numpy()
    _, bound = mm_ref(A, B, sa, sb)
    assert np.all(np.abs(mixed - fp8) <= 2 * MFMA_TOL * bound)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x32])
@pytest.mark.parametrize("split", [2, 4])
def test_split_k(N_, kernel, split):
    rng = np.random.default_rng(split * 100 + kernel)
    M, Nn, K = 64, 512, 8192
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    one = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    s1 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    s2 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    assert np.array_equal(s1, s2)
    check(s1, A, B, sa, sb, MFMA_TOL)
    _, bound = mm_ref(A, B, sa, sb)
    assert np.all(np.abs(s1 - one) <= 2 * MFMA_TOL * bound)


@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC])
def test_nan_modes_touch_a_only(N_, kernel):
    """A holds NaN bytes (0x7F, 0xFF) in three rows; two rows of B are 0x7F / 0xFF everywhere - finite e2m1 pairs (6.0 | 1.5, -6.0 | -1.5).
    FP8MI_NAN_ZERO: A's NaN bytes count as zero and B's bytes keep their values; FP8MI_NAN_PROPAGATE: exactly the rows of A that hold a
    NaN byte are NaN."""
    rng = np.random.default_rng(13)
    M, Nn, K = 70, 72, 544
    A, B = rand_exact_a(rng, M, K), rand_fp4(rng, Nn, K)
    A[3, 5] = 0x7F
    A[17, 300] = 0xFF
    A[17, 31] = 0x7F
    A[66, 543] = 0xFF
    B[5] = 0x7F
    B[9] = 0xFF
    sa, sb = ones(M, K), ones(Nn, K)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=L.NAN_ZERO)
    exact, _ = mm_ref(A, B, sa, sb, nan_zero=True)
    assert not np.isnan(got).any()
    assert np.array_equal(got, exact)                    # exact data: the sums are fp32 values
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=L.NAN_PROPAGATE)
    want = np.zeros((M, Nn), bool)
    want[[3, 17, 66]] = True
    assert np.array_equal(np.isnan(got), want)
    assert np.array_equal(got[~want], exact[~want])


@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC])
def test_special_scales(N_, kernel, nan_mode):
    rng = np.random.default_rng(5)
    M, Nn, K = 64, 64, 256
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), np.full((Nn, K // 32), 147, np.uint8)
    sa[3, 2] = 0x00                       # 2^-127 (times 2^20 of the other side: a normal fp32 sum)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=nan_mode)
    check(got, A, B, sa, sb, tol_of(kernel))
    sb[9, 4] = 0xFF                       # E8M0 NaN on the B side: the whole output column that sums the block is NaN
    sa[20, 7] = 0xFF                      # ... and on the A side: the whole row
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=nan_mode)
    want = np.zeros((M, Nn), bool)
    want[:, 9] = True
    want[20] = True
    assert np.array_equal(np.isnan(got), want)
    rows, cols = [m for m in range(M) if m != 20], [n for n in range(Nn) if n != 9]
    check(got[np.ix_(rows, cols)], A[rows], B[cols], sa[rows], sb[cols], tol_of(kernel))


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x64, L.KERNEL_GENERIC])
def test_epilogue_bias_scale_result_and_out_dtypes(N_, kernel):
    rng = np.random.default_rng(17)
    M, Nn, K = 130, 136, 416
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32, 119, 125), rand_scales(rng, Nn, K // 32, 119, 125)   # 2^-8 .. 2^-2: the sums stay inside float16
    exact, bound = mm_ref(A, B, sa, sb)
    assert np.max(np.abs(exact)) < 4096
    bias = (rng.standard_normal(Nn) * 50.0).astype(np.float32)
    sr = np.float32(0.37)
    for bias_t in (torch.from_numpy(bias), torch.from_numpy(bias).to(torch.bfloat16)):
        b64 = bias_t.double().numpy()
        want = (exact + b64[None, :]) * np.float64(sr)
        for out_dtype, eps in ((torch.float32, 2.0 ** -22), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, bias=bias_t.to(DEV), scale_result=torch.tensor([sr]).to(DEV), out_dtype=out_dtype)
            assert np.all(np.abs(got - want) <= tol_of(kernel) * bound * 0.37 + eps * np.abs(want) + 1e-30), (out_dtype, bias_t.dtype)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_AUTO])
def test_padded_strides_and_sentinels_around_c(N_, kernel):
    """lda, ldb and ldc larger than dense (16-byte multiples), read and written in place; the bytes around C keep a sentinel"""
    rng = np.random.default_rng(19)
    M, Nn, K = 150, 136, 416
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    dense = N_.fp8_scaled_mm_mxw4a8(t(A), t(B), t(sa), t(sb), kernel=kernel, split_k=1, out_dtype=torch.bfloat16)
    a = torch.full((M, K + 48), 0x7E, dtype=torch.uint8, device=DEV)[:, 16:16 + K]
    a.copy_(t(A))
    b = torch.full((Nn, K // 2 + 80), 0x7E, dtype=torch.uint8, device=DEV)[:, 32:32 + K // 2]
    b.copy_(t(B))
    assert a.stride(0) == K + 48 and a.data_ptr() % 16 == 0 and b.stride(0) % 16 == 0 and b.data_ptr() % 16 == 0
    SENT = -12352.0
    buf = torch.full((M + 16, Nn + 24), SENT, dtype=torch.bfloat16, device=DEV)
    C = buf[8:8 + M, 8:8 + Nn]
    got = N_.fp8_scaled_mm_mxw4a8(a, b, t(sa), t(sb), kernel=kernel, split_k=1, out_dtype=torch.bfloat16, out=C)
    torch.cuda.synchronize()
    assert got is C and torch.equal(C, dense)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[8:8 + M, 8:8 + Nn] = False
    assert bool((buf[mask] == SENT).all())
    check(C.float().cpu().numpy().astype(np.float64), A, B, sa, sb, MFMA_TOL + 2.0 ** -8)


def test_an_operand_offset_by_8_bytes_runs_the_generic_kernel_under_auto(N_):
    rng = np.random.default_rng(23)
    M, Nn, K = 40, 72, 288
    A, B = rand_a(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    flat = torch.zeros(8 + M * K, dtype=torch.uint8, device=DEV)
    a = flat[8:].view(M, K)
    a.copy_(t(A))
    assert a.data_ptr() % 16 == 8
    auto = N_.fp8_scaled_mm_mxw4a8(a, t(B), t(sa), t(sb))
    generic = N_.fp8_scaled_mm_mxw4a8(t(A), t(B), t(sa), t(sb), kernel=L.KERNEL_GENERIC)
    torch.cuda.synchronize()
    assert torch.equal(auto, generic)
    check(auto.double().cpu().numpy(), A, B, sa, sb, FP32_TOL)
    with pytest.raises(RuntimeError):
        N_.fp8_scaled_mm_mxw4a8(a, t(B), t(sa), t(sb), kernel=L.KERNEL_GEMM_64x64)   # a forced tile cannot read it


def test_linear_mxw4a8_and_its_reason_to_exist(N_):
    """fp8_linear_mxw4a8 against mm_ref of its own quantised operands; on randn data its relative error against the float64 product is
    below that of fp8_linear_mxfp4 on the same data"""
    from mxfp8_ref import to_mxfp8_ref
    g = torch.Generator().manual_seed(1234)
    K, Nn = 1024, 256
    w = torch.randn(Nn, K, generator=g) * 0.02
    x = torch.randn(32, K, generator=g)
    wq, ws = N_.fp8_quantize_mxfp4(w.to(DEV))
    y = N_.fp8_linear_mxw4a8(x.to(DEV), wq, ws, out_dtype=torch.float32).double().cpu().numpy()
    xs, xq = to_mxfp8_ref(x)
    exact, bound = mm_ref(xq.numpy(), wq.view(torch.uint8).cpu().numpy(), xs.numpy(), ws.view(torch.uint8).cpu().numpy())
    assert np.all(np.abs(y - exact) <= MFMA_TOL * bound)
    true = (x.double() @ w.double().T).numpy()
    y4 = N_.fp8_linear_mxfp4(x.to(DEV), wq, ws, out_dtype=torch.float32).double().cpu().numpy()
    rel, rel4 = np.linalg.norm(y - true) / np.linalg.norm(true), np.linalg.norm(y4 - true) / np.linalg.norm(true)
    print(f"relative error against the float64 product: mxw4a8 {rel:.4f}, mxfp4 {rel4:.4f}")
    assert rel < rel4, (rel, rel4)
    assert N_.fp8_linear_mxw4a8(x.to(torch.bfloat16).to(DEV).reshape(4, 8, K), wq, ws).shape == (4, 8, Nn)


def test_graph_capture_replays_the_same_bits(N_):
    rng = np.random.default_rng(31)
    M, Nn, K = 64, 1024, 8192
    A, B = t(rand_a(rng, M, K)), t(rand_fp4(rng, Nn, K))
    sa, sb = t(rand_scales(rng, M, K // 32)), t(rand_scales(rng, Nn, K // 32))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager = N_.fp8_scaled_mm_mxw4a8(A, B, sa, sb, out_dtype=torch.bfloat16)   # warm-up: the workspace exists before capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = N_.fp8_scaled_mm_mxw4a8(A, B, sa, sb, out_dtype=torch.bfloat16)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
