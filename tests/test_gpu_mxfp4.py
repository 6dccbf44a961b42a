"""GPU (MI355X): the MXFP4 (e2m1 x e2m1, block-scaled) GEMM, quantizer and dequantizer, and the patched torch._scaled_mm with
float4_e2m1fn_x2 operands and E8M0 scales.

Matmul bar: |gpu - exact| <= 1e-3 sum_k |a 2^sa| |b 2^sb| against the float64 reference of the decoded codes and scales (the MXFP8
tests' bar); the generic kernel sums in IEEE fp32 (4e-6).  With every scale 2^0 and K <= 4096 every product is a multiple of 0.25 up
to 36 and every partial sum is an fp32 value: the result must be exact (profiles/mxfp4_operand_map.txt)."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from mxfp4_ref import E2M1, mm_ref, scaled_operand, to_mxfp4_ref, unpack

pytestmark = pytest.mark.gpu

MFMA_TOL = 1.0e-3
FP32_TOL = 4e-6
MX_TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
            L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
DEV = "cuda"


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


def rand_fp4(rng, rows, K):
    return rng.integers(0, 256, size=(rows, K // 2), dtype=np.uint8)


def rand_scales(rng, rows, nb, lo=117, hi=137):
    return rng.integers(lo, hi + 1, size=(rows, nb), dtype=np.uint8)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(N_, A, B, sa, sb, **kw):
    out = N_.fp8_scaled_mm_mxfp4(t(A), t(B), t(sa), t(sb), **kw)
    torch.cuda.synchronize()
    return out.float().cpu().numpy().astype(np.float64)


def check(got, A, B, sa, sb, tol):
    exact, bound = mm_ref(A, B, sa, sb)
    err = np.abs(got - exact)
    assert np.all(err <= tol * bound + 1e-30), f"max err / bound {np.max(err / (bound + 1e-300)):.3e}"


@pytest.mark.parametrize("kernel", MX_TILES + [L.KERNEL_GENERIC])
def test_scale_map_every_kernel(N_, kernel):
    """Each (row, block) of both operands gets its own scale, one power of two apart from its neighbours along K, M and N, on
    asymmetric data: a kernel that ignores a scale, swaps the operands' scales, applies a block's scale to another block or
    pairs the wrong halves of a K-step fails."""
    rng = np.random.default_rng(kernel)
    M, Nn, K = 96, 80, 512
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    nb = K // 32
    sa = (112 + (np.arange(M)[:, None] * 3 + np.arange(nb)[None, :] * 2) % 31).astype(np.uint8)
    sb = (100 + (np.arange(Nn)[:, None] * 5 + np.arange(nb)[None, :] * 7) % 29).astype(np.uint8)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)
    # one-hot: one (row, block) of each operand at 2^1 / 2^2, everything else 2^0 - the sums stay exact, so the result must be
    # the reference bit for bit
    one = np.full((M, nb), 127, np.uint8)
    oneb = np.full((Nn, nb), 127, np.uint8)
    one[17, 5] = 128
    oneb[3, 9] = 129
    got = run(N_, A, B, one, oneb, kernel=kernel, split_k=1)
    exact, _ = mm_ref(A, B, one, oneb)
    assert np.array_equal(got, exact)


@pytest.mark.parametrize("M", [1, 7, 33, 64, 128, 300, 512])
@pytest.mark.parametrize("K", [32, 96, 160, 4096, 4128])
def test_shapes_auto(N_, M, K):
    rng = np.random.default_rng(M * 7 + K)
    Nn = 200
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    check(run(N_, A, B, sa, sb), A, B, sa, sb, MFMA_TOL)


@pytest.mark.parametrize("kernel", MX_TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO])
@pytest.mark.parametrize("K", [256, 4096])
def test_unit_scales_are_exact(N_, kernel, K):
    rng = np.random.default_rng(K + kernel)
    M, Nn = 70, 96
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    A[:3] = 0x77                        # rows of 6.0 x 6.0 products: |sum| up to 36 K
    B[:2] = 0x77
    s1, s2 = np.full((M, K // 32), 127, np.uint8), np.full((Nn, K // 32), 127, np.uint8)
    got = run(N_, A, B, s1, s2, kernel=kernel, split_k=1)
    exact, _ = mm_ref(A, B, s1, s2)
    assert np.array_equal(got, exact)


def test_c3_full_size_wide_scales(N_):
    rng = np.random.default_rng(3)
    M, Nn, K = 512, 4096, 4096
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32, 97, 157), rand_scales(rng, Nn, K // 32, 97, 157)   # 2^-30 ... 2^30
    for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128x64):
        check(run(N_, A, B, sa, sb, kernel=kernel, out_dtype=torch.float32), A, B, sa, sb, MFMA_TOL)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32])
@pytest.mark.parametrize("split", [2, 4])
def test_split_k(N_, kernel, split):
    rng = np.random.default_rng(split * 100 + kernel)
    M, Nn, K = 64, 512, 8192
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    one = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    s1 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    s2 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    assert np.array_equal(s1, s2)
    check(s1, A, B, sa, sb, MFMA_TOL)
    _, bound = mm_ref(A, B, sa, sb)
    assert np.all(np.abs(s1 - one) <= 2 * MFMA_TOL * bound)


def test_every_unsplit_fp4_tile_kernel_gives_the_same_bits(N_):
    rng = np.random.default_rng(11)
    M, Nn, K = 130, 200, 1024
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    outs = [run(N_, A, B, sa, sb, kernel=k, split_k=1) for k in MX_TILES]
    for k, o in zip(MX_TILES[1:], outs[1:]):
        assert np.array_equal(o, outs[0]), k


@pytest.mark.parametrize("kernel", MX_TILES + [L.KERNEL_GENERIC])
def test_bytes_7f_ff_are_finite_next_to_a_nan_scale_row(N_, kernel):
    """Bytes 0x7F (6.0, 1.5) and 0xFF (-6.0, -1.5) are finite e2m1 pairs.  Row 5 of A has a 0xFF (NaN) scale in the same tile:
    its outputs are NaN, every other output is exact - a NaN check with a scrubbed redo left in the fp4 kernels would zero
    those bytes and change them."""
    rng = np.random.default_rng(13)
    M, Nn, K = 64, 64, 512
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    A[:, ::7] = 0x7F
    A[:, 3::11] = 0xFF
    B[:, ::5] = 0xFF
    B[:, 2::9] = 0x7F
    sa, sb = np.full((M, K // 32), 127, np.uint8), np.full((Nn, K // 32), 127, np.uint8)
    sa[5, 3] = 0xFF
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    assert np.all(np.isnan(got[5]))
    rows = [m for m in range(M) if m != 5]
    exact, _ = mm_ref(A[rows], B, sa[rows], sb)
    assert np.array_equal(got[rows], exact)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC])
def test_special_scales(N_, kernel):
    rng = np.random.default_rng(5)
    M, Nn, K = 64, 64, 256
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), np.full((Nn, K // 32), 147, np.uint8)
    sa[3, 2] = 0x00                       # 2^-127 (times 2^20 of the other side: a normal fp32 sum)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)
    sb[9, 4] = 0xFF                       # E8M0 NaN on the B side: the whole output column that sums the block is NaN
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    assert np.all(np.isnan(got[:, 9]))
    cols = [n for n in range(Nn) if n != 9]
    check(got[:, cols], A, B[cols], sa, sb[cols], FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)


def _adversarial(rows=64, cols=256, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, 1), generator=g).float())
    x[0, :32] = 0.0                                                     # all zeros
    x[0, 32:64] = 1e-42                                                 # tiny (fp32 subnormal) block
    x[1, 5] = float("nan")                                              # NaN block
    x[2, 40] = float("inf"); x[3, 70] = float("-inf")                   # inf blocks
    x[4, :32] = torch.randn(32, generator=g) * 2.0 ** -140              # subnormal range
    x[5, :32] = torch.tensor([6.0, 2.5 + 2.0 ** -20, -2.5, 0.25, 0.75, 5.0, 3.5, 1.25, 1.75, -0.25, 0.5, 0.2578125] + [0.0] * 20)  # ties
    for j in range(8):                                                  # 6 2^k (1 + j 2^-23): the log2 edge
        x[6 + j, 96:128] = torch.randn(32, generator=g).clamp(-1, 1)
        x[6 + j, 100] = 6.0 * 2.0 ** (j - 4) * (1 + j * 2.0 ** -23)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_quantizer_matches_torch_recipe(N_, dtype):
    x = _adversarial(dtype=dtype)
    q, s = N_.fp8_quantize_mxfp4(x.to(DEV))
    torch.cuda.synchronize()
    want_s, want_q = to_mxfp4_ref(x.float() if dtype == torch.float16 else x)
    assert s.dtype == torch.float8_e8m0fnu and q.dtype == torch.float4_e2m1fn_x2 and q.shape == (64, 128)
    assert torch.equal(s.view(torch.uint8).cpu(), want_s)
    assert torch.equal(q.view(torch.uint8).cpu(), want_q)


def test_quantizer_row_strided_input(N_):
    x = _adversarial(cols=256)
    big = torch.zeros(64, 320)
    big[:, :256] = x
    q, s = N_.fp8_quantize_mxfp4(big.to(DEV)[:, :256])
    want_s, want_q = to_mxfp4_ref(x)
    assert torch.equal(s.view(torch.uint8).cpu(), want_s) and torch.equal(q.view(torch.uint8).cpu(), want_q)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dequant_is_exact(N_, out_dtype):
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, size=(48, 128), dtype=np.uint8)
    s = rand_scales(rng, 48, 8, 0, 254)
    s[0, 0] = 0xFF
    got = N_.fp8_dequantize_mxfp4(t(q).view(torch.float4_e2m1fn_x2), t(s), out_dtype=out_dtype).cpu()
    want = torch.from_numpy(scaled_operand(q, s)).float().to(out_dtype)
    assert got.shape == (48, 256)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    m = ~torch.isnan(want)
    assert torch.equal(got[m], want[m])


def test_patched_scaled_mm_with_fp4_operands():
    import fp8_mi355x_native as N
    import fp8_mps_patch
    rng = np.random.default_rng(21)
    M, Nn, K = 200, 384, 4128                 # K / 32 = 129 blocks: torch's padded scale rows hold 132 (4 mod 8)
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    nbp = (K // 32 + 3) // 4 * 4
    pa = np.full(((M + 127) // 128 * 128, nbp), 127, np.uint8)
    pb = np.full(((Nn + 127) // 128 * 128, nbp), 127, np.uint8)
    pa[:M, :K // 32], pb[:Nn, :K // 32] = sa, sb
    a = t(A).view(torch.float4_e2m1fn_x2)
    b = t(B).view(torch.float4_e2m1fn_x2)
    esa = t(pa).view(torch.float8_e8m0fnu).reshape(-1)          # torch's padded, flattened allocation
    esb = t(pb).view(torch.float8_e8m0fnu).reshape(-1)
    fp8_mps_patch.install()
    try:
        out = torch._scaled_mm(a, b.t(), scale_a=esa, scale_b=esb, out_dtype=torch.bfloat16)
    finally:
        fp8_mps_patch.uninstall()
    direct = N.fp8_scaled_mm_mxfp4(a, b, t(sa), t(sb), out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert out.shape == (M, Nn) and out.dtype == torch.bfloat16
    assert torch.equal(out, direct)
    exact, bound = mm_ref(A, B, sa, sb)
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - exact) <= MFMA_TOL * bound + 2.0 ** -8 * np.abs(exact))


def test_graph_capture_replays_the_same_bits(N_):
    rng = np.random.default_rng(31)
    M, Nn, K = 64, 1024, 8192
    A, B = t(rand_fp4(rng, M, K)), t(rand_fp4(rng, Nn, K))
    sa, sb = t(rand_scales(rng, M, K // 32)), t(rand_scales(rng, Nn, K // 32))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager = N_.fp8_scaled_mm_mxfp4(A, B, sa, sb, out_dtype=torch.bfloat16)   # warm-up: the workspace exists before capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = N_.fp8_scaled_mm_mxfp4(A, B, sa, sb, out_dtype=torch.bfloat16)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# e2m1 code -> the e4m3 byte of the same value (every e2m1 value is exact in e4m3)
_E4M3_OF = np.array([0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C, 0x80, 0xB0, 0xB8, 0xBC, 0xC0, 0xC4, 0xC8, 0xCC], np.uint8)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_AUTO])
def test_fp4_agrees_with_the_same_values_through_mxfp8(N_, kernel):
    rng = np.random.default_rng(41)
    M, Nn, K = 100, 144, 1024
    A, B = rand_fp4(rng, M, K), rand_fp4(rng, Nn, K)
    a8, b8 = _E4M3_OF[unpack(A)], _E4M3_OF[unpack(B)]
    assert np.array_equal(E2M1[unpack(A)], scaled_operand(A, np.full((M, K // 32), 127, np.uint8)))
    ones_a, ones_b = np.full((M, K // 32), 127, np.uint8), np.full((Nn, K // 32), 127, np.uint8)
    fp4 = run(N_, A, B, ones_a, ones_b, kernel=kernel, split_k=1)
    fp8 = N_.fp8_scaled_mm_mxfp8(t(a8), t(b8), t(ones_a), t(ones_b), kernel=kernel, split_k=1).double().cpu().numpy()
    assert np.array_equal(fp4, fp8)              # exact sums on both paths
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    fp4 = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    fp8 = N_.fp8_scaled_mm_mxfp8(t(a8), t(b8), t(sa), t(sb), kernel=kernel, split_k=1).double().cpu().numpy()
    _, bound = mm_ref(A, B, sa, sb)
    assert np.all(np.abs(fp4 - fp8) <= 2 * MFMA_TOL * bound)


def test_linear_mxfp4_matches_its_quantized_operands(N_):
    g = torch.Generator().manual_seed(1234)
    K, Nn = 1024, 256
    w = torch.randn(Nn, K, generator=g) * 0.02
    x = torch.randn(32, K, generator=g)
    wq, ws = N_.fp8_quantize_mxfp4(w.to(DEV))
    y = N_.fp8_linear_mxfp4(x.to(DEV), wq, ws, out_dtype=torch.float32).double().cpu().numpy()
    xs, xq = to_mxfp4_ref(x)
    exact, bound = mm_ref(xq.numpy(), wq.view(torch.uint8).cpu().numpy(), xs.numpy(), ws.view(torch.uint8).cpu().numpy())
    assert np.all(np.abs(y - exact) <= MFMA_TOL * bound)
    rel = np.linalg.norm(y - (x.double() @ w.double().T).numpy()) / np.linalg.norm((x.double() @ w.double().T).numpy())
    assert rel < 0.25, rel                       # an fp4 linear: coarse, but the product of the right operands
