"""GPU (MI355X): the MXFP8 (block-scaled) GEMM, quantizer and dequantizer, and the patched torch._scaled_mm with E8M0 scales.

Matmul bar: |gpu - exact| <= 1e-3 sum_k |a 2^sa| |b 2^sb| against the float64 reference of the decoded bytes and scales
(the MFMA bar of tests/test_gpu_parity.py); the generic kernel sums in IEEE fp32 (4e-6)."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from mxfp8_ref import mm_ref, scaled_operand, to_mxfp8_ref

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


def rand_bytes(rng, shape):
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def rand_scales(rng, rows, nb, lo=117, hi=137):
    return rng.integers(lo, hi + 1, size=(rows, nb), dtype=np.uint8)


def run(N_, A, B, sa, sb, **kw):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = N_.fp8_scaled_mm_mxfp8(t(A), t(B), t(sa), t(sb), **kw)
    torch.cuda.synchronize()
    return out.float().cpu().numpy().astype(np.float64)


def check(got, A, B, sa, sb, tol, nan_zero=True):
    exact, bound = mm_ref(A, B, sa, sb, nan_zero)
    err = np.abs(got - exact)
    assert np.all(err <= tol * bound + 1e-30), f"max err / bound {np.max(err / (bound + 1e-300)):.3e}"


@pytest.mark.parametrize("kernel", MX_TILES + [L.KERNEL_GENERIC])
def test_scale_map_every_kernel(N_, kernel):
    """Scales that differ along K, along M and along N, on asymmetric data: a kernel that ignores a scale, swaps the operands'
    scales or applies a block's scale to another block fails."""
    rng = np.random.default_rng(kernel)
    M, Nn, K = 96, 80, 384
    A = rand_bytes(rng, (M, K))
    B = rand_bytes(rng, (Nn, K))
    sa = rand_scales(rng, M, K // 32, 112, 142)
    sb = rand_scales(rng, Nn, K // 32, 100, 130)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)


@pytest.mark.parametrize("M", [1, 7, 33, 64, 128, 300, 512])
@pytest.mark.parametrize("K", [32, 96, 160, 4096, 4128])
def test_shapes_auto(N_, M, K):
    rng = np.random.default_rng(M * 7 + K)
    Nn = 200
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    check(run(N_, A, B, sa, sb), A, B, sa, sb, MFMA_TOL)


def test_c3_full_size_wide_scales(N_):
    rng = np.random.default_rng(3)
    M, Nn, K = 512, 4096, 4096
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32, 97, 157), rand_scales(rng, Nn, K // 32, 97, 157)   # 2^-30 ... 2^30
    for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128x64):
        check(run(N_, A, B, sa, sb, kernel=kernel, out_dtype=torch.float32), A, B, sa, sb, MFMA_TOL)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32])
@pytest.mark.parametrize("split", [2, 4])
def test_split_k(N_, kernel, split):
    rng = np.random.default_rng(split * 100 + kernel)
    M, Nn, K = 64, 512, 4096
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    one = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    s1 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    s2 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    assert np.array_equal(s1, s2)
    check(s1, A, B, sa, sb, MFMA_TOL)
    _, bound = mm_ref(A, B, sa, sb)
    assert np.all(np.abs(s1 - one) <= 2 * MFMA_TOL * bound)


def test_every_unsplit_mx_tile_kernel_gives_the_same_bits(N_):
    rng = np.random.default_rng(11)
    M, Nn, K = 130, 200, 512
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    outs = [run(N_, A, B, sa, sb, kernel=k, split_k=1) for k in MX_TILES]
    for k, o in zip(MX_TILES[1:], outs[1:]):
        assert np.array_equal(o, outs[0]), k


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC])
def test_special_scales(N_, kernel):
    rng = np.random.default_rng(5)
    M, Nn, K = 64, 64, 256
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32), np.full((Nn, K // 32), 147, np.uint8)
    sa[3, 2] = 0x00                       # 2^-127 (times 2^20 of the other side: a normal fp32 sum)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)
    sa[5, 1] = 0xFF                       # E8M0 NaN: the whole output row that sums the block is NaN
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1)
    assert np.all(np.isnan(got[5]))
    rows = [m for m in range(M) if m != 5]
    check(got[rows], A[rows], B, sa[rows], sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128x64, L.KERNEL_GENERIC])
@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
def test_nan_bytes(N_, kernel, nan_mode):
    rng = np.random.default_rng(9)
    M, Nn, K = 64, 64, 256
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    A[2, 40] = 0x7F
    B[7, 200] = 0xFF
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    got = run(N_, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=nan_mode)
    if nan_mode == L.NAN_ZERO:
        check(got, A, B, sa, sb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL, nan_zero=True)
    else:
        assert np.all(np.isnan(got[2])) and np.all(np.isnan(got[:, 7]))
        rows = [m for m in range(M) if m != 2]
        cols = [n for n in range(Nn) if n != 7]
        check(got[np.ix_(rows, cols)], A[rows], B[cols], sa[rows], sb[cols], FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)


def _adversarial(rows=64, cols=256, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, 1), generator=g).float())
    x[0, :32] = 0.0                                                     # all zeros
    x[1, 5] = float("nan")                                              # NaN block
    x[2, 40] = float("inf"); x[3, 70] = float("-inf")                   # inf blocks
    x[4, :32] = torch.randn(32, generator=g) * 2.0 ** -140              # subnormal range
    for j in range(8):                                                  # 448 2^k (1 + j 2^-23): the log2 edge
        x[5 + j, 96:128] = torch.randn(32, generator=g).clamp(-1, 1) * 100
        x[5 + j, 100] = 448.0 * 2.0 ** (j - 4) * (1 + j * 2.0 ** -23)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_quantizer_matches_torch_recipe(N_, dtype):
    x = _adversarial(dtype=dtype)
    if dtype == torch.float16:
        x = torch.nan_to_num(x, nan=float("nan"), posinf=float("inf"), neginf=float("-inf"))
    q, s = N_.fp8_quantize_mxfp8(x.to(DEV))
    torch.cuda.synchronize()
    want_s, want_q = to_mxfp8_ref(x.float() if dtype == torch.float16 else x)
    assert s.dtype == torch.float8_e8m0fnu and q.dtype == torch.uint8
    assert torch.equal(s.view(torch.uint8).cpu(), want_s)
    assert torch.equal(q.cpu(), want_q)


def test_quantizer_row_strided_input(N_):
    x = _adversarial(cols=256)
    big = torch.zeros(64, 320)
    big[:, :256] = x
    q, s = N_.fp8_quantize_mxfp8(big.to(DEV)[:, :256])
    want_s, want_q = to_mxfp8_ref(x)
    assert torch.equal(s.view(torch.uint8).cpu(), want_s) and torch.equal(q.cpu(), want_q)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dequant_is_exact(N_, out_dtype):
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, size=(48, 256), dtype=np.uint8)
    s = rand_scales(rng, 48, 8, 0, 254)
    s[0, 0] = 0xFF
    got = N_.fp8_dequantize_mxfp8(torch.from_numpy(q).to(DEV), torch.from_numpy(s).to(DEV), out_dtype=out_dtype).cpu()
    want = torch.from_numpy(scaled_operand(q, s, nan_zero=False)).float().to(out_dtype)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    m = ~torch.isnan(want)
    assert torch.equal(got[m], want[m])


def test_patched_scaled_mm_with_e8m0_scales():
    import fp8_mps_patch
    rng = np.random.default_rng(21)
    M, Nn, K = 256, 384, 512
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    a = torch.from_numpy(A).to(DEV).view(torch.float8_e4m3fn)
    b = torch.from_numpy(B).to(DEV).view(torch.float8_e4m3fn)
    esa = torch.from_numpy(sa).to(DEV).view(torch.float8_e8m0fnu)
    esb = torch.from_numpy(sb).to(DEV).view(torch.float8_e8m0fnu)
    fp8_mps_patch.install()
    try:
        out = torch._scaled_mm(a, b.t(), scale_a=esa, scale_b=esb, out_dtype=torch.bfloat16)
    finally:
        fp8_mps_patch.uninstall()
    torch.cuda.synchronize()
    exact, bound = mm_ref(A, B, sa, sb)
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - exact) <= MFMA_TOL * bound + 2.0 ** -8 * np.abs(exact))
    try:
        ref = fp8_mps_patch._original_scaled_mm(a, b.t(), scale_a=esa, scale_b=esb, out_dtype=torch.bfloat16)
        torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001 - the unpatched op does not serve this call on this build of torch
        pytest.skip(f"the unpatched torch._scaled_mm does not run MXFP8 here ({type(e).__name__}); the f64 comparison passed")
    r = ref.float().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - r) <= 2 * MFMA_TOL * bound + 2.0 ** -7 * np.abs(exact))


def test_mx_linear_beats_per_tensor_on_outlier_weights(N_):
    """A weight whose few outliers (1e5 x the bulk) set the per-tensor scale pushes the bulk into e4m3's subnormal range; one
    scale per 32 weights keeps it in the normal range.  Per output feature (weight row) against the float64 product, the
    median relative error of fp8_linear_mxfp8 is far below fp8_linear's."""
    g = torch.Generator().manual_seed(1234)
    K, Nn = 1024, 512
    w = torch.randn(Nn, K, generator=g) * 0.02
    idx = torch.randint(0, Nn * K, (16,), generator=g)
    w.view(-1)[idx] = 2000.0 * torch.sign(torch.randn(16, generator=g))   # a few outliers
    x = torch.randn(32, K, generator=g)
    ref = x.double() @ w.double().T
    wq, ws = N_.fp8_quantize_mxfp8(w.to(DEV))
    y_mx = N_.fp8_linear_mxfp8(x.to(DEV), wq, ws, out_dtype=torch.float32).double().cpu()
    wq_t, ws_t = N_.fp8_quantize(w.to(DEV))
    y_t = N_.fp8_linear(x.to(DEV), wq_t, ws_t, out_dtype=torch.float32).double().cpu()
    e_mx = ((y_mx - ref).norm(dim=0) / ref.norm(dim=0)).median().item()
    e_t = ((y_t - ref).norm(dim=0) / ref.norm(dim=0)).median().item()
    assert e_mx < 0.5 * e_t, (e_mx, e_t)


def test_graph_capture_replays_the_same_bits(N_):
    rng = np.random.default_rng(31)
    M, Nn, K = 64, 1024, 4096
    A = torch.from_numpy(rand_bytes(rng, (M, K))).to(DEV)
    B = torch.from_numpy(rand_bytes(rng, (Nn, K))).to(DEV)
    sa = torch.from_numpy(rand_scales(rng, M, K // 32)).to(DEV)
    sb = torch.from_numpy(rand_scales(rng, Nn, K // 32)).to(DEV)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager = N_.fp8_scaled_mm_mxfp8(A, B, sa, sb, out_dtype=torch.bfloat16)   # warm-up: the workspace exists before capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = N_.fp8_scaled_mm_mxfp8(A, B, sa, sb, out_dtype=torch.bfloat16)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("kernel", MX_TILES)
def test_unit_scales_reproduce_the_tensorwise_bits(N_, kernel):
    """The ring kernels' K order is the instruction's own (profiles/mxfp8_scale_map.txt): with every scale 2^0 (0x7F) the
    block-scaled kernel computes exactly what its tensorwise twin computes with per-tensor scales of 1."""
    rng = np.random.default_rng(40 + kernel)
    M, Nn, K = 100, 144, 640
    A = torch.from_numpy(rand_bytes(rng, (M, K))).to(DEV)
    B = torch.from_numpy(rand_bytes(rng, (Nn, K))).to(DEV)
    one = torch.ones(1, device=DEV)
    s7f = torch.full((max(M, Nn), K // 32), 0x7F, dtype=torch.uint8, device=DEV)
    mx = N_.fp8_scaled_mm_mxfp8(A, B, s7f[:M], s7f[:Nn], kernel=kernel, split_k=1)
    tw = N_.fp8_scaled_mm(A, B, one, one, kernel=kernel, split_k=1)
    torch.cuda.synchronize()
    assert torch.equal(mx, tw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_stand_alone_quantiser_output_off_16_byte_alignment(N_, fmt, dtype):
    """The stand-alone MX quantisers (both formats are one kernel) store a block byte by byte where it is not 16-byte aligned - a layout
    the op layer never produces, so through the C ABI: the output 4 bytes into its buffer with rows 4 bytes apart (blocks at 4, 8, 12 and 0
    mod 16), scale rows of 5 bytes for 3 blocks, the input a column slab of a wider buffer.  Bytes and scales are the op layer's on the
    same data, byte for byte, and nothing else in the two 0xAA-filled buffers is touched."""
    rows, cols, per_byte = 5, 96, 2 if fmt == "mxfp4" else 1
    row_bytes, nb, ld_s = cols // per_byte, cols // 32, 5
    ld_out = row_bytes + 4
    g = torch.Generator().manual_seed(11)
    wide = torch.randn(rows, cols + 8, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, 1), generator=g).float())
    wide[1, 8 + 32:8 + 64] = 0.0                      # an all-zero block
    wide[2, 8 + 3], wide[3, 8 + 70], wide[4, 8 + 95] = float("nan"), float("inf"), -float("inf")
    wide = wide.to(dtype).to(DEV)
    x = wide[:, 8:]
    want_q, want_s = N_.fp8_quantize_mxfp8(x) if fmt == "mxfp8" else N_.fp8_quantize_mxfp4(x)
    out = torch.full((4 + rows * ld_out + 12,), 0xAA, dtype=torch.uint8, device=DEV)
    sc = torch.full((rows * ld_s + 3,), 0xAA, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 16 == 0 and x.data_ptr() == wide.data_ptr() + 8 * wide.element_size()
    rc = getattr(L.load(), f"fp8mi_quantize_{fmt}")(x.data_ptr(), {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}[dtype], rows, cols,
                                                     cols + 8, out.data_ptr() + 4, ld_out, sc.data_ptr(), ld_s, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().fp8mi_last_error()
    torch.cuda.synchronize()
    out, sc = out.cpu().numpy(), sc.cpu().numpy()
    want_out, want_sc = np.full_like(out, 0xAA), np.full_like(sc, 0xAA)
    want_q, want_s = want_q.view(torch.uint8).cpu().numpy(), want_s.view(torch.uint8).cpu().numpy()
    assert want_q.shape == (rows, row_bytes) and want_s.shape == (rows, nb)
    for r in range(rows):
        want_out[4 + r * ld_out:4 + r * ld_out + row_bytes] = want_q[r]
        want_sc[r * ld_s:r * ld_s + nb] = want_s[r]
    assert np.array_equal(out, want_out), np.argwhere(out != want_out)[:8].ravel()
    assert np.array_equal(sc, want_sc), np.argwhere(sc != want_sc)[:8].ravel()
