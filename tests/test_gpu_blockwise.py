"""GPU (MI355X): the blockwise (1x128 / 128x128 fp32 scales) GEMM, quantizer and dequantizer, and the patched torch._scaled_mm
with torch's blockwise scale shapes.

Matmul bar (include/fp8mi.h): |gpu - oracle| <= (1e-3 + nkb 2^-23) sum_b |sa sb| sum_k |a b| - the MFMA accuracy note weighted
per block by the scale product, plus the fp32 rounding of the fold; the generic kernel sums each block in IEEE fp32."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from blockwise_ref import mm_ref, quantize_blockwise_ref

pytestmark = pytest.mark.gpu

MFMA_TOL = 1.0e-3
FP32_TOL = 128 * 2.0 ** -24
TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
         L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
PAIRS = [(1, 128), (1, 1), (128, 1), (128, 128)]
DEV = "cuda"


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


def rand_bytes(rng, shape):
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def rand_scales(rng, rows, K, block, lo=-20, hi=20):
    """random non-power-of-two fp32 scales spanning 2^lo .. 2^hi, random signs: (ceil(rows / block), ceil(K / 128))"""
    shape = (-(-rows // block), -(-K // 128))
    v = np.exp2(rng.uniform(lo, hi, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(N_, A, B, sa, sb, ba=1, bb=128, **kw):
    sa_t = sa if isinstance(sa, torch.Tensor) else t(sa)
    sb_t = sb if isinstance(sb, torch.Tensor) else t(sb)
    out = N_.fp8_scaled_mm_blockwise(t(A), t(B), sa_t, sb_t, block_a=ba, block_b=bb, **kw)
    torch.cuda.synchronize()
    return out.float().cpu().numpy().astype(np.float64)


def check(got, A, B, sa, sb, ba, bb, tol, nan_zero=True):
    exact, bound = mm_ref(A, B, sa, sb, ba, bb, nan_zero)
    nkb = -(-A.shape[1] // 128)
    err = np.abs(got - exact)
    lim = (tol + nkb * 2.0 ** -23) * bound
    assert np.all(err <= lim + 1e-30), f"max err / bound {np.max(err / (bound + 1e-300)):.3e}"


@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO])
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("MNK", [(130, 200, 400), (64, 96, 48), (33, 140, 1024)])
def test_parity_every_kernel_every_pair(N_, kernel, pair, MNK):
    M, Nn, K = MNK
    ba, bb = pair
    rng = np.random.default_rng(kernel * 1000 + ba * 3 + bb + K)
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K, ba), rand_scales(rng, Nn, K, bb)
    got = run(N_, A, B, sa, sb, ba, bb, kernel=kernel, split_k=1)
    check(got, A, B, sa, sb, ba, bb, FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL)


@pytest.mark.parametrize("pair", PAIRS)
def test_exact_data_every_kernel_equals_the_oracle(N_, pair):
    ba, bb = pair
    rng = np.random.default_rng(17 + ba + bb)
    M, Nn, K = 100, 136, 992                                   # (the ring tiles take K % 16 == 0; a partial last block)
    vals = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=np.uint8)   # 0, +-1, +-2, +-3, +-4
    A, B = vals[rng.integers(0, len(vals), (M, K))], vals[rng.integers(0, len(vals), (Nn, K))]
    sa = np.exp2(rng.integers(-2, 3, size=(-(-M // ba), -(-K // 128)))).astype(np.float32)
    sb = np.exp2(rng.integers(-2, 3, size=(-(-Nn // bb), -(-K // 128)))).astype(np.float32)
    exact, _ = mm_ref(A, B, sa, sb, ba, bb)
    for kernel in TILES + [L.KERNEL_GENERIC]:
        assert np.array_equal(run(N_, A, B, sa, sb, ba, bb, kernel=kernel, split_k=1), exact), kernel


def test_every_unsplit_tile_gives_the_same_bits(N_):
    rng = np.random.default_rng(11)
    M, Nn, K = 130, 200, 512
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    for ba, bb in PAIRS:
        sa, sb = rand_scales(rng, M, K, ba), rand_scales(rng, Nn, K, bb)
        outs = [run(N_, A, B, sa, sb, ba, bb, kernel=k, split_k=1) for k in TILES]
        for k, o in zip(TILES[1:], outs[1:]):
            assert np.array_equal(o, outs[0]), (k, ba, bb)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32])
@pytest.mark.parametrize("split", [2, 3])
def test_split_k(N_, kernel, split):
    rng = np.random.default_rng(split * 100 + kernel)
    M, Nn, K = 64, 512, 4096 + 48
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K, 1), rand_scales(rng, Nn, K, 128)
    s1 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    s2 = run(N_, A, B, sa, sb, kernel=kernel, split_k=split)
    assert np.array_equal(s1, s2)
    check(s1, A, B, sa, sb, 1, 128, MFMA_TOL)


def test_scale_layouts_read_in_place_give_the_same_bits(N_):
    rng = np.random.default_rng(4)
    M, Nn, K = 192, 256, 640
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K, 1), rand_scales(rng, Nn, K, 128)
    sa_rm = t(sa)                                    # row-major (M, K/128)
    sa_om = t(sa.T.copy()).t()                       # torch's outer-dim-major: (M, K/128) with stride (1, M)
    sb_ds = t(sb)                                    # DeepSeek's weight_scale_inv (N/128, K/128), row-major
    sb_tv = t(sb.T.copy()).t()                       # torch's (K/128, N/128) seen through .t()
    assert sa_om.stride() == (1, M)
    for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_64x64, L.KERNEL_GENERIC):
        ref = run(N_, A, B, sa_rm, sb_ds, kernel=kernel)
        for a_, b_ in ((sa_om, sb_ds), (sa_rm, sb_tv), (sa_om, sb_tv)):
            assert np.array_equal(run(N_, A, B, a_, b_, kernel=kernel), ref), kernel


@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
def test_special_scales_and_nan_bytes_ring_equals_generic(N_, nan_mode):
    rng = np.random.default_rng(5)
    M, Nn, K = 64, 256, 384
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    A[7, 200] = 0x7F                        # a NaN byte in block 1 of row 7
    B[9, 10] = 0xFF                         # ... in block 0 of column 9
    for ba, bb in ((1, 128), (1, 1)):
        sa, sb = rand_scales(rng, M, K, ba, -4, 4), rand_scales(rng, Nn, K, bb, -4, 4)
        sa[3, 2] = 0.0
        sa[5, 1] = np.inf
        nan_cols = slice(128, 256) if bb == 128 else slice(20, 21)
        sb[1 if bb == 128 else 20, 0] = np.nan
        gen = run(N_, A, B, sa, sb, ba, bb, kernel=L.KERNEL_GENERIC, nan_mode=nan_mode)
        exact, bound = mm_ref(A, B, sa, sb, ba, bb, nan_mode == L.NAN_ZERO)
        for kernel in (L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GEMM_32x32, L.KERNEL_AUTO):
            got = run(N_, A, B, sa, sb, ba, bb, kernel=kernel, split_k=1, nan_mode=nan_mode)
            assert np.array_equal(np.isnan(got), np.isnan(gen)), kernel
            assert np.array_equal(np.isinf(got), np.isinf(gen)), kernel
            fin = np.isfinite(gen)
            assert np.all(np.abs(got[fin] - exact[fin]) <= (MFMA_TOL + 3 * 2.0 ** -23) * bound[fin] + 1e-30), kernel
        assert not np.isfinite(gen[5]).any()                 # the inf scale reaches every output of its row
        assert np.isnan(gen[:, nan_cols]).all()              # the NaN scale poisons its column(s)
        if nan_mode == L.NAN_PROPAGATE:
            assert np.isnan(gen[7]).all() and np.isnan(gen[:, 9]).all()
        else:
            assert np.isfinite(gen[7, :20]).all() and np.isfinite(gen[[0, 1, 2, 3, 4, 6], 9]).all()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_out_dtypes_bias_scale_result(N_, out_dtype):
    rng = np.random.default_rng(8)
    M, Nn, K = 96, 160, 512
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa, sb = rand_scales(rng, M, K, 1, -8, -4), rand_scales(rng, Nn, K, 128, -8, -4)
    bias = torch.randn(Nn, generator=torch.Generator().manual_seed(1)).to(DEV)
    sr = torch.tensor([0.75], device=DEV)
    for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128, L.KERNEL_GENERIC):
        f32 = N_.fp8_scaled_mm_blockwise(t(A), t(B), t(sa), t(sb), kernel=kernel, out_dtype=torch.float32)
        got = N_.fp8_scaled_mm_blockwise(t(A), t(B), t(sa), t(sb), kernel=kernel, out_dtype=out_dtype, bias=bias, scale_result=sr)
        want = ((f32 + bias) * sr).to(out_dtype)
        assert torch.equal(got, want), kernel


def test_transposed_epilogue_with_128x1_blocks(N_):
    rng = np.random.default_rng(9)
    M, Nn, K = 72, 256, 768
    X, W = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sx, sw = rand_scales(rng, M, K, 1), rand_scales(rng, Nn, K, 128)
    bias = torch.randn(Nn, generator=torch.Generator().manual_seed(2)).to(DEV)
    for kernel in (L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC):
        ref = N_.fp8_scaled_mm_blockwise(t(X), t(W), t(sx), t(sw), block_a=1, block_b=128, bias=bias, kernel=kernel, split_k=1)
        tr = N_.fp8_scaled_mm_blockwise(t(W), t(X), t(sw), t(sx), block_a=128, block_b=1, bias=bias, kernel=kernel, split_k=1,
                                        transposed_epilogue=True)
        assert torch.equal(tr.t(), ref), kernel


@pytest.mark.parametrize("block_rows", [1, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_quantizer_matches_the_reference_byte_for_byte(N_, block_rows, dtype):
    g = torch.Generator().manual_seed(block_rows + 3)
    x = (torch.randn(300, 1000, generator=g) * torch.exp2(torch.randint(-12, 12, (300, 1), generator=g).float())).to(dtype)
    x[0:128, 0:128] = 0.0                                   # an all-zero block (both block sizes)
    x[2, 300] = float("nan")                                # NaN blocks
    x[150, 700] = float("inf")                              # inf blocks: inf / inf is NaN, finite / inf is 0
    x[151, 705] = -float("inf")
    x[290, 999] = 3.0e4
    wide = torch.zeros(300, 1032, dtype=dtype)
    wide[:, :1000] = x
    src = wide.to(DEV)[:, :1000]                            # row-strided input
    q, s = N_.fp8_quantize_blockwise(src, block_rows)
    rq, rs = quantize_blockwise_ref(x, block_rows)
    assert torch.equal(q.cpu(), rq)
    assert torch.equal(s.cpu().view(torch.int32), rs.view(torch.int32))
    # dequantisation is exact: float(dec(q)) * s rounded once, then to out_dtype
    full = rs.repeat_interleave(block_rows, 0).repeat_interleave(128, 1)[:300, :1000]
    for out_dtype in (torch.float32, torch.float16, torch.bfloat16):
        d = N_.fp8_dequantize_blockwise(q, s, block_rows, out_dtype).cpu()
        want = (rq.view(torch.float8_e4m3fn).float() * full).to(out_dtype)
        assert torch.equal(torch.isnan(d), torch.isnan(want))
        fin = ~torch.isnan(want)
        assert torch.equal(d[fin], want[fin])


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scale_b_kind", ["128x128", "1x128"])
def test_patched_scaled_mm_equals_the_native_op(N_, out_dtype, scale_b_kind):
    import fp8_mps_patch
    rng = np.random.default_rng(12)
    M, Nn, K = 96, 384, 640
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa = t(rand_scales(rng, M, K, 1))                                            # (M, K/128)
    bb = 128 if scale_b_kind == "128x128" else 1
    sb_nk = rand_scales(rng, Nn, K, bb)                                           # (N/bb, K/128)
    sb = t(sb_nk.T.copy())                                                        # torch's (K/128, N/bb)
    a8 = t(A).view(torch.float8_e4m3fn)
    b8 = t(B).view(torch.float8_e4m3fn).t()                                      # (K, N) column-major
    fp8_mps_patch.install()
    try:
        got = torch._scaled_mm(a8, b8, scale_a=sa, scale_b=sb, out_dtype=out_dtype)
    finally:
        fp8_mps_patch.uninstall()
    want = N_.fp8_scaled_mm_blockwise(t(A), t(B), sa, t(sb_nk), block_a=1, block_b=bb, out_dtype=out_dtype)
    assert got.dtype == out_dtype and torch.equal(got, want)


def test_linear_blockwise_beats_tensorwise_on_outlier_weights(N_):
    g = torch.Generator().manual_seed(21)
    M, K, Nn = 64, 2048, 512
    x = torch.randn(M, K, generator=g)
    w = torch.randn(Nn, K, generator=g) * 0.02
    w[::97, ::331] = 1000.0                 # outliers set the per-tensor scale: the other weights fall into e4m3's subnormals
    x[:, ::331] = 0.0                       # (their input channels are silent: the error measured is the weight quantisation's)
    x, w = x.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = torch.nn.functional.linear(x.float(), w.float())
    wq_b, ws_b = N_.fp8_quantize_blockwise(w.to(DEV), 128)
    yb = N_.fp8_linear_blockwise(x.to(DEV), wq_b, ws_b).float().cpu()
    wq_t, ws_t = N_.fp8_quantize(w.to(DEV))
    yt = N_.fp8_linear(x.to(DEV), wq_t, ws_t).float().cpu()
    eb = ((yb - ref).norm() / ref.norm()).item()
    et = ((yt - ref).norm() / ref.norm()).item()
    assert eb < et, (eb, et)
    assert eb < 0.06, eb


def test_graph_capture_replays_the_same_bits(N_):
    rng = np.random.default_rng(31)
    M, Nn, K = 64, 1024, 2048
    A, B = t(rand_bytes(rng, (M, K))), t(rand_bytes(rng, (Nn, K)))
    sa, sb = t(rand_scales(rng, M, K, 1)), t(rand_scales(rng, Nn, K, 128))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = N_.fp8_scaled_mm_blockwise(A, B, sa, sb, out_dtype=torch.bfloat16)   # warm-up: the stream's split-K workspace
        out = torch.empty_like(eager)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        N_.fp8_scaled_mm_blockwise(A, B, sa, sb, out_dtype=torch.bfloat16, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
