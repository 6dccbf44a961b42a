"""GPU (MI355X): the edges of the three microscaling GEMMs (MXFP8, MXFP4 and MXW4A8: e4m3 A against e2m1 B) that
tests/test_gpu_mxfp8.py, tests/test_gpu_mxfp4.py and tests/test_gpu_mxw4a8.py leave out - the fused epilogue (bias, scale_result,
bf16 / f16 output, the transposed form), the scale layouts callers really pass (torch's padded allocation, wide and offset
views) with every padding byte poisoned by the E8M0 NaN 0xFF, strided operands and `out=`, exact scale-map checks, split-K
edges, a seeded sweep of AUTO, a tall M and degenerate shapes.  Every test runs on all three formats through a small adapter;
the third is asymmetric: A holds K bytes a row and may hold NaN bytes, B holds K / 2 and has no NaN encoding.

The reference is always the float64 `mm_ref` of the decoded bytes and scales (tests/mxfp8_ref.py, tests/mxfp4_ref.py,
tests/mxw4a8_ref.py).  Bars, as in the files named above: |gpu - exact| <= 1e-3 sum_k |a 2^sa| |b 2^sb| on the matrix-core tiles, 4e-6 on the generic
kernel (IEEE fp32 sums).  Fused bf16 / f16 output, bias and scale_result are pinned bit for bit to
((f32 + bias) * scale_result).to(out_dtype), where f32 is the same kernel's plain fp32 result and is itself held to the bar.
Where two runs of the product are compared bit for bit, one of them is also held to `mm_ref`."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import mxfp4_ref
import mxfp8_ref
import mxw4a8_ref

pytestmark = pytest.mark.gpu

MFMA_TOL = 1.0e-3
FP32_TOL = 4e-6
DEV = "cuda"
TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
         L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
OUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
E_UNSUPPORTED = -4   # include/fp8mi.h


# ---- the three formats ------------------------------------------------------------------------------------------------
# rand_a / rand_b, small_ints_a / small_ints_b: the builders of the A and the B operand (one function where the format is symmetric);
# kdiv_a / kdiv_b: K elements per byte of each; seed: what the format mixes into its seeds; a_nan / b_nan: the side has NaN bytes
class _MXFP8:
    name = "mxfp8"
    kdiv_a = kdiv_b = seed = 1
    a_nan = b_nan = True
    mm_name, linear_name = "fp8_scaled_mm_mxfp8", "fp8_linear_mxfp8"
    quant_a_name = quant_b_name = "fp8_quantize_mxfp8"
    epi_scales = (116, 122)                    # 2^-11 .. 2^-5 per side: sums of e4m3 products land in f16's range
    _INTS = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=np.uint8)   # 0, +-1, +-2, +-3, +-4

    @staticmethod
    def rand_operand(rng, rows, K):
        b = rng.integers(0, 256, size=(rows, K), dtype=np.uint8)
        b[(b & 0x7F) == 0x7F] ^= 1             # no NaN bytes unless a test asks for them
        return b

    rand_a = rand_b = rand_operand

    @staticmethod
    def ref(A, B, sa, sb, nan_zero=True):
        return mxfp8_ref.mm_ref(A, B, sa, sb, nan_zero)

    @staticmethod
    def one_hot(M, K, ks):
        A = np.zeros((M, K), np.uint8)
        A[np.arange(M), ks] = 0x38             # 1.0
        return A

    @classmethod
    def small_ints(cls, rng, rows, K):
        return cls._INTS[rng.integers(0, len(cls._INTS), (rows, K))]

    small_ints_a = small_ints_b = small_ints

    @staticmethod
    def c_call(lib, A, B, C, sa, ld_sa, sb, ld_sb, M, N, K, lda, ldb, ldc, kernel, stream):
        return lib.fp8mi_scaled_mm_mxfp8(A, B, C, sa, ld_sa, sb, ld_sb, None, None, M, N, K, lda, ldb, ldc, L.F32, L.F32,
                                         L.NAN_ZERO, kernel, 1, None, 0, stream)


class _MXFP4:
    name = "mxfp4"
    kdiv_a = kdiv_b = seed = 2
    a_nan = b_nan = False
    mm_name, linear_name = "fp8_scaled_mm_mxfp4", "fp8_linear_mxfp4"
    quant_a_name = quant_b_name = "fp8_quantize_mxfp4"
    epi_scales = (124, 130)
    _INTS = np.array([0x0, 0x2, 0x4, 0x5, 0x6, 0x7, 0xA, 0xC, 0xD, 0xE, 0xF], dtype=np.uint8)   # 0, +-1, +-2, +-3, +-4, +-6

    @staticmethod
    def rand_operand(rng, rows, K):
        return rng.integers(0, 256, size=(rows, K // 2), dtype=np.uint8)

    rand_a = rand_b = rand_operand

    @staticmethod
    def ref(A, B, sa, sb, nan_zero=True):
        return mxfp4_ref.mm_ref(A, B, sa, sb)

    @staticmethod
    def one_hot(M, K, ks):
        A = np.zeros((M, K // 2), np.uint8)
        A[np.arange(M), ks // 2] = (0x2 << (4 * (ks & 1))).astype(np.uint8)   # code 2 = 1.0: low nibble for even k
        return A

    @classmethod
    def small_ints(cls, rng, rows, K):
        codes = cls._INTS[rng.integers(0, len(cls._INTS), (rows, K))]
        return ((codes[:, 1::2] << 4) | codes[:, 0::2]).astype(np.uint8)

    small_ints_a = small_ints_b = small_ints

    @staticmethod
    def c_call(lib, A, B, C, sa, ld_sa, sb, ld_sb, M, N, K, lda, ldb, ldc, kernel, stream):
        return lib.fp8mi_scaled_mm_mxfp4(A, B, C, sa, ld_sa, sb, ld_sb, None, None, M, N, K, lda, ldb, ldc, L.F32, L.F32,
                                         kernel, 1, None, 0, stream)


class _MXW4A8:
    """A as in MXFP8 (K bytes a row, nan_mode), B as in MXFP4 (K / 2 bytes a row); lda counts A's bytes, ldb B's"""
    name = "mxw4a8"
    kdiv_a, kdiv_b, seed = 1, 2, 3
    a_nan, b_nan = True, False                 # (B's bytes 0x7F / 0xFF are the finite pairs 6.0 | 1.5 and -6.0 | -1.5)
    mm_name, linear_name = "fp8_scaled_mm_mxw4a8", "fp8_linear_mxw4a8"
    quant_a_name, quant_b_name = "fp8_quantize_mxfp8", "fp8_quantize_mxfp4"
    epi_scales = (119, 125)                    # 2^-8 .. 2^-2 per side: max |exact| < 65504 at every epilogue shape (tests/test_mxw4a8_host.py)
    rand_a, rand_b = staticmethod(mxw4a8_ref.rand_a), staticmethod(mxw4a8_ref.rand_b)
    small_ints_a, small_ints_b = staticmethod(mxw4a8_ref.small_ints_a), staticmethod(mxw4a8_ref.small_ints_b)
    one_hot = staticmethod(mxw4a8_ref.one_hot_a)
    ref = staticmethod(mxw4a8_ref.mm_ref)

    @staticmethod
    def c_call(lib, A, B, C, sa, ld_sa, sb, ld_sb, M, N, K, lda, ldb, ldc, kernel, stream):
        return lib.fp8mi_scaled_mm_mxw4a8(A, B, C, sa, ld_sa, sb, ld_sb, None, None, M, N, K, lda, ldb, ldc, L.F32, L.F32,
                                          L.NAN_ZERO, kernel, 1, None, 0, stream)


@pytest.fixture(params=[_MXFP8, _MXFP4, _MXW4A8], ids=lambda f: f.name)
def fx(request):
    return request.param


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


# ---- helpers ----------------------------------------------------------------------------------------------------------
def t(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rand_scales(rng, rows, nb, lo=117, hi=137):
    return rng.integers(lo, hi + 1, size=(rows, nb), dtype=np.uint8)


def run(N_, fx, A, B, sa, sb, **kw):
    out = getattr(N_, fx.mm_name)(t(A), t(B), t(sa), t(sb), **kw)
    torch.cuda.synchronize()
    return out


def f64(x):
    return x.float().cpu().numpy().astype(np.float64)


def tol_of(kernel):
    return FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL


def check(got, exact, bound, tol, what=""):
    err = np.abs(f64(got) - exact)
    assert np.all(err <= tol * bound + 1e-30), f"{what}: max err / bound {np.max(err / (bound + 1e-300)):.3e} (bar {tol:g})"


def counters_zero(N_):
    ws = N_._workspace(torch.device(DEV, torch.cuda.current_device()))
    torch.cuda.synchronize()
    return int(ws[:L.WS_COUNTER_BYTES].view(torch.int32).abs().sum().item()) == 0


def make_bias(n, seed, dtype=torch.float32):
    """A non-symmetric vector; bias[i] = i at a few indices, so that a bias shifted by a column (or indexed by the wrong one of
    m / n) is visible."""
    b = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3.0 + 0.5
    for i in (0, 3, 29, 77, 130, 300, 519, n - 1):
        if 0 <= i < n:
            b[i] = float(i)
    return b.to(dtype).to(DEV)


_PROBLEMS = {}


def problem(fx, M, Nn, K, lo, hi, seed=0):
    """(A, B, sa, sb, exact, bound) of a seeded random problem, computed once per module run."""
    key = (fx.name, M, Nn, K, lo, hi, seed)
    if key not in _PROBLEMS:
        rng = np.random.default_rng([seed, M, Nn, K, fx.seed])
        A, B = fx.rand_a(rng, M, K), fx.rand_b(rng, Nn, K)
        sa, sb = rand_scales(rng, M, K // 32, lo, hi), rand_scales(rng, Nn, K // 32, lo, hi)
        _PROBLEMS[key] = (A, B, sa, sb) + tuple(fx.ref(A, B, sa, sb))
    return _PROBLEMS[key]


def fused(f32, bias, sr, out_dtype):
    want = f32
    if bias is not None:
        want = want + bias.float()
    if sr is not None:
        want = want * sr
    return want.to(out_dtype)


# ---- 1. the fused epilogue --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO])
def test_epilogue_bias_scale_result_every_kernel(N_, fx, kernel, out_dtype):
    """(300, 520): interior and ragged tiles together (the direct epilogue on the ragged ones); (512, 768): only full tiles,
    the LDS-staged epilogue.  The kernels run the shared epilogue with per-tensor factors of 1 and no scale pointers: the plain
    fp32 result is held to mm_ref, and every (bias type, scale_result) form to ((f32 + bias) * sr).to(out_dtype) bit for bit."""
    lo, hi = fx.epi_scales
    for M, Nn, K in ((300, 520, 384), (512, 768, 384)):
        A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, lo, hi)
        a, b, sa_t, sb_t = t(A), t(B), t(sa), t(sb)
        f32 = run(N_, fx, a, b, sa_t, sb_t, kernel=kernel, split_k=1, out_dtype=torch.float32)
        check(f32, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel} {M}x{Nn}x{K} f32")
        sr = torch.tensor([0.75], device=DEV)
        for bias_dtype in OUT_DTYPES:
            bias = make_bias(Nn, 7, bias_dtype)
            for s in (None, sr):
                got = run(N_, fx, a, b, sa_t, sb_t, kernel=kernel, split_k=1, out_dtype=out_dtype, bias=bias, scale_result=s)
                assert got.dtype == out_dtype and got.shape == (M, Nn)
                assert torch.equal(got, fused(f32, bias, s, out_dtype)), (fx.name, kernel, (M, Nn, K), bias_dtype, s is not None)
        got = run(N_, fx, a, b, sa_t, sb_t, kernel=kernel, split_k=1, out_dtype=out_dtype, scale_result=sr)   # scale_result alone
        assert torch.equal(got, fused(f32, None, sr, out_dtype)), (fx.name, kernel, (M, Nn, K))


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("MNK", [(70, 1, 256), (130, 77, 384), (1, 77, 256)])
def test_epilogue_single_and_odd_columns(N_, fx, MNK, out_dtype):
    """N = 1 and N = 77: rows of C that are not 16-byte aligned, so no store of the epilogue is a vector store."""
    M, Nn, K = MNK
    lo, hi = fx.epi_scales
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, lo, hi)
    bias, sr = make_bias(Nn, 8), torch.tensor([1.5], device=DEV)
    for kernel in TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO]:
        f32 = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1)
        check(f32, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel} {MNK}")
        got = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1, out_dtype=out_dtype, bias=bias, scale_result=sr)
        assert got.shape == (M, Nn) and torch.equal(got, fused(f32, bias, sr, out_dtype)), (fx.name, kernel)


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC])
def test_transposed_epilogue(N_, fx, kernel, out_dtype):
    """C^T = W X^T with the bias along M (FP8MI_EPILOGUE_TRANSPOSED): bit for bit the transpose of the plain call, whose own
    fp32 product is held to mm_ref.  (256, 72): full and ragged tiles in both orientations.
    MXW4A8: A must be the e4m3 operand, so the operands cannot be swapped - the transposed epilogue runs on the same (A, B) with a
    bias of length M and is the plain product plus bias[:, None], bit for bit; a bias of length N is refused."""
    M, Nn, K = 72, 256, 768
    lo, hi = fx.epi_scales
    X, W, sx, sw, exact, bound = problem(fx, M, Nn, K, lo, hi, seed=2)
    bias = make_bias(Nn, 9)
    plain = run(N_, fx, X, W, sx, sw, kernel=kernel, split_k=1)
    check(plain, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel}")
    ref = run(N_, fx, X, W, sx, sw, bias=bias, kernel=kernel, split_k=1, out_dtype=out_dtype)
    assert torch.equal(ref, fused(plain, bias, None, out_dtype))
    if fx.kdiv_a != fx.kdiv_b:
        bias_m = make_bias(M, 9)
        tr = run(N_, fx, X, W, sx, sw, bias=bias_m, kernel=kernel, split_k=1, out_dtype=out_dtype, transposed_epilogue=True)
        assert tr.shape == (M, Nn) and torch.equal(tr, fused(plain, bias_m[:, None], None, out_dtype))
        with pytest.raises(AssertionError):                   # N != M: the bias along N is not a transposed bias
            run(N_, fx, X, W, sx, sw, bias=bias, kernel=kernel, split_k=1, transposed_epilogue=True)
        return
    tr = run(N_, fx, W, X, sw, sx, bias=bias, kernel=kernel, split_k=1, out_dtype=out_dtype, transposed_epilogue=True)
    assert tr.shape == (Nn, M) and torch.equal(tr.t(), ref)
    with pytest.raises(AssertionError):                       # the transposed bias runs along M (here: Nn rows of W)
        run(N_, fx, W, X, sw, sx, bias=make_bias(M, 9), kernel=kernel, split_k=1, transposed_epilogue=True)


def test_linear_with_bias_3d_input_and_f16_output(N_, fx):
    g = torch.Generator().manual_seed(77)
    K, Nn = 512, 200                             # (below the K from which AUTO may slice K: the f32 and f16 runs sum alike)
    w = torch.randn(Nn, K, generator=g) * 0.05
    x = torch.randn(2, 17, K, generator=g)
    bias = make_bias(Nn, 10, torch.float16)
    quant_a, quant_b, linear = getattr(N_, fx.quant_a_name), getattr(N_, fx.quant_b_name), getattr(N_, fx.linear_name)
    wq, ws = quant_b(w.to(DEV))
    y = linear(x.to(DEV), wq, ws, bias=bias, out_dtype=torch.float16)
    assert y.shape == (2, 17, Nn) and y.dtype == torch.float16
    xq, xs = quant_a(x.to(DEV).reshape(-1, K))
    chain = run(N_, fx, xq, wq, xs, ws, bias=bias, out_dtype=torch.float16)
    assert torch.equal(y.reshape(-1, Nn), chain)
    f32 = run(N_, fx, xq, wq, xs, ws)
    assert torch.equal(chain, fused(f32, bias, None, torch.float16))
    u8 = lambda q: q.view(torch.uint8).cpu().numpy()
    exact, bound = fx.ref(u8(xq), u8(wq), u8(xs), u8(ws))
    check(f32, exact, bound, MFMA_TOL, fx.name)


# ---- 2. scale layouts with poisoned padding ---------------------------------------------------------------------------
def _wide_cols(nb):
    return 64 if nb <= 64 else (nb + 3) // 4 * 4 + 60


def scale_layout(kind, s):
    """The (rows, nb) scales `s` in one of the layouts a caller passes; every byte that is not a scale is 0xFF (the E8M0 NaN).
    -> (device tensor to pass, expected row stride, True if the matrix-core kernels read it in place)."""
    rows, nb = s.shape
    if kind == "tight":
        return t(s), nb, nb % 4 == 0
    if kind == "padded":                                   # (a) torch's flat allocation: 128 ceil(rows / 128) x round_up(nb, 4)
        nbp = (nb + 3) // 4 * 4
        p = np.full(((rows + 127) // 128 * 128, nbp), 0xFF, np.uint8)
        p[:rows, :nb] = s
        return t(p).reshape(-1), nbp, True
    base, W = {"wide": (0, _wide_cols(nb)),                # (b) a 2-D view of a wider buffer
               "wide_base4": (4, _wide_cols(nb)),          # (c) ... at a 4-byte but not 16-byte aligned address
               "wide_base2": (2, _wide_cols(nb)),          # (d) ... at an address the 4-byte scale reads cannot take
               "wide_ld_odd": (0, _wide_cols(nb) + 2)}[kind]   # (d) ... or with such a row stride
    flat = np.full(base + (rows + 5) * W, 0xFF, np.uint8)
    flat[base:].reshape(rows + 5, W)[:rows, :nb] = s
    dev = t(flat)
    assert dev.data_ptr() % 16 == 0
    view = dev[base:].view(rows + 5, W)[:rows, :nb]
    return view, W, base % 4 == 0 and W % 4 == 0


@pytest.mark.parametrize("kind", ["padded", "wide", "wide_base4", "wide_base2", "wide_ld_odd"])
@pytest.mark.parametrize("K", [96, 160, 4128])
def test_scale_layouts_with_poisoned_padding(N_, fx, K, kind):
    """K / 32 = 3, 5, 129: every scale row ends inside a 4-byte K-step, and the last K-step's other bytes - like the rows past M
    and N - hold 0xFF.  Only the kernels' own guard (blocks past K and rows past the tensor read as 2^0) keeps 0 x NaN out of the
    sums: the results are finite and the bits of the run on tight scales, which is held to mm_ref."""
    M, Nn = 100, 200
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=3)
    la, ld_a, inplace_a = scale_layout(kind, sa)
    lb, ld_b, inplace_b = scale_layout(kind, sb)
    dev = la.device
    for lay, rows, ld, inplace in ((la, M, ld_a, inplace_a), (lb, Nn, ld_b, inplace_b)):
        got, got_ld = N_._mx_scales(lay, rows, K, dev, "scale")
        if inplace:                                       # (a) - (c) reach the kernel uncopied
            assert got.data_ptr() == lay.data_ptr() and got_ld == ld, kind
        else:                                             # (d) is copied once into a layout the 4-byte reads can take
            assert got.data_ptr() != lay.data_ptr() and got_ld % 4 == 0 and got.data_ptr() % 4 == 0, kind
    for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_GENERIC):
        tight = run(N_, fx, A, B, sa, sb, kernel=kernel)
        check(tight, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel} K={K}")
        got = run(N_, fx, A, B, la, lb, kernel=kernel)
        assert bool(torch.isfinite(got).all()), (fx.name, kernel, kind)
        assert torch.equal(got, tight), (fx.name, kernel, kind)


def test_c_abi_forced_tile_refuses_unaligned_scale_stride(N_, fx):
    """ld_sa = 5: a forced matrix-core tile is FP8MI_E_UNSUPPORTED (before any launch); AUTO takes the generic kernel."""
    lib = L.load()
    M, Nn, K = 100, 200, 160
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=3)
    a, b, sa_t, sb_t = t(A), t(B), t(sa), t(sb)
    lda, ldb = K // fx.kdiv_a, K // fx.kdiv_b       # bytes of a row of each operand
    st = torch.cuda.current_stream().cuda_stream

    def call(kernel, ld_sa):
        C = torch.full((M, Nn), -7.0, device=DEV)
        rc = fx.c_call(lib, a.data_ptr(), b.data_ptr(), C.data_ptr(), sa_t.data_ptr(), ld_sa, sb_t.data_ptr(), 5, M, Nn, K, lda, ldb, Nn,
                       kernel, st)
        torch.cuda.synchronize()
        return rc, C

    for kernel in (L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x64):
        rc, C = call(kernel, 5)
        assert rc == E_UNSUPPORTED and bool((C == -7.0).all()), kernel
    rc, auto = call(L.KERNEL_AUTO, 5)
    assert rc == 0
    rc, gen = call(L.KERNEL_GENERIC, 5)
    assert rc == 0 and torch.equal(auto, gen)
    check(auto, exact, bound, FP32_TOL, fx.name)


# ---- 3. operand layouts -----------------------------------------------------------------------------------------------
def _col_slice(x, left, right, fill):
    """x as the column slice [left : left + cols] of a wider device buffer filled with `fill`."""
    rows, cols = x.shape
    big = np.full((rows, left + cols + right), fill, x.dtype)
    big[:, left:left + cols] = x
    return t(big)[:, left:left + cols]


@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x64, L.KERNEL_GENERIC])
def test_row_strided_operands_read_in_place(N_, fx, kernel):
    """lda, ldb > K (bytes) at 16-byte aligned strides and bases: read in place by every kernel, the bits of the contiguous run.
    MXW4A8 (lda in A's bytes, K; ldb in B's, K / 2): also an A whose neighbours are the e4m3 NaN 0x7F, under NAN_PROPAGATE - K = 416 ends
    32 bytes into A's second sub-step of the last K-step, and only the mask of A's K tail keeps the bytes behind the row out of the sums."""
    M, Nn, K = 150, 136, 416
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=4)
    dense = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1)
    check(dense, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel}")
    a, b = _col_slice(A, 16, 32, 0x7E), _col_slice(B, 32, 48, 0x7E)     # (the neighbours are large finite values in every format)
    assert a.stride(0) == A.shape[1] + 48 and a.data_ptr() % 16 == 0 and b.stride(0) % 16 == 0
    assert torch.equal(run(N_, fx, a, b, sa, sb, kernel=kernel, split_k=1), dense)
    if fx is _MXW4A8:
        a_nan = _col_slice(A, 16, 32, 0x7F)
        got = run(N_, fx, a_nan, b, sa, sb, kernel=kernel, split_k=1, nan_mode=L.NAN_PROPAGATE)
        assert not bool(torch.isnan(got).any()) and torch.equal(got, dense), (fx.name, kernel)


def test_operand_views_the_matrix_core_path_cannot_read(N_, fx):
    """A stride or a base that is not a multiple of 16 bytes, and a K-major (transposed) view: AUTO still meets the bar - it
    computes what the forced generic kernel computes on contiguous copies."""
    M, Nn, K = 150, 136, 416
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=4)
    gen = run(N_, fx, A, B, sa, sb, kernel=L.KERNEL_GENERIC)
    check(gen, exact, bound, FP32_TOL, fx.name)
    ring = run(N_, fx, A, B, sa, sb)
    check(ring, exact, bound, MFMA_TOL, fx.name)
    for a, b in ((_col_slice(A, 8, 32, 0x7E), t(B)),                 # base and stride 8 mod 16
                 (t(A), _col_slice(B, 16, 7, 0x7E)),                 # stride 7 mod 16
                 (_col_slice(A, 3, 2, 0x7E), _col_slice(B, 1, 0, 0x7E))):
        got = run(N_, fx, a, b, sa, sb)
        check(got, exact, bound, MFMA_TOL, fx.name)
        assert torch.equal(got, gen)
        assert torch.equal(run(N_, fx, a, b, sa, sb, kernel=L.KERNEL_GENERIC), gen)
        with pytest.raises(L.Fp8miError):
            run(N_, fx, a, b, sa, sb, kernel=L.KERNEL_GEMM_64x64)
    a_kmajor = t(np.ascontiguousarray(A.T)).t()                       # (M, K bytes) with strides (1, M): copied by the op layer
    assert a_kmajor.stride() == (1, M)
    assert torch.equal(run(N_, fx, a_kmajor, B, sa, sb), ring)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x64, L.KERNEL_GENERIC])
def test_out_as_a_column_slice(N_, fx, kernel, out_dtype):
    """ldc > N through `out=`: with 16-byte aligned rows (vector and staged stores) and without; the bytes around the slice stay."""
    M, Nn, K = 200, 136, 256
    lo, hi = fx.epi_scales
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, lo, hi, seed=5)
    bias = make_bias(Nn, 11)
    f32 = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1)
    check(f32, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel}")
    want = fused(f32, bias, None, out_dtype)
    for left, right in ((8, 16), (3, 2)):
        big = torch.full((M + 2, left + Nn + right), -7.0, dtype=out_dtype, device=DEV)
        out = big[1:M + 1, left:left + Nn]
        ret = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1, bias=bias, out_dtype=out_dtype, out=out)
        assert ret.data_ptr() == out.data_ptr()
        assert torch.equal(out, want), (fx.name, kernel, left)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:M + 1, left:left + Nn] = False
        assert bool((big[mask] == -7.0).all()), (fx.name, kernel, left)


# ---- 4. exact scale-map checks ----------------------------------------------------------------------------------------
def selector_inputs(fx):
    """-> (A, B, sa, sb) of test_selector_pins_every_scale_to_its_row_and_block (host only: tests/test_mxw4a8_host.py reads them too)"""
    M, Nn, K = 128, 80, 512
    rng = np.random.default_rng(41 + fx.seed)
    ks = (37 * np.arange(M) + 5) % K
    A, B = fx.one_hot(M, K, ks), fx.rand_b(rng, Nn, K)
    return A, B, rand_scales(rng, M, K // 32, 90, 159), rand_scales(rng, Nn, K // 32, 90, 159)


def small_int_inputs(fx):
    """-> (A, B, sa, sb) of test_small_integers_with_mixed_scales_are_exact"""
    M, Nn, K = 100, 136, 992
    rng = np.random.default_rng(43 + fx.seed)
    A, B = fx.small_ints_a(rng, M, K), fx.small_ints_b(rng, Nn, K)
    return A, B, rand_scales(rng, M, K // 32, 126, 128), rand_scales(rng, Nn, K // 32, 126, 128)


def test_selector_pins_every_scale_to_its_row_and_block(N_, fx):
    """A holds a single 1.0 per row, at k_m = (37 m + 5) mod K; the scales of both operands are independent random bytes in
    [90, 159].  C[m, n] = b[n, k_m] 2^(sa[m, k_m / 32] - 127) 2^(sb[n, k_m / 32] - 127), one product and no rounding: every
    kernel must give mm_ref bit for bit.  Any wrong (row, block) <-> scale pairing of either operand changes an exponent."""
    A, B, sa, sb = selector_inputs(fx)
    exact, _ = fx.ref(A, B, sa, sb)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact) and np.count_nonzero(exact) > exact.size // 2
    for kernel in TILES + [L.KERNEL_GENERIC]:
        assert np.array_equal(f64(run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1)), exact), (fx.name, kernel)


def test_small_integers_with_mixed_scales_are_exact(N_, fx):
    """Integer data (0, +-1 .. +-4; an e2m1 operand also +-6) and scales 2^-1, 2^0, 2^1 drawn per (row, block): every product is a multiple
    of 2^-2 no larger than 2^8, every partial sum an fp32 value, and the products of an output lie within a 2^10 range - inside
    the 2^12 the matrix core was measured to sum exactly (profiles/mfma_numerics_r01.txt, profiles/mxfp8_scale_map.txt,
    profiles/mxfp4_operand_map.txt).  Every kernel must give mm_ref bit for bit; K = 992 ends in a partial K-step."""
    A, B, sa, sb = small_int_inputs(fx)
    exact, _ = fx.ref(A, B, sa, sb)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    for kernel in TILES + [L.KERNEL_GENERIC]:
        assert np.array_equal(f64(run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1)), exact), (fx.name, kernel)


@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GENERIC])
@pytest.mark.parametrize("fx", [_MXFP8, _MXW4A8], ids=lambda f: f.name)
def test_nan_scale_is_contained_in_its_row(N_, fx, kernel):
    """The formats with a nan_mode, NAN_ZERO: one 0xFF scale in row 5 makes the tile's accumulators NaN, which triggers the NaN-byte
    check and the scrubbed redo of the whole tile.  Row 5 is NaN; every other row keeps the bits it had before the scale was poisoned."""
    M, Nn, K = 64, 64, 256
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=6)
    before = run(N_, fx, A, B, sa, sb, kernel=kernel, split_k=1, nan_mode=L.NAN_ZERO)
    check(before, exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel}")
    bad = sa.copy()
    bad[5, 1] = 0xFF
    after = run(N_, fx, A, B, bad, sb, kernel=kernel, split_k=1, nan_mode=L.NAN_ZERO)
    assert bool(torch.isnan(after[5]).all())
    rows = [m for m in range(M) if m != 5]
    assert torch.equal(after[rows], before[rows])


# ---- 5. split-K edges -------------------------------------------------------------------------------------------------
SPLIT_CASES = [
    (100, 200, 2976, L.KERNEL_GEMM_128x64, 3),     # ragged tile, a K tail in the last slice
    (40, 130, 1056, L.KERNEL_GEMM_64x128, 16),     # more slices asked for than K has ring stages
    (9, 130, 2976, L.KERNEL_GEMM_32x64, 5),
    (70, 96, 4096, L.KERNEL_GEMM_32x32, 7),
    (130, 70, 4128, L.KERNEL_GEMM_64x64, 2),
    (16, 4096, 8192, L.KERNEL_AUTO, 0),
    (64, 512, 14336, L.KERNEL_AUTO, 0),
    (33, 512, 14336, L.KERNEL_AUTO, 0)]


@pytest.mark.parametrize("M,Nn,K,kernel,split", SPLIT_CASES)
def test_split_k_edges(N_, fx, M, Nn, K, kernel, split):
    """K cut into slices whose fp32 partials meet in the workspace; the epilogue runs once, behind the combine.  The plain fp32
    result is held to mm_ref; with a bias it is (f32 + bias) bit for bit, in bf16 within that format's rounding of the exact
    value (and, for a forced tile, exactly the cast); every run repeats bit for bit; the tile counters are left zero.
    A 0xFF scale (and a NaN byte, on each side that has them) inside a late slice reaches exactly its row / column through the
    combine, and every other output keeps its bits.  MXW4A8: the bytes 0x7F / 0xFF are NaN in A and finite pairs in B - B's column
    holds no NaN under either mode and keeps the bar."""
    rng = np.random.default_rng([M, Nn, K, split, fx.seed])
    A, B = fx.rand_a(rng, M, K), fx.rand_b(rng, Nn, K)
    sa, sb = rand_scales(rng, M, K // 32), rand_scales(rng, Nn, K // 32)
    exact, bound = fx.ref(A, B, sa, sb)
    a, b, sa_t, sb_t = t(A), t(B), t(sa), t(sb)
    kw = dict(kernel=kernel, split_k=split)
    what = f"{fx.name} {M}x{Nn}x{K} kernel {kernel} split {split}"
    f32 = run(N_, fx, a, b, sa_t, sb_t, **kw)
    check(f32, exact, bound, MFMA_TOL, what)
    assert torch.equal(run(N_, fx, a, b, sa_t, sb_t, **kw), f32), what
    bias = make_bias(Nn, 12)
    with_bias = run(N_, fx, a, b, sa_t, sb_t, bias=bias, **kw)
    assert torch.equal(with_bias, f32 + bias), what
    assert torch.equal(run(N_, fx, a, b, sa_t, sb_t, bias=bias, **kw), with_bias), what
    bf = run(N_, fx, a, b, sa_t, sb_t, bias=bias, out_dtype=torch.bfloat16, **kw)
    assert torch.equal(run(N_, fx, a, b, sa_t, sb_t, bias=bias, out_dtype=torch.bfloat16, **kw), bf), what
    want = exact + f64(bias)[None, :]
    assert np.all(np.abs(f64(bf) - want) <= MFMA_TOL * bound + 2.0 ** -8 * np.abs(want) + 1e-30), what
    if kernel != L.KERNEL_AUTO:                      # (AUTO may pick another tile or slice count for another output type)
        assert torch.equal(bf, with_bias.to(torch.bfloat16)), what

    # a NaN scale in a late slice: exactly its row is NaN, the others keep their bits
    row, blk = 3, (K // 32) * 7 // 10
    bad = sa.copy()
    bad[row, blk] = 0xFF
    got = run(N_, fx, a, b, t(bad), sb_t, **kw)
    others = [m for m in range(M) if m != row]
    assert bool(torch.isnan(got[row]).all()) and torch.equal(got[others], f32[others]), what

    if fx.a_nan:                                     # a NaN byte in a late slice of A, a byte 0xFF in a late slice of B
        col, ka, kb = 5, blk * 32 + 9, (K // 32) * 9 // 10 * 32 + 1
        A2, B2 = A.copy(), B.copy()
        A2[row, ka], B2[col, kb // fx.kdiv_b] = 0x7F, 0xFF
        keep = torch.ones(M, Nn, dtype=torch.bool, device=DEV)
        keep[row, :] = False
        keep[:, col] = False
        z = run(N_, fx, A2, B2, sa_t, sb_t, nan_mode=L.NAN_ZERO, **kw)
        assert torch.equal(z[keep], f32[keep]), what
        e_row, b_row = fx.ref(A2[row:row + 1], B2, sa[row:row + 1], sb, True)
        e_col, b_col = fx.ref(A2, B2[col:col + 1], sa, sb[col:col + 1], True)
        check(z[row:row + 1], e_row, b_row, MFMA_TOL, what + " NaN byte row")
        check(z[:, col:col + 1], e_col, b_col, MFMA_TOL, what + " NaN byte column")
        pr = run(N_, fx, A2, B2, sa_t, sb_t, nan_mode=L.NAN_PROPAGATE, **kw)
        nan = torch.isnan(pr)
        if fx.b_nan:
            assert bool(nan[row, :].all()) and bool(nan[:, col].all()) and int(nan.sum()) == M + Nn - 1, what
        else:                                        # the row alone; B's column holds its finite values
            assert bool(nan[row, :].all()) and int(nan.sum()) == Nn and not bool(torch.isnan(z).any()), what
            check(pr[others, col:col + 1], e_col[others], b_col[others], MFMA_TOL, what + " byte 0xFF in B, NAN_PROPAGATE")
        assert torch.equal(pr[keep], f32[keep]), what
    assert counters_zero(N_), what


# ---- 6. fuzz, tall and degenerate -------------------------------------------------------------------------------------
def test_random_shapes_auto_dispatch_fuzz(N_, fx):
    """Seeded sweep of 60 problems through AUTO: random shape, scales in [112, 142], bias, output type, split_k request and scale
    layout (tight, torch's padded allocation or a wide view, the padding 0xFF).  Every element is held to
    1e-3 (bound + |bias|) - the fp32 bar of tests/test_gpu_parity.py - plus one rounding to the 8- / 11-bit significand of a
    bf16 / f16 output (2^-24, f16's subnormal quantum, below its normal range; a value past f16's largest finite one is inf)."""
    rng = np.random.default_rng(2025 + fx.seed)
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    for it in range(60):
        M = int(pick([1, 2, 3, 7, 16, 31, 33, 48, 64, 65, 100, 128, 129, 200, 256, 300, 511, 640]))
        Nn = int(pick([1, 5, 16, 63, 64, 65, 127, 128, 130, 255, 256, 384, 500, 777, 1024]))
        K = int(pick([32, 64, 96, 128, 160, 256, 512, 1056, 2048, 4096, 4128, 6144]))
        if M * Nn * K > 6.0e8:   # keep the float64 reference quick
            K = 512
        A, B = fx.rand_a(rng, M, K), fx.rand_b(rng, Nn, K)
        sa, sb = rand_scales(rng, M, K // 32, 112, 142), rand_scales(rng, Nn, K // 32, 112, 142)
        bias = make_bias(Nn, 100 + it) if rng.random() < 0.5 else None
        od = pick(OUT_DTYPES)
        split = int(pick([0, 0, 0, 1, 2, 3, 5, 8]))
        kind = pick(["tight", "padded", "wide"])
        case = f"case {it}: {fx.name} M={M} N={Nn} K={K} bias={bias is not None} out={od} split_k={split} scales={kind}"
        got = f64(run(N_, fx, A, B, scale_layout(kind, sa)[0], scale_layout(kind, sb)[0], bias=bias, out_dtype=od, split_k=split))
        exact, bound = fx.ref(A, B, sa, sb)
        if bias is not None:
            exact = exact + f64(bias)[None, :]
            bound = bound + np.abs(f64(bias))[None, :]
        eps = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[od]
        lim = MFMA_TOL * bound + eps * np.abs(exact) + (2.0 ** -24 if od == torch.float16 else 0.0) + 1e-30
        if od == torch.float16:
            F16_MAX = 65504.0
            surely_inf = np.abs(exact) - lim > F16_MAX * (1 + 2.0 ** -11)
            surely_fin = np.abs(exact) + lim < F16_MAX
            assert np.all(np.isinf(got[surely_inf]) & (np.sign(got[surely_inf]) == np.sign(exact[surely_inf]))), case
            assert np.all(np.isfinite(got[surely_fin])), case
            assert not np.isnan(got).any(), case
            fin = np.isfinite(got)
            err = np.abs(got[fin] - np.clip(exact[fin], -F16_MAX, F16_MAX))
            assert np.all(err <= lim[fin]), f"{case}: max err / limit {np.max(err / lim[fin]):.3e}"
        else:
            err = np.abs(got - exact)
            assert np.all(err <= lim), f"{case}: max err / limit {np.max(err / lim):.3e}"
    assert counters_zero(N_)


@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GENERIC])
def test_tall_m_beyond_65535_rows(N_, fx, kernel):
    """M = 70003: more m-tiles than one 16-bit grid dimension holds, and a ragged last one."""
    M, Nn, K = 70003, 24, 32
    A, B, sa, sb, exact, bound = problem(fx, M, Nn, K, 117, 137, seed=7)
    check(run(N_, fx, A, B, sa, sb, kernel=kernel), exact, bound, tol_of(kernel), f"{fx.name} kernel {kernel}")


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
def test_degenerate_shapes(N_, fx, out_dtype):
    rng = np.random.default_rng(5)
    K = 64
    opa = lambda rows, k=K: fx.rand_a(rng, rows, k)
    opb = lambda rows, k=K: fx.rand_b(rng, rows, k)
    sc = lambda rows, k=K: rand_scales(rng, rows, k // 32)
    got = run(N_, fx, opa(0), opb(24), sc(0), sc(24), out_dtype=out_dtype)
    assert got.shape == (0, 24) and got.dtype == out_dtype
    got = run(N_, fx, opa(24), opb(0), sc(24), sc(0), out_dtype=out_dtype)
    assert got.shape == (24, 0) and got.dtype == out_dtype
    # K = 0: the empty sum, then the epilogue
    bias, sr = make_bias(24, 13), torch.tensor([0.75], device=DEV)
    got = run(N_, fx, opa(7, 0), opb(24, 0), sc(7, 0), sc(24, 0), bias=bias, scale_result=sr, out_dtype=out_dtype)
    assert got.shape == (7, 24) and torch.equal(got, (bias * sr).to(out_dtype).expand(7, 24))
    with pytest.raises(AssertionError):                                  # K % 32 != 0
        run(N_, fx, opa(4, 96)[:, :48 // fx.kdiv_a], opb(4, 96)[:, :48 // fx.kdiv_b], sc(4, 32), sc(4, 32), out_dtype=out_dtype)
    for kernel in (L.KERNEL_SKINNY, L.KERNEL_GEMM_256W):                # no block-scaled form
        with pytest.raises(L.Fp8miError):
            run(N_, fx, opa(8), opb(24), sc(8), sc(24), kernel=kernel, out_dtype=out_dtype)
