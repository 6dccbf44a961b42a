"""GPU (MI355X): the edges of the blockwise (1x128 / 128x128 fp32 scales) GEMM, quantizer and dequantizer that
tests/test_gpu_blockwise.py leaves out - every scale pinned to its (row block, K block), scale layouts inside NaN-poisoned
buffers (padded, offset, transposed, stride-0 broadcasts), K edges (a single partial block, an odd number of blocks on the
two-step tiles, more than 64 blocks on the generic kernel), split-K, the fused epilogue on every kernel, strided operands and
`out=`, a tall M, degenerate shapes, a seeded sweep of AUTO, the quantizer's partial blocks, strides and subnormal scales, the
_scaled_mm route, graph replay and a plain-C caller.

The reference is always the float64 `mm_ref` of tests/blockwise_ref.py.  Bars, as in tests/test_gpu_blockwise.py and
include/fp8mi.h: |gpu - exact| <= (1e-3 + nkb 2^-23) bound on the ring tiles, (128 2^-24 + nkb 2^-23) bound on the generic
kernel, bound = sum_b |fl32(sa sb)| sum_k |a b| (the second result of mm_ref).  Fused bf16 / f16 output, bias and scale_result
are pinned bit for bit to ((f32 + bias) * scale_result).to(out_dtype), where f32 is the same kernel's plain fp32 result and is
itself held to the bar.  Where two runs are compared bit for bit, one of them is also held to `mm_ref`.  The quantizer is
compared byte for byte (scales bit for bit) with `quantize_blockwise_ref`."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from blockwise_ref import mm_ref, quantize_blockwise_ref
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

MFMA_TOL = 1.0e-3
FP32_TOL = 128 * 2.0 ** -24
DEV = "cuda"
TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
         L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
PAIRS = [(1, 128), (1, 1), (128, 1), (128, 128)]
OUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
E_UNSUPPORTED = -4   # include/fp8mi.h
ONE = 0x38           # e4m3 1.0


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


# ---- helpers ----------------------------------------------------------------------------------------------------------
def t(x):
    return x.to(DEV) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rand_bytes(rng, shape):
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def nblk(n, block=128):
    return -(-n // block)


def rand_scales(rng, rows, K, block, lo=-20, hi=20):
    """random non-power-of-two fp32 scales spanning 2^lo .. 2^hi, random signs: (ceil(rows / block), ceil(K / 128))"""
    shape = (nblk(rows, block), nblk(K))
    v = np.exp2(rng.uniform(lo, hi, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32)


def run(N_, A, B, sa, sb, pair=(1, 128), **kw):
    out = N_.fp8_scaled_mm_blockwise(t(A), t(B), t(sa), t(sb), block_a=pair[0], block_b=pair[1], **kw)
    torch.cuda.synchronize()
    return out


def f64(x):
    return x.float().cpu().numpy().astype(np.float64)


def tol_of(kernel):
    return FP32_TOL if kernel == L.KERNEL_GENERIC else MFMA_TOL


def check(got, exact, bound, tol, K, what=""):
    err = np.abs(f64(got) - exact)
    bar = tol + nblk(K) * 2.0 ** -23
    assert np.all(err <= bar * bound + 1e-30), f"{what}: max err / bound {np.max(err / (bound + 1e-300)):.3e} (bar {bar:.3e})"


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


def fused(f32, bias, sr, out_dtype):
    want = f32
    if bias is not None:
        want = want + bias.float()
    if sr is not None:
        want = want * sr
    return want.to(out_dtype)


_PROBLEMS = {}


def problem(M, Nn, K, pair=(1, 128), lo=-20, hi=20, seed=0):
    """(A, B, sa, sb, exact, bound) of a seeded random problem, computed once per module run."""
    key = (M, Nn, K, pair, lo, hi, seed)
    if key not in _PROBLEMS:
        rng = np.random.default_rng([seed, M, Nn, K, pair[0], pair[1]])
        A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
        sa, sb = rand_scales(rng, M, K, pair[0], lo, hi), rand_scales(rng, Nn, K, pair[1], lo, hi)
        _PROBLEMS[key] = (A, B, sa, sb) + tuple(mm_ref(A, B, sa, sb, pair[0], pair[1]))
    return _PROBLEMS[key]


def chosen(M, Nn, K, out_dtype, pair, lda=None, ldb=None, has_ws=0, split=1):
    return L.load().fp8mi_choose_kernel_blockwise(M, Nn, K, K if lda is None else lda, K if ldb is None else ldb, Nn, CODE[out_dtype],
                                                  pair[0], pair[1], has_ws, split)


# ---- 1. every scale pinned to its row block and K block ---------------------------------------------------------------
def _one_hot(rows, K):
    """(rows, K) bytes with a single 1.0 per row, and the K block it lies in.  The positions walk through the first and the last
    valid k of every 128-block, the partial last block included."""
    cands = np.array([k for b in range(nblk(K)) for k in (128 * b, min(128 * b + 127, K - 1))])
    r = np.arange(rows)
    ks = cands[(7 * r + r // 128) % len(cands)]
    X = np.zeros((rows, K), np.uint8)
    X[r, ks] = ONE
    assert set(ks // 128) == set(range(nblk(K))) and K - 1 in ks and 0 in ks
    return X, ks // 128


def _distinct_scales(rows, K, block):
    """all different, exact in fp32 and in every product with 1: integers times 2^-4"""
    nrb, nkb = nblk(rows, block), nblk(K)
    return ((1 + np.arange(nrb * nkb).reshape(nrb, nkb)) * 2.0 ** -4).astype(np.float32)


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("MNK", [(300, 390, 400), (130, 520, 1168)])
def test_selector_pins_every_scale_to_its_row_block_and_k_block(N_, MNK, pair):
    """One operand holds a single 1.0 per row (at k_r), the other only 1.0; the one-hot operand's scales are all distinct and
    the other's are 1.  Then C[m, n] is exactly the scale of (row block of the one-hot row, k_r / 128): any wrong (row block,
    K block) <-> scale pairing shows as a wrong value.  Run once per operand."""
    M, Nn, K = MNK
    ba, bb = pair
    ones_a, ones_b = np.full((M, K), ONE, np.uint8), np.full((Nn, K), ONE, np.uint8)
    hot_a, blk_a = _one_hot(M, K)
    hot_b, blk_b = _one_hot(Nn, K)
    sa, sb = _distinct_scales(M, K, ba), _distinct_scales(Nn, K, bb)
    unit_a, unit_b = np.ones_like(sa), np.ones_like(sb)
    want_a = np.broadcast_to(sa[np.arange(M) // ba, blk_a].astype(np.float64)[:, None], (M, Nn))
    want_b = np.broadcast_to(sb[np.arange(Nn) // bb, blk_b].astype(np.float64)[None, :], (M, Nn))
    for kernel in TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO]:
        got = f64(run(N_, hot_a, ones_b, sa, unit_b, pair, kernel=kernel, split_k=1))
        assert np.array_equal(got, want_a), (kernel, "scale_a", np.argwhere(got != want_a)[:4].tolist())
        got = f64(run(N_, ones_a, hot_b, unit_a, sb, pair, kernel=kernel, split_k=1))
        assert np.array_equal(got, want_b), (kernel, "scale_b", np.argwhere(got != want_b)[:4].tolist())


# ---- 2. scale layouts inside poisoned buffers -------------------------------------------------------------------------
LAYOUTS = ["row_padded", "outer_padded", "outer_off1", "outer_off3", "t_of_padded", "bcast_rows", "bcast_k", "bcast_both"]


def scale_layout(kind, vals):
    """The (rows, ncols) scales `vals` as a view into a larger fp32 device buffer whose every other float is NaN.
    -> (view, the (rows, ncols) values the view holds: `vals`, or their broadcast first row / column / element)."""
    rows, nc = vals.shape
    nan = lambda *shape: np.full(shape, np.nan, np.float32)
    if kind == "row_padded":                                  # row stride > ncols
        buf = nan(rows + 2, nc + 3)
        buf[:rows, :nc] = vals
        return t(buf)[:rows, :nc], vals
    if kind in ("outer_padded", "outer_off1", "outer_off3"):  # torch's outer-dim-major, stride (1, rows + 3), at a storage offset
        off = {"outer_padded": 0, "outer_off1": 1, "outer_off3": 3}[kind]
        flat = nan(off + nc * (rows + 3))
        flat[off:].reshape(nc, rows + 3)[:, :rows] = vals.T
        view = t(flat)[off:].view(nc, rows + 3)[:, :rows].t()
        assert view.stride() == (1, rows + 3) and view.storage_offset() == off
        return view, vals
    if kind == "t_of_padded":                                 # .t() of a padded (K/128, rows) tensor
        buf = nan(nc + 2, rows + 5)
        buf[1:nc + 1, 2:rows + 2] = vals.T
        return t(buf)[1:nc + 1, 2:rows + 2].t(), vals
    if kind == "bcast_rows":                                  # stride 0 along the rows
        buf = nan(3, nc + 2)
        buf[1, 1:nc + 1] = vals[0]
        return t(buf)[1:2, 1:nc + 1].expand(rows, nc), np.broadcast_to(vals[0:1], vals.shape).copy()
    if kind == "bcast_k":                                     # stride 0 along K
        buf = nan(rows + 2, 3)
        buf[:rows, 1] = vals[:, 0]
        return t(buf)[:rows, 1:2].expand(rows, nc), np.broadcast_to(vals[:, 0:1], vals.shape).copy()
    assert kind == "bcast_both"                               # one float
    buf = nan(3)
    buf[1] = vals[0, 0]
    return t(buf)[1:2].view(1, 1).expand(rows, nc), np.full_like(vals, vals[0, 0])


_LAYOUT_REFS = {}


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("K", [96, 384, 1168])
def test_scale_layouts_inside_nan_poisoned_buffers(N_, K, kind):
    """Every float around the scales is NaN: a read one float off - a neighbour that would pass as a plausible scale in clean
    memory - poisons an output.  The results hold no NaN and are the bits of the run on a contiguous copy of the same values,
    which is held to mm_ref."""
    M, Nn = 192, 260
    for pair in ((1, 128), (1, 1), (128, 128)):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=3)
        la, va = scale_layout(kind, sa)
        lb, vb = scale_layout(kind, sb)
        if kind.startswith("bcast"):
            key = (kind, pair, K)
            if key not in _LAYOUT_REFS:
                _LAYOUT_REFS[key] = mm_ref(A, B, va, vb, pair[0], pair[1])
            exact, bound = _LAYOUT_REFS[key]
        assert tuple(la.shape) == sa.shape and tuple(lb.shape) == sb.shape
        for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_GENERIC):
            dense = run(N_, A, B, va, vb, pair, kernel=kernel, split_k=1)
            check(dense, exact, bound, tol_of(kernel), K, f"kernel {kernel} pair {pair} K={K}")
            got = run(N_, A, B, la, lb, pair, kernel=kernel, split_k=1)
            assert not bool(torch.isnan(got).any()), (kernel, pair, kind)
            assert torch.equal(got, dense), (kernel, pair, kind)


@pytest.mark.parametrize("K", [96, 1168])
def test_scale_buffer_that_ends_at_the_last_scale(N_, K):
    """The allocation ends exactly at the last float the kernels may read (NaN in front of the first): the same bits."""
    M, Nn = 192, 260
    for pair in ((1, 128), (1, 1), (128, 128)):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=3)

        def at_end(vals, outer):
            rows, nc = vals.shape
            flat = np.full(5 + rows * nc, np.nan, np.float32)
            flat[5:] = (vals.T if outer else vals).reshape(-1)
            dev = t(flat)
            view = dev[5:].view(nc, rows).t() if outer else dev[5:].view(rows, nc)
            last = view.data_ptr() + 4 * ((rows - 1) * view.stride(0) + (nc - 1) * view.stride(1) + 1)
            assert last == dev.data_ptr() + 4 * dev.numel()
            return view

        for kernel in (L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x32, L.KERNEL_GENERIC):
            dense = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1)
            check(dense, exact, bound, tol_of(kernel), K, f"kernel {kernel} pair {pair} K={K}")
            for outer in (False, True):
                got = run(N_, A, B, at_end(sa, outer), at_end(sb, outer), pair, kernel=kernel, split_k=1)
                assert torch.equal(got, dense), (kernel, pair, outer)


# ---- 3. K edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(1, 128), (128, 128)])
@pytest.mark.parametrize("K", [16, 48, 112, 128, 144, 384, 640, 1168])
def test_k_edges_every_kernel(N_, K, pair):
    """A single partial block (K < 128), one block and 16 more, and 3, 5 and 9 + 1/8 blocks: on the two-step tiles the last
    stage's second K-step then has no block and loads no scale."""
    M, Nn = 70, 100
    A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=5)
    for kernel in TILES + [L.KERNEL_GENERIC]:
        check(run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1), exact, bound, tol_of(kernel), K, f"kernel {kernel} K={K} pair {pair}")


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("K", [48, 1168])
def test_exact_small_integers_at_k_edges(N_, K, pair):
    """Integer data (0, +-1 .. +-4) and power-of-two scales: every kernel gives the oracle bit for bit (as
    test_exact_data_every_kernel_equals_the_oracle of tests/test_gpu_blockwise.py, at a single partial block and at 9 + 1/8)."""
    ba, bb = pair
    rng = np.random.default_rng(17 + ba + bb + K)
    M, Nn = 70, 100
    vals = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=np.uint8)
    A, B = vals[rng.integers(0, len(vals), (M, K))], vals[rng.integers(0, len(vals), (Nn, K))]
    sa = np.exp2(rng.integers(-2, 3, size=(nblk(M, ba), nblk(K)))).astype(np.float32)
    sb = np.exp2(rng.integers(-2, 3, size=(nblk(Nn, bb), nblk(K)))).astype(np.float32)
    exact, _ = mm_ref(A, B, sa, sb, ba, bb)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    for kernel in TILES + [L.KERNEL_GENERIC]:
        assert np.array_equal(f64(run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1)), exact), kernel


@pytest.mark.parametrize("pair", [(1, 128), (128, 128)])
@pytest.mark.parametrize("K", [100, 130])
def test_unaligned_k_goes_to_generic_and_a_forced_tile_refuses(N_, K, pair):
    M, Nn = 70, 100
    A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=6)
    assert chosen(M, Nn, K, torch.float32, pair) == L.KERNEL_GENERIC
    auto = run(N_, A, B, sa, sb, pair)
    check(auto, exact, bound, FP32_TOL, K, f"AUTO K={K}")
    assert torch.equal(auto, run(N_, A, B, sa, sb, pair, kernel=L.KERNEL_GENERIC))
    for kernel in TILES:                                       # the documented refusal: FP8MI_E_UNSUPPORTED before any launch
        out = torch.full((M, Nn), float("nan"), device=DEV)
        with pytest.raises(L.Fp8miError, match=f"code {E_UNSUPPORTED}"):
            run(N_, A, B, sa, sb, pair, kernel=kernel, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), kernel


@pytest.mark.parametrize("pair", [(1, 1), (128, 128)])
def test_generic_kernel_loops_over_more_than_64_blocks(N_, pair):
    """K = 8368 is 66 blocks: the generic kernel's lanes take a second round of blocks (two of them, the last partial)."""
    M, Nn, K = 9, 11, 8368
    A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=7)
    check(run(N_, A, B, sa, sb, pair, kernel=L.KERNEL_GENERIC), exact, bound, FP32_TOL, K, f"pair {pair}")


# ---- 4. split-K -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("MNK", [(64, 256, 2048 + 48), (33, 130, 1280)])
def test_split_k_every_pair(N_, MNK, pair):
    """K cut into 2, 3 and 5 slices of whole ring stages (256 k on these tiles: 9 and 5 stages), and into 16 - more than there
    are stages, which resolve_split (fp8mi_gemm_epi.h) documents as clamped to one stage per slice: the bar holds there too.
    Every run repeats bit for bit and leaves the workspace's tile counters zero."""
    M, Nn, K = MNK
    A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=8)
    a, b, sa_t, sb_t = t(A), t(B), t(sa), t(sb)
    for kernel in (L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64):
        for split in (2, 3, 5, 16):
            what = f"{MNK} pair {pair} kernel {kernel} split {split}"
            s1 = run(N_, a, b, sa_t, sb_t, pair, kernel=kernel, split_k=split)
            check(s1, exact, bound, MFMA_TOL, K, what)
            assert torch.equal(run(N_, a, b, sa_t, sb_t, pair, kernel=kernel, split_k=split), s1), what
            assert counters_zero(N_), what


@pytest.mark.parametrize("MNK", [(16, 512, 4096), (64, 1024, 2048 + 16)])
def test_auto_split_against_the_oracle(N_, MNK):
    """split_k = 0 with a workspace (K >= 1024): AUTO's own slice count, held to mm_ref; finite where the unsplit run is."""
    M, Nn, K = MNK
    for pair in PAIRS:
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=9)
        auto = run(N_, A, B, sa, sb, pair, split_k=0)
        check(auto, exact, bound, MFMA_TOL, K, f"{MNK} pair {pair} split_k=0")
        one = run(N_, A, B, sa, sb, pair, split_k=1)
        check(one, exact, bound, MFMA_TOL, K, f"{MNK} pair {pair} split_k=1")
        assert torch.equal(torch.isfinite(auto), torch.isfinite(one)) and bool(torch.isfinite(auto).all())
        assert torch.equal(run(N_, A, B, sa, sb, pair, split_k=0), auto)
    assert counters_zero(N_)


@pytest.mark.parametrize("nan_mode", [L.NAN_ZERO, L.NAN_PROPAGATE])
@pytest.mark.parametrize("pair", [(1, 128), (1, 1)])
def test_nan_bytes_and_a_nan_scale_under_split_k(N_, pair, nan_mode):
    """A NaN byte in a late slice of each operand and a NaN scale in a middle one, K in 3 slices: the isnan / isinf pattern is
    the generic kernel's, and every finite output meets the bar."""
    ba, bb = pair
    rng = np.random.default_rng(50 + bb)
    M, Nn, K = 64, 256, 2048 + 48
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    A[7, 1500] = 0x7F
    B[9, 2090] = 0xFF
    sa, sb = rand_scales(rng, M, K, ba, -4, 4), rand_scales(rng, Nn, K, bb, -4, 4)
    sb[1 if bb == 128 else 20, 12] = np.nan
    nan_cols = slice(128, 256) if bb == 128 else slice(20, 21)
    gen = f64(run(N_, A, B, sa, sb, pair, kernel=L.KERNEL_GENERIC, nan_mode=nan_mode))
    exact, bound = mm_ref(A, B, sa, sb, ba, bb, nan_mode == L.NAN_ZERO)
    assert np.isnan(gen[:, nan_cols]).all()
    if nan_mode == L.NAN_PROPAGATE:
        assert np.isnan(gen[7]).all() and np.isnan(gen[:, 9]).all()
    else:
        assert np.isfinite(gen[7, :20]).all() and np.isfinite(gen[:, 9]).all()
    fin = np.isfinite(gen)
    assert np.all(np.abs(gen[fin] - exact[fin]) <= (FP32_TOL + nblk(K) * 2.0 ** -23) * bound[fin] + 1e-30)
    for kernel in (L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128x64):
        got = f64(run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=3, nan_mode=nan_mode))
        assert np.array_equal(np.isnan(got), np.isnan(gen)), kernel
        assert np.array_equal(np.isinf(got), np.isinf(gen)), kernel
        assert np.all(np.abs(got[fin] - exact[fin]) <= (MFMA_TOL + nblk(K) * 2.0 ** -23) * bound[fin] + 1e-30), kernel
    assert counters_zero(N_)


# ---- 5. the fused epilogue, `out=` and operand views ------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("kernel", TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO])
def test_epilogue_bias_scale_result_every_kernel(N_, kernel, out_dtype):
    """(130, 77): rows of C that are not 16-byte aligned, so no store is a vector store; (96, 160): vector stores.  Scales of
    2^-8 .. 2^-4 per side keep the sums inside f16's range."""
    for (M, Nn, K), pair in (((130, 77, 384), (1, 128)), ((130, 77, 384), (128, 1)), ((96, 160, 512), (1, 128)), ((96, 160, 512), (128, 128))):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, -8, -4, seed=10)
        a, b, sa_t, sb_t = t(A), t(B), t(sa), t(sb)
        f32 = run(N_, a, b, sa_t, sb_t, pair, kernel=kernel, split_k=1)
        check(f32, exact, bound, tol_of(kernel), K, f"kernel {kernel} {M}x{Nn}x{K} pair {pair}")
        sr = torch.tensor([0.75], device=DEV)
        for bias_dtype in OUT_DTYPES:
            bias = make_bias(Nn, 7, bias_dtype)
            for s in (None, sr):
                got = run(N_, a, b, sa_t, sb_t, pair, kernel=kernel, split_k=1, out_dtype=out_dtype, bias=bias, scale_result=s)
                assert got.dtype == out_dtype and got.shape == (M, Nn)
                assert torch.equal(got, fused(f32, bias, s, out_dtype)), (kernel, (M, Nn, K), pair, bias_dtype, s is not None)
        got = run(N_, a, b, sa_t, sb_t, pair, kernel=kernel, split_k=1, out_dtype=out_dtype, scale_result=sr)
        assert torch.equal(got, fused(f32, None, sr, out_dtype)), (kernel, (M, Nn, K), pair)


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("MNK", [(70, 1, 256), (1, 77, 256), (1, 1, 256)])
def test_epilogue_single_row_and_single_column(N_, MNK, out_dtype):
    M, Nn, K = MNK
    bias, sr = make_bias(Nn, 8), torch.tensor([1.5], device=DEV)
    for pair in ((1, 128), (128, 128)):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, -8, -4, seed=11)
        for kernel in TILES + [L.KERNEL_GENERIC, L.KERNEL_AUTO]:
            f32 = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1)
            check(f32, exact, bound, tol_of(kernel), K, f"kernel {kernel} {MNK} pair {pair}")
            got = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1, out_dtype=out_dtype, bias=bias, scale_result=sr)
            assert got.shape == (M, Nn) and torch.equal(got, fused(f32, bias, sr, out_dtype)), (kernel, pair)


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_128, L.KERNEL_GENERIC])
def test_transposed_epilogue_every_out_dtype(N_, kernel, out_dtype):
    """C^T = W X^T with the bias along M and the block sizes swapped: bit for bit the transpose of the plain call."""
    M, Nn, K = 72, 256, 768
    X, W, sx, sw, exact, bound = problem(M, Nn, K, (1, 128), -8, -4, seed=12)
    bias = make_bias(Nn, 9)
    plain = run(N_, X, W, sx, sw, (1, 128), kernel=kernel, split_k=1)
    check(plain, exact, bound, tol_of(kernel), K, f"kernel {kernel}")
    ref = run(N_, X, W, sx, sw, (1, 128), bias=bias, kernel=kernel, split_k=1, out_dtype=out_dtype)
    assert torch.equal(ref, fused(plain, bias, None, out_dtype))
    tr = run(N_, W, X, sw, sx, (128, 1), bias=bias, kernel=kernel, split_k=1, out_dtype=out_dtype, transposed_epilogue=True)
    assert tr.shape == (Nn, M) and tr.dtype == out_dtype and torch.equal(tr.t(), ref)
    with pytest.raises(AssertionError):                       # the transposed bias runs along M (here: the Nn rows of W)
        run(N_, W, X, sw, sx, (128, 1), bias=make_bias(M, 9), kernel=kernel, split_k=1, transposed_epilogue=True)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x64, L.KERNEL_GENERIC])
def test_out_as_a_column_slice(N_, kernel, out_dtype):
    """ldc > N through `out=`: rows that are 16-byte aligned (vector and staged stores) and rows that are not; everything
    around the slice stays NaN."""
    M, Nn, K = 200, 136, 256
    esz = torch.empty(0, dtype=out_dtype).element_size()
    for pair in ((1, 128), (128, 128)):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, -8, -4, seed=13)
        bias = make_bias(Nn, 11)
        f32 = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1)
        check(f32, exact, bound, tol_of(kernel), K, f"kernel {kernel} pair {pair}")
        want = fused(f32, bias, None, out_dtype)
        for left, right, aligned in ((8, 16, True), (3, 2, False)):
            ldc = left + Nn + right
            assert (ldc * esz % 16 == 0) == aligned
            big = torch.full((M + 2, ldc), float("nan"), dtype=out_dtype, device=DEV)
            out = big[1:M + 1, left:left + Nn]
            ret = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1, bias=bias, out_dtype=out_dtype, out=out)
            assert ret.data_ptr() == out.data_ptr()
            assert torch.equal(out, want), (kernel, pair, left)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[1:M + 1, left:left + Nn] = False
            assert bool(torch.isnan(big[mask]).all()), (kernel, pair, left)


def _col_slice(x, left, right, fill):
    """x as the column slice [left : left + cols] of a wider device buffer filled with `fill`."""
    rows, cols = x.shape
    big = np.full((rows, left + cols + right), fill, x.dtype)
    big[:, left:left + cols] = x
    return t(big)[:, left:left + cols]


@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_32x64, L.KERNEL_GENERIC])
def test_row_strided_operands_read_in_place(N_, kernel):
    """lda, ldb > K at 16-byte aligned strides and bases: read in place (the op passes the view's own pointer and stride; AUTO
    still chooses a ring tile).  The padding is the NaN byte 0x7F, and under NAN_PROPAGATE a read of it would poison an output."""
    M, Nn, K = 150, 136, 416
    for pair in ((1, 128), (128, 128)):
        A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=14)
        a, b = _col_slice(A, 16, 32, 0x7F), _col_slice(B, 32, 48, 0x7F)
        assert a.stride(0) == K + 48 and a.data_ptr() % 16 == 0 and b.stride(0) % 16 == 0 and b.data_ptr() % 16 == 0
        assert chosen(M, Nn, K, torch.float32, pair, a.stride(0), b.stride(0)) in TILES
        for nan_mode in (L.NAN_ZERO, L.NAN_PROPAGATE):
            dense = run(N_, A, B, sa, sb, pair, kernel=kernel, split_k=1, nan_mode=nan_mode)
            check(dense, exact, bound, tol_of(kernel), K, f"kernel {kernel} pair {pair}")
            got = run(N_, a, b, sa, sb, pair, kernel=kernel, split_k=1, nan_mode=nan_mode)
            assert torch.equal(got, dense), (kernel, pair, nan_mode)


def test_operand_views_the_ring_path_cannot_read(N_):
    """A row stride or a base that is not a multiple of 16 bytes: AUTO runs the generic kernel and meets its bar (the bits of
    the forced generic kernel on contiguous copies); a forced tile refuses."""
    M, Nn, K = 150, 136, 416
    pair = (1, 128)
    A, B, sa, sb, exact, bound = problem(M, Nn, K, pair, seed=14)
    gen = run(N_, A, B, sa, sb, pair, kernel=L.KERNEL_GENERIC)
    check(gen, exact, bound, FP32_TOL, K, "generic")
    for a, b in ((_col_slice(A, 8, 32, 0x7F), t(B)),                 # base and stride 8 mod 16
                 (t(A), _col_slice(B, 16, 7, 0x7F)),                 # stride 7 mod 16
                 (_col_slice(A, 1, 15, 0x7F), t(B)),                 # a base offset of one byte, the stride a multiple of 16
                 (_col_slice(A, 3, 2, 0x7F), _col_slice(B, 1, 0, 0x7F))):
        assert chosen(M, Nn, K, torch.float32, pair, a.stride(0), b.stride(0)) == L.KERNEL_GENERIC or a.data_ptr() % 16 or b.data_ptr() % 16
        got = run(N_, a, b, sa, sb, pair, nan_mode=L.NAN_PROPAGATE)
        check(got, exact, bound, FP32_TOL, K, "AUTO on a view")
        assert torch.equal(got, gen)
        with pytest.raises(L.Fp8miError, match=f"code {E_UNSUPPORTED}"):
            run(N_, a, b, sa, sb, pair, kernel=L.KERNEL_GEMM_64x64)


# ---- 6. shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [L.KERNEL_AUTO, L.KERNEL_GENERIC])
def test_tall_m_beyond_65535_rows(N_, kernel):
    """M = 65536 + 130 with one distinct scale per row: more rows than one 16-bit grid dimension holds - a row index that wrapped
    would pick another row's bytes and scale.  Then the transposed problem (N tall, blocks (128, 1))."""
    M, Nn, K = 65536 + 130, 8, 128
    rng = np.random.default_rng(60)
    A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
    sa = ((1 + np.arange(M)) * 2.0 ** -12).astype(np.float32).reshape(M, 1)
    sb = rand_scales(rng, Nn, K, 128, -4, 4)
    rows = np.unique(np.concatenate([[0, 1, 127, 128, 65534, 65535, 65536, 65537, M - 1], rng.integers(0, M, 64)]))
    exact, bound = mm_ref(A[rows], B, sa[rows], sb, 1, 128)
    got = run(N_, A, B, sa, sb, (1, 128), kernel=kernel)
    assert got.shape == (M, Nn)
    check(got[t(rows)], exact, bound, tol_of(kernel), K, f"kernel {kernel}")
    got = run(N_, B, A, sb, sa, (128, 1), kernel=kernel)
    assert got.shape == (Nn, M)
    check(got[:, t(rows)], exact.T, bound.T, tol_of(kernel), K, f"kernel {kernel} transposed")


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
def test_degenerate_shapes(N_, out_dtype):
    rng = np.random.default_rng(5)
    for pair in PAIRS:
        ba, bb = pair
        K = 256
        got = run(N_, rand_bytes(rng, (0, K)), rand_bytes(rng, (24, K)), rand_scales(rng, 0, K, ba), rand_scales(rng, 24, K, bb), pair,
                  out_dtype=out_dtype)
        assert got.shape == (0, 24) and got.dtype == out_dtype
        got = run(N_, rand_bytes(rng, (24, K)), rand_bytes(rng, (0, K)), rand_scales(rng, 24, K, ba), rand_scales(rng, 0, K, bb), pair,
                  out_dtype=out_dtype)
        assert got.shape == (24, 0) and got.dtype == out_dtype
        # K = 0: the empty sum, then the epilogue; the scale tensors are (rows, 0)
        bias, sr = make_bias(24, 13), torch.tensor([0.75], device=DEV)
        sa0, sb0 = np.zeros((nblk(7, ba), 0), np.float32), np.zeros((nblk(24, bb), 0), np.float32)
        for kernel in (L.KERNEL_AUTO, L.KERNEL_GENERIC):
            got = run(N_, np.zeros((7, 0), np.uint8), np.zeros((24, 0), np.uint8), sa0, sb0, pair, bias=bias, scale_result=sr,
                      out_dtype=out_dtype, kernel=kernel)
            assert got.shape == (7, 24) and torch.equal(got, (bias * sr).to(out_dtype).expand(7, 24))
        got = run(N_, np.zeros((7, 0), np.uint8), np.zeros((24, 0), np.uint8), sa0, sb0, pair, out_dtype=out_dtype)
        assert torch.equal(got, torch.zeros(7, 24, dtype=out_dtype, device=DEV))


FUZZ_SEED = 2026


def _fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    cases = []
    for it in range(40):
        M, Nn, K = int(rng.integers(1, 301)), int(rng.integers(1, 401)), 16 * int(rng.integers(1, 129))
        if it >= 32:      # a grid that fills the chip: the only shapes at which AUTO leaves GEMM_32x32 / GEMM_128
            M, K = int(rng.integers(600, 2049)), 16 * int(rng.integers(1, 17))
        pair = PAIRS[int(rng.integers(4))]
        od = OUT_DTYPES[int(rng.integers(3))]
        cases.append((it, M, Nn, K, pair, od, bool(rng.random() < 0.5), int(rng.integers(1 << 30))))
    return cases


def test_random_shapes_auto_dispatch_fuzz(N_):
    """Seeded sweep of 40 problems through AUTO (split_k = 0, the default): M <= 300, N <= 400, K = 16 j <= 2048, a random block
    pair, output type and bias.  Every element is held to the ring bar on (bound + |bias|) plus one rounding to the 8- / 11-bit
    significand of a bf16 / f16 output (2^-24, f16's subnormal quantum, below its normal range) - the form of the fuzz test of
    tests/test_gpu_mx_edges.py.  With M <= 300 and N <= 400 the cost model only ever chooses GEMM_32x32 and (K <= 128) GEMM_128,
    so the last eight cases draw M from 600 .. 2048 with K <= 256; the seed was picked on the host so that AUTO exercises at
    least three distinct ring tiles."""
    kernels = set()
    for it, M, Nn, K, pair, od, with_bias, seed in _fuzz_cases():
        rng = np.random.default_rng(seed)
        A, B = rand_bytes(rng, (M, K)), rand_bytes(rng, (Nn, K))
        sa, sb = rand_scales(rng, M, K, pair[0], -8, -4), rand_scales(rng, Nn, K, pair[1], -8, -4)
        bias = make_bias(Nn, 100 + it) if with_bias else None
        case = f"case {it}: M={M} N={Nn} K={K} pair={pair} bias={with_bias} out={od}"
        kernels.add(chosen(M, Nn, K, od, pair, has_ws=1 if K >= 1024 else 0, split=0 if K >= 1024 else 1))
        got = f64(run(N_, A, B, sa, sb, pair, bias=bias, out_dtype=od))
        exact, bound = mm_ref(A, B, sa, sb, pair[0], pair[1])
        if bias is not None:
            exact = exact + f64(bias)[None, :]
            bound = bound + np.abs(f64(bias))[None, :]
        eps = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[od]
        lim = (MFMA_TOL + nblk(K) * 2.0 ** -23) * bound + eps * np.abs(exact) + (2.0 ** -24 if od == torch.float16 else 0.0) + 1e-30
        assert od != torch.float16 or np.all(np.abs(exact) + lim < 65504.0), case      # (inside f16's range: no overflow to weigh)
        err = np.abs(got - exact)
        assert np.all(err <= lim), f"{case}: max err / limit {np.max(err / lim):.3e}"
    assert len(kernels & set(TILES)) >= 3 and kernels <= set(TILES), kernels
    assert counters_zero(N_)


# ---- 7. quantizer / dequantizer ---------------------------------------------------------------------------------------
QSHAPES = [(1, 1), (1, 127), (5, 129), (3, 257), (129, 130), (257, 384), (130, 1000)]


def assert_quantizes_like_the_reference(N_, x, block_rows, what=""):
    q, s = N_.fp8_quantize_blockwise(x.to(DEV), block_rows)
    torch.cuda.synchronize()
    rq, rs = quantize_blockwise_ref(x, block_rows)
    assert q.shape == rq.shape and s.shape == rs.shape, what
    bad = (q.cpu() != rq).nonzero()
    assert bad.shape[0] == 0, (what, bad.shape[0], [(int(r), int(c), hex(int(q[r, c])), hex(int(rq[r, c]))) for r, c in bad[:6]])
    assert torch.equal(s.cpu().view(torch.int32), rs.view(torch.int32)), (what, s.cpu().reshape(-1)[:6], rs.reshape(-1)[:6])
    return q, s


@pytest.mark.parametrize("block_rows", [1, 128])
@pytest.mark.parametrize("dtype", OUT_DTYPES)
def test_quantizer_partial_blocks_and_odd_sizes(N_, dtype, block_rows):
    """Block counts that are not multiples of 4 (the surplus waves of the last workgroup return early), odd column counts (a lane
    that owns one column), single partial blocks, one row; empty inputs."""
    g = torch.Generator().manual_seed(block_rows + 5)
    for rows, cols in QSHAPES:
        x = (torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, 1), generator=g).float())).to(dtype)
        assert_quantizes_like_the_reference(N_, x, block_rows, f"{rows}x{cols}")
    for rows, cols in ((0, 256), (7, 0)):
        q, s = N_.fp8_quantize_blockwise(torch.zeros(rows, cols, dtype=dtype, device=DEV), block_rows)
        assert q.shape == (rows, cols) and s.shape == (nblk(rows, block_rows), nblk(cols))
        d = N_.fp8_dequantize_blockwise(q, s, block_rows, dtype)
        assert d.shape == (rows, cols) and d.dtype == dtype


@pytest.mark.parametrize("block_rows", [1, 128])
def test_quantizer_subnormal_and_smallest_normal_scales(N_, block_rows):
    """f32 blocks whose amax is 2^-126 448 (the scale is the smallest normal), 2^-120 and 2^-140 (subnormal scales), mixed with
    smaller elements; bf16 / f16 rows whose amax is a quarter of the smallest normal, and rows holding the largest finite value.
    The kernel's IEEE divisions and fp32 denormals must give the CPU's bytes and scale bits."""
    g = torch.Generator().manual_seed(9)
    frac = torch.rand(6, 384, generator=g) * 2 - 1
    x = frac.clone()
    for r, amax in enumerate((2.0 ** -126 * 448, 2.0 ** -120, 2.0 ** -140, 2.0 ** -126 * 448, 2.0 ** -120, 2.0 ** -140)):
        x[r] = frac[r] * amax
        for cb in range(3):
            x[r, 128 * cb + 17 * (r + 1)] = amax if cb != 1 else -amax
    x[3:5, 128:256] *= 2.0 ** -5              # (a second magnitude in the same 128-row block)
    _, s = assert_quantizes_like_the_reference(N_, x, block_rows, "f32")
    assert bool((s > 0).all()) and bool((s.cpu() < 2.0 ** -118).all())
    for dtype in (torch.bfloat16, torch.float16):
        fi = torch.finfo(dtype)
        y = (frac[:4, :300] * 0.5).to(dtype)
        y[0] = (frac[0, :300] * (fi.smallest_normal / 4)).to(dtype)
        y[0, 5] = fi.smallest_normal / 4
        y[1, 130] = fi.max
        y[2, 299] = -fi.max
        y[3] = (frac[3, :300] * fi.smallest_normal).to(dtype)
        assert_quantizes_like_the_reference(N_, y, block_rows, str(dtype))


@pytest.mark.parametrize("block_rows", [1, 128])
@pytest.mark.parametrize("amax", [1e-44, 1.4e-45])
def test_quantizer_amax_whose_scale_underflows(N_, amax, block_rows):
    """f32 blocks whose amax / 448 underflows to 0 (amax below about 448 2^-150): the scale is 1, as for an all-zero block, and
    finite input gives no NaN byte.  (With s = 1 only when amax == 0 the scale was 0, the nonzero elements +-448 and the zeros
    0 / 0 = NaN = 0x7F.)"""
    x = torch.zeros(130, 300)
    x[0, 3], x[5, 129], x[129, 299], x[128, 0] = amax, -amax, amax, amax
    assert bool((x != 0).any()) and (x.abs().max() / 448.0).item() == 0.0     # (the fp32 quotient)
    q, s = assert_quantizes_like_the_reference(N_, x, block_rows)
    assert not bool(((q & 0x7F) == 0x7F).any())
    assert bool(torch.isfinite(s).all()) and bool((s != 0).all())
    for out_dtype in OUT_DTYPES:
        assert not bool(torch.isnan(N_.fp8_dequantize_blockwise(q, s, block_rows, out_dtype)).any())


@pytest.mark.parametrize("block_rows", [1, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantizer_leading_dimensions_and_strided_scales_through_the_c_abi(N_, dtype, block_rows):
    """ld_in > cols, ld_out > cols with the 0xAA padding left alone, and the scales written outer-dim-major (torch's layout:
    s_stride_row = 1, s_stride_k = row blocks) or at stride (col blocks + 3, 1) into a NaN-filled buffer whose other floats
    stay NaN.  Both layouts then feed fp8mi_dequant_blockwise and the GEMM in place: the bits of the contiguous run."""
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    rows, cols = 130, 400
    nrb, ncb = nblk(rows, block_rows), nblk(cols)
    g = torch.Generator().manual_seed(31 + block_rows)
    wide = (torch.randn(rows, cols + 9, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, 1), generator=g).float())).to(dtype)
    x = wide[:, :cols].contiguous()
    rq, rs = quantize_blockwise_ref(x, block_rows)
    xd = wide.to(DEV)
    rng = np.random.default_rng(32)
    W, sw = rand_bytes(rng, (96, cols)), rand_scales(rng, 96, cols, 128, -4, 4)
    for ld_out in (cols + 5, cols + 16):
        for layout in ("outer", "padded"):
            out = torch.full((rows, ld_out), 0xAA, dtype=torch.uint8, device=DEV)
            if layout == "outer":
                buf = torch.full((ncb, nrb), float("nan"), device=DEV)
                view, s_sr, s_sk = buf.t(), 1, nrb
            else:
                buf = torch.full((nrb + 1, ncb + 3), float("nan"), device=DEV)
                view, s_sr, s_sk = buf[:nrb, :ncb], ncb + 3, 1
            rc = lib.fp8mi_quantize_blockwise(xd.data_ptr(), CODE[dtype], rows, cols, cols + 9, block_rows, out.data_ptr(), ld_out,
                                              buf.data_ptr(), s_sr, s_sk, st)
            assert rc == 0, lib.fp8mi_last_error()
            torch.cuda.synchronize()
            what = (ld_out, layout)
            assert torch.equal(out[:, :cols].cpu(), rq) and bool(out[:, cols:].eq(0xAA).all()), what
            assert torch.equal(view.cpu().contiguous().view(torch.int32), rs.view(torch.int32)), what
            assert int(torch.isnan(buf).sum()) == buf.numel() - nrb * ncb, what
            q_view = out[:, :cols]
            for od in OUT_DTYPES:                         # dequantize from the strided bytes and scales
                dense = N_.fp8_dequantize_blockwise(t(rq), t(rs), block_rows, od)
                got = torch.empty(rows, cols, dtype=od, device=DEV)
                rc = lib.fp8mi_dequant_blockwise(out.data_ptr(), rows, cols, ld_out, block_rows, buf.data_ptr(), s_sr, s_sk, got.data_ptr(),
                                                 CODE[od], st)
                assert rc == 0, lib.fp8mi_last_error()
                torch.cuda.synchronize()
                assert torch.equal(got, dense) and torch.equal(N_.fp8_dequantize_blockwise(q_view, view, block_rows, od), dense), what
            # the GEMM on the strided bytes and scales; a row stride of cols + 5 bytes sends AUTO to the generic kernel
            pair = (block_rows, 128)
            exact, bound = mm_ref(rq.numpy(), W, rs.numpy(), sw, block_rows, 128)
            for kernel in [L.KERNEL_GENERIC] + ([L.KERNEL_AUTO, L.KERNEL_GEMM_64x64] if ld_out % 16 == 0 else []):
                dense = run(N_, rq, W, rs, sw, pair, kernel=kernel)
                check(dense, exact, bound, tol_of(kernel), cols, str(what))
                assert torch.equal(run(N_, q_view, W, view, sw, pair, kernel=kernel), dense), (what, kernel)
            if ld_out % 16:
                assert torch.equal(run(N_, q_view, W, view, sw, pair), dense), what


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
def test_dequantizer_every_byte_and_special_scales(N_, out_dtype):
    """All 256 bytes times 0, inf, NaN, a subnormal, negative and ordinary scales: the fp32 product rounded once, then to
    out_dtype, as torch's CPU ops give it - the NaN pattern equal, everything else bit for bit."""
    specials = np.array([0.0, np.inf, np.nan, 1e-40, -0.37, 3.0e4, -np.inf, 2.0 ** -126, 1.7e-3, 448.0], np.float32)
    n = len(specials)
    q1 = np.tile(np.arange(256, dtype=np.uint8), (n, 1))                       # block_rows = 1: one scale pair per row
    s1 = np.stack([specials, np.roll(specials, 3)], axis=1)
    q128 = ((np.arange(130)[:, None] * 7 + np.arange(256)[None, :]) % 256).astype(np.uint8)   # block_rows = 128, rows = 130
    for q, block_rows, scales in [(q1, 1, s1)] + [(q128, 128, np.roll(specials, k)[:4].reshape(2, 2)) for k in range(0, n, 2)]:
        full = torch.from_numpy(scales).repeat_interleave(block_rows, 0).repeat_interleave(128, 1)[:q.shape[0], :256]
        want = (torch.from_numpy(q).view(torch.float8_e4m3fn).float() * full).to(out_dtype)
        got = N_.fp8_dequantize_blockwise(t(q), t(scales), block_rows, out_dtype).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), block_rows
        ok = ~torch.isnan(want)
        assert torch.equal(got[ok], want[ok]), (block_rows, (got[ok] != want[ok]).nonzero()[:6])


def test_linear_blockwise_end_to_end(N_):
    """bf16 x (70, 400) and w (200, 400) with per-row magnitudes 2^+-6, through fp8_linear_blockwise on a 3-D input with a
    bias: bit for bit fp8_scaled_mm_blockwise on the reference quantizer's bytes and scales, whose fp32 product meets the bar.
    Against float64 x @ w.T the relative Frobenius error measured on MI355X is 3.690e-02 (blockwise) next to 4.040e-02 for
    fp8_linear (one scale per tensor) on the same data; the test asserts the order only (both runs are deterministic)."""
    g = torch.Generator().manual_seed(70)
    K, Nn = 400, 200
    x = (torch.randn(70, K, generator=g) * torch.exp2(torch.randint(-6, 7, (70, 1), generator=g).float())).to(torch.bfloat16)
    w = (torch.randn(Nn, K, generator=g) * torch.exp2(torch.randint(-6, 7, (Nn, 1), generator=g).float())).to(torch.bfloat16)
    xq, xs = quantize_blockwise_ref(x, 1)
    wq, ws = quantize_blockwise_ref(w, 128)
    gq, gs = N_.fp8_quantize_blockwise(w.to(DEV), 128)
    assert torch.equal(gq.cpu(), wq) and torch.equal(gs.cpu().view(torch.int32), ws.view(torch.int32))
    f32 = run(N_, xq, wq, xs, ws)
    exact, bound = mm_ref(xq.numpy(), wq.numpy(), xs.numpy(), ws.numpy(), 1, 128)
    check(f32, exact, bound, MFMA_TOL, K, "quantized product")
    bias = make_bias(Nn, 14, torch.bfloat16)
    for od in OUT_DTYPES:
        y = N_.fp8_linear_blockwise(x.to(DEV).reshape(2, 35, K), gq, gs, bias=bias, out_dtype=od)
        assert y.shape == (2, 35, Nn) and y.dtype == od
        chain = run(N_, xq, wq, xs, ws, bias=bias, out_dtype=od)
        assert torch.equal(y.reshape(-1, Nn), chain), od
        assert torch.equal(chain, fused(f32, bias, None, od)), od
    ref = x.double() @ w.double().t()
    rel = lambda y: float((y.double().cpu() - ref).norm() / ref.norm())
    eb = rel(N_.fp8_linear_blockwise(x.to(DEV), gq, gs, out_dtype=torch.float32))
    tq, ts = N_.fp8_quantize(w.to(DEV))
    et = rel(N_.fp8_linear(x.to(DEV), tq, ts, out_dtype=torch.float32))
    print(f"relative error against float64 x @ w.T: blockwise {eb:.3e}, tensorwise {et:.3e}")
    assert eb <= et, (eb, et)


# ---- 8. the _scaled_mm route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_b_kind", ["128x128", "1x128"])
@pytest.mark.parametrize("scale_a_layout", ["outer_dim_major", "row_major"])
def test_patched_scaled_mm_with_bias_and_every_out_dtype(N_, scale_a_layout, scale_b_kind):
    import fp8_mps_patch
    M, Nn, K = 200, 260, 384                                                     # M is no multiple of 128; three K blocks
    bb = 128 if scale_b_kind == "128x128" else 1
    A, B, sa, sb, exact, bound = problem(M, Nn, K, (1, bb), -8, -4, seed=15)
    sa_t = t(sa.T.copy()).t() if scale_a_layout == "outer_dim_major" else t(sa)
    assert sa_t.stride() == ((1, M) if scale_a_layout == "outer_dim_major" else (3, 1))
    sb_t = t(sb.T.copy())                                                        # torch's (K/128, N/bb)
    a8 = t(A).view(torch.float8_e4m3fn)
    b8 = t(B).view(torch.float8_e4m3fn).t()                                      # (K, N) column-major
    assert fp8_mps_patch.scale_route(a8, b8, sa_t, sb_t) == "blockwise"
    f32 = run(N_, A, B, sa, sb, (1, bb))
    check(f32, exact, bound, MFMA_TOL, K, "native")
    fp8_mps_patch.install()
    try:
        for od in OUT_DTYPES:
            for bias in (None, make_bias(Nn, 16, od if od != torch.float32 else torch.bfloat16)):
                got = torch._scaled_mm(a8, b8, scale_a=sa_t, scale_b=sb_t, bias=bias, out_dtype=od)
                want = N_.fp8_scaled_mm_blockwise(t(A), t(B), t(sa), t(sb), block_a=1, block_b=bb, bias=bias, out_dtype=od)
                assert got.dtype == od and torch.equal(got, want), (od, bias is not None)
                assert torch.equal(want, fused(f32, bias, None, od)), (od, bias is not None)
    finally:
        fp8_mps_patch.uninstall()


@pytest.mark.parametrize("K", [96, 128])
def test_patched_scaled_mm_where_blockwise_and_rowwise_shapes_coincide(N_, K):
    """K <= 128: (M, 1) and (1, N) are rowwise scales and 1x128 x 1x128 blockwise ones; scale_route sends them to the tensorwise
    kernels.  The two are the same mathematics, so the result meets the blockwise bar against the blockwise oracle."""
    import fp8_mps_patch
    M, Nn = 70, 200
    A, B, sa, sb, exact, bound = problem(M, Nn, K, (1, 1), -8, -4, seed=16)
    a8 = t(A).view(torch.float8_e4m3fn)
    b8 = t(B).view(torch.float8_e4m3fn).t()
    sa_t, sb_t = t(sa), t(sb.T.copy())
    assert sa_t.shape == (M, 1) and sb_t.shape == (1, Nn)
    assert fp8_mps_patch.scale_route(a8, b8, sa_t, sb_t) == "tensorwise"
    fp8_mps_patch.install()
    try:
        got = torch._scaled_mm(a8, b8, scale_a=sa_t, scale_b=sb_t, out_dtype=torch.float32)
    finally:
        fp8_mps_patch.uninstall()
    check(got, exact, bound, MFMA_TOL, K, "rowwise route")
    check(run(N_, A, B, sa, sb, (1, 1)), exact, bound, MFMA_TOL, K, "blockwise op")


# ---- 9. graph replay --------------------------------------------------------------------------------------------------
def test_graph_replays_quantizer_then_gemm_on_new_inputs(N_):
    """One capture of fp8_quantize_blockwise followed by the GEMM into `out=` (a linear chain on one stream); replayed twice
    after the input's contents changed, each replay gives what the eager ops give on that input."""
    g = torch.Generator().manual_seed(41)
    M, Nn, K = 64, 200, 640
    rng = np.random.default_rng(41)
    W, sw = t(rand_bytes(rng, (Nn, K))), t(rand_scales(rng, Nn, K, 128, -8, -4))
    inputs = [(torch.randn(M, K, generator=g) * s).to(torch.bfloat16).to(DEV) for s in (1.0, 0.01, 30.0)]

    def eager(x):
        q, s = N_.fp8_quantize_blockwise(x, 1)
        return N_.fp8_scaled_mm_blockwise(q, W, s, sw, out_dtype=torch.bfloat16)

    x_static = inputs[0].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = torch.empty_like(eager(x_static))                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        q, s = N_.fp8_quantize_blockwise(x_static, 1)
        N_.fp8_scaled_mm_blockwise(q, W, s, sw, out_dtype=torch.bfloat16, out=out)
    want0 = eager(inputs[0])
    rq, rs = quantize_blockwise_ref(inputs[0].cpu(), 1)
    exact, bound = mm_ref(rq.numpy(), W.cpu().numpy(), rs.numpy(), sw.cpu().numpy(), 1, 128)
    check(run(N_, rq, W, rs, sw), exact, bound, MFMA_TOL, K, "eager f32")
    assert torch.equal(want0, run(N_, rq, W, rs, sw, out_dtype=torch.bfloat16))
    for x in inputs[1:] + inputs[:1]:
        x_static.copy_(x)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager(x))
        assert bool((out != 0).any())


# ---- 10. a plain C caller ---------------------------------------------------------------------------------------------
def test_c_abi_blockwise_roundtrip_without_torch(tmp_path):
    exe = str(tmp_path / "blockwise_roundtrip")
    cmd = ["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "blockwise_roundtrip.c"), "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lfp8mi", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "blockwise C ABI round trip: ok" in out.stdout
