"""Helpers of the grouped (MoE) GEMM tests (not a test module): tests/test_gpu_grouped.py and tests/test_gpu_grouped_edges.py.

The contract they check (include/fp8mi.h): every group's rows equal, BIT FOR BIT, the single-problem call on those rows
with the same ring tile and split_k=1; rows no group owns, and everything around C, stay untouched.  C sits between guard rows, prefilled
with a sentinel.  Nothing here depends on a module global of a test file: M_total, G, N and K come in as parameters or with the Case."""
import numpy as np
import torch

import fp8_mi355x_lib as L

DEV = "cuda"
TILES = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
         L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
# (BM, BN) of the ring tiles (with_product_tile, csrc/fp8mi_gemm.hip)
TILE_DIMS = {L.KERNEL_GEMM_128: (128, 128), L.KERNEL_GEMM_128x64: (128, 64), L.KERNEL_GEMM_64x128: (64, 128), L.KERNEL_GEMM_64x64: (64, 64),
             L.KERNEL_GEMM_32x64: (32, 64), L.KERNEL_GEMM_32x32: (32, 32), L.KERNEL_GEMM_128D: (128, 128)}
CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
GUARD = 8
SENTINEL = -12352.0   # exact in bfloat16 and float16
MFMA_TOL = 1.0e-3     # include/fp8mi.h: |gpu - exact| <= 1e-3 sum_k |a b| |sa sb| on the matrix core
EXACT_VALS = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=np.uint8)   # 0, +-1, +-2, +-3, +-4


def t(x):
    return x.to(DEV) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rand_bytes(rng, shape):
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def clamped_groups(offs, m_total):
    """[(start, end)] by the definition: start_0 = 0, start_g = end_{g-1}, end_g = clamp(offs[g], start_g, M_total)"""
    out, start = [], 0
    for o in offs:
        end = min(max(int(o), start), m_total)
        out.append((start, end))
        start = end
    return out


class Case:
    """One problem on the device, made once per (offs, M_total, N, K, seed) and never modified: G = len(offs) experts."""

    def __init__(self, offs, m_total, n, k, seed=1):
        rng = np.random.default_rng(seed)
        self.offs_np = np.asarray(offs, dtype=np.int32)
        self.G, self.m_total, self.n, self.k = len(self.offs_np), m_total, n, k
        G = self.G
        self.A_np, self.B_np = rand_bytes(rng, (m_total, k)), rand_bytes(rng, (G, n, k))
        self.sa_np = np.exp2(rng.uniform(-3, 3, m_total)).astype(np.float32)
        self.sb_np = np.exp2(rng.uniform(-3, 3, (G, n))).astype(np.float32)
        self.A, self.B = t(self.A_np), t(self.B_np)
        self.sa = {L.SCALE_ROW: t(self.sa_np), L.SCALE_TENSOR: t(self.sa_np[:1])}
        self.sb = {L.SCALE_ROW: t(self.sb_np), L.SCALE_TENSOR: t(self.sb_np[:, 0])}
        self.bias_np = rng.standard_normal((G, n)).astype(np.float32) * 50.0
        self.bias = t(self.bias_np)
        self.sr = t(np.array([0.37], dtype=np.float32))
        self.offs = t(self.offs_np)
        self.groups = clamped_groups(self.offs_np, m_total)


def guarded(dtype, m_total, n, ldc=None):
    """-> (whole buffer, its C view): m_total rows of n columns (row stride ldc) between GUARD rows, everything prefilled with SENTINEL"""
    buf = torch.full((GUARD + m_total + GUARD, n if ldc is None else ldc), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + m_total, :n]


def assert_untouched(buf, n, groups):
    """guard rows, the columns behind n, and the rows no group owns still hold the sentinel"""
    owned = torch.zeros(buf.shape[0], dtype=torch.bool, device=DEV)
    for s, e in groups:
        owned[GUARD + s:GUARD + e] = True
    assert bool((buf[~owned] == SENTINEL).all()), "a row outside every group was written"
    assert bool((buf[:, n:] == SENTINEL).all()), "a column behind N was written"


def resolved_tile(c, tile, out_dtype, ldc=None):
    """the ring tile a grouped call on Case c runs: `tile` itself, or what AUTO chooses (fp8mi_choose_kernel_grouped)"""
    if tile != L.KERNEL_AUTO:
        return tile
    got = L.load().fp8mi_choose_kernel_grouped(c.G, c.m_total, c.n, c.k, c.k, c.k, c.n if ldc is None else ldc, CODE[out_dtype])
    assert got in TILES, got
    return got


def reference_rows(N_, c, g, s, e, sa_mode, sb_mode, epi, out_dtype, tile, A=None, nan_mode=None, B=None, bias=None):
    """what a caller can do today for one group: fp8_scaled_mm on its rows with the same tile, unsplit"""
    A = c.A if A is None else A
    B = c.B if B is None else B
    bias = c.bias if bias is None else bias
    sa = c.sa[sa_mode][s:e] if sa_mode == L.SCALE_ROW else c.sa[sa_mode]
    sb = c.sb[sb_mode][g] if sb_mode == L.SCALE_ROW else c.sb[sb_mode][g:g + 1]
    return N_.fp8_scaled_mm(A[s:e], B[g], sa, sb, bias=bias[g] if epi else None, scale_result=c.sr if epi else None,
                            out_dtype=out_dtype, kernel=tile, split_k=1, nan_mode=nan_mode)


def run_and_compare(N_, c, tile, out_dtype, sa_mode, sb_mode, epi, A=None, ldc=None, offs=None, groups=None, nan_mode=None, B=None, bias=None,
                    bits=False):
    """One grouped launch on Case c into a guarded C; every group's rows against reference_rows, then the sentinel check.
    `bits`: compare bit patterns (NaN != NaN).  -> (whole buffer, C)"""
    groups = c.groups if groups is None else groups
    buf, C = guarded(out_dtype, c.m_total, c.n, ldc)
    got = N_.fp8_scaled_mm_grouped(c.A if A is None else A, c.B if B is None else B, c.sa[sa_mode], c.sb[sb_mode], c.offs if offs is None else offs,
                                   bias=(c.bias if bias is None else bias) if epi else None, scale_result=c.sr if epi else None,
                                   out_dtype=out_dtype, kernel=tile, out=C, nan_mode=nan_mode)
    assert got is C
    ref_tile = resolved_tile(c, tile, out_dtype, ldc)
    for g, (s, e) in enumerate(groups):
        if e > s:
            want = reference_rows(N_, c, g, s, e, sa_mode, sb_mode, epi, out_dtype, ref_tile, A, nan_mode, B, bias)
            if bits:
                iv = torch.int32 if out_dtype == torch.float32 else torch.int16
                assert torch.equal(C[s:e].contiguous().view(iv), want.view(iv)), (tile, out_dtype, sa_mode, sb_mode, epi, g)
            else:
                assert torch.equal(C[s:e], want), (tile, out_dtype, sa_mode, sb_mode, epi, g)
    assert_untouched(buf, c.n, groups)
    return buf, C


# ---- blockwise -----------------------------------------------------------------------------------------------------------------

def blockwise_scales(rng, m_total, G, n, k, block_b):
    """-> (scale_a (m_total, ceil(k / 128)), scale_b (G, ceil(n / block_b), ceil(k / 128))) float32 numpy: 2^-6 .. 2^6, random signs"""
    nkb, nrb = -(-k // 128), -(-n // block_b)
    sa = (np.exp2(rng.uniform(-6, 6, (m_total, nkb))) * rng.choice([-1.0, 1.0], (m_total, nkb))).astype(np.float32)
    sb = (np.exp2(rng.uniform(-6, 6, (G, nrb, nkb))) * rng.choice([-1.0, 1.0], (G, nrb, nkb))).astype(np.float32)
    return sa, sb


def run_and_compare_blockwise(N_, c, sa, sb, block_b, tile, out_dtype, epi, A=None, B=None, ldc=None, offs=None, groups=None, nan_mode=None,
                              bias=None, bits=False, sa_ref=None, sb_ref=None):
    """run_and_compare for fp8_scaled_mm_grouped_blockwise against fp8_scaled_mm_blockwise per group.  sa / sb: device tensors (any strides);
    the per-group calls read sa_ref / sb_ref (default: the same tensors)."""
    groups = c.groups if groups is None else groups
    A = c.A if A is None else A
    B = c.B if B is None else B
    bias = c.bias if bias is None else bias
    sa_ref = sa if sa_ref is None else sa_ref
    sb_ref = sb if sb_ref is None else sb_ref
    buf, C = guarded(out_dtype, c.m_total, c.n, ldc)
    got = N_.fp8_scaled_mm_grouped_blockwise(A, B, sa, sb, c.offs if offs is None else offs, block_b=block_b, bias=bias if epi else None,
                                             scale_result=c.sr if epi else None, out_dtype=out_dtype, kernel=tile, out=C, nan_mode=nan_mode)
    assert got is C
    ref_tile = resolved_tile(c, tile, out_dtype, ldc)
    for g, (s, e) in enumerate(groups):
        if e > s:
            want = N_.fp8_scaled_mm_blockwise(A[s:e], B[g], sa_ref[s:e], sb_ref[g], block_a=1, block_b=block_b, bias=bias[g] if epi else None,
                                              scale_result=c.sr if epi else None, out_dtype=out_dtype, kernel=ref_tile, split_k=1,
                                              nan_mode=nan_mode)
            if bits:
                iv = torch.int32 if out_dtype == torch.float32 else torch.int16
                assert torch.equal(C[s:e].contiguous().view(iv), want.view(iv)), (tile, block_b, out_dtype, g)
            else:
                assert torch.equal(C[s:e], want), (tile, block_b, out_dtype, g)
    assert_untouched(buf, c.n, groups)
    return buf, C


# ---- exact data ------------------------------------------------------------------------------------------------------------------

def exact_problem(oracle, offs, m_total, n, k, seed):
    """Bytes that decode to 0, +-1 .. +-4 and power-of-two row scales: every partial sum is an integer below 2^24 times a power of two, so
    any summation order gives the same fp32.  -> (A, B, sa, sb numpy, expected (m_total, n) float32 with SENTINEL in the rows no group owns)"""
    decode = oracle.decode
    rng = np.random.default_rng(seed)
    G = len(offs)
    A, B = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (m_total, k))], EXACT_VALS[rng.integers(0, len(EXACT_VALS), (G, n, k))]
    sa = np.exp2(rng.integers(-2, 3, m_total)).astype(np.float32)
    sb = np.exp2(rng.integers(-2, 3, (G, n))).astype(np.float32)
    assert k * 16 * 16 < 2 ** 24
    exact = np.full((m_total, n), SENTINEL, dtype=np.float32)
    a64 = decode(A).astype(np.float64)
    for g, (s, e) in enumerate(clamped_groups(offs, m_total)):
        if e > s:
            exact[s:e] = (a64[s:e] @ decode(B[g]).astype(np.float64).T) * sa[s:e, None] * sb[g][None, :]
    return A, B, sa, sb, exact
