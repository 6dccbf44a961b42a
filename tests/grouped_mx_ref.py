"""Helpers of the grouped MXFP8 / MXFP4 / MXW4A8 GEMM tests and of the MX MoE tests (not a test module): tests/test_gpu_grouped_mx.py and
tests/test_gpu_moe_mx.py.

The contract (include/fp8mi.h): every group's rows equal, bit for bit (a NaN matches a NaN), fp8_scaled_mm_mxfp8 /
_mxfp4 / _mxw4a8 on those rows with the same ring tile and split_k=1; rows no group owns and everything around C stay untouched.  A problem is made once per
(format, sizes, K, seed) on the host and on the device and is never modified."""
import numpy as np
import torch

import fp8_mi355x_lib as L
import mxfp4_ref
import mxfp8_ref
import mxw4a8_ref
from grouped_ref import DEV, EXACT_VALS, SENTINEL, TILE_DIMS, assert_untouched, clamped_groups, guarded, rand_bytes, t   # noqa: F401 (re-exported)

FORMATS = ("mxfp8", "mxfp4", "mxw4a8")
EXACT_CODES = np.array([0, 2, 4, 5, 6, 10, 12, 13, 14], dtype=np.uint8)   # e2m1: 0, +-1, +-2, +-3, +-4


def pad4(n):
    return (n + 3) // 4 * 4


def group_sizes(rng, G, bm):
    """G sizes from {0, 1, BM-1, BM, BM+1, 2 BM+3}: every one of the six as long as G allows, then random draws; shuffled"""
    pool = [0, 1, bm - 1, bm, bm + 1, 2 * bm + 3]
    if G == 1:
        return [bm + 1]
    sizes = [pool[i] for i in rng.permutation(6)[:min(G, 6)]] + [pool[i] for i in rng.integers(0, 6, max(G - 6, 0))]
    return [sizes[i] for i in rng.permutation(G)]


class MxCase:
    """A (M_total, kb_a) operand bytes, B (G, N, kb_b), E8M0 scales in rows of pad4(K / 32) bytes (pad bytes 0x7F), the blocks random in 120 .. 134: 2^-7 .. 2^7, so that no finite sum leaves fp32.
    kb: bytes of K in a row of A; K = kb elements (MXFP8, MXW4A8) or 2 kb (MXFP4).  kb_a = kb; kb_b: bytes of K in a row of B - kb, or K / 2 for
    MXW4A8, whose A is e4m3 bytes and whose B is e2m1 pairs.  tail: unowned rows behind the last group."""

    def __init__(self, fmt, sizes, n, kb, seed, tail=3, exact=False):
        rng = np.random.default_rng(seed)
        self.fmt, self.fp4, self.w4a8 = fmt, fmt == "mxfp4", fmt == "mxw4a8"
        self.offs_np = np.cumsum(sizes).astype(np.int32)
        self.G, self.n, self.kb = len(sizes), n, kb
        self.m_total = int(self.offs_np[-1]) + tail
        self.K = 2 * kb if self.fp4 else kb
        self.kb_a, self.kb_b = kb, kb // 2 if self.w4a8 else kb
        kb_b = self.kb_b
        a_fp4, b_fp4 = self.fp4, self.fp4 or self.w4a8               # two e2m1 codes per byte on that side
        self.nb, self.ld_s = self.K // 32, pad4(self.K // 32)
        G, M, nb = self.G, self.m_total, self.nb
        if exact:
            def pick(shape, fp4):
                vals = EXACT_CODES if fp4 else EXACT_VALS
                one = lambda: vals[rng.integers(0, len(vals), shape)]   # noqa: E731
                return (one() | (one() << 4)).astype(np.uint8) if fp4 else one()
            self.A_np, self.B_np = pick((M, kb), a_fp4), pick((G, n, kb_b), b_fp4)
            lo, hi = 126, 128
        else:
            raw = lambda shape, fp4: rng.integers(0, 256, size=shape, dtype=np.uint8) if fp4 else rand_bytes(rng, shape)   # noqa: E731
            self.A_np, self.B_np = raw((M, kb), a_fp4), raw((G, n, kb_b), b_fp4)
            lo, hi = 120, 134
        self.sa_np = np.full((M, self.ld_s), 0x7F, dtype=np.uint8)
        self.sb_np = np.full((G, n, self.ld_s), 0x7F, dtype=np.uint8)
        self.sa_np[:, :nb] = rng.integers(lo, hi + 1, (M, nb), dtype=np.uint8)
        self.sb_np[:, :, :nb] = rng.integers(lo, hi + 1, (G, n, nb), dtype=np.uint8)
        self.bias_np = rng.standard_normal((G, n)).astype(np.float32) * 50.0
        self.A, self.B, self.sa, self.sb = t(self.A_np), t(self.B_np), t(self.sa_np), t(self.sb_np)
        self.bias = t(self.bias_np)
        self.sr = t(np.array([0.37], dtype=np.float32))
        self.offs = t(self.offs_np)
        self.groups = clamped_groups(self.offs_np, self.m_total)


def grouped_op(N_, fmt):
    return getattr(N_, "fp8_scaled_mm_grouped_" + fmt)


def single_op(N_, fmt):
    return getattr(N_, "fp8_scaled_mm_" + fmt)


def chosen_tile(c, out_code=L.F32):
    """the ring tile AUTO runs on MxCase c (dense operands and C): what the format's grouped chooser names"""
    lib = L.load()
    if c.w4a8:
        return lib.fp8mi_choose_kernel_grouped_mxw4a8(c.G, c.m_total, c.n, c.K, c.kb_a, c.kb_b, c.n, out_code)
    return lib.fp8mi_choose_kernel_grouped_mx(L.MX_FP4 if c.fp4 else L.MX_FP8, c.G, c.m_total, c.n, c.K, c.kb_a, c.kb_b, c.n, out_code)


def same_bits(got, want):
    """bit patterns equal; a NaN matches a NaN at the same position"""
    iv = torch.int32 if got.dtype == torch.float32 else torch.int16
    g, w = got.contiguous(), want.contiguous()
    nan_g, nan_w = torch.isnan(g), torch.isnan(w)
    return bool(torch.equal(nan_g, nan_w)) and bool(torch.equal(g.view(iv)[~nan_g], w.view(iv)[~nan_w]))


def run_and_compare(N_, c, tile, out_dtype=torch.float32, epi=False, bias=None, A=None, B=None, sa=None, sb=None, ldc=None, offs=None, groups=None,
                    nan_mode=None, ref_tile=None):
    """One grouped launch on MxCase c into a guarded C; (a) every group's rows against the single-problem call on the same tile, (b) the
    sentinel check.  A / B / sa / sb: device tensors in place of the case's (any layout the ops read in place); -> (whole buffer, C)"""
    groups = c.groups if groups is None else groups
    A, B = c.A if A is None else A, c.B if B is None else B
    sa, sb = c.sa if sa is None else sa, c.sb if sb is None else sb
    bias = (c.bias if bias is None else bias) if epi else None
    kw = {} if c.fp4 or nan_mode is None else {"nan_mode": nan_mode}
    buf, C = guarded(out_dtype, c.m_total, c.n, ldc)
    got = grouped_op(N_, c.fmt)(A, B, sa[:, :c.nb], sb[:, :, :c.nb], c.offs if offs is None else offs, bias=bias, scale_result=c.sr if epi else None,
                                out_dtype=out_dtype, kernel=tile, out=C, **kw)
    assert got is C
    ref_tile = tile if ref_tile is None else ref_tile
    for g, (s, e) in enumerate(groups):
        if e > s:
            want = single_op(N_, c.fmt)(A[s:e], B[g], sa[s:e, :c.nb], sb[g][:, :c.nb], bias=bias[g] if epi else None,
                                        scale_result=c.sr if epi else None, out_dtype=out_dtype, kernel=ref_tile, split_k=1, **kw)
            assert same_bits(C[s:e], want), (c.fmt, tile, out_dtype, epi, g, s, e)
    assert_untouched(buf, c.n, groups)
    return buf, C


def reference_f64(c, nan_zero=True):
    """-> (exact (M_total, N) float64 of the dequantised operands per group, the bound sum |a 2^sa| |b 2^sb|); NaN rows where no group owns"""
    exact = np.full((c.m_total, c.n), np.nan)
    bound = np.zeros((c.m_total, c.n))
    for g, (s, e) in enumerate(c.groups):
        if e > s:
            if c.fp4:
                exact[s:e], bound[s:e] = mxfp4_ref.mm_ref(c.A_np[s:e], c.B_np[g], c.sa_np[s:e, :c.nb], c.sb_np[g][:, :c.nb])
            else:
                mm_ref = mxw4a8_ref.mm_ref if c.w4a8 else mxfp8_ref.mm_ref
                exact[s:e], bound[s:e] = mm_ref(c.A_np[s:e], c.B_np[g], c.sa_np[s:e, :c.nb], c.sb_np[g][:, :c.nb], nan_zero)
    return exact, bound


def owned_rows(c):
    m = np.zeros(c.m_total, dtype=bool)
    for s, e in c.groups:
        m[s:e] = True
    return m


__all__ = ["DEV", "FORMATS", "SENTINEL", "TILE_DIMS", "MxCase", "group_sizes", "grouped_op", "single_op", "chosen_tile", "same_bits", "run_and_compare",
           "reference_f64", "owned_rows", "pad4", "L"]
