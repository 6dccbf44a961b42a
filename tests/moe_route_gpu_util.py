"""What tests/test_gpu_moe_route.py and tests/test_gpu_moe_route_edges.py share: guarded outputs, the runners of the three C entry points
(every output between guard elements prefilled with a sentinel) and their checks against tests/moe_route_ref.py and the existing
quantisers, the MoE layer's weights and the forward's reference.  A plain module: no fixtures, no tests."""
import torch

import fp8_mi355x_lib as L
from moe_route_ref import combine_f64, combine_ref, route_ref

DEV = "cuda"
GUARD = 64               # elements on either side of every output
SENT_I, SENT_B, SENT_F = -7777, 0xA5, -12352.0   # (the float is exact in bfloat16 and float16)
CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
CHUNK, SINGLE = L.MOE_ROUTE_CHUNK, L.MOE_ROUTE_SINGLE_MAX
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
TILE = L.KERNEL_GEMM_32x64   # the one fixed ring tile of the forward comparisons
MANT = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}   # significand bits p: rounding v to the format moves it by at most 2^-p |v|


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(count, dtype, fill):
    buf = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + count]


def guards_intact(buf, count, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + count:] == fill).all())


def bits(t):
    """a float tensor as its bit patterns: NaNs compare"""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- route -----------------------------------------------------------------------------------------------------------------------------

def run_route(lib, ids, G, with_src=True):
    """fp8mi_moe_route on `ids` (any shape, int32 / int64, on the device) -> (offs, row_of, src_of_row) on the CPU; guards checked"""
    n = ids.numel()
    offs_buf, offs = guarded(G, torch.int32, SENT_I)
    row_buf, row_of = guarded(n, torch.int32, SENT_I)
    src_buf, src = guarded(n, torch.int32, SENT_I)
    need = lib.fp8mi_moe_route_workspace_bytes(n, G)
    assert need >= 0 and (need == 0) == (n <= SINGLE)
    ws_buf, ws = guarded(need, torch.uint8, SENT_B)
    with L.kernel_timer(8) as kt:
        rc = lib.fp8mi_moe_route(ids.data_ptr(), ids.element_size(), n, G, offs.data_ptr(), row_of.data_ptr(), src.data_ptr() if with_src else None,
                                 ws.data_ptr() if need else None, need, stream())
    L.check(rc, "fp8mi_moe_route")
    torch.cuda.synchronize()
    assert len(kt.ms) == (1 if n <= SINGLE else 3)
    assert guards_intact(offs_buf, G, SENT_I) and guards_intact(row_buf, n, SENT_I) and guards_intact(src_buf, n, SENT_I)
    assert guards_intact(ws_buf, need, SENT_B)
    if not with_src:
        assert bool((src == SENT_I).all())
    return offs.cpu(), row_of.cpu(), src.cpu()


def check_route(lib, ids_cpu, G, dtype, with_src=True):
    offs, row_of, src = run_route(lib, ids_cpu.to(dtype).to(DEV), G, with_src)
    w_offs, w_row_of, w_src = route_ref(ids_cpu, G)
    what = (tuple(ids_cpu.shape), G, dtype)
    assert torch.equal(offs, w_offs), what
    assert torch.equal(row_of, w_row_of), what
    if with_src:
        assert torch.equal(src, w_src), what


def random_ids(gen, T, k, G, dropped=0.1):
    ids = torch.randint(0, G, (T, k), generator=gen, dtype=torch.int64)
    drop = torch.tensor([-1, G, INT32_MIN, INT32_MAX])[torch.randint(0, 4, (T, k), generator=gen)]
    return torch.where(torch.rand((T, k), generator=gen) < dropped, drop, ids)


# ---- scatter-quantise ------------------------------------------------------------------------------------------------------------------

def run_scatter(lib, x, row_of, rows_out, group, enc, ld_out=None, s_sr=None, s_sk=1):
    """fp8mi_moe_scatter_quantize -> (out (rows_out, ld_out) bytes, the whole scale allocation), guards checked"""
    T, cols = x.shape
    ncb = (cols + 127) // 128
    ld_out = cols if ld_out is None else ld_out
    s_sr = (ncb if group else 1) if s_sr is None else s_sr
    out_buf, out = guarded(rows_out * ld_out, torch.uint8, SENT_B)
    n_sc = (rows_out - 1) * s_sr + ((ncb - 1) * s_sk if group else 0) + 1
    sc_buf, sc = guarded(n_sc, torch.float32, SENT_F)
    row_dev = row_of.to(torch.int32).to(DEV).contiguous()
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_moe_scatter_quantize(x.data_ptr(), CODE[x.dtype], T, cols, x.stride(0), row_dev.data_ptr(), row_of.shape[1], out.data_ptr(), rows_out,
                                            ld_out, sc.data_ptr(), s_sr, s_sk, L.QSCALE_GROUP128 if group else L.QSCALE_ROW, L.FMT_E4M3, enc, stream())
    L.check(rc, "fp8mi_moe_scatter_quantize")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1
    assert guards_intact(out_buf, rows_out * ld_out, SENT_B) and guards_intact(sc_buf, n_sc, SENT_F)
    return out.reshape(rows_out, ld_out).cpu(), sc.cpu()


def check_scatter(lib, N_, x, row_of, group, enc, rows_out=None, ld_out=None, s_sr=None, s_sk=1):
    """Every byte of `out` and every float of `scales`: an owned row holds its token's quantisation, everything else the sentinel."""
    T, cols = x.shape
    k = row_of.shape[1]
    rows_out = T * k if rows_out is None else rows_out
    ncb = (cols + 127) // 128
    if group:
        q, s = N_.fp8_act_quantize(x, "none", False, "block128")
    else:
        q, s = N_.fp8_quantize_rowwise(x, encode_mode=enc)
    q, s = q.cpu(), s.cpu()
    out, sc = run_scatter(lib, x, row_of, rows_out, group, enc, ld_out, s_sr, s_sk)
    ld_out = out.shape[1]
    s_sr = (ncb if group else 1) if s_sr is None else s_sr
    want_out = torch.full((rows_out, ld_out), SENT_B, dtype=torch.uint8)
    want_sc = torch.full_like(sc, SENT_F)
    owned = 0
    for t in range(T):
        for j in range(k):
            r = int(row_of[t, j])
            if 0 <= r < rows_out:
                want_out[r, :cols] = q[t]
                for b in range(ncb if group else 1):
                    want_sc[r * s_sr + b * s_sk] = s[t, b]
                owned += 1
    assert 0 < owned
    what = (x.dtype, cols, group, enc)
    assert torch.equal(out, want_out), what
    assert torch.equal(bits(sc), bits(want_sc)), what


# ---- combine ---------------------------------------------------------------------------------------------------------------------------

def run_combine(lib, y, row_of, weights, out_dtype, ld_out=None, out_offset=0, ld_y=None):
    """fp8mi_moe_combine -> (T, N) on the CPU; guards and the padding columns checked.  out_offset: elements by which the output starts
    behind the (256-byte aligned) guard: a base that is aligned to fewer bytes.  ld_y: passed in place of y's row stride"""
    rows, N = y.shape
    T, k = row_of.shape
    ld_out = N if ld_out is None else ld_out
    ld_y = (y.stride(0) if rows > 1 else N) if ld_y is None else ld_y
    out_buf, out = guarded(T * ld_out + out_offset, out_dtype, SENT_F)
    out = out[out_offset:]
    row_dev = row_of.to(DEV).contiguous()
    w_dev = weights.to(DEV).contiguous() if weights is not None else None
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_moe_combine(y.data_ptr(), CODE[y.dtype], rows, N, ld_y, row_dev.data_ptr(),
                                   w_dev.data_ptr() if w_dev is not None else None, T, k, out.data_ptr(), CODE[out_dtype], ld_out, stream())
    L.check(rc, "fp8mi_moe_combine")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1 and guards_intact(out_buf, T * ld_out + out_offset, SENT_F)
    assert bool((out_buf[GUARD:GUARD + out_offset] == SENT_F).all())
    out = out.reshape(T, ld_out).cpu()
    assert bool((out[:, N:] == SENT_F).all())
    return out[:, :N]


def equal_bits_or_both_nan(got, want):
    """Bit equality, +-inf and signed zeros included, wherever `want` is a number; where it is NaN, `got` is NaN too (the CPU loop and the
    GPU give NaNs of different bit patterns: inf - inf is 0xFFC00000 from torch on the CPU and the positive default NaN on the GPU)."""
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def check_combine(lib, y, row_of, weights, out_dtype, ld_out=None, gone_tokens=(), out_offset=0, exact_only_tokens=None, ld_y=None):
    """Bit equality with the sequential float32 loop, the derived bound around the float64 sum, zeros for a token without a valid
    assignment; `gone_tokens` must be such tokens.  exact_only_tokens: the tokens whose terms hold an inf, a NaN or a subnormal on
    purpose - reference NaNs then compare as NaNs, and the bound (whose model has neither overflow nor underflow) is taken for the
    other tokens only."""
    got = run_combine(lib, y, row_of, weights, out_dtype, ld_out, out_offset, ld_y)
    what = (y.dtype, out_dtype, tuple(y.shape), row_of.shape[1], weights is None)
    want = combine_ref(y, row_of, weights, out_dtype)
    keep = torch.ones(row_of.shape[0], dtype=torch.bool)
    if exact_only_tokens is None:
        assert torch.equal(bits(got), bits(want)), what
    else:
        assert equal_bits_or_both_nan(got, want), what
        keep[list(exact_only_tokens)] = False
    # the independent bound: k products and k sums in fp32, each within 2^-24 relative, then one rounding to out_dtype.  The last term is
    # the RELATIVE bound 2^-p |v| on that rounding - at least half an ulp of v and up to twice it - not half an ulp itself: the exact check
    # is the bit equality above
    k = row_of.shape[1]
    total, mag = combine_f64(y, row_of, weights)
    err32 = (k + 1) * 2.0 ** -24 * mag
    tol = err32 + 2.0 ** -MANT[out_dtype] * (total.abs() + err32) + (2.0 ** -25 if out_dtype == torch.float16 else 0.0)
    assert bool(((got.double() - total).abs() <= tol)[keep].all()), what
    gone = ((row_of < 0) | (row_of >= y.shape[0])).all(dim=1)
    assert all(bool(gone[t]) for t in gone_tokens) and bool((got[gone] == 0).all())
    return got


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

class Layer:
    """One MoE layer's weights on the device in both recipes, made once per shape"""

    def __init__(self, N_, G, K, H, N, seed):
        gen = torch.Generator().manual_seed(seed)
        W1 = (torch.randn((G, 2 * H, K), generator=gen) * K ** -0.5).to(DEV)
        W2 = (torch.randn((G, N, H), generator=gen) * H ** -0.5).to(DEV)
        self.G, self.K, self.H, self.N = G, K, H, N
        q1, s1 = N_.fp8_quantize_rowwise(W1.reshape(G * 2 * H, K), encode_mode=L.ENC_RNE)
        q2, s2 = N_.fp8_quantize_rowwise(W2.reshape(G * N, H), encode_mode=L.ENC_RNE)
        self.row = (q1.reshape(G, 2 * H, K), s1.reshape(G, 2 * H), q2.reshape(G, N, H), s2.reshape(G, N))
        b1 = [N_.fp8_quantize_blockwise(W1[g], 128) for g in range(G)]
        b2 = [N_.fp8_quantize_blockwise(W2[g], 128) for g in range(G)]
        self.block = (torch.stack([q for q, _ in b1]), torch.stack([s for _, s in b1]), torch.stack([q for q, _ in b2]), torch.stack([s for _, s in b2]))
        self.bias1 = torch.randn((G, 2 * H), generator=gen).to(DEV)
        self.bias2 = torch.randn((G, N), generator=gen).to(DEV)


def forward_pair(N_, recipe):
    return (N_.fp8_moe_forward_rowwise, N_.fp8_moe_mlp_rowwise) if recipe == "row" else (N_.fp8_moe_forward_blockwise, N_.fp8_moe_mlp_blockwise)


def forward_reference(N_, recipe, layer, x, ids, wts, out_dtype=None, bias=False):
    """reference route -> fp8_moe_mlp_* on the gathered rows with the fixed tile -> the float32 combine over the rows below offs[-1]"""
    _fwd, mlp = forward_pair(N_, recipe)
    k = ids.shape[1]
    offs, row_of, src = route_ref(ids, layer.G)
    xs = x[(src.clamp(min=0) // k).long().to(DEV)]
    weights = layer.row if recipe == "row" else layer.block
    y = mlp(xs, offs.to(DEV), *weights, bias1=layer.bias1 if bias else None, bias2=layer.bias2 if bias else None, kernel=TILE)
    return combine_ref(y[:int(offs[-1])], row_of.reshape(ids.shape), wts, y.dtype if out_dtype is None else out_dtype)


def gate(gen, T, k, G, dropped=0.0):
    ids = torch.topk(torch.rand((T, G), generator=gen), k, dim=1).indices
    if dropped:
        ids = torch.where(torch.rand((T, k), generator=gen) < dropped, torch.tensor(-1), ids)
    return ids, torch.softmax(torch.randn((T, k), generator=gen), dim=1)
