"""GPU (MI355X): the MoE layer on the MXFP8 / MXFP4 recipes - fp8mi_moe_scatter_quantize_mx, fp8_moe_linear_mx*, fp8_moe_mlp_mx* and
fp8_moe_forward_mx* (include/fp8mi.h).

  scatter   every byte of `out` and of `scales`, both prefilled with 0xFF between guards: a named row holds fp8_quantize_mxfp8 / _mxfp4 of its
            token byte for byte, the pad bytes of its scale row 0x7F; everything else keeps the prefill.
  linear / mlp   bit-equal to the per-expert loop of the single-problem ops on a forced tile.
  forward   bit-equal to the chain run by hand: fp8_quantize_mx* of the gathered tokens -> the single-problem MX GEMM per expert ->
            fp8_act_quantize(., scale) -> GEMM -> the sequential float32 combine on the CPU; eagerly and from a replayed graph."""
import pytest
import torch

import fp8_mi355x_lib as L
from grouped_mx_ref import DEV, pad4, single_op
from moe_route_gpu_util import CODE, INT32_MAX, INT32_MIN, SINGLE, TILE, bits, gate, guarded, guards_intact, stream
from moe_route_ref import combine_ref, route_ref

pytestmark = pytest.mark.gpu

FORMATS = ("mxfp8", "mxfp4")   # (the MoE ops on the MXW4A8 recipe: tests/test_gpu_grouped_mxw4a8.py)
FILL = 0xFF
MX = {"mxfp8": L.MX_FP8, "mxfp4": L.MX_FP4}
# the column counts on both sides of every row_rung boundary (one wave per row up to 8 pieces of 16 bytes per lane, four up to 32, eight - fp32
# only - up to 64), and the largest row
EDGES = {torch.float32: (2048, 2080, 8192, 8224, 16384), torch.float16: (4096, 4128, 16384), torch.bfloat16: (4096, 4128, 16384)}


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


@pytest.fixture(scope="module")
def lib():
    return L.load()


def quantize(N_, fmt, x):
    q, s = (N_.fp8_quantize_mxfp4 if fmt == "mxfp4" else N_.fp8_quantize_mxfp8)(x)
    return q.view(torch.uint8), s.view(torch.uint8)


# ---- scatter-quantise ----------------------------------------------------------------------------------------------------------------------

def tokens(gen, T, cols, dtype):
    """random rows; token 0: an all-zero block and a NaN (where the row has a second block); the last token: the largest finite value"""
    x = (torch.randn((T, cols), generator=gen) * torch.exp2(torch.randint(-12, 12, (T, 1), generator=gen).float())).to(dtype)
    x[0, :32] = 0
    if cols >= 64:
        x[0, 40] = float("nan")
    x[T - 1, cols - 1] = torch.finfo(dtype).max
    return x.to(DEV)


def plan(gen, T, k, dropped=0.2):
    """a permutation of the T k rows over the assignments, some of them dropped (-1) or out of range"""
    rows = torch.randperm(T * k, generator=gen).reshape(T, k).to(torch.int64)
    bad = torch.tensor([-1, T * k, INT32_MIN, INT32_MAX])[torch.randint(0, 4, (T, k), generator=gen)]
    row_of = torch.where(torch.rand((T, k), generator=gen) < dropped, bad, rows)
    row_of[0, 0] = rows[0, 0]   # at least one named row
    return row_of.to(torch.int32)


def check_scatter_mx(lib, N_, fmt, x, row_of, ld_s=None, sc_offset=0):
    T, cols = x.shape
    k = row_of.shape[1]
    rows_out, nb = T * k, cols // 32
    row_bytes = cols // 2 if fmt == "mxfp4" else cols
    ld_s = pad4(nb) if ld_s is None else ld_s
    out_buf, out = guarded(rows_out * row_bytes, torch.uint8, FILL)
    sc_buf, sc = guarded(rows_out * ld_s + sc_offset, torch.uint8, FILL)
    sc = sc[sc_offset:]
    row_dev = row_of.to(DEV).contiguous()
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_moe_scatter_quantize_mx(x.data_ptr(), CODE[x.dtype], T, cols, x.stride(0), row_dev.data_ptr(), k, out.data_ptr(), rows_out,
                                               row_bytes, sc.data_ptr(), ld_s, MX[fmt], stream())
    L.check(rc, "fp8mi_moe_scatter_quantize_mx")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1
    assert guards_intact(out_buf, rows_out * row_bytes, FILL) and guards_intact(sc_buf, rows_out * ld_s + sc_offset, FILL)
    q, s = quantize(N_, fmt, x)
    want_out = torch.full((rows_out, row_bytes), FILL, dtype=torch.uint8, device=DEV)
    want_sc = torch.full((rows_out, ld_s), FILL, dtype=torch.uint8, device=DEV)
    flat = row_dev.reshape(-1).long()
    named = (flat >= 0) & (flat < rows_out)
    tok = torch.arange(T, device=DEV).repeat_interleave(k)[named]
    want_out[flat[named]] = q[tok]
    want_sc[flat[named], :nb] = s[tok]
    if ld_s >= pad4(nb):
        want_sc[flat[named], nb:pad4(nb)] = 0x7F
    what = (fmt, x.dtype, T, k, cols, ld_s)
    assert int(named.sum()) > 0
    assert torch.equal(out.reshape(rows_out, row_bytes), want_out), what
    assert torch.equal(sc.reshape(rows_out, ld_s), want_sc), what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fmt", FORMATS)
def test_scatter_rows_equal_the_mx_quantisers_byte_for_byte(lib, N_, fmt, dtype):
    gen = torch.Generator().manual_seed(31)
    cases = [(1, 1, 32), (3, 65, 160), (64, 8, 4096), (5, 8, 32), (1, 65, 4096), (64, 1, 160)] + [(5, 8, c) for c in EDGES[dtype]]
    for T, k, cols in cases:
        check_scatter_mx(lib, N_, fmt, tokens(gen, T, cols, dtype), plan(gen, T, k))


@pytest.mark.parametrize("fmt", FORMATS)
def test_scatter_scale_layouts(lib, N_, fmt):
    """160 columns, five blocks: rows of 8 bytes (the default: three pad bytes 2^0), of 12 (the bytes behind the pad keep the prefill), of 5 (no
    room: no pad byte is written), and rows of 8 at a base that is 2 mod 4 (byte stores, pad bytes still written)"""
    gen = torch.Generator().manual_seed(32)
    for dtype in (torch.float32, torch.bfloat16):
        x, row_of = tokens(gen, 5, 160, dtype), plan(gen, 5, 8)
        for ld_s, off in ((8, 0), (12, 0), (5, 0), (8, 2), (7, 0)):
            check_scatter_mx(lib, N_, fmt, x, row_of, ld_s, off)


@pytest.mark.parametrize("fmt", FORMATS)
def test_scatter_op(N_, fmt):
    """fp8_moe_scatter_quantize(scale=...) -> (q, uint8 scales (T k, round_up(K/32, 4))) whose named rows the grouped GEMM reads in place"""
    gen = torch.Generator().manual_seed(33)
    T, k, K = 7, 3, 160
    x = tokens(gen, T, K, torch.bfloat16)
    row_of = torch.randperm(T * k, generator=gen).reshape(T, k).to(torch.int32)
    q, sc = N_.fp8_moe_scatter_quantize(x, row_of, fmt)
    assert sc.dtype == torch.uint8 and tuple(sc.shape) == (T * k, 8) and q.shape[0] == T * k
    wq, ws = quantize(N_, fmt, x)
    tok = torch.arange(T).repeat_interleave(k).to(DEV)
    rows = row_of.reshape(-1).long().to(DEV)
    assert torch.equal(q.view(torch.uint8)[rows], wq[tok]) and torch.equal(sc[rows, :5], ws[tok]) and bool((sc[:, 5:] == 0x7F).all())


# ---- the experts' layers -------------------------------------------------------------------------------------------------------------------

class Layer:
    """G experts of a gated MLP (K -> 2H -> N) with MX-quantised weights: (w1_q, w1_s, w2_q, w2_s) per format"""

    def __init__(self, N_, G, K=256, H=128, N=160, seed=3):
        gen = torch.Generator().manual_seed(seed)
        W1 = (torch.randn((G, 2 * H, K), generator=gen) * K ** -0.5).to(DEV)
        W2 = (torch.randn((G, N, H), generator=gen) * H ** -0.5).to(DEV)
        self.G, self.K, self.H, self.N = G, K, H, N
        self.w = {}
        for fmt in FORMATS:
            q1, s1 = quantize(N_, fmt, W1.reshape(G * 2 * H, K))
            q2, s2 = quantize(N_, fmt, W2.reshape(G * N, H))
            self.w[fmt] = (q1.reshape(G, 2 * H, -1), s1.reshape(G, 2 * H, -1), q2.reshape(G, N, -1), s2.reshape(G, N, -1))
        self.bias1 = torch.randn((G, 2 * H), generator=gen).to(DEV)
        self.bias2 = torch.randn((G, N), generator=gen).to(DEV)


@pytest.fixture(scope="module")
def layers(N_):
    return {G: Layer(N_, G) for G in (8, 64)}


def mlp_by_hand(N_, fmt, layer, xs, offs, dtype, bias=False, linear=False):
    """the per-expert loop of the single-problem ops on the fixed tile over rows sorted by expert; rows no expert owns stay zero"""
    w1_q, w1_s, w2_q, w2_s = layer.w[fmt]
    mm = single_op(N_, fmt)
    y = torch.zeros((xs.shape[0], 2 * layer.H if linear else layer.N), dtype=dtype, device=DEV)
    start = 0
    for g, end in enumerate(int(o) for o in offs):
        if end > start:
            xq, xsc = (N_.fp8_quantize_mxfp4 if fmt == "mxfp4" else N_.fp8_quantize_mxfp8)(xs[start:end])
            h = mm(xq, w1_q[g], xsc, w1_s[g], bias=layer.bias1[g] if bias else None, out_dtype=dtype, kernel=TILE, split_k=1)
            if linear:
                y[start:end] = h
            else:
                hq, hs = N_.fp8_act_quantize(h, "silu", True, fmt)
                y[start:end] = mm(hq, w2_q[g], hs, w2_s[g], bias=layer.bias2[g] if bias else None, out_dtype=dtype, kernel=TILE, split_k=1)
        start = end
    return y


@pytest.mark.parametrize("fmt", FORMATS)
def test_moe_linear_and_mlp_equal_the_per_expert_loop(N_, layers, fmt):
    layer = layers[8]
    gen = torch.Generator().manual_seed(41)
    sizes = [0, 33, 1, 64, 0, 31, 40, 2]
    offs = torch.cumsum(torch.tensor(sizes), 0).to(torch.int32)
    M = int(offs[-1]) + 5
    x = torch.randn((M, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    w1_q, w1_s, w2_q, w2_s = layer.w[fmt]
    linear = N_.fp8_moe_linear_mxfp4 if fmt == "mxfp4" else N_.fp8_moe_linear_mxfp8
    mlp = N_.fp8_moe_mlp_mxfp4 if fmt == "mxfp4" else N_.fp8_moe_mlp_mxfp8
    own = int(offs[-1])
    with L.kernel_timer(8) as kt:
        got = linear(x, offs.to(DEV), w1_q, w1_s, bias=layer.bias1, kernel=TILE)
    assert len(kt.ms) == 2 and got.dtype == torch.bfloat16
    assert torch.equal(bits(got[:own]), bits(mlp_by_hand(N_, fmt, layer, x, offs, torch.bfloat16, bias=True, linear=True)[:own]))
    for bias in (False, True):
        with L.kernel_timer(8) as kt:
            got = mlp(x, offs.to(DEV), w1_q, w1_s, w2_q, w2_s, bias1=layer.bias1 if bias else None, bias2=layer.bias2 if bias else None, kernel=TILE)
        assert len(kt.ms) == 4
        assert torch.equal(bits(got[:own]), bits(mlp_by_hand(N_, fmt, layer, x, offs, torch.bfloat16, bias=bias)[:own]))


# ---- forward -------------------------------------------------------------------------------------------------------------------------------

def forward_op(N_, fmt):
    return N_.fp8_moe_forward_mxfp4 if fmt == "mxfp4" else N_.fp8_moe_forward_mxfp8


def forward_by_hand(N_, fmt, layer, x, ids, wts, bias=False):
    k = ids.shape[1]
    offs, row_of, src = route_ref(ids, layer.G)
    xs = x[(src.clamp(min=0) // k).long().to(DEV)]
    y = mlp_by_hand(N_, fmt, layer, xs, offs, x.dtype, bias=bias)
    return combine_ref(y[:int(offs[-1])], row_of.reshape(ids.shape), wts, x.dtype)


@pytest.mark.parametrize("T", [1, 64, 200, 300])
@pytest.mark.parametrize("G", [8, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_equals_the_chain_by_hand(N_, layers, fmt, G, T):
    gen = torch.Generator().manual_seed(100 * T + G)
    layer, k = layers[G], 4
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids, wts = gate(gen, T, k, G)
    with L.kernel_timer(16) as kt:
        got = forward_op(N_, fmt)(x, ids.to(DEV), wts.to(DEV), *layer.w[fmt], kernel=TILE)
    torch.cuda.synchronize()
    assert len(kt.ms) == (6 if T * k <= SINGLE else 8)   # T = 300 (1200 assignments): the three-launch route, eight launches
    assert torch.equal(bits(got.cpu()), bits(forward_by_hand(N_, fmt, layer, x, ids, wts)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_skewed_dropped_and_empty(N_, layers, fmt):
    gen = torch.Generator().manual_seed(7)
    layer, T, k = layers[8], 64, 4
    fwd = forward_op(N_, fmt)
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    # one expert takes most rows, several are empty; some assignments dropped; biases
    ids = torch.where(torch.rand((T, k), generator=gen) < 0.8, torch.tensor(5), torch.randint(0, 3, (T, k), generator=gen))
    ids = torch.where(torch.rand((T, k), generator=gen) < 0.1, torch.tensor(-1), ids)
    wts = torch.softmax(torch.randn((T, k), generator=gen), dim=1)
    got = fwd(x, ids.to(DEV), wts.to(DEV), *layer.w[fmt], bias1=layer.bias1, bias2=layer.bias2, kernel=TILE)
    assert torch.equal(bits(got.cpu()), bits(forward_by_hand(N_, fmt, layer, x, ids, wts, bias=True)))
    # every id dropped: +0 everywhere
    none = fwd(x, torch.full((T, k), -1).to(DEV), wts.to(DEV), *layer.w[fmt], kernel=TILE)
    assert tuple(none.shape) == (T, layer.N) and bool((bits(none) == 0).all())
    # no tokens
    empty = fwd(x[:0], ids[:0].to(DEV), wts[:0].to(DEV), *layer.w[fmt], kernel=TILE)
    assert tuple(empty.shape) == (0, layer.N) and empty.dtype == torch.bfloat16


@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_captured_into_a_graph_follows_a_new_routing_on_replay(N_, layers, fmt):
    gen = torch.Generator().manual_seed(6)
    layer, T, k = layers[64], 3, 8
    fwd = forward_op(N_, fmt)
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    (ids1, wts1), (ids2, wts2) = gate(gen, T, k, 64), gate(gen, T, k, 64)
    ids, wts = ids1.to(DEV), wts1.to(DEV)
    eager1 = fwd(x, ids, wts, *layer.w[fmt], kernel=TILE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a host sync or a read of the routing inside the capture would fail it)
        out = fwd(x, ids, wts, *layer.w[fmt], kernel=TILE)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager1))
    ids.copy_(ids2.to(DEV))
    wts.copy_(wts2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(forward_by_hand(N_, fmt, layer, x, ids2, wts2)))
    assert not torch.equal(bits(out), bits(eager1))
