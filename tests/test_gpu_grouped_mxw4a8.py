"""GPU (MI355X): the grouped MXW4A8 GEMM (fp8mi_scaled_mm_grouped_mxw4a8) and the MoE ops on the recipe - fp8_moe_linear / _mlp / _forward
_mxw4a8 and fp8_moe_layer(recipe="mxw4a8") (include/fp8mi.h).

Grouped GEMM, per case: (a) every group's rows equal, bit for bit (a NaN matches a NaN), fp8_scaled_mm_mxw4a8 on those rows with the same
ring tile and split_k = 1, under either nan_mode; (b) the rows behind offs[-1] and the guard rows around C keep a sentinel; (c) the float64
product of the decoded operands per group under the matrix-core bar, |gpu - exact| <= 1e-3 sum |a 2^sa| |b 2^sb|.
MoE ops: bit-equal to the per-expert chain of the single-problem ops run by hand."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
from grouped_ref import DEV, MFMA_TOL, SENTINEL, TILE_DIMS, TILES, assert_untouched, clamped_groups, guarded, rand_bytes, t
from grouped_mx_ref import pad4, same_bits
from moe_route_gpu_util import TILE, bits, gate
from moe_route_ref import combine_ref, route_ref
from mxw4a8_ref import mm_ref

pytestmark = pytest.mark.gpu

N = 72


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


class Case:
    """A (M_total, K) e4m3 bytes, B (G, N, K / 2) e2m1 pairs, E8M0 scales in rows of pad4(K / 32) bytes (pad bytes 0x7F), the blocks random
    in 120 .. 134; `tail` unowned rows behind the last group.  Made once, never modified."""

    def __init__(self, offs, m_total, n, K, seed):
        rng = np.random.default_rng(seed)
        self.offs_np = np.asarray(offs, dtype=np.int32)
        self.G, self.n, self.K, self.m_total = len(offs), n, K, m_total
        self.nb, self.ld_s = K // 32, pad4(K // 32)
        G, M, nb = self.G, m_total, self.nb
        self.A_np = rand_bytes(rng, (M, K))
        self.B_np = rng.integers(0, 256, size=(G, n, K // 2), dtype=np.uint8)
        self.sa_np = np.full((M, self.ld_s), 0x7F, dtype=np.uint8)
        self.sb_np = np.full((G, n, self.ld_s), 0x7F, dtype=np.uint8)
        self.sa_np[:, :nb] = rng.integers(120, 135, (M, nb), dtype=np.uint8)
        self.sb_np[:, :, :nb] = rng.integers(120, 135, (G, n, nb), dtype=np.uint8)
        self.groups = clamped_groups(self.offs_np, m_total)
        # NaN bytes in A on both sides of the first boundary between two non-empty groups: the two nan modes differ
        owned = [g for g, (s, e) in enumerate(self.groups) if e > s]
        if len(owned) >= 2:
            self.A_np[self.groups[owned[0]][1] - 1, 5] = 0x7F
            self.A_np[self.groups[owned[1]][0], K - 3] = 0xFF
        self.A, self.B, self.sa, self.sb, self.offs = t(self.A_np), t(self.B_np), t(self.sa_np), t(self.sb_np), t(self.offs_np)


def sizes_for(G, bm):
    """group sizes that include 0, 1, BM - 1 and BM + 1; G = 9 goes past the batch of eight of the offs walk"""
    return [bm - 1, 0, bm + 1] if G == 3 else [bm + 1, 0, 1, bm - 1, 7, 0, bm, 33, 2]


def run_and_compare(N_, c, tile, nan_mode, out_dtype=torch.float32, groups=None):
    groups = c.groups if groups is None else groups
    buf, C = guarded(out_dtype, c.m_total, c.n)
    got = N_.fp8_scaled_mm_grouped_mxw4a8(c.A, c.B, c.sa[:, :c.nb], c.sb[:, :, :c.nb], c.offs, out_dtype=out_dtype, kernel=tile, out=C, nan_mode=nan_mode)
    assert got is C
    for g, (s, e) in enumerate(groups):
        if e > s:
            want = N_.fp8_scaled_mm_mxw4a8(c.A[s:e], c.B[g], c.sa[s:e, :c.nb], c.sb[g][:, :c.nb], out_dtype=out_dtype, kernel=tile, split_k=1,
                                           nan_mode=nan_mode)
            assert same_bits(C[s:e], want), (tile, nan_mode, g, s, e)
    assert_untouched(buf, c.n, groups)
    return C


def check_f64(c, C, nan_zero):
    got = C.float().cpu().numpy().astype(np.float64)
    for g, (s, e) in enumerate(c.groups):
        if e > s:
            exact, bound = mm_ref(c.A_np[s:e], c.B_np[g], c.sa_np[s:e, :c.nb], c.sb_np[g][:, :c.nb], nan_zero)
            nan = np.isnan(exact)
            assert np.array_equal(np.isnan(got[s:e]), nan), (g, "NaN rows")
            err = np.abs(got[s:e] - exact)[~nan]
            assert np.all(err <= MFMA_TOL * bound[~nan] + 1e-30), f"group {g}: max err / bound {np.max(err / (bound[~nan] + 1e-300)):.3e}"


@pytest.mark.parametrize("K", [544, 2048])
@pytest.mark.parametrize("tile", TILES)
def test_groups_equal_the_single_problem_call_and_the_float64_product(N_, tile, K):
    bm = TILE_DIMS[tile][0]
    for G in (3, 9):
        sizes = sizes_for(G, bm)
        offs = np.cumsum(sizes)
        c = Case(offs, int(offs[-1]) + 3, N, K, seed=1000 * tile + 10 * G + K)
        for nan_mode in (L.NAN_ZERO, L.NAN_PROPAGATE):
            C = run_and_compare(N_, c, tile, nan_mode)
            check_f64(c, C, nan_mode == L.NAN_ZERO)
            assert bool(torch.isnan(C[:int(offs[-1])]).any()) == (nan_mode == L.NAN_PROPAGATE)


@pytest.mark.parametrize("tile", [L.KERNEL_GEMM_32x64, L.KERNEL_GEMM_128x64])
def test_a_non_monotone_offs_touches_nothing_outside_the_rows(N_, tile):
    """offs that go back, and one past M_total: the groups are the clamped ones of the definition; nothing outside the M_total rows is written"""
    m_total = 150
    offs = [40, 10, 300, 50]      # -> [0, 40) [40, 40) [40, 150) [150, 150)
    c = Case(offs, m_total, N, 544, seed=7)
    assert c.groups == [(0, 40), (40, 40), (40, 150), (150, 150)]
    C = run_and_compare(N_, c, tile, L.NAN_ZERO, torch.bfloat16)
    assert not bool(torch.isnan(C).any())


def test_auto_runs_the_tile_the_chooser_names(N_):
    bm = 32
    offs = np.cumsum(sizes_for(9, bm))
    c = Case(offs, int(offs[-1]), N, 544, seed=11)
    tile = L.load().fp8mi_choose_kernel_grouped_mxw4a8(c.G, c.m_total, N, c.K, c.K, c.K // 2, N, L.F32)
    assert tile in TILES
    buf, C = guarded(torch.float32, c.m_total, N)
    N_.fp8_scaled_mm_grouped_mxw4a8(c.A, c.B, c.sa[:, :c.nb], c.sb[:, :, :c.nb], c.offs, kernel=L.KERNEL_AUTO, out=C)
    want = run_and_compare(N_, c, tile, None)
    assert same_bits(C, want)


# ---- the MoE ops ---------------------------------------------------------------------------------------------------------------------------

class Layer:
    """G experts of a gated MLP (K -> 2H -> N) with MXFP4-quantised weights"""

    def __init__(self, N_, G=4, K=256, H=128, Nout=160, seed=3):
        gen = torch.Generator().manual_seed(seed)
        W1 = (torch.randn((G, 2 * H, K), generator=gen) * K ** -0.5).to(DEV)
        W2 = (torch.randn((G, Nout, H), generator=gen) * H ** -0.5).to(DEV)
        self.G, self.K, self.H, self.N = G, K, H, Nout
        q1, s1 = N_.fp8_quantize_mxfp4(W1.reshape(G * 2 * H, K))
        q2, s2 = N_.fp8_quantize_mxfp4(W2.reshape(G * Nout, H))
        u8 = lambda x: x.view(torch.uint8)   # noqa: E731
        self.w = (u8(q1).reshape(G, 2 * H, -1), u8(s1).reshape(G, 2 * H, -1), u8(q2).reshape(G, Nout, -1), u8(s2).reshape(G, Nout, -1))
        self.bias1 = torch.randn((G, 2 * H), generator=gen).to(DEV)
        self.bias2 = torch.randn((G, Nout), generator=gen).to(DEV)


@pytest.fixture(scope="module")
def layer(N_):
    return Layer(N_)


def mlp_by_hand(N_, layer, xs, offs, dtype, bias=False, linear=False):
    """the per-expert loop of the single-problem ops on the fixed tile over rows sorted by expert; rows no expert owns stay zero"""
    w1_q, w1_s, w2_q, w2_s = layer.w
    mm = N_.fp8_scaled_mm_mxw4a8
    y = torch.zeros((xs.shape[0], 2 * layer.H if linear else layer.N), dtype=dtype, device=DEV)
    start = 0
    for g, end in enumerate(int(o) for o in offs):
        if end > start:
            xq, xsc = N_.fp8_quantize_mxfp8(xs[start:end])
            h = mm(xq, w1_q[g], xsc, w1_s[g], bias=layer.bias1[g] if bias else None, out_dtype=dtype, kernel=TILE, split_k=1)
            if linear:
                y[start:end] = h
            else:
                hq, hs = N_.fp8_act_quantize(h, "silu", True, "mxfp8")
                y[start:end] = mm(hq, w2_q[g], hs, w2_s[g], bias=layer.bias2[g] if bias else None, out_dtype=dtype, kernel=TILE, split_k=1)
        start = end
    return y


def test_moe_linear_and_mlp_equal_the_per_expert_loop(N_, layer):
    gen = torch.Generator().manual_seed(41)
    sizes = [0, 33, 1, 64]
    offs = torch.cumsum(torch.tensor(sizes), 0).to(torch.int32)
    own = int(offs[-1])
    x = torch.randn((own + 5, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    w1_q, w1_s, w2_q, w2_s = layer.w
    with L.kernel_timer(8) as kt:
        got = N_.fp8_moe_linear_mxw4a8(x, offs.to(DEV), w1_q, w1_s, bias=layer.bias1, kernel=TILE)
    assert len(kt.ms) == 2 and got.dtype == torch.bfloat16
    assert torch.equal(bits(got[:own]), bits(mlp_by_hand(N_, layer, x, offs, torch.bfloat16, bias=True, linear=True)[:own]))
    for bias in (False, True):
        with L.kernel_timer(8) as kt:
            got = N_.fp8_moe_mlp_mxw4a8(x, offs.to(DEV), w1_q, w1_s, w2_q, w2_s, bias1=layer.bias1 if bias else None,
                                        bias2=layer.bias2 if bias else None, kernel=TILE)
        assert len(kt.ms) == 4
        assert torch.equal(bits(got[:own]), bits(mlp_by_hand(N_, layer, x, offs, torch.bfloat16, bias=bias)[:own]))
    # ... and the dense op itself, expert by expert (K = 256: no split-K, and every unsplit tile gives the same bits)
    start = 0
    for g, end in enumerate(int(o) for o in offs):
        if end > start:
            want = N_.fp8_mlp_mxw4a8(x[start:end], w1_q[g], w1_s[g], w2_q[g], w2_s[g], bias1=layer.bias1[g], bias2=layer.bias2[g])
            assert torch.equal(bits(got[start:end]), bits(want)), g
        start = end


def forward_by_hand(N_, layer, x, ids, wts, bias=False):
    k = ids.shape[1]
    offs, row_of, src = route_ref(ids, layer.G)
    xs = x[(src.clamp(min=0) // k).long().to(DEV)]
    y = mlp_by_hand(N_, layer, xs, offs, x.dtype, bias=bias)
    return combine_ref(y[:int(offs[-1])], row_of.reshape(ids.shape), wts, x.dtype)


def test_forward_equals_the_chain_by_hand_with_a_dropped_id(N_, layer):
    gen = torch.Generator().manual_seed(5)
    T, k = 5, 2
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    ids, wts = gate(gen, T, k, layer.G)
    ids[2, 1] = -1                      # one assignment dropped
    with L.kernel_timer(16) as kt:
        got = N_.fp8_moe_forward_mxw4a8(x, ids.to(DEV), wts.to(DEV), *layer.w, kernel=TILE)
    torch.cuda.synchronize()
    assert len(kt.ms) == 6
    assert torch.equal(bits(got.cpu()), bits(forward_by_hand(N_, layer, x, ids, wts)))
    got = N_.fp8_moe_forward_mxw4a8(x, ids.to(DEV), wts.to(DEV), *layer.w, bias1=layer.bias1, bias2=layer.bias2, kernel=TILE)
    assert torch.equal(bits(got.cpu()), bits(forward_by_hand(N_, layer, x, ids, wts, bias=True)))
    # no tokens: the empty tensor without a launch
    with L.kernel_timer(4) as kt:
        empty = N_.fp8_moe_forward_mxw4a8(x[:0], ids[:0].to(DEV), wts[:0].to(DEV), *layer.w, kernel=TILE)
    assert len(kt.ms) == 0 and tuple(empty.shape) == (0, layer.N) and empty.dtype == torch.bfloat16


def test_forward_captured_into_a_graph_follows_new_ids_on_replay(N_, layer):
    gen = torch.Generator().manual_seed(6)
    T, k = 5, 2
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    (ids1, wts1), (ids2, wts2) = gate(gen, T, k, layer.G), gate(gen, T, k, layer.G)
    ids, wts = ids1.to(DEV), wts1.to(DEV)
    eager1 = N_.fp8_moe_forward_mxw4a8(x, ids, wts, *layer.w, kernel=TILE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a host sync or a read of the routing inside the capture would fail it)
        out = N_.fp8_moe_forward_mxw4a8(x, ids, wts, *layer.w, kernel=TILE)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager1))
    ids.copy_(ids2.to(DEV))
    wts.copy_(wts2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager2 = N_.fp8_moe_forward_mxw4a8(x, ids, wts, *layer.w, kernel=TILE)
    assert torch.equal(bits(out), bits(eager2))
    assert torch.equal(bits(out.cpu()), bits(forward_by_hand(N_, layer, x, ids2, wts2)))
    assert not torch.equal(bits(out), bits(eager1))


def test_moe_layer_equals_gate_plus_forward(N_, layer):
    gen = torch.Generator().manual_seed(8)
    T, k = 5, 2
    x = torch.randn((T, layer.K), generator=gen).to(torch.bfloat16).to(DEV)
    logits = torch.randn((T, layer.G), generator=gen).to(DEV)
    with L.kernel_timer(16) as kt:
        got = N_.fp8_moe_layer(x, logits, k, *layer.w, recipe="mxw4a8", renormalize=True, kernel=TILE)
    assert len(kt.ms) == 7
    ids, wts = N_.fp8_moe_gate(logits, k, renormalize=True)
    want = N_.fp8_moe_forward_mxw4a8(x, ids, wts, *layer.w, kernel=TILE)
    assert torch.equal(bits(got), bits(want))
