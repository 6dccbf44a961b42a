#!/usr/bin/env python3
"""Times the MoE routing ops - fp8_moe_route, fp8_moe_scatter_quantize, fp8_moe_combine and fp8_moe_forward_rowwise - each against the torch
chain it replaces, on the same device in the same run:
  route             torch.sort(stable=True) + torch.bincount + torch.cumsum (+ the cast of offs to int32)
  scatter-quantise  index_select of the (T, K) activations into (T k, K) + fp8_quantize_rowwise over T k rows
  combine           index_select of the (T k, N) results + mul by the weights + sum over k (+ the cast back to bf16)
  forward           that chain around fp8_moe_mlp_rowwise (sort, bincount, cumsum, inverse permutation, index_select, the four launches of
                    the MLP, index_select, mul, sum)
Sizes: T in {64, 1024, 8192} tokens, k = 8, G in {8, 64, 256} experts, K = N = 7168, bf16; the forward's experts have H = 2048 (gated).

Both sides go through the op layer (the chain IS op-layer code), ALTERNATING call by call after warm-up; median of --iters (>= 20).  Clocks:
  kernels   ours only: the sum of the launches' own durations (fp8mi_profile_begin / _end: the dispatch packets' timestamps);
  stream    two events around the candidate's calls: what the stream is busy for, launch gaps and any host sync included, less the interval
            the same bracket measures around nothing (printed as `empty bracket`).
Launch counts: ours from the profile hook; the chain's from one torch.profiler pass (kernels + memcpys; `n/a` if the profiler is not usable).
Next to the times: scatter-quantise's (esz + k) T K bytes and combine's (k + 1) esz T N bytes over the kernel time, as a fraction of --ceiling
(the swept read ceiling the README quotes, 6.2 TB/s).  The ids are a random top-k (every id valid, experts evenly loaded).
    python tools/time_moe_route.py [--iters 30] [--no-forward] [--no-chain-count]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

KK = NN = 7168
H = 2048
TOP_K = 8
TOKENS = (64, 1024, 8192)
EXPERTS = (8, 64, 256)


def med(v):
    return statistics.median(v)


def bracket(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def chain_launches(fn, skip=False):
    if skip:
        return "n/a"
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return str(n) if n else "n/a"
    except Exception:   # noqa: BLE001 - the count is a courtesy column
        return "n/a"


def measure(ours, chain, iters, ovh, max_launches=16):
    """-> (our kernel us, our launches, our stream us, the chain's stream us): medians of `iters` alternating calls"""
    for _ in range(3):
        ours()
        chain()
    torch.cuda.synchronize()
    k, launches = [], 0
    for _ in range(iters):
        with L.kernel_timer(max_launches) as p:
            ours()
        launches = len(p.ms)
        k.append(sum(p.ms) * 1e3)
        chain()
    torch.cuda.synchronize()
    so, sc = [], []
    for _ in range(iters):
        eo = bracket(ours)
        ec = bracket(chain)
        torch.cuda.synchronize()
        so.append(max(0.0, eo[0].elapsed_time(eo[1]) * 1e3 - ovh))
        sc.append(max(0.0, ec[0].elapsed_time(ec[1]) * 1e3 - ovh))
    return med(k), launches, med(so), med(sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--ceiling", type=float, default=6.2e12, help="bytes per second the byte counts are compared with")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--no-chain-count", action="store_true", help="skip the torch.profiler pass that counts the chain's launches")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    empty = [bracket(lambda: None) for _ in range(50)]
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    print(f"{torch.cuda.get_device_name(0)}; k = {TOP_K}, K = N = {KK}, bf16 (forward: H = {H}, gated silu, AUTO tile); times in us, median of {a.iters} "
          f"alternating calls; empty bracket {ovh:.2f} us (subtracted from the stream columns); byte fractions against {a.ceiling / 1e12:.1f} TB/s")
    print(f"{'op':>16s} {'T':>5s} {'G':>4s} | {'our kernels':>11s} {'of ceiling':>10s} {'launches':>8s} | {'our stream':>10s} {'chain stream':>12s} {'ratio':>6s} "
          f"{'chain launches':>14s}")

    def count(fn):
        return chain_launches(fn, a.no_chain_count)

    def row(op, T, G, kern, launches, so, sc, nbytes, chain_n):
        frac = f"{nbytes / (kern * 1e-6) / a.ceiling:10.3f}" if nbytes else f"{'':>10s}"
        print(f"{op:>16s} {T:5d} {G:4d} | {kern:11.2f} {frac} {launches:8d} | {so:10.2f} {sc:12.2f} {so / sc:6.3f} {chain_n:>14s}", flush=True)

    for G in EXPERTS:
        if not a.no_forward:
            w1 = torch.randint(0, 0x7F, (G, 2 * H, KK), device=dev, generator=gen, dtype=torch.uint8)
            w2 = torch.randint(0, 0x7F, (G, NN, H), device=dev, generator=gen, dtype=torch.uint8)
            s1 = (torch.rand((G, 2 * H), device=dev, generator=gen) + 0.5) * 1e-3
            s2 = (torch.rand((G, NN), device=dev, generator=gen) + 0.5) * 1e-3
        for T in TOKENS:
            x = torch.randn((T, KK), device=dev, generator=gen).to(torch.bfloat16)
            ids = torch.topk(torch.rand((T, G), device=dev, generator=gen), TOP_K, dim=1).indices
            wts = torch.softmax(torch.randn((T, TOP_K), device=dev, generator=gen), dim=1)
            y = torch.randn((T * TOP_K, NN), device=dev, generator=gen).to(torch.bfloat16)
            offs, row_of, src = N.fp8_moe_route(ids, G)
            rows = row_of.reshape(-1).long()
            toks = (src // TOP_K).long()

            def chain_route():
                flat = ids.reshape(-1)
                _sorted, order = torch.sort(flat, stable=True)
                return torch.cumsum(torch.bincount(flat, minlength=G), 0).to(torch.int32), order

            def chain_scatter():
                return N.fp8_quantize_rowwise(x.index_select(0, toks))

            def chain_combine():
                return (y.index_select(0, rows).view(T, TOP_K, NN) * wts[:, :, None]).sum(1).to(torch.bfloat16)

            c_offs, c_order = chain_route()
            assert torch.equal(c_offs, offs) and torch.equal(c_order.to(torch.int32), src), "the chain and fp8_moe_route differ"
            q, s = N.fp8_moe_scatter_quantize(x, row_of)
            cq, cs = chain_scatter()
            assert torch.equal(q, cq) and torch.equal(s, cs), "the chain and fp8_moe_scatter_quantize differ"

            k, n, so, sc = measure(lambda: N.fp8_moe_route(ids, G), chain_route, a.iters, ovh)
            row("route", T, G, k, n, so, sc, 0, count(chain_route))
            k, n, so, sc = measure(lambda: N.fp8_moe_scatter_quantize(x, row_of), chain_scatter, a.iters, ovh)
            row("scatter-quantise", T, G, k, n, so, sc, (2 + TOP_K) * T * KK, count(chain_scatter))
            k, n, so, sc = measure(lambda: N.fp8_moe_combine(y, row_of, wts), chain_combine, a.iters, ovh)
            row("combine", T, G, k, n, so, sc, (TOP_K + 1) * 2 * T * NN, count(chain_combine))
            if a.no_forward:
                continue

            def ours_forward():
                return N.fp8_moe_forward_rowwise(x, ids, wts, w1, s1, w2, s2)

            def chain_forward():
                flat = ids.reshape(-1)
                _sorted, order = torch.sort(flat, stable=True)
                f_offs = torch.cumsum(torch.bincount(flat, minlength=G), 0).to(torch.int32)
                inverse = torch.empty_like(order)
                inverse[order] = torch.arange(order.numel(), device=dev)
                out = N.fp8_moe_mlp_rowwise(x.index_select(0, order // TOP_K), f_offs, w1, s1, w2, s2)
                return (out.index_select(0, inverse).view(T, TOP_K, NN) * wts[:, :, None]).sum(1).to(torch.bfloat16)

            k, n, so, sc = measure(ours_forward, chain_forward, a.iters, ovh)
            row("forward rowwise", T, G, k, n, so, sc, 0, count(chain_forward))
        if not a.no_forward:
            del w1, w2


if __name__ == "__main__":
    main()
