#!/usr/bin/env python3
"""tools/time_moe_route.py for the MX recipes: fp8_moe_scatter_quantize(scale="mxfp8" | "mxfp4") and fp8_moe_forward_mxfp8 / _mxfp4, each
against what a caller has without them, on the same device in the same run:
  scatter-quantise  index_select of the (T, K) activations into (T k, K) + fp8_quantize_mxfp8 / _mxfp4 over T k rows
  forward           torch.sort + bincount + cumsum, the group sizes copied to the HOST (a sync), index_select, fp8_quantize_mx* over T k rows,
                    then a Python loop over the experts - fp8_scaled_mm_mx*, fp8_act_quantize(scale=...), fp8_scaled_mm_mx* per non-empty
                    expert - and index_select, mul, sum for the combine: the loop DESIGN.md 5.10 was written to remove
Sizes: T in {64, 1024} tokens, k = 8, G in {8, 64} experts, K = N = 7168, H = 2048 (gated silu), bf16, AUTO tiles on both sides.

Both sides go through the op layer, ALTERNATING call by call after warm-up; median of --iters (>= 20); the clocks, the launch counts and the byte
fraction of the scatter ((esz + k) T K bytes for MXFP8, (esz + k / 2) T K for MXFP4, scale bytes aside) are tools/time_moe_route.py's.
    python tools/time_moe_mx.py [--iters 30] [--no-forward]"""
import argparse

import torch

from time_moe_route import H, KK, NN, TOP_K, N, bracket, chain_launches, measure, med

TOKENS = (64, 1024)
EXPERTS = (8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--ceiling", type=float, default=6.2e12, help="bytes per second the byte counts are compared with")
    ap.add_argument("--no-forward", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    empty = [bracket(lambda: None) for _ in range(50)]
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    print(f"{torch.cuda.get_device_name(0)}; k = {TOP_K}, K = N = {KK}, bf16 (forward: H = {H}, gated silu, AUTO tiles); times in us, median of {a.iters} "
          f"alternating calls; empty bracket {ovh:.2f} us (subtracted from the stream columns); byte fractions against {a.ceiling / 1e12:.1f} TB/s")
    print(f"{'op':>22s} {'T':>5s} {'G':>4s} | {'our kernels':>11s} {'of ceiling':>10s} {'launches':>8s} | {'our stream':>10s} {'chain stream':>12s} {'ratio':>6s} "
          f"{'chain launches':>14s}")

    def row(op, T, G, kern, launches, so, sc, nbytes, chain_n):
        frac = f"{nbytes / (kern * 1e-6) / a.ceiling:10.3f}" if nbytes else f"{'':>10s}"
        print(f"{op:>22s} {T:5d} {G:4d} | {kern:11.2f} {frac} {launches:8d} | {so:10.2f} {sc:12.2f} {so / sc:6.3f} {chain_n:>14s}", flush=True)

    for G in EXPERTS:
        for fmt in ("mxfp8", "mxfp4"):
            per = 2 if fmt == "mxfp4" else 1
            quant = N.fp8_quantize_mxfp4 if per == 2 else N.fp8_quantize_mxfp8
            mm = N.fp8_scaled_mm_mxfp4 if per == 2 else N.fp8_scaled_mm_mxfp8
            fwd = N.fp8_moe_forward_mxfp4 if per == 2 else N.fp8_moe_forward_mxfp8
            if not a.no_forward:
                w1 = torch.randint(0, 0x7F, (G, 2 * H, KK // per), device=dev, generator=gen, dtype=torch.uint8)
                w2 = torch.randint(0, 0x7F, (G, NN, H // per), device=dev, generator=gen, dtype=torch.uint8)
                s1 = torch.randint(112, 120, (G, 2 * H, KK // 32), device=dev, generator=gen, dtype=torch.uint8)
                s2 = torch.randint(112, 120, (G, NN, H // 32), device=dev, generator=gen, dtype=torch.uint8)
            for T in TOKENS:
                x = torch.randn((T, KK), device=dev, generator=gen).to(torch.bfloat16)
                ids = torch.topk(torch.rand((T, G), device=dev, generator=gen), TOP_K, dim=1).indices
                wts = torch.softmax(torch.randn((T, TOP_K), device=dev, generator=gen), dim=1)
                _offs, row_of, src = N.fp8_moe_route(ids, G)
                toks = (src // TOP_K).long()

                def chain_scatter():
                    return quant(x.index_select(0, toks))

                q, s = N.fp8_moe_scatter_quantize(x, row_of, fmt)
                cq, cs = chain_scatter()
                assert torch.equal(q.view(torch.uint8), cq.view(torch.uint8)) and torch.equal(s[:, :KK // 32], cs.view(torch.uint8)), \
                    "the chain and fp8_moe_scatter_quantize differ"
                k, n, so, sc = measure(lambda: N.fp8_moe_scatter_quantize(x, row_of, fmt), chain_scatter, a.iters, ovh)
                row(f"scatter-quantise {fmt}", T, G, k, n, so, sc, (2 * per + TOP_K) * T * KK // per, chain_launches(chain_scatter))
                if a.no_forward:
                    continue

                def ours_forward():
                    return fwd(x, ids, wts, w1, s1, w2, s2)

                def chain_forward():
                    flat = ids.reshape(-1)
                    _sorted, order = torch.sort(flat, stable=True)
                    ends = torch.cumsum(torch.bincount(flat, minlength=G), 0).tolist()   # the host sync of the loop
                    inverse = torch.empty_like(order)
                    inverse[order] = torch.arange(order.numel(), device=dev)
                    xq, xs = quant(x.index_select(0, order // TOP_K))
                    out = torch.empty((order.numel(), NN), device=dev, dtype=torch.bfloat16)
                    start = 0
                    for g, end in enumerate(ends):
                        if end > start:
                            h = mm(xq[start:end], w1[g], xs[start:end], s1[g], out_dtype=torch.bfloat16)
                            hq, hs = N.fp8_act_quantize(h, "silu", True, fmt)
                            mm(hq, w2[g], hs, s2[g], out_dtype=torch.bfloat16, out=out[start:end])
                        start = end
                    return (out.index_select(0, inverse).view(T, TOP_K, NN) * wts[:, :, None]).sum(1).to(torch.bfloat16)

                k, n, so, sc = measure(ours_forward, chain_forward, a.iters, ovh)
                row(f"forward {fmt}", T, G, k, n, so, sc, 0, chain_launches(chain_forward))
            if not a.no_forward:
                del w1, w2


if __name__ == "__main__":
    main()
