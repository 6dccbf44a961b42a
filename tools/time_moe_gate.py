#!/usr/bin/env python3
"""Times the MoE gate - fp8_moe_gate, and fp8_moe_layer which starts with it - against the torch chain it replaces, on the same device in the
same run:
  softmax      torch.softmax (float32) + topk + sum + div (+ the cast of the ids to int32): plain softmax top-k, renormalised
  v3           the DeepSeek-V3 gate: sigmoid, + bias, view / topk(2) / sum for the group scores, topk over the groups, scatter for the mask,
               expand / masked_fill, topk, gather of the unbiased scores, sum, div, mul by 2.5, the cast of the ids (G = 256: 8 groups, 4 kept)
  layer        fp8_moe_layer (v3 gate, rowwise recipe) against fp8_moe_forward_rowwise fed by that chain; T = 64 and 1024, G = 256, H = 2048
Sizes: T in {64, 1024, 8192} tokens, G in {8, 64, 256} experts, k = 8 (k = 2 at G = 8), bf16 logits.

Both sides are called ALTERNATING call by call after warm-up; median of --iters (>= 20).  Clocks:
  kernels   ours only: the sum of the launches' own durations (fp8mi_profile_begin / _end: the dispatch packets' timestamps);
  stream    two events around the candidate's calls: what the stream is busy for, launch gaps included, less the interval the same bracket
            measures around nothing (printed as `empty bracket`).
Launch counts: ours from the profile hook; the chain's from one torch.profiler pass (`n/a` if the profiler is not usable).  `same ids`: the
share of tokens for which the chain selects the same set of experts (ties and float32 rounding of the scores may differ).
    python tools/time_moe_gate.py [--iters 30] [--no-layer] [--no-chain-count]"""
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
TOKENS = (64, 1024, 8192)
EXPERTS = (8, 64, 256)
V3 = dict(scoring="sigmoid", renormalize=True, scale=2.5, n_group=8, topk_group=4, group_score="top2")


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


def chain_softmax(logits, k):
    w, ids = torch.softmax(logits.float(), dim=-1).topk(k, dim=-1)
    return ids.to(torch.int32), w / (w.sum(dim=-1, keepdim=True) + 1e-20)


def chain_v3(logits, bias, k):
    T, G = logits.shape
    n_group, topk_group = V3["n_group"], V3["topk_group"]
    s = torch.sigmoid(logits.float())
    keys = s + bias
    group_scores = keys.view(T, n_group, -1).topk(2, dim=-1).values.sum(dim=-1)
    group_ids = group_scores.topk(topk_group, dim=-1, sorted=False).indices
    mask = torch.zeros_like(group_scores).scatter_(1, group_ids, 1.0)
    mask = mask.unsqueeze(-1).expand(T, n_group, G // n_group).reshape(T, G)
    ids = keys.masked_fill(mask == 0, float("-inf")).topk(k, dim=-1).indices
    w = s.gather(1, ids)
    return ids.to(torch.int32), w / (w.sum(dim=-1, keepdim=True) + 1e-20) * V3["scale"]


def same_sets(a, b):
    return float((a.sort(dim=1).values == b.sort(dim=1).values).all(dim=1).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--no-chain-count", action="store_true", help="skip the torch.profiler pass that counts the chain's launches")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    empty = [bracket(lambda: None) for _ in range(50)]
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    print(f"{torch.cuda.get_device_name(0)}; bf16 logits, k = 8 (2 at G = 8); layer: K = N = {KK}, H = {H}, gated silu, rowwise recipe, AUTO tile; times in us, "
          f"median of {a.iters} alternating calls; empty bracket {ovh:.2f} us (subtracted from the stream columns)")
    print(f"{'op':>14s} {'T':>5s} {'G':>4s} | {'our kernels':>11s} {'launches':>8s} | {'our stream':>10s} {'chain stream':>12s} {'ratio':>6s} {'chain launches':>14s} "
          f"{'same ids':>8s}")

    def row(op, T, G, kern, launches, so, sc, chain_n, same):
        print(f"{op:>14s} {T:5d} {G:4d} | {kern:11.2f} {launches:8d} | {so:10.2f} {sc:12.2f} {so / sc:6.3f} {chain_n:>14s} {same:8.4f}", flush=True)

    def count(fn):
        return chain_launches(fn, a.no_chain_count)

    for G in EXPERTS:
        k = 2 if G == 8 else 8
        bias = 0.1 * torch.randn((G,), device=dev, generator=gen)
        for T in TOKENS:
            logits = (2.0 * torch.randn((T, G), device=dev, generator=gen)).to(torch.bfloat16)
            ours = lambda: N.fp8_moe_gate(logits, k, "softmax", True)   # noqa: E731
            chain = lambda: chain_softmax(logits, k)                     # noqa: E731
            same = same_sets(ours()[0], chain()[0])
            kern, n, so, sc = measure(ours, chain, a.iters, ovh)
            row("gate softmax", T, G, kern, n, so, sc, count(chain), same)
            if G != 256:
                continue
            ours = lambda: N.fp8_moe_gate(logits, k, bias=bias, **V3)    # noqa: E731
            chain = lambda: chain_v3(logits, bias, k)                    # noqa: E731
            same = same_sets(ours()[0], chain()[0])
            kern, n, so, sc = measure(ours, chain, a.iters, ovh)
            row("gate v3", T, G, kern, n, so, sc, count(chain), same)
    if a.no_layer:
        return
    G, k = 256, 8
    w1 = torch.randint(0, 0x7F, (G, 2 * H, KK), device=dev, generator=gen, dtype=torch.uint8)
    w2 = torch.randint(0, 0x7F, (G, NN, H), device=dev, generator=gen, dtype=torch.uint8)
    s1 = (torch.rand((G, 2 * H), device=dev, generator=gen) + 0.5) * 1e-3
    s2 = (torch.rand((G, NN), device=dev, generator=gen) + 0.5) * 1e-3
    bias = 0.1 * torch.randn((G,), device=dev, generator=gen)
    for T in (64, 1024):
        x = torch.randn((T, KK), device=dev, generator=gen).to(torch.bfloat16)
        logits = (2.0 * torch.randn((T, G), device=dev, generator=gen)).to(torch.bfloat16)
        ours = lambda: N.fp8_moe_layer(x, logits, k, w1, s1, w2, s2, "rowwise", bias=bias, **V3)          # noqa: E731
        chain = lambda: N.fp8_moe_forward_rowwise(x, *chain_v3(logits, bias, k), w1, s1, w2, s2)          # noqa: E731
        same = same_sets(N.fp8_moe_gate(logits, k, bias=bias, **V3)[0], chain_v3(logits, bias, k)[0])
        kern, n, so, sc = measure(ours, chain, a.iters, ovh)
        row("layer v3", T, G, kern, n, so, sc, count(chain), same)


if __name__ == "__main__":
    main()
