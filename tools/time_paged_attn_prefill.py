#!/usr/bin/env python3
"""Times the LDS-tiled paged attention for prompt chunks (fp8_paged_attention(kernel="tile"): fp8mi_paged_attention_prefill) against the
streaming multi-token kernel (kernel="stream": fp8mi_paged_attention_varlen) on the same inputs, and writes
profiles/paged_attn_prefill_timing.txt.
Shape: Hq / Hkv = 32 / 8 (32 tokens to a workgroup tile, 4 to a streaming one), D = 128, block_size 16, bf16 q and output, num_splits = 0
(each entry's own choice).  Rows: (a) chunked prefill, B = 1, 512 tokens over 8 k; (b) full prefill, B = 4, q_len = seq_len = 2048; (c) B = 8,
128 tokens over 8 k; (d) speculative rows, B = 64, q_len in {4, 8} over 8 k; then a sweep of q_len at B = 8 over 8 k for the crossing.
The two kernels ALTERNATE call by call in this one process; a time is the sum of a call's launches' own durations (fp8mi_profile_begin /
_end: the dispatch packets' timestamps), median of --iters with [min, max].  `below` = the tile entry's [min, max] lies wholly below the
stream entry's.  max|diff| / max|V| compares the two outputs (each is within its bound of the float64 attention).
    python tools/time_paged_attn_prefill.py [--iters 20] [--out profiles/paged_attn_prefill_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
ROWS = [("a", 1, 512, 8192), ("b", 4, 2048, 2048), ("c", 8, 128, 8192), ("d", 64, 4, 8192), ("d", 64, 8, 8192)] + \
       [("sweep", 8, n, 8192) for n in (8, 16, 32, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_attn_prefill_timing.txt"))
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"tools/time_paged_attn_prefill.py on {torch.cuda.get_device_name(0)}: fp8_paged_attention with cu_seqlens_q, Hq / Hkv = {HQ} / {HKV}, D = {D}, "
             f"block_size {BS}, bf16 q and out, num_splits = 0; `tile` and `stream` alternate call by call; times in us per call, median of {a.iters} [min, max]",
             f"{'row':>5s} {'B':>3s} {'q_len':>5s} {'ctx':>5s} | {'kernel':>6s} {'launches':>8s} {'median':>9s} {'min':>9s} {'max':>9s} | {'stream / tile':>13s} {'below':>5s} "
             f"{'max|diff| / max|V|':>18s}"]
    print("\n".join(lines), flush=True)
    for row, B, n, ctx in ROWS:
        nblk = ctx // BS
        nb = B * nblk
        kc = torch.randint(0, 0x78, (nb, HKV, BS, D), dtype=torch.uint8, device=dev, generator=gen)   # |value| < 256, no NaN pattern
        kc |= torch.randint(0, 2, kc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
        vc = torch.randint(0, 0x78, (nb, HKV, D, BS), dtype=torch.uint8, device=dev, generator=gen)
        vc |= torch.randint(0, 2, vc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
        table = torch.randperm(nb, device=dev, generator=gen).to(torch.int32).reshape(B, nblk)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        q = torch.randn((B * n, HQ, D), device=dev, generator=gen).to(torch.bfloat16)
        cu = (torch.arange(B + 1, device=dev) * n).to(torch.int32)
        ks, vs = torch.tensor([0.002], device=dev), torch.tensor([0.01], device=dev)
        forms = {k: (lambda k=k: N.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=ctx, kernel=k, cu_seqlens_q=cu, max_q_len=n))
                 for k in ("tile", "stream")}
        outs = {}
        for name, fn in forms.items():
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        diff = float((outs["tile"].float() - outs["stream"].float()).abs().max()) / (240.0 * 0.01)   # the largest byte below 0x78 decodes to 240
        t, launches = {k: [] for k in forms}, {}
        for _ in range(a.iters):
            for name, fn in forms.items():
                with L.kernel_timer(4) as p:
                    fn()
                launches[name] = len(p.ms)
                t[name].append(sum(p.ms) * 1e3)
        for name in forms:
            md = statistics.median(t[name])
            line = f"{row:>5s} {B:3d} {n:5d} {ctx:5d} | {name:>6s} {launches[name]:8d} {md:9.2f} {min(t[name]):9.2f} {max(t[name]):9.2f} | "
            if name == "tile":
                line += f"{statistics.median(t['stream']) / md:13.2f} {str(max(t['tile']) < min(t['stream'])):>5s} {diff:18.5f}"
            print(line, flush=True)
            lines.append(line)
        del kc, vc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
