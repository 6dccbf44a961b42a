#!/usr/bin/env python3
"""Times the multi-token paged attention (fp8_paged_attention with cu_seqlens_q: fp8mi_paged_attention_varlen) against the workaround it
replaces - the decode entry on the expanded batch, one row per query token with the table row duplicated and seq_len shortened to the
token's causal limit - and writes profiles/paged_attn_varlen_timing.txt.
Shape: Hq / Hkv = 32 / 8 (TQ = 4 tokens to a tile), D = 128, block_size 16, bf16 q and output, num_splits = 0 (each entry's own choice).
Rows: speculative verification, B in {8, 64} sequences of 8 k context with q_len in {1, 2, 4, 8} new tokens each; one chunked-prefill row,
B = 1, q_len = 512 over 8 k.  The two forms ALTERNATE call by call in this one process; a time is the sum of a call's launches' own
durations (fp8mi_profile_begin / _end: the dispatch packets' timestamps), median of --iters, with the spread [min, max] and the
interquartile range beside it.  bytes = the K and V bytes the form's workgroups must read (a tile reads to the limit of its last token; the
expanded batch reads every token's own limit); `of ceiling` = bytes / time / 6.2 TB/s, the swept streaming-read ceiling the README records.
    python tools/time_paged_attn_varlen.py [--iters 20] [--out profiles/paged_attn_varlen_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

HQ, HKV, D, BS, CTX = 32, 8, 128, 16, 8192
TQ = 16 // (HQ // HKV)
READ_CEILING = 6.2e12   # bytes / s
ROWS = [(B, n) for B in (8, 64) for n in (1, 2, 4, 8)] + [(1, 512)]


def stats(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), min(v), max(v), q[2] - q[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_attn_varlen_timing.txt"))
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"tools/time_paged_attn_varlen.py on {torch.cuda.get_device_name(0)}: fp8_paged_attention, Hq / Hkv = {HQ} / {HKV} (TQ = {TQ}), D = {D}, block_size {BS}, "
             f"bf16 q and out, context {CTX} including the new tokens, num_splits = 0; `varlen` = cu_seqlens_q, `expanded` = the decode entry, one row per token; "
             f"the two alternate call by call; bit-equal: the two outputs compared (they are the same bits whenever the two entries chose the same split count - `launches` 1 = unsplit - and may differ when they did not); times in us: median of {a.iters} [min, max] iqr; of ceiling = bytes / time / {READ_CEILING / 1e12:.1f} TB/s",
             f"{'B':>3s} {'q_len':>5s} | {'form':>8s} {'launches':>8s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>7s} {'MiB read':>9s} {'of ceiling':>10s} | "
             f"{'expanded / varlen':>17s} {'bit-equal':>9s}"]
    print("\n".join(lines), flush=True)
    nblk = CTX // BS
    for B, n in ROWS:
        nb = B * nblk
        kc = torch.randint(0, 0x78, (nb, HKV, BS, D), dtype=torch.uint8, device=dev, generator=gen)   # |value| < 256, no NaN pattern
        kc |= torch.randint(0, 2, kc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
        vc = torch.randint(0, 0x78, (nb, HKV, D, BS), dtype=torch.uint8, device=dev, generator=gen)
        vc |= torch.randint(0, 2, vc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
        table = torch.randperm(nb, device=dev, generator=gen).to(torch.int32).reshape(B, nblk)
        lens = torch.full((B,), CTX, dtype=torch.int32, device=dev)
        T = B * n
        q = torch.randn((T, HQ, D), device=dev, generator=gen).to(torch.bfloat16)
        cu = (torch.arange(B + 1, device=dev) * n).to(torch.int32)
        ks, vs = torch.tensor([0.002], device=dev), torch.tensor([0.01], device=dev)
        limits = (CTX - n + 1 + torch.arange(n, device=dev)).repeat(B).to(torch.int32)          # row b n + j: CTX - n + j + 1
        table_x = table.repeat_interleave(n, dim=0).contiguous()
        forms = {"varlen": lambda: N.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=CTX, cu_seqlens_q=cu, max_q_len=n),
                 "expanded": lambda: N.fp8_paged_attention(q, kc, vc, table_x, limits, ks, vs, max_seq_len=CTX)}
        tile_last = [CTX - n + min((i + 1) * TQ, n) for i in range((n + TQ - 1) // TQ)]                # the limit of every tile's last token
        nbytes = {"varlen": 2 * B * HKV * D * sum(tile_last), "expanded": 2 * B * HKV * D * sum(CTX - n + j + 1 for j in range(n))}
        outs = {}
        for name, fn in forms.items():
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        same = torch.equal(outs["varlen"].view(torch.int16), outs["expanded"].view(torch.int16))
        t, launches = {k: [] for k in forms}, {}
        for _ in range(a.iters):
            for name, fn in forms.items():
                with L.kernel_timer(4) as p:
                    fn()
                launches[name] = len(p.ms)
                t[name].append(sum(p.ms) * 1e3)
        m = {k: stats(v) for k, v in t.items()}
        for name in forms:
            md, lo, hi, iqr = m[name]
            line = (f"{B:3d} {n:5d} | {name:>8s} {launches[name]:8d} {md:9.2f} {lo:9.2f} {hi:9.2f} {iqr:7.2f} {nbytes[name] / 2 ** 20:9.1f} "
                    f"{nbytes[name] / (md * 1e-6) / READ_CEILING:10.3f} | " + (f"{m['expanded'][0] / m['varlen'][0]:17.2f} {str(same):>9s}" if name == "varlen" else ""))
            print(line, flush=True)
            lines.append(line)
        del kc, vc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
