#!/usr/bin/env python3
"""Times the single-query decode attention over the FP8 paged KV cache (fp8_paged_attention) and writes profiles/paged_attn_timing.txt.
Cases: B in {1, 8, 64} sequences, Hq / Hkv = 32 / 8, D = 128, block_size 16, contexts of 1 k, 8 k and 32 k positions (every sequence full),
bf16 q and output; unsplit (num_splits = 1, one launch) and with the library's own choice (num_splits = 0; `splits` is what it chose,
read from the launch count: 2 launches = split).
Clocks:
  kernels   the sum of the launches' own durations (fp8mi_profile_begin / _end: the dispatch packets' timestamps), median of --iters;
  floor     the cache bytes the call must read (K and V of every position, B Hkv ctx D 2 bytes) at the swept streaming-read ceiling the
            README records (6.2 TB/s); `of ceiling` = floor / kernels;
  chain     the torch chain on the same device in the same run: gather the blocks through the table, view as float8_e4m3fn, convert to
            bf16, multiply by the scales, scaled_dot_product_attention with the KV heads repeated - two events around it, less the empty
            bracket; median of --iters (5 where the gathered bf16 cache passes 2 GiB).
    python tools/time_paged_attn.py [--iters 20] [--out profiles/paged_attn_timing.txt]"""
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
READ_CEILING = 6.2e12   # bytes / s: the swept streaming-read ceiling (README.md, tools/probes/read_sweep.hip)


def med(v):
    return statistics.median(v)


def bracket(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def chain(q, kc, vc, table, ks, vs):
    B, nblk = table.shape
    idx = table.long()
    k = kc[idx].permute(0, 2, 1, 3, 4).reshape(B, HKV, nblk * BS, D)          # (B, nblk, Hkv, bs, D) -> (B, Hkv, L, D)
    v = vc[idx].permute(0, 2, 1, 4, 3).reshape(B, HKV, nblk * BS, D)          # (B, nblk, Hkv, D, bs) -> (B, Hkv, L, D)
    k = k.view(torch.float8_e4m3fn).to(torch.bfloat16) * ks.to(torch.bfloat16)
    v = v.view(torch.float8_e4m3fn).to(torch.bfloat16) * vs.to(torch.bfloat16)
    g = HQ // HKV
    k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    return torch.nn.functional.scaled_dot_product_attention(q.unsqueeze(2), k, v).squeeze(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_attn_timing.txt"))
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    empty = [bracket(lambda: None) for _ in range(50)]
    torch.cuda.synchronize()
    ovh = med([x.elapsed_time(y) * 1e3 for x, y in empty][10:])
    lines = [f"tools/time_paged_attn.py on {torch.cuda.get_device_name(0)}: fp8_paged_attention, Hq / Hkv = {HQ} / {HKV}, D = {D}, block_size {BS}, bf16 q and out, "
             f"every sequence at the full context; times in us, median of {a.iters} calls; empty bracket {ovh:.2f} us (subtracted from the chain column); "
             f"floor = cache bytes / {READ_CEILING / 1e12:.1f} TB/s",
             f"{'B':>3s} {'context':>7s} {'cache MiB':>9s} | {'form':>8s} {'launches':>8s} {'kernels':>9s} {'floor':>8s} {'of ceiling':>10s} {'TB/s':>6s} | "
             f"{'torch chain':>11s} {'chain / ours':>12s} {'max |diff|':>10s}"]
    print("\n".join(lines), flush=True)
    for B in (1, 8, 64):
        for ctx in (1024, 8192, 32768):
            nblk = ctx // BS
            nb = B * nblk
            # bytes below 0x78 in magnitude: |value| < 256, no NaN pattern
            kc = torch.randint(0, 0x78, (nb, HKV, BS, D), dtype=torch.uint8, device=dev, generator=gen)
            kc |= torch.randint(0, 2, kc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
            vc = torch.randint(0, 0x78, (nb, HKV, D, BS), dtype=torch.uint8, device=dev, generator=gen)
            vc |= torch.randint(0, 2, vc.shape, dtype=torch.uint8, device=dev, generator=gen) << 7
            table = torch.randperm(nb, device=dev, generator=gen).to(torch.int32).reshape(B, nblk)
            lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            q = torch.randn((B, HQ, D), device=dev, generator=gen).to(torch.bfloat16)
            ks, vs = torch.tensor([0.002], device=dev), torch.tensor([0.01], device=dev)
            cache_bytes = 2 * B * HKV * ctx * D
            floor = cache_bytes / READ_CEILING * 1e6
            chain_iters = a.iters if cache_bytes * 2 * (HQ // HKV) < (2 << 30) else 5
            ref = lambda: chain(q, kc, vc, table, ks, vs)   # noqa: E731
            want = ref().float()
            for _ in range(2):
                ref()
            torch.cuda.synchronize()
            sc = []
            for _ in range(chain_iters):
                e = bracket(ref)
                torch.cuda.synchronize()
                sc.append(max(0.0, e[0].elapsed_time(e[1]) * 1e3 - ovh))
            for form, splits in (("unsplit", 1), ("auto", 0)):
                ours = lambda: N.fp8_paged_attention(q, kc, vc, table, lens, ks, vs, max_seq_len=ctx, num_splits=splits)   # noqa: E731
                for _ in range(3):
                    got = ours()
                torch.cuda.synchronize()
                diff = float((got.float() - want).abs().max())
                k, launches = [], 0
                for _ in range(a.iters):
                    with L.kernel_timer(4) as p:
                        ours()
                    launches = len(p.ms)
                    k.append(sum(p.ms) * 1e3)
                kern = med(k)
                line = (f"{B:3d} {ctx:7d} {cache_bytes / 2 ** 20:9.1f} | {form:>8s} {launches:8d} {kern:9.2f} {floor:8.2f} {floor / kern:10.3f} "
                        f"{cache_bytes / kern / 1e6:6.2f} | {med(sc):11.2f} {med(sc) / kern:12.1f} {diff:10.4f}")
                print(line, flush=True)
                lines.append(line)
            del kc, vc, want
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
