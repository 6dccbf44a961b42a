#!/usr/bin/env python3
"""Times the multi-token MLA attention (fp8_mla_paged_attention with cu_seqlens_q, fp8mi_mla_attention_varlen) against the only way to run
these shapes without it: the decode entry on the one-sequence-per-token expansion (that token's q rows, the sequence's table row,
seq_len = limit) - and writes profiles/mla_varlen_timing.txt (or the path given as the first argument).
    python tools/time_mla_varlen.py            (on an MI355X, after __graft_entry__.build())
Every sequence holds `ctx` positions, its q_len query tokens included.  The two alternate in one process after warm-up; medians of 20 with
[min, max] of the library's per-launch device events (fp8_mi355x_lib.kernel_timer, both launches of a split call summed), as tools/time_mla.py
takes them.  The outputs are compared bit for bit at every timed shape.  No threshold: the file reports what was measured."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

BS, REPS, SCALE = 64, 20, 192 ** -0.5
ROWS = [(B, Hq, ctx, q) for B in (1, 8, 64) for Hq in (16, 128) for ctx in (1024, 32768) for q in (2, 4)] + [(1, 16, 8192, 512), (1, 128, 8192, 512)]


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lib = L.load()
    lines = [f"tools/time_mla_varlen.py on {torch.cuda.get_device_name(0)}: fp8_mla_paged_attention(cu_seqlens_q=), q_len query tokens per sequence at the end of ctx positions, "
             f"against the decode entry on the one-sequence-per-token expansion; block_size {BS}, bf16 q and out, num_splits = 0; kernel microseconds from per-launch device "
             f"events, median of {REPS} [min, max], alternating in one process",
             "   B   Hq    ctx q_len | tiles splits |      multi-token us       | exp. splits |        expansion us        | expansion / multi-token | bits"]
    for B, Hq, ctx, qn in ROWS:
        nb, T = B * ctx // BS, B * qn
        cache = torch.randint(0, 0x78, (nb, BS, 576), dtype=torch.uint8, device=dev, generator=g)   # finite e4m3 bytes of either sign
        cache |= torch.randint(0, 2, (nb, BS, 576), dtype=torch.uint8, device=dev, generator=g) << 7
        table = torch.randperm(nb, device=dev, generator=g).to(torch.int32).reshape(B, ctx // BS)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * qn
        q = torch.randn(T, Hq, 576, device=dev, generator=g).to(torch.bfloat16)
        ql, qp = q[..., :512].contiguous(), q[..., 512:].contiguous()
        kvs = torch.tensor([1.0 / 64], device=dev)
        x_table = table.repeat_interleave(qn, dim=0).contiguous()
        x_lens = (ctx - qn + 1 + torch.arange(qn, dtype=torch.int32, device=dev)).repeat(B)
        multi = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, kvs, SCALE, max_seq_len=ctx, cu_seqlens_q=cu, max_q_len=qn)   # noqa: E731
        expansion = lambda: N.fp8_mla_paged_attention(ql, qp, cache, x_table, x_lens, kvs, SCALE, max_seq_len=ctx)   # noqa: E731
        for _ in range(3):
            multi(), expansion()
        torch.cuda.synchronize()
        tm, tx = [], []
        for _ in range(REPS):
            with L.kernel_timer(4) as kt:
                out = multi()
            tm.append(sum(kt.ms) * 1e3)
            with L.kernel_timer(4) as kt:
                ref = expansion()
            tx.append(sum(kt.ms) * 1e3)
        # the library's own counts differ between the two calls: the bits are compared at the expansion's count, forced on both
        ns = lib.fp8mi_mla_attention_splits(T, Hq, ctx, 1 << 62)
        same = torch.equal(N.fp8_mla_paged_attention(ql, qp, cache, table, lens, kvs, SCALE, max_seq_len=ctx, num_splits=ns, cu_seqlens_q=cu, max_q_len=qn).view(torch.int16),
                           N.fp8_mla_paged_attention(ql, qp, cache, x_table, x_lens, kvs, SCALE, max_seq_len=ctx, num_splits=ns).view(torch.int16))
        mm, mx = statistics.median(tm), statistics.median(tx)
        lines.append(f"{B:4d} {Hq:4d} {ctx:6d} {qn:5d} | {B * ((qn * Hq + 63) // 64):5d} {lib.fp8mi_mla_attention_varlen_splits(T, B, qn, Hq, ctx, 1 << 62):6d} | "
                     f"{mm:8.1f} [{min(tm):7.1f}, {max(tm):8.1f}] | {ns:11d} | {mx:8.1f} [{min(tx):7.1f}, {max(tx):8.1f}] | {mx / mm:22.2f}x | {'equal' if same else 'DIFFER'}")
        print(lines[-1], flush=True)
        del cache, table, x_table, out, ref
        torch.cuda.empty_cache()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mla_varlen_timing.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
