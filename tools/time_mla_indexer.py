#!/usr/bin/env python3
"""Times the lightning indexer (fp8_mla_index_logits, fp8_mla_index_topk, fp8_mla_indexer) against what a caller does without it, and writes
profiles/mla_indexer_timing.txt (or the path given as the first argument).
    python tools/time_mla_indexer.py            (on an MI355X, after __graft_entry__.build())
  (a) logits   the torch chain on the SAME cache: gather the sequences' blocks through the table, view the key bytes as float8_e4m3fn and
               dequantise to bf16 with the stored scales, einsum with the bf16 q, relu, the weighted head sum.
  (b) top-k    mask the columns at or beyond the limit with -inf, torch.topk, sort the positions: on the logits of our kernel.
  (c) sparse   fp8_mla_indexer + fp8_mla_paged_attention(indices=) against the dense MLA call over the whole context (Hq 128).
bf16 q, Hi 64, block_size 64, topk 2048; one token per sequence, and one MTP row set (two tokens per sequence).  "read us" is the time of reading
the sequences' key caches once, 132 bytes a position, at the 8 TB/s of the data sheet: the floor the logits kernel is held against.  The calls
alternate in one process after warm-up; medians of REPS with [min, max]; every figure is all launches between two events on the stream.  No
threshold: the file reports what was measured."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import fp8_mi355x_native as N  # noqa: E402

BS, HI, HQ, TOPK, SCALE, PEAK = 64, 64, 128, 2048, 192 ** -0.5, 8.0e12
ROWS = [(B, ctx, 1) for B in (1, 8, 64) for ctx in (8192, 32768, 131072)] + [(8, 32768, 2)]


def med(xs):
    return f"{statistics.median(xs):9.1f} [{min(xs):8.1f}, {max(xs):9.1f}]"


def timed(fn, into):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    into.append(a.elapsed_time(b) * 1e3)
    return out


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"tools/time_mla_indexer.py on {torch.cuda.get_device_name(0)}: bf16 q, Hi {HI}, block_size {BS}, topk {TOPK}, sparse / dense attention at Hq {HQ}; microseconds, median "
             "[min, max], alternating in one process, all launches between two stream events; read us = B ctx 132 bytes at 8 TB/s",
             "   B    ctx  q | read us |          logits us           |      (a) torch logits us     | (a)/ours |           top-k us           |      (b) torch top-k us      "
             "| (b)/ours |   indexer + sparse attn us   |     (c) dense MLA attn us    | (c)/ours | checks"]
    for B, ctx, ql in ROWS:
        reps = 20 if B * ctx <= 8 * 32768 else 8
        nb, T = B * ctx // BS, B * ql
        icache = N.fp8_mla_index_cache_alloc(nb, BS, device=dev)
        table = torch.randperm(nb, device=dev, generator=g).to(torch.int32).reshape(B, ctx // BS)
        slots = (table.long()[:, :, None] * BS + torch.arange(BS, device=dev)).reshape(-1)
        for at in range(0, B * ctx, 1 << 20):   # the append, a million tokens a call
            n = min(1 << 20, B * ctx - at)
            N.fp8_mla_index_cache_append(torch.randn(n, 128, device=dev, generator=g).to(torch.bfloat16), icache, slots[at:at + n])
        cache = torch.randint(0, 0x78, (nb, BS, 576), dtype=torch.uint8, device=dev, generator=g)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        cu = torch.arange(0, T + 1, ql, dtype=torch.int32, device=dev)
        rows = dict(cu_seqlens_q=cu, max_q_len=ql) if ql > 1 else {}
        seq = torch.arange(B, device=dev).repeat_interleave(ql)
        limit = (ctx - ql + 1 + torch.arange(T, device=dev) % ql)[:, None]
        q = torch.randn(T, HI, 128, device=dev, generator=g).to(torch.bfloat16)
        w = torch.randn(T, HI, device=dev, generator=g) * HI ** -0.5
        aq = torch.randn(T, HQ, 576, device=dev, generator=g).to(torch.bfloat16)
        a_lat, a_pe, kvs = aq[..., :512].contiguous(), aq[..., 512:].contiguous(), torch.tensor([1.0 / 64], device=dev)
        logits = torch.empty((T, ctx), device=dev)
        cols = torch.arange(ctx, device=dev)

        def torch_logits():
            blocks = icache[table.long()]                                                            # (B, blocks, BS 132)
            keys = blocks[..., :BS * 128].reshape(B, ctx, 128).view(torch.float8_e4m3fn).to(torch.bfloat16)
            scales = blocks[..., BS * 128:].contiguous().view(torch.float32).reshape(B, ctx)
            dots = torch.einsum("thd,tpd->thp", q, keys[seq] if ql > 1 else keys).float().relu_()
            return (dots * w[:, :, None]).sum(1) * (scales[seq] if ql > 1 else scales)

        def torch_topk():
            return torch.topk(logits.masked_fill(cols >= limit, float("-inf")), TOPK, dim=1).indices.sort(dim=1).values.to(torch.int32)

        ours_logits = lambda: N.fp8_mla_index_logits(q, w, icache, table, lens, max_seq_len=ctx, out=logits, **rows)   # noqa: E731
        ours_topk = lambda: N.fp8_mla_index_topk(logits, lens, TOPK, **rows)   # noqa: E731
        sparse = lambda: N.fp8_mla_paged_attention(a_lat, a_pe, cache, table, lens, kvs, SCALE,   # noqa: E731
                                                   indices=N.fp8_mla_indexer(q, w, icache, table, lens, TOPK, max_seq_len=ctx, logits=logits, **rows), **rows)
        dense = lambda: N.fp8_mla_paged_attention(a_lat, a_pe, cache, table, lens, kvs, SCALE, max_seq_len=ctx, **rows)   # noqa: E731
        fns = dict(logits=ours_logits, t_logits=torch_logits, topk=ours_topk, t_topk=torch_topk, sparse=sparse, dense=dense)
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(reps):
            out = {k: timed(fn, t[k]) for k, fn in fns.items()}
        # the torch chain rounds nothing of q: agreement is to bf16-product accuracy only; the selection must be the same set where no tie is cut
        rel = float(((out["logits"] - out["t_logits"]).masked_fill(cols >= limit, 0.0).abs().max() / out["t_logits"].abs().max()))
        same = float((out["topk"] == out["t_topk"]).float().mean())
        m = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"{B:4d} {ctx:6d} {ql:2d} | {B * ctx * 132 / PEAK * 1e6:7.1f} | {med(t['logits'])} | {med(t['t_logits'])} | {m['t_logits'] / m['logits']:7.2f}x | {med(t['topk'])} | "
                     f"{med(t['t_topk'])} | {m['t_topk'] / m['topk']:7.2f}x | {med(t['sparse'])} | {med(t['dense'])} | {m['dense'] / m['sparse']:7.2f}x | "
                     f"logits vs torch {rel:.1e}, top-k equal {same:.4f}")
        print(lines[-1], flush=True)
        del icache, cache, table, slots, logits, out, cols
        torch.cuda.empty_cache()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mla_indexer_timing.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
