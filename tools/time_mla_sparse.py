#!/usr/bin/env python3
"""Times the sparse (top-k indexed) MLA attention (fp8_mla_paged_attention with indices, fp8mi_mla_attention_sparse) against the two things a
caller can do without it, and writes profiles/mla_sparse_timing.txt (or the path given as the first argument).
    python tools/time_mla_sparse.py            (on an MI355X, after __graft_entry__.build())
  (a) gather   a torch gather of the selected rows into a compacted cache (slot arithmetic, one index_select, a static table) and the decode
               entry on it with max_seq_len = topk: every launch of the chain between two events on the stream.  The sparse call is timed the
               same way beside it, so the ratio compares like with like; its bits are compared with the chain's at every shape.
  (b) dense    the decode entry over the whole context: a reference point only, it computes something else.
One query token per sequence, topk random distinct positions of a ctx-long context per token.  The calls alternate in one process after
warm-up; medians of 20 with [min, max]; "kernel us" are the library's per-launch device events (fp8_mi355x_lib.kernel_timer, both launches of
a split call summed), "chain us" the event pairs.  No threshold: the file reports what was measured."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

BS, REPS, SCALE, TOPK = 64, 20, 192 ** -0.5, 2048
ROWS = [(B, Hq, ctx) for B in (1, 8, 64) for Hq in (16, 128) for ctx in (8192, 32768)]


def med(xs):
    return f"{statistics.median(xs):8.1f} [{min(xs):7.1f}, {max(xs):8.1f}]"


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lib = L.load()
    lines = [f"tools/time_mla_sparse.py on {torch.cuda.get_device_name(0)}: fp8_mla_paged_attention(indices=), one query token per sequence, topk {TOPK} random distinct "
             f"positions of ctx; block_size {BS}, bf16 q and out, num_splits = 0; microseconds, median of {REPS} [min, max], alternating in one process; kernel: per-launch "
             "device events; chain: all launches between two stream events; (a) torch gather into a compacted cache + decode entry, (b) dense decode entry over ctx",
             "   B   Hq    ctx | splits |      sparse kernel us      |      sparse chain us       |     (a) gather chain us    | (a) / sparse |   (b) dense kernel us      "
             "| decode at ctx 2048 kernel us | bits (a)"]
    for B, Hq, ctx in ROWS:
        nb = B * ctx // BS
        cache = torch.randint(0, 0x78, (nb, BS, 576), dtype=torch.uint8, device=dev, generator=g)   # finite e4m3 bytes of either sign
        cache |= torch.randint(0, 2, (nb, BS, 576), dtype=torch.uint8, device=dev, generator=g) << 7
        table = torch.randperm(nb, device=dev, generator=g).to(torch.int32).reshape(B, ctx // BS)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
        idx = torch.stack([torch.randperm(ctx, device=dev, generator=g)[:TOPK] for _ in range(B)]).to(torch.int32)
        q = torch.randn(B, Hq, 576, device=dev, generator=g).to(torch.bfloat16)
        ql, qp = q[..., :512].contiguous(), q[..., 512:].contiguous()
        kvs = torch.tensor([1.0 / 64], device=dev)
        c_table = torch.arange(B * TOPK // BS, dtype=torch.int32, device=dev).reshape(B, TOPK // BS)
        c_lens = torch.full((B,), TOPK, dtype=torch.int32, device=dev)
        s_table, s_lens = table[:, :TOPK // BS].contiguous(), c_lens   # the decode entry at a 2 k context: what a sparse call is expected to cost
        flat = cache.view(-1, 576)

        def gather():
            slots = torch.gather(table, 1, (idx // BS).long()).long() * BS + (idx % BS)
            return N.fp8_mla_paged_attention(ql, qp, flat.index_select(0, slots.reshape(-1)).view(-1, BS, 576), c_table, c_lens, kvs, SCALE, max_seq_len=TOPK)

        sparse = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, kvs, SCALE, indices=idx)   # noqa: E731
        dense = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, kvs, SCALE, max_seq_len=ctx)   # noqa: E731
        short = lambda: N.fp8_mla_paged_attention(ql, qp, cache, s_table, s_lens, kvs, SCALE, max_seq_len=TOPK)   # noqa: E731
        for _ in range(3):
            sparse(), gather(), dense(), short()
        torch.cuda.synchronize()
        t = {k: [] for k in ("sparse", "sparse chain", "gather chain", "dense", "short")}

        def chain(fn, key):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            t[key].append(a.elapsed_time(b) * 1e3)
            return out

        for _ in range(REPS):
            for fn, key in ((sparse, "sparse"), (dense, "dense"), (short, "short")):
                with L.kernel_timer(4) as kt:
                    fn()
                t[key].append(sum(kt.ms) * 1e3)
            out, ref = chain(sparse, "sparse chain"), chain(gather, "gather chain")
        same = torch.equal(out.view(torch.int16), ref.view(torch.int16))   # both at the library's choice for topk: the same rule on the same counts
        ratio = statistics.median(t["gather chain"]) / statistics.median(t["sparse chain"])
        lines.append(f"{B:4d} {Hq:4d} {ctx:6d} | {lib.fp8mi_mla_attention_sparse_splits(B, B, 1, Hq, TOPK, 1 << 62):6d} | {med(t['sparse'])} | {med(t['sparse chain'])} | "
                     f"{med(t['gather chain'])} | {ratio:11.2f}x | {med(t['dense'])} | {med(t['short'])}  | {'equal' if same else 'DIFFER'}")
        print(lines[-1], flush=True)
        del cache, table, flat, out, ref
        torch.cuda.empty_cache()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mla_sparse_timing.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
