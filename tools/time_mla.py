#!/usr/bin/env python3
"""Times the MLA decode attention over the FP8 latent cache (fp8_mla_paged_attention) against the torch chain a caller has without it -
gather the blocks, dequantise, einsum, softmax, einsum in bf16 - and writes profiles/mla_timing.txt.
    python tools/time_mla.py            (on an MI355X, after __graft_entry__.build())
Kernel and chain alternate in one process after warm-up; medians of 20 with [min, max], from device events: the library's per-launch events
(fp8_mi355x_lib.kernel_timer, both launches of a split call summed) for the kernel, as tools/time_paged_attn.py takes them, and a pair of
events around the chain less an empty pair.  The `call` column is the same pair of events around the whole op-layer call on an idle device,
host work included, for comparison with the chain on equal terms at the small shapes, where both are bound by their host side.  The
condition the file is held to: on every row the kernel's slowest run is below the chain's fastest."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

BS, REPS, SCALE = 64, 20, 192 ** -0.5
READ_CEILING = 6.2e12   # bytes/s, the swept read ceiling of DESIGN.md 5.18


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out   # microseconds


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    empty = [timed(lambda: None)[0] for _ in range(50)]
    ovh = statistics.median(empty[10:])
    lines = [f"tools/time_mla.py on {torch.cuda.get_device_name(0)}: fp8_mla_paged_attention, block_size {BS}, bf16 q and out, num_splits = 0, against the torch chain "
             f"(gather, dequantise, einsum, softmax, einsum in bf16); microseconds, median of {REPS} [min, max], alternating in one process; empty event pair "
             f"{ovh:.1f} us (subtracted from chain and call)",
             "   B   Hq    ctx splits |  call us |        kernel us         |         chain us          | chain/kernel | cache GB/s (% of 6.2 TB/s) | MFMA TFLOP/s | max|diff|/max|latent|"]
    ok = True
    for B in (1, 8, 64):
        for Hq in (16, 128):
            for ctx in (1024, 8192, 32768):
                nb = B * ctx // BS
                cache = torch.randint(0, 0x78, (nb, BS, 576), dtype=torch.uint8, generator=g).to(dev)   # finite e4m3 bytes of either sign
                cache |= (torch.randint(0, 2, (nb, BS, 576), dtype=torch.uint8, generator=g) << 7).to(dev)
                table = torch.randperm(nb, generator=g).to(torch.int32).reshape(B, ctx // BS).to(dev)
                lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                q = torch.randn(B, Hq, 576, generator=g).to(dev, torch.bfloat16)
                ql, qp = q[..., :512].contiguous(), q[..., 512:].contiguous()
                kvs = torch.tensor([1.0 / 64], device=dev)
                ours = lambda: N.fp8_mla_paged_attention(ql, qp, cache, table, lens, kvs, SCALE, max_seq_len=ctx)   # noqa: E731

                def chain():
                    rows = cache[table.long()].reshape(B, ctx, 576).view(torch.float8_e4m3fn).to(torch.bfloat16) * kvs.to(torch.bfloat16)
                    p = torch.softmax(torch.einsum("bhd,bpd->bhp", q, rows).float() * SCALE, dim=-1).to(torch.bfloat16)
                    return torch.einsum("bhp,bpd->bhd", p, rows[..., :512])

                for _ in range(3):
                    ours(), chain()
                torch.cuda.synchronize()
                tk, tc, tcall = [], [], []
                for _ in range(REPS):
                    with L.kernel_timer(4) as kt:
                        out = ours()
                    tk.append(sum(kt.ms) * 1e3)
                    t, ref = timed(chain)
                    tc.append(max(t - ovh, 0.0))
                    torch.cuda.synchronize()
                    tcall.append(max(timed(ours)[0] - ovh, 0.0))
                rows = cache[table.long()].reshape(B, ctx, 576).view(torch.float8_e4m3fn)[..., :512].float() * kvs
                diff = ((out.float() - ref.float()).abs().max() / rows.abs().max()).item()
                mk, mc = statistics.median(tk), statistics.median(tc)
                splits = N._l.load().fp8mi_mla_attention_splits(B, Hq, ctx, 1 << 62)
                gbs = B * ctx * 576 / (mk * 1e-6)
                flops = 2.0 * B * Hq * ctx * (640 + 512) / (mk * 1e-6)   # the MFMAs issued: five K-steps of 128 for a score, 512 channels of P.V
                ok &= max(tk) < min(tc)
                lines.append(f"{B:4d} {Hq:4d} {ctx:6d} {splits:6d} | {statistics.median(tcall):8.1f} | {mk:8.1f} [{min(tk):7.1f}, {max(tk):8.1f}] | {mc:9.1f} [{min(tc):8.1f}, {max(tc):9.1f}] | {mc / mk:11.1f}x | "
                             f"{gbs / 1e9:8.0f} ({100 * gbs / READ_CEILING:5.1f} %)       | {flops / 1e12:10.1f}   | {diff:.4f}" + ("" if max(tk) < min(tc) else "   <-- CONDITION MISSED"))
                print(lines[-1], flush=True)
                del cache, table, rows
                torch.cuda.empty_cache()
    lines.append("condition (the kernel's slowest of 20 below the chain's fastest, every row): " + ("MET" if ok else "MISSED"))
    with open(os.path.join(ROOT, "profiles", "mla_timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
