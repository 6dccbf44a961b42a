#!/usr/bin/env python3
"""Times the FP8 flash attention over contiguous K / V (fp8_attention: fp8mi_attention_prefill) against what a caller has today.
Each row alternates its candidates in one process: median [min, max] of 20 runs, the library's kernels on its per-launch events, torch's SDPA on
stream events around the call.  FLOP/s are 2 pairs (DQK + DV) over the visible (query, key) pairs.
  (a) B = 4 prompts of 2048 tokens, 32 / 8 heads, causal, against fp8_paged_attention(kernel="tile") on the same tokens appended to a cache
  (b) FLUX: 1 x 24 heads x 4608 tokens, not causal, against torch's bf16 SDPA
  (c) MLA prefill: 128 heads, 192 / 128, 4 k and 16 k tokens, causal, against torch's SDPA on the dequantised inputs
Usage: python tools/time_flash_attn.py [--runs 20] > profiles/flash_attn_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fp8-mps-metal_amd"))
import torch  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

DEV = "cuda"


def lib_ms(fn):
    with L.kernel_timer(16) as kt:
        fn()
    torch.cuda.synchronize()
    return sum(kt.ms)


def torch_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def row(name, pairs, dims, candidates, runs):
    """candidates: [(label, timer, fn)], run alternately"""
    for _label, timer, fn in candidates:
        timer(fn), timer(fn)   # warm
    ms = {label: [] for label, _t, _f in candidates}
    for _ in range(runs):
        for label, timer, fn in candidates:
            ms[label].append(timer(fn))
    print(name)
    for label, t in ms.items():
        med = statistics.median(t)
        print(f"    {label:34s} {med:9.4f} ms [{min(t):.4f}, {max(t):.4f}]  {2 * pairs * dims / med / 1e9:8.1f} TFLOP/s")
    return ms


def prompts(B, S, Hq, Hkv, DQK, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(1)
    q = torch.randn((B * S, Hq, DQK), generator=g).to(DEV).to(dtype)
    k, v = (torch.randn((B * S, Hkv, 128), generator=g).to(DEV).to(dtype) for _ in range(2))
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=DEV)
    return q, k, v, cu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    runs = ap.parse_args().runs
    one = torch.ones(1, device=DEV) * 0.01
    # (a)
    B, S, Hq, Hkv = 4, 2048, 32, 8
    q, k, v, cu = prompts(B, S, Hq, Hkv, 128)
    k8, v8 = N.fp8_attention_kv_quantize(k, one), N.fp8_attention_kv_quantize(v, one)
    kc, vc = N.fp8_kv_cache_alloc(B * S // 128, 128, Hkv, 128, device=DEV)
    N.fp8_kv_cache_append(k, v, kc, vc, torch.arange(B * S, device=DEV), one, one)
    table = torch.arange(B * S // 128, dtype=torch.int32, device=DEV).reshape(B, -1)
    lens = torch.full((B,), S, dtype=torch.int32, device=DEV)
    ms = row(f"(a) B={B} q_len=seq_len={S} Hq={Hq} Hkv={Hkv} D=128 causal", B * Hq * S * (S + 1) // 2, 256, [
        ("fp8_attention (flash)", lib_ms, lambda: N.fp8_attention(q, k8, v8, one, one, cu_seqlens_q=cu, cu_seqlens_k=cu, max_q_len=S, max_k_len=S, causal=True)),
        ('fp8_paged_attention(kernel="tile")', lib_ms, lambda: N.fp8_paged_attention(q, kc, vc, table, lens, one, one, max_seq_len=S, kernel="tile", cu_seqlens_q=cu, max_q_len=S)),
    ], runs)
    met = max(ms["fp8_attention (flash)"]) < min(ms['fp8_paged_attention(kernel="tile")'])
    print(f"    row (a) {'met' if met else 'LOST'}: the flash kernel's slowest run against the tile kernel's fastest")
    # (b)
    H, S = 24, 4608
    q4, k4, v4 = (torch.randn((1, H, S, 128), device=DEV, dtype=torch.bfloat16) for _ in range(3))
    row(f"(b) FLUX B=1 H={H} S={S} D=128 not causal", H * S * S, 256, [
        ("fp8_sdpa (quantise K, V + flash)", lib_ms, lambda: N.fp8_sdpa(q4, k4, v4)),
        ("torch SDPA bf16", torch_ms, lambda: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4)),
    ], runs)
    # (c)
    for S in (4096, 16384):
        H = 128
        q, k, v, cu = prompts(1, S, H, H, 192)
        kr = torch.randn((S, 1, 64), device=DEV, dtype=torch.bfloat16)
        k8, v8, r8 = (N.fp8_attention_kv_quantize(x, one) for x in (k, v, kr))
        kd = torch.cat([k, kr.expand(S, H, 64)], dim=2).transpose(0, 1)[None]
        qd, vd = q.transpose(0, 1)[None], v.transpose(0, 1)[None]
        cands = [("fp8_attention (flash, 192 / 128)", lib_ms, lambda: N.fp8_attention(q, k8, v8, one, one, k_rope=r8, cu_seqlens_q=cu, cu_seqlens_k=cu, max_q_len=S,
                                                                                     max_k_len=S, causal=True))]
        if S <= 4096:   # torch has no fused kernel for 192 / 128: its path materialises the H x S x S scores, 64 GiB at 16 k
            cands.append(("torch SDPA bf16 (192 / 128)", torch_ms, lambda: torch.nn.functional.scaled_dot_product_attention(qd, kd, vd, is_causal=True)))
        row(f"(c) MLA prefill H={H} S={S} 192 / 128 causal", H * S * (S + 1) // 2, 320, cands, runs if S < 16384 else max(runs // 4, 3))


if __name__ == "__main__":
    main()
