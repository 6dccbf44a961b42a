#!/usr/bin/env python3
"""Times the fused rotary embedding (+ head RMSNorm) + FP8 cache append (fp8_rope_kv_cache_append, fp8_mla_rope_cache_append)
against the chain a caller runs without it: torch's rotation of q and k (rms_norm first where normed), then the existing append.  Each row
alternates its candidates in one process: median [min, max] of 20 runs, both on stream events around the call (the chain's torch kernels are not
the library's); the fused kernel alone on the library's per-launch events as a third line.  A row is met when the fused launch's slowest run is below the chain's fastest.
  (a) decode: 64 tokens, 32 / 8 heads, D = 128, bf16        (b) prefill append: 8192 tokens with consecutive slots, and the V bytes alone
  (c) MLA: 64 and 4096 tokens, 128 heads, the latent norm   (d) (a) with q / k norm   (e) 128 tokens: the tiled kernel at its smallest
Usage: python tools/time_rope_append.py [--runs 20] > profiles/rope_append_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fp8-mps-metal_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

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


def row(name, candidates, runs, nbytes=None):
    """candidates: [(label, timer, fn)], run alternately; the first is the fused launch, the second the chain"""
    for _label, timer, fn in candidates:
        timer(fn), timer(fn)   # warm
    ms = {label: [] for label, _t, _f in candidates}
    for _ in range(runs):
        for label, timer, fn in candidates:
            ms[label].append(timer(fn))
    print(name)
    for label, t in ms.items():
        med = statistics.median(t)
        rate = f"  {nbytes / med / 1e6:8.1f} GB/s" if nbytes else ""
        print(f"    {label:44s} {med * 1e3:9.1f} us [{min(t) * 1e3:.1f}, {max(t) * 1e3:.1f}]{rate}")
    (a, _t, _f), (b, _t2, _f2) = candidates[:2]
    print(f"    {'met' if max(ms[a]) < min(ms[b]) else 'LOST'}: the fused launch's slowest run against the chain's fastest")
    return ms


def neox(x, cos, sin):
    """torch's rotation as serving stacks write it, in the input dtype"""
    a, b = x.chunk(2, dim=-1)
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)


def gptj(x, cos, sin):
    a, b = x[..., 0::2], x[..., 1::2]
    return torch.stack([a * cos - b * sin, b * cos + a * sin], dim=-1).flatten(-2)


def kv_case(T, norm, runs, tag):
    Hq, Hkv, D, bs = 32, 8, 128, 16
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn((T, (Hq + 2 * Hkv) * D), generator=g).to(DEV).to(torch.bfloat16)
    q, k, v = (x.view(T, -1, D) for x in qkv.split([Hq * D, Hkv * D, Hkv * D], dim=1))
    ang = torch.rand((T + 16, D // 2), generator=g) * 6.3
    table = torch.cat([ang.cos(), ang.sin()], dim=1).to(DEV)
    pos = torch.arange(T, device=DEV)
    slots = torch.arange(T, device=DEV) if T > 64 else (torch.randperm(T * 4, generator=g)[:T] * bs).to(DEV)   # decode: one slot a sequence
    nb = (int(slots.max()) + bs) // bs
    kc, vc = N.fp8_kv_cache_alloc(nb, bs, Hkv, D, device=DEV)
    one = torch.full((1,), 0.02, device=DEV)
    qw, kw = (torch.ones(D, device=DEV), torch.ones(D, device=DEV)) if norm else (None, None)
    qo = torch.empty((T, Hq, D), dtype=torch.bfloat16, device=DEV)
    table16, qw16, kw16 = table.to(torch.bfloat16), (qw.bfloat16() if norm else None), (kw.bfloat16() if norm else None)   # a caller's: made once

    def chain():   # what a step costs a careful caller: the table rows of this step's positions, the rotation (its result used as it is), the append
        cs = table16[pos][:, None, :]
        cos, sin = cs[..., :D // 2], cs[..., D // 2:]
        qn, kn = (F.rms_norm(q, (D,), qw16, 1e-6), F.rms_norm(k, (D,), kw16, 1e-6)) if norm else (q, k)
        q_rot = neox(qn, cos, sin)
        N.fp8_kv_cache_append(neox(kn, cos, sin), v, kc, vc, slots, one, one)
        return q_rot

    fused = lambda: N.fp8_rope_kv_cache_append(q, k, v, pos, table, kc, vc, slots, one, one, q_weight=qw, k_weight=kw, q_out=qo)   # noqa: E731
    nbytes = T * (Hq * D * 4 + 2 * Hkv * D * 3)   # q read and written, k and v read, their bytes written
    row(f"({tag}) T={T} Hq={Hq} Hkv={Hkv} D={D} bf16{' q/k norm' if norm else ''}", [("fp8_rope_kv_cache_append", torch_ms, fused), ("torch rotation + fp8_kv_cache_append", torch_ms, chain), ("fp8_rope_kv_cache_append, kernel alone", lib_ms, fused)],
        runs, nbytes)
    if T > 64:   # what the 16-byte V stores buy: the V rows alone through both entries (Hq = 0; the K rows ride along in both)
        row(f"({tag}) the same k, v alone: V-cache bytes {T * Hkv * D / 1e6:.1f} MB", [
            ("fp8_rope_kv_cache_append (no q)", lib_ms, lambda: N.fp8_rope_kv_cache_append(None, k, v, pos, table, kc, vc, slots, one, one)),
            ("fp8_kv_cache_append", lib_ms, lambda: N.fp8_kv_cache_append(k, v, kc, vc, slots, one, one))], runs, T * Hkv * D * 6)


def mla_case(T, runs):
    Hq, bs = 128, 64
    g = torch.Generator().manual_seed(2)
    kv = torch.randn((T, 576), generator=g).to(DEV).to(torch.bfloat16)
    kv_c, k_pe = kv[:, :512], kv[:, 512:]
    q_pe = torch.randn((T, Hq, 64), generator=g).to(DEV).to(torch.bfloat16)
    ang = torch.rand((T + 16, 32), generator=g) * 6.3
    table = torch.cat([ang.cos(), ang.sin()], dim=1).to(DEV)
    pos, slots = torch.arange(T, device=DEV), torch.arange(T, device=DEV)
    cache = N.fp8_mla_cache_alloc((T + bs - 1) // bs, bs, device=DEV)
    one, w, qo = torch.full((1,), 0.05, device=DEV), torch.ones(512, device=DEV), torch.empty_like(q_pe)

    table16, w16 = table.to(torch.bfloat16), w.bfloat16()

    def chain():
        cs = table16[pos]
        cos, sin = cs[:, :32], cs[:, 32:]
        q_rot = gptj(q_pe, cos[:, None], sin[:, None])
        N.fp8_mla_cache_append(F.rms_norm(kv_c, (512,), w16, 1e-6), gptj(k_pe, cos, sin), cache, slots, one)
        return q_rot

    fused = lambda: N.fp8_mla_rope_cache_append(kv_c, k_pe, q_pe, pos, table, cache, slots, one, kv_weight=w, q_pe_out=qo)   # noqa: E731
    row(f"(c) MLA T={T} Hq={Hq} bf16, latent norm", [("fp8_mla_rope_cache_append", torch_ms, fused), ("torch norm + rotation + fp8_mla_cache_append", torch_ms, chain), ("fp8_mla_rope_cache_append, kernel alone", lib_ms, fused)], runs,
        T * (Hq * 64 * 4 + 576 * 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    runs = ap.parse_args().runs
    kv_case(64, False, runs, "a")
    kv_case(8192, False, runs, "b")
    mla_case(64, runs)
    mla_case(4096, runs)
    kv_case(64, True, runs, "d")
    kv_case(128, False, runs, "e")   # just past the threshold between the two kernels: 16 workgroups of the tiled one


if __name__ == "__main__":
    main()
