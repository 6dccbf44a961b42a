#!/usr/bin/env python3
"""Times the fused producers with MXFP8 / MXFP4 output (fp8mi_act_quantize_mx / fp8mi_norm_quantize_mx) against the chains that give the
same operand without them: torch's activation (and gate product), or torch's norm / residual / modulation passes, on the GPU, then
fp8_quantize_mxfp8 / fp8_quantize_mxfp4; and fp8_mlp_mx* / fp8_norm_linear_mx* against fp8_linear_mx*, torch's activation or norm,
fp8_linear_mx*.

The method is that of tools/time_act_quant.py and tools/time_norm_quant.py.  The library's launches are timed per dispatch
(fp8mi_profile_begin / _end: the dispatch packet's timestamps).  Torch's kernels are not visible to that hook: each torch op is
bracketed by two events on the stream, and the interval around a one-element torch kernel (printed as `event overhead`) is SUBTRACTED
from every bracket, which errs in the chain's favour.  The chain's figure is the SUM of its kernels, gaps between them not included; the
uncorrected sum is printed beside it.  The MLPs and norm-linears are bracketed by events as a whole, both candidates alike.
After warm-up the candidates ALTERNATE call by call in one process; median of --iters (>= 20).  The tensors rotate over enough copies
to exceed the 256 MiB of last-level cache (at most 64).  Bytes/s are over the bytes the recipe has to move once.
    python tools/time_mx_fused.py [--iters 30] [--buffers N] [--no-ops] [--out profiles/mx_fused_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fp8-mps-metal_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fp8_mi355x_lib as L  # noqa: E402
import fp8_mi355x_native as N  # noqa: E402

FORMATS = ("mxfp8", "mxfp4")
QUANT = {"mxfp8": N.fp8_quantize_mxfp8, "mxfp4": N.fp8_quantize_mxfp4}
LINEAR = {"mxfp8": N.fp8_linear_mxfp8, "mxfp4": N.fp8_linear_mxfp4}
MLP = {"mxfp8": N.fp8_mlp_mxfp8, "mxfp4": N.fp8_mlp_mxfp4}
NORM_LINEAR = {"mxfp8": N.fp8_norm_linear_mxfp8, "mxfp4": N.fp8_norm_linear_mxfp4}
# (rows, output columns, gated, acts): FLUX's MLP hidden; a Llama-3 8B gate_up output; the FLUX activation itself against the quantisers
ACT_LINES = [(4096, 12288, False, ("silu",)), (4096, 14336, True, ("silu", "gelu_tanh")), (4096, 3072, False, ("none",))]
# (name, rows, cols, norm, weight, residual, rows per modulation row)
NORM_LINES = [("FLUX adaLN", 4096, 3072, "layer", False, False, 1024), ("FLUX adaLN", 64, 3072, "layer", False, False, 64),
              ("FLUX adaLN", 1, 3072, "layer", False, False, 1),
              ("8B rms + w + residual", 4096, 4096, "rms", True, True, 0), ("8B rms + w + residual", 64, 4096, "rms", True, True, 0),
              ("8B rms + w + residual", 1, 4096, "rms", True, True, 0)]
# (name, M, K, H, N, act, gated)
MLPS = [("FLUX gelu_tanh", 4096, 3072, 12288, 3072, "gelu_tanh", False), ("FLUX gelu_tanh", 64, 3072, 12288, 3072, "gelu_tanh", False),
        ("8B SwiGLU", 4096, 4096, 14336, 4096, "silu", True), ("8B SwiGLU", 64, 4096, 14336, 4096, "silu", True)]
# (name, M, K, N, norm, weight, residual, rows per modulation row): FLUX's adaLN -> qkv; an 8B block's rms(x + res) w -> qkv
NORM_LINEARS = [("FLUX adaLN qkv", 4096, 3072, 9216, "layer", False, False, 1024), ("FLUX adaLN qkv", 64, 3072, 9216, "layer", False, False, 64),
                ("8B rms qkv", 4096, 4096, 6144, "rms", True, True, 0), ("8B rms qkv", 64, 4096, 6144, "rms", True, True, 0)]
CACHE_BYTES = 256 << 20
EPS = 1e-6
TORCH_ACT = {"none": lambda t: t, "silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "gelu_erf": F.gelu}
OUT = None


def say(line=""):
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def kernel_us(fn):
    with L.kernel_timer(16) as prof:
        fn()
    return [t * 1e3 for t in prof.ms]


class Events:
    """brackets of torch ops on the current stream; .us() after a synchronize"""

    def __init__(self):
        self.pairs = []

    def run(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.pairs.append((a, b))
        return out

    def us(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in self.pairs]


def med(v):
    return statistics.median(v)


def act_chain(x, act, gated, fmt, overhead=0.0):
    ev = Events()
    if not gated:
        y = x if act == "none" else ev.run(lambda: TORCH_ACT[act](x))
    else:
        g, u = x.chunk(2, -1)
        a = g if act == "none" else ev.run(lambda: TORCH_ACT[act](g))
        y = ev.run(lambda: a * u)
    t_torch = [max(0.0, t - overhead) for t in ev.us()]
    return t_torch, kernel_us(lambda: QUANT[fmt](y))


def torch_norm(x, norm, w, res, mod, ev):
    C = x.shape[-1]
    run = ev.run if ev is not None else (lambda fn: fn())
    h = x if res is None else run(lambda: x + res)
    y = run(lambda: F.layer_norm(h, (C,), w, None, EPS)) if norm == "layer" else run(lambda: F.rms_norm(h, (C,), w, EPS))
    if mod is not None:
        sc, sh = mod
        t = run(lambda: 1 + sc)
        y = run(lambda: y * t)
        y = run(lambda: y + sh)
    return y, h


def norm_chain(x, norm, w, res, mod, fmt, overhead=0.0):
    ev = Events()
    y, _ = torch_norm(x, norm, w, res, mod, ev)
    t_torch = [max(0.0, t - overhead) for t in ev.us()]
    y2 = y.reshape(-1, x.shape[-1])
    return t_torch, kernel_us(lambda: QUANT[fmt](y2))


def compare(name, shape, fmt, need, fused, chained, iters, ovh):
    for i in range(5):
        fused(i)
        chained(i, 0.0)
    tf, tc, tt, tq, traw, nk = [], [], [], [], [], 0
    for i in range(iters):
        k = kernel_us(lambda: fused(i))
        assert len(k) == 1, "one launch"
        tf.append(k[0])
        t_torch, t_q = chained(i, ovh)
        nk = len(t_torch) + len(t_q)
        tt.append(sum(t_torch))
        tq.append(sum(t_q))
        traw.append(sum(t_torch) + len(t_torch) * ovh + sum(t_q))
        tc.append(sum(t_torch) + sum(t_q))
    f_us, c_us = med(tf), med(tc)
    say(f"{name:24s} {shape:>18s} {fmt:6s} {f_us:9.2f} {need / f_us * 1e-6:6.2f} | {c_us:9.2f} {med(tt):8.2f} {med(tq):13.2f} {need / c_us * 1e-6:6.2f} "
        f"{med(traw):12.2f} {nk:4d} | {f_us / c_us:13.3f}")


def time_producers(a, dev, g, ovh):
    bf = torch.bfloat16
    say(f"{'line (bf16)':24s} {'tensor':>18s} {'format':6s} {'fused us':>9s} {'TB/s':>6s} | {'chain us':>9s} {'(torch':>8s} {'+ quantiser)':>13s} {'TB/s':>6s} "
        f"{'uncorrected':>12s} {'ops':>4s} | {'fused / chain':>13s}")
    rnd = lambda *s: torch.randn(s, device=dev, generator=g, dtype=torch.float32)   # noqa: E731
    for rows, cols, gated, acts in ACT_LINES:
        width = 2 * cols if gated else cols
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (2 * rows * width))))
        xs = [rnd(rows, width).to(bf) for _ in range(nbuf)]
        for act in acts:
            for fmt in FORMATS:
                need = rows * cols * (2 * (2 if gated else 1) + (0.5 if fmt == "mxfp4" else 1.0) + 1 / 32)
                compare(("gated " if gated else "") + act, f"{rows} x {'2 x ' if gated else ''}{cols}", fmt, need,
                        lambda i: N.fp8_act_quantize(xs[i % nbuf], act, gated, fmt), lambda i, o: act_chain(xs[i % nbuf], act, gated, fmt, o), a.iters, ovh)
        del xs
    for name, rows, cols, norm, has_w, has_res, rpm in NORM_LINES:
        per_copy = (2 + (2 if has_res else 0)) * rows * cols
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // per_copy)))
        B = rows // rpm if rpm else 1
        shape = (B, rpm, cols) if rpm else (rows, cols)
        xs = [rnd(*shape).to(bf) for _ in range(nbuf)]
        rs = [rnd(*shape).to(bf) for _ in range(nbuf)] if has_res else None
        w = (1 + 0.1 * rnd(cols)).to(bf) if has_w else None
        mod = ((0.1 * rnd(B, 1, cols)).to(bf), (0.1 * rnd(B, 1, cols)).to(bf)) if rpm else None
        for fmt in FORMATS:
            need = rows * cols * (2 + (4 if has_res else 0) + (0.5 if fmt == "mxfp4" else 1.0) + 1 / 32)
            compare(name, f"{rows} x {cols}", fmt, need,
                    lambda i: N.fp8_norm_quantize(xs[i % nbuf], norm, weight=w, eps=EPS, residual=rs[i % nbuf] if has_res else None,
                                                  mod_scale=mod[0] if mod else None, mod_shift=mod[1] if mod else None, scale=fmt),
                    lambda i, o: norm_chain(xs[i % nbuf], norm, w, rs[i % nbuf] if has_res else None, mod, fmt, o), a.iters, ovh)
        del xs, rs


def bracket(fused, composed, iters):
    for i in range(5):
        fused(i)
        composed(i)
    torch.cuda.synchronize()
    tf, tc = [], []
    for i in range(iters):
        for fn, acc in ((fused, tf), (composed, tc)):
            ev = Events()
            ev.run(lambda: fn(i))
            acc.append(ev.us()[0])
    return med(tf), med(tc)


def time_ops(a, dev, g):
    bf = torch.bfloat16
    rnd = lambda *s: torch.randn(s, device=dev, generator=g, dtype=torch.float32)   # noqa: E731
    say()
    say(f"{'op (bf16)':18s} {'M':>5s} {'K':>6s} {'H':>6s} {'N':>6s} {'format':>7s} | {'fused op us':>11s} | {'linear, torch, linear us':>25s} | {'op / chain':>11s}")
    for name, M, K, H, Nn, act, gated in MLPS:
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (M * K * 3))))
        xs = [rnd(M, K).to(bf) for _ in range(nbuf)]
        w1, w2 = rnd((2 if gated else 1) * H, K) * 0.02, rnd(Nn, H) * 0.02
        for fmt in FORMATS:
            (w1q, w1s), (w2q, w2s) = QUANT[fmt](w1), QUANT[fmt](w2)
            lin = LINEAR[fmt]

            def composed(i):
                h = lin(xs[i % nbuf], w1q, w1s)
                if gated:
                    gg, uu = h.chunk(2, -1)
                    h = TORCH_ACT[act](gg) * uu
                else:
                    h = TORCH_ACT[act](h)
                return lin(h, w2q, w2s)

            tf, tc = bracket(lambda i: MLP[fmt](xs[i % nbuf], w1q, w1s, w2q, w2s, act=act, gated=gated), composed, a.iters)
            say(f"{'mlp ' + name:18s} {M:5d} {K:6d} {H:6d} {Nn:6d} {fmt:>7s} | {tf:11.2f} | {tc:25.2f} | {tf / tc:11.3f}")
        del xs
    for name, M, K, Nn, norm, has_w, has_res, rpm in NORM_LINEARS:
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (M * K * (4 if has_res else 2)))))
        B = M // rpm if rpm else 1
        shape = (B, rpm, K) if rpm else (M, K)
        xs = [rnd(*shape).to(bf) for _ in range(nbuf)]
        rs = [rnd(*shape).to(bf) for _ in range(nbuf)] if has_res else None
        nw = (1 + 0.1 * rnd(K)).to(bf) if has_w else None
        mod = ((0.1 * rnd(B, 1, K)).to(bf), (0.1 * rnd(B, 1, K)).to(bf)) if rpm else None
        w = rnd(Nn, K) * 0.02
        for fmt in FORMATS:
            wq, ws = QUANT[fmt](w)

            def fused(i):
                return NORM_LINEAR[fmt](xs[i % nbuf], wq, ws, norm, nw, None, EPS, rs[i % nbuf] if has_res else None, mod[0] if mod else None,
                                        mod[1] if mod else None)

            def composed(i):
                y, h = torch_norm(xs[i % nbuf], norm, nw, rs[i % nbuf] if has_res else None, mod, None)
                return LINEAR[fmt](y, wq, ws), h

            tf, tc = bracket(fused, composed, a.iters)
            say(f"{'nl ' + name:18s} {M:5d} {K:6d} {'':>6s} {Nn:6d} {fmt:>7s} | {tf:11.2f} | {tc:25.2f} | {tf / tc:11.3f}")
        del xs, rs


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=0)
    ap.add_argument("--no-ops", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    say(f"{torch.cuda.get_device_name(0)}; bf16; times in us, median of {a.iters} alternating calls; tools/time_mx_fused.py")
    one = torch.zeros(1, device=dev)
    ev = Events()
    for _ in range(50):
        ev.run(lambda: one + 1)
    ovh = med(ev.us()[10:])
    say(f"event overhead (a bracket around a one-element torch kernel): median {ovh:.2f} us, subtracted from every torch bracket below")
    time_producers(a, dev, g, ovh)
    if not a.no_ops:
        time_ops(a, dev, g)
    if OUT is not None:
        OUT.close()


if __name__ == "__main__":
    main()
