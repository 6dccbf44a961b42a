#!/usr/bin/env python3
"""Times the fused normalisation + quantisation launch (fp8mi_norm_quantize) against the chain that gives the same operand without it:
torch's layer_norm / rms_norm (and the residual add or the adaLN modulation) on the GPU, then fp8_quantize_rowwise or
fp8_quantize_blockwise(., 1).  The method is tools/time_act_quant.py's:

The library's launches are timed per dispatch (fp8mi_profile_begin / _end: the dispatch packet's timestamps).  Torch's kernels are not
visible to that hook: each torch op is bracketed by two events on the stream, and the interval around a one-element torch kernel (printed
as `event overhead`) is SUBTRACTED from every bracket, which errs in the chain's favour.  The chain's figure is the SUM of its kernels, gaps
between them not included; the uncorrected sum is printed beside it.  After warm-up the candidates ALTERNATE call by call in one process;
median of --iters (>= 20).  The tensors rotate over enough copies to exceed the 256 MiB of last-level cache (at most 64).  TB/s are over
the bytes the recipe has to move once: x (and the residual) read, h written, one FP8 byte written per element.
    timeout -k 10 420 python tools/time_norm_quant.py [--iters 30] [--buffers N]
It is one process on the GPU with no time limit of its own: run it under `timeout`, as above (a minute on an MI355X)."""
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

# (name, rows, cols, norm, weight, residual, modulation: rows per image or 0)
LINES = [("FLUX adaLN", 4096, 3072, "layer", False, False, 1024),
         ("8B rms + w + residual", 4096, 4096, "rms", True, True, 0), ("8B rms + w + residual", 64, 4096, "rms", True, True, 0),
         ("8B rms + w + residual", 1, 4096, "rms", True, True, 0),
         ("rms", 4096, 12288, "rms", False, False, 0)]
CACHE_BYTES = 256 << 20
EPS = 1e-6


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


def chain(x, norm, w, res, mod, scale, overhead=0.0):
    """eager torch up to y, each op bracketed, then the existing quantiser -> (us of torch's kernels less `overhead` each, us of the quantiser)"""
    ev = Events()
    C = x.shape[-1]
    h = x if res is None else ev.run(lambda: x + res)
    y = ev.run(lambda: F.layer_norm(h, (C,), w, None, EPS)) if norm == "layer" else ev.run(lambda: F.rms_norm(h, (C,), w, EPS))
    if mod is not None:
        sc, sh = mod
        t = ev.run(lambda: 1 + sc)
        y = ev.run(lambda: y * t)
        y = ev.run(lambda: y + sh)
    t_torch = [max(0.0, t - overhead) for t in ev.us()]
    y2 = y.reshape(-1, C)
    t_q = kernel_us(lambda: N.fp8_quantize_rowwise(y2, encode_mode=L.ENC_RNE) if scale == "row" else N.fp8_quantize_blockwise(y2, 1))
    return t_torch, t_q


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=0)
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}; bf16; times in us, median of {a.iters} alternating calls")
    one = torch.zeros(1, device=dev)
    ev = Events()
    for _ in range(50):
        ev.run(lambda: one + 1)
    ovh = med(ev.us()[10:])
    print(f"event overhead (a bracket around a one-element torch kernel): median {ovh:.2f} us, subtracted from every torch bracket below")
    print(f"{'line':22s} {'tensor':>13s} {'scale':9s} {'fused us':>9s} {'TB/s':>6s} | {'chain us':>9s} {'(torch':>8s} {'+ quantiser)':>13s} {'TB/s':>6s} "
          f"{'uncorrected':>12s} {'ops':>8s} | {'fused / chain':>13s}")
    bf = torch.bfloat16
    for name, rows, cols, norm, has_w, has_res, rpm in LINES:
        need = (2 + (4 if has_res else 0) + 1) * rows * cols
        per_copy = (2 + (2 if has_res else 0)) * rows * cols
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // per_copy)))
        rnd = lambda *s: torch.randn(s, device=dev, generator=g, dtype=torch.float32)   # noqa: E731
        B = rows // rpm if rpm else 1
        shape = (B, rpm, cols) if rpm else (rows, cols)
        xs = [rnd(*shape).to(bf) for _ in range(nbuf)]
        rs = [rnd(*shape).to(bf) for _ in range(nbuf)] if has_res else None
        w = (1 + 0.1 * rnd(cols)).to(bf) if has_w else None
        mod = ((0.1 * rnd(B, 1, cols)).to(bf), (0.1 * rnd(B, 1, cols)).to(bf)) if rpm else None
        for scale in ("row", "block128"):
            def fused(i):
                return N.fp8_norm_quantize(xs[i % nbuf], norm, weight=w, eps=EPS, residual=rs[i % nbuf] if has_res else None,
                                           mod_scale=mod[0] if mod else None, mod_shift=mod[1] if mod else None, scale=scale, encode_mode=L.ENC_RNE)

            def chained(i, o=0.0):
                return chain(xs[i % nbuf], norm, w, rs[i % nbuf] if has_res else None, mod, scale, o)

            for i in range(5):
                fused(i)
                chained(i)
            tf, tc, tt, tq, traw, nk = [], [], [], [], [], 0
            for i in range(a.iters):
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
            print(f"{name:22s} {f'{rows} x {cols}':>13s} {scale:9s} {f_us:9.2f} {need / f_us * 1e-6:6.2f} | {c_us:9.2f} {med(tt):8.2f} {med(tq):13.2f} "
                  f"{need / c_us * 1e-6:6.2f} {med(traw):12.2f} {nk:8d} | {f_us / c_us:13.3f}", flush=True)
        del xs, rs


if __name__ == "__main__":
    main()
