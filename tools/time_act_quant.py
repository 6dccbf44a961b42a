#!/usr/bin/env python3
"""Times the fused activation (+ gate product) + quantisation launch (fp8mi_act_quantize) against the chain that gives the same result
without it: torch's activation (and multiply) on the GPU, then fp8_quantize_rowwise or fp8_quantize_blockwise(., 1); and fp8_mlp_rowwise /
fp8_mlp_blockwise against fp8_linear_*, torch's activation, fp8_linear_*.

The library's launches are timed per dispatch (fp8mi_profile_begin / _end: the dispatch packet's timestamps).  Torch's kernels are not
visible to that hook: each torch op is bracketed by two events on the stream.  So that both candidates are on one clock, the interval
around a one-element torch kernel (printed as `event overhead`: the bracket plus that kernel's own microsecond or two) is SUBTRACTED from
every bracket, which errs in the chain's favour.  The chain's figure is the SUM of its kernels (torch ops by corrected events, the quantiser
by its dispatch), gaps between them not included; the uncorrected sum is printed beside it.  The MLPs are bracketed by events as a whole,
both candidates alike.
After warm-up, the candidates ALTERNATE call by call in one process; median of --iters (>= 20).  Bytes/s are over the bytes the recipe has
to move once: (gated ? 2 : 1) esz + 1 per output element.

The tensors rotate over enough copies to exceed the 256 MiB of last-level cache (at most 64), so a call does not find its input where
the previous call left it.
    python tools/time_act_quant.py [--iters 30] [--buffers N] [--no-mlps]
FP8MI_LIB_PATH=<another build of the library> runs the same lines on that build (how profiles/act_quant_hold_or_recompute.txt was made:
the chain's columns, which never touch the new kernels, are the control between the two runs).
    python tools/time_act_quant.py --report      the largest byte share / scale distance against tests/act_quant_ref.py per activation"""
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

ACTS = ("silu", "gelu_tanh", "gelu_erf")
# (rows, output columns, gated, acts): FLUX's MLP hidden; a Llama-3 8B gate_up output at prefill and at decode; the FLUX activation itself
TENSORS = [(4096, 12288, False, ACTS), (4096, 14336, True, ACTS), (64, 14336, True, ("silu",)), (1, 14336, True, ("silu",)),
           (4096, 3072, False, ("none",))]
MLPS = [("FLUX gelu_tanh", 4096, 3072, 12288, 3072, "gelu_tanh", False), ("8B SwiGLU", 4096, 4096, 14336, 4096, "silu", True),
        ("8B SwiGLU decode", 64, 4096, 14336, 4096, "silu", True)]
CACHE_BYTES = 256 << 20
TORCH_ACT = {"none": lambda t: t, "silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "gelu_erf": F.gelu}


def kernel_us(fn):
    """-> the kernel times (us) of the library launches one call of fn makes"""
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


def torch_y(x, act, gated, ev):
    """the activation (and the gate product) with torch ops, each bracketed: what eager torch runs between the two linears"""
    if not gated:
        return x if act == "none" else ev.run(lambda: TORCH_ACT[act](x))
    g, u = x.chunk(2, -1)
    a = g if act == "none" else ev.run(lambda: TORCH_ACT[act](g))
    return ev.run(lambda: a * u)


def chain(x, act, gated, scale, overhead=0.0):
    """-> (us of torch's kernels, each bracket less `overhead`; us of the quantiser's launches)"""
    ev = Events()
    y = torch_y(x, act, gated, ev)
    t_torch = [max(0.0, t - overhead) for t in ev.us()]
    t_q = kernel_us(lambda: N.fp8_quantize_rowwise(y, encode_mode=L.ENC_RNE) if scale == "row" else N.fp8_quantize_blockwise(y, 1))
    return t_torch, t_q


def med(v):
    return statistics.median(v)


def time_tensors(a, dev, g):
    one = torch.zeros(1, device=dev)
    ev = Events()
    for _ in range(50):
        ev.run(lambda: one + 1)
    ovh = med(ev.us()[10:])
    print(f"event overhead (a bracket around a one-element torch kernel): median {ovh:.2f} us, subtracted from every torch bracket below")
    print(f"{'tensor (bf16)':26s} {'act':10s} {'scale':9s} {'fused us':>9s} {'TB/s':>6s} | {'chain us':>9s} {'(torch':>8s} {'+ quantiser)':>13s} {'TB/s':>6s} "
          f"{'uncorrected':>12s} | {'fused / chain':>13s}")
    for rows, cols, gated, acts in TENSORS:
        width = 2 * cols if gated else cols
        need = (2 * (2 if gated else 1) + 1) * rows * cols
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // need)))
        xs = [torch.randn((rows, width), device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16) for _ in range(nbuf)]
        for act in acts:
            for scale in ("row", "block128"):
                fused = lambda i: N.fp8_act_quantize(xs[i % nbuf], act, gated, scale, encode_mode=L.ENC_RNE)   # noqa: E731
                for i in range(5):
                    fused(i)
                    chain(xs[i % nbuf], act, gated, scale)
                tf, tc, tt, tq, traw = [], [], [], [], []
                for i in range(a.iters):
                    k = kernel_us(lambda: fused(i))
                    assert len(k) == 1, "one launch"
                    tf.append(k[0])
                    t_torch, t_q = chain(xs[i % nbuf], act, gated, scale, ovh)
                    tt.append(sum(t_torch))
                    traw.append(sum(t_torch) + len(t_torch) * ovh + sum(t_q))
                    tq.append(sum(t_q))
                    tc.append(sum(t_torch) + sum(t_q))
                f_us, c_us = med(tf), med(tc)
                name = f"{rows} x {'2 x ' if gated else ''}{cols}"
                print(f"{name:26s} {act:10s} {scale:9s} {f_us:9.2f} {need / f_us * 1e-6:6.2f} | {c_us:9.2f} {med(tt):8.2f} {med(tq):13.2f} "
                      f"{need / c_us * 1e-6:6.2f} {med(traw):12.2f} | {f_us / c_us:13.3f}", flush=True)
        del xs


def time_mlps(a, dev, g):
    print()
    print(f"{'MLP (bf16)':18s} {'M':>5s} {'K':>6s} {'H':>6s} {'N':>6s} {'recipe':>10s} | {'fp8_mlp us':>11s} | {'linear, torch act, linear us':>29s} | {'mlp / composition':>18s}")
    for name, M, K, H, Nn, act, gated in MLPS:
        nbuf = a.buffers or min(64, max(2, -(-2 * CACHE_BYTES // (M * K * 3))))
        xs = [torch.randn((M, K), device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16) for _ in range(nbuf)]
        w1 = torch.randn(((2 if gated else 1) * H, K), device=dev, generator=g) * 0.02
        w2 = torch.randn((Nn, H), device=dev, generator=g) * 0.02
        for recipe in ("rowwise", "blockwise"):
            if recipe == "rowwise":
                (w1q, w1s), (w2q, w2s) = N.fp8_quantize_rowwise(w1), N.fp8_quantize_rowwise(w2)
                mlp, lin = N.fp8_mlp_rowwise, N.fp8_linear_rowwise
            else:
                (w1q, w1s), (w2q, w2s) = N.fp8_quantize_blockwise(w1, 128), N.fp8_quantize_blockwise(w2, 128)
                mlp, lin = N.fp8_mlp_blockwise, N.fp8_linear_blockwise

            def fused(i):
                return mlp(xs[i % nbuf], w1q, w1s, w2q, w2s, act=act, gated=gated)

            def composed(i):
                h = lin(xs[i % nbuf], w1q, w1s)
                if gated:
                    gg, uu = h.chunk(2, -1)
                    h = TORCH_ACT[act](gg) * uu
                else:
                    h = TORCH_ACT[act](h)
                return lin(h, w2q, w2s)

            for i in range(5):
                fused(i)
                composed(i)
            torch.cuda.synchronize()
            tf, tc = [], []
            for i in range(a.iters):
                for fn, acc in ((fused, tf), (composed, tc)):
                    ev = Events()
                    ev.run(lambda: fn(i))
                    acc.append(ev.us()[0])
            print(f"{name:18s} {M:5d} {K:6d} {H:6d} {Nn:6d} {recipe:>10s} | {med(tf):11.2f} | {med(tc):29.2f} | {med(tf) / med(tc):18.3f}", flush=True)
        del xs


def report(dev):
    """the largest share of bytes off by one and the largest relative scale distance against the float64-derived reference, per act"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import act_quant_ref as A
    rng = np.random.default_rng(0)
    print(f"{torch.cuda.get_device_name(0)}; fp8mi_act_quantize against tests/act_quant_ref.py (float64, rounded once), OCP rounding; 257 rows with "
          "magnitudes 2^-8 .. 2^7")
    print(f"{'act':10s} {'gated':>5s} {'dtype':>9s} {'scale':>9s} {'cols':>6s} | {'bytes off by one':>17s} {'largest distance':>17s} {'scales, relative':>17s}")
    for act in ACTS:
        for gated in (False, True):
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                for cols in (7, 1024, 4100, 16400):
                    x = rng.standard_normal((257, 2 * cols if gated else cols)) * np.exp2(rng.integers(-8, 8, size=(257, 1)))
                    x = torch.from_numpy(x.astype(np.float32)).to(dt)
                    y = A.act_y(x, act, gated)
                    for scale in ("row", "block128"):
                        q, s = N.fp8_act_quantize(x.to(dev), act, gated, scale, encode_mode=L.ENC_RNE)
                        wq, ws, _ = A.act_quantize_ref(None, scale=scale, mode=L.ENC_RNE, y=y)
                        d = np.abs(q.cpu().numpy().astype(np.int32) - wq.astype(np.int32))
                        gs = s.cpu().numpy().reshape(ws.shape).astype(np.float64)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            rel = np.where(gs == ws, 0.0, np.abs(gs - ws) / np.abs(ws))
                        print(f"{act:10s} {int(gated):5d} {str(dt)[6:]:>9s} {scale:>9s} {cols:6d} | {(d != 0).mean():17.2e} {int(d.max()):17d} {rel.max():17.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=0)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--no-mlps", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 20, "median of at least 20"
    dev = torch.device("cuda")
    if a.report:
        return report(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}; times in us, median of {a.iters} alternating calls")
    time_tensors(a, dev, g)
    if not a.no_mlps:
        time_mlps(a, dev, g)


if __name__ == "__main__":
    main()
