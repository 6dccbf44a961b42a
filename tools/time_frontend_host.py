"""Host cost of the op layer's front ends, without a GPU: the fused producers and the dense layer ops of two checkouts of the package - a
parent and a change - each called on its plain (4, 64) bfloat16 case with the library replaced by a stub whose every entry point returns 0
(what tests/gemm_frontend_cases.py's recorder does, without its bookkeeping), so that what is timed is the Python between the caller and the
one ctypes call: validation, views, allocations, argument tuples.

    python tools/time_frontend_host.py --parent PARENT_PACKAGE_DIR [--change PACKAGE_DIR] [--calls 2000] [--rounds 5]

Both modules live in ONE process (loaded under two names; fp8_mi355x_lib is the change's, which a front-end refactor does not touch, and
its load() is replaced for the whole process: this tool is for a process of its own) and
take turns: a round times every function on one side and at once on the other, the side that goes first alternating from round to round;
a round's figure per function is the median of `calls` perf_counter_ns intervals.  Per function the limit is
    slowest parent round x (1 + the largest relative difference between any two parent rounds)
and the change's figure is the median of its rounds.  Also printed: the median of change / parent over all functions."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name, package_dir):
    spec = importlib.util.spec_from_file_location(name, os.path.join(package_dir, "fp8_mi355x_native.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


class Stub:
    def __getattr__(self, entry):
        return lambda *args: 0


def calls_of(native):
    """-> {function name: a call of it on its plain case}"""
    import torch
    bf16, u8 = torch.bfloat16, torch.uint8
    K, N, H = 64, 32, 32
    x = torch.zeros(4, K, dtype=bf16)
    row_of = torch.zeros(4, 2, dtype=torch.int32)
    e8m0 = lambda rows, k: torch.full((rows, k // 32), 127, dtype=u8)   # noqa: E731
    # recipe -> (the suffix of its linear (None: fp8_linear alone), elements per weight byte, the scales of a (rows, k) weight)
    dense = {"tensor": (None, 1, lambda rows, k: torch.ones(1)), "rowwise": ("_rowwise", 1, lambda rows, k: torch.ones(rows)),
             "blockwise": ("_blockwise", 1, lambda rows, k: torch.ones((rows + 127) // 128, (k + 127) // 128)),
             "mxfp8": ("_mxfp8", 1, e8m0), "mxfp4": ("_mxfp4", 2, e8m0), "mxw4a8": ("_mxw4a8", 2, e8m0)}
    out = {"fp8_act_quantize": lambda: native.fp8_act_quantize(x, "silu"), "fp8_norm_quantize": lambda: native.fp8_norm_quantize(x),
           "fp8_moe_scatter_quantize": lambda: native.fp8_moe_scatter_quantize(x, row_of)}
    for suffix, per_byte, scales in dense.values():
        weight = lambda rows, k: (torch.zeros(rows, k // per_byte, dtype=u8), scales(rows, k))   # noqa: E731
        (w, ws), (w1, w1s), (w2, w2s) = weight(N, K), weight(2 * H, K), weight(N, H)
        out["fp8_linear" + (suffix or "")] = lambda f=getattr(native, "fp8_linear" + (suffix or "")), w=w, ws=ws: f(x, w, ws)
        if suffix:
            out["fp8_mlp" + suffix] = lambda f=getattr(native, "fp8_mlp" + suffix), a=(w1, w1s, w2, w2s): f(x, *a)
            out["fp8_norm_linear" + suffix] = lambda f=getattr(native, "fp8_norm_linear" + suffix), w=w, ws=ws: f(x, w, ws)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", default=os.path.join(ROOT, "fp8-mps-metal_amd"))
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, a.change)
    import fp8_mi355x_lib as L
    sides = {"parent": load("native_parent", a.parent), "change": load("native_change", a.change)}
    L.load = lambda: Stub()
    for native in sides.values():
        assert native._l is L
        native.DEVICE_TYPE, native._stream = "cpu", (lambda dev: 0)
        native._workspace_on = lambda dev, stream, ws=__import__("torch").zeros(64, dtype=__import__("torch").uint8): ws
    calls = {side: calls_of(native) for side, native in sides.items()}
    names = list(calls["parent"])
    assert len(names) == 19
    rounds = {side: {n: [] for n in names} for side in sides}
    clock = time.perf_counter_ns
    for r in range(a.rounds + 1):   # (round 0 warms both sides up and is not kept)
        for n in names:
            for side in (("parent", "change") if r % 2 else ("change", "parent")):   # neither side is always the one that runs second
                fn, ts = calls[side][n], []
                for _ in range(a.calls if r else 200):
                    t0 = clock()
                    fn()
                    ts.append(clock() - t0)
                if r:
                    rounds[side][n].append(statistics.median(ts) / 1e3)
    print(f"{a.rounds} rounds, per function parent then change or change then parent in turn, {a.calls} calls per function and round; a round's figure: the median call, us")
    print(f"{'function':28s} | {'parent rounds':>34s} | {'change rounds':>34s} | {'limit':>7s} {'change':>7s} {'within':>6s} {'change / parent':>15s}")
    ratios, missed = [], []
    for n in names:
        p, c = rounds["parent"][n], rounds["change"][n]
        limit = max(p) * (1.0 + (max(p) - min(p)) / min(p))
        figure = statistics.median(c)
        ratios.append(figure / statistics.median(p))
        if figure > limit:
            missed.append(n)
        fmt = lambda v: " ".join(f"{t:6.2f}" for t in v)   # noqa: E731
        print(f"{n:28s} | {fmt(p):>34s} | {fmt(c):>34s} | {limit:7.2f} {figure:7.2f} {str(figure <= limit):>6s} {ratios[-1]:15.3f}")
    print(f"median of change / parent over the {len(names)} functions: {statistics.median(ratios):.3f} (smallest {min(ratios):.3f}, largest {max(ratios):.3f})")
    print(f"functions over their limit: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
