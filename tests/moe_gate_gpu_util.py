"""What tests/test_gpu_moe_gate.py and tests/test_gpu_moe_gate_edges.py share: the runner of fp8mi_moe_gate (both outputs between guard
elements prefilled with a sentinel) and the two checks against tests/moe_gate_ref.py.  A plain module: no fixtures, no tests."""
import numpy as np
import torch

import fp8_mi355x_lib as L
from moe_gate_ref import ABS, REL, SKIP_CAP, gate_ref, weights_at
from moe_route_gpu_util import DEV, SENT_F, SENT_I, bits, guarded, guards_intact, stream

CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
SCORING = {"softmax": L.GATE_SOFTMAX, "sigmoid": L.GATE_SIGMOID}
GROUP_SCORE = {"max": L.GATE_GROUP_MAX, "top2": L.GATE_GROUP_TOP2}


def run_gate(lib, logits, k, scoring="softmax", renormalize=False, scale=1.0, bias=None, n_group=1, topk_group=1, group_score="max"):
    """fp8mi_moe_gate on a (T, G) device tensor with a unit column stride, read in place -> (ids (T, k) int32, weights (T, k) float32) on the
    CPU.  One launch; the guards around both outputs intact; every weight written; every token's ids k distinct experts."""
    T, G = logits.shape
    assert logits.stride(1) == 1 or G == 1
    ids_buf, ids = guarded(T * k, torch.int32, SENT_I)
    w_buf, w = guarded(T * k, torch.float32, SENT_F)
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_moe_gate(logits.data_ptr(), CODE[logits.dtype], T, G, logits.stride(0) if T > 1 else G, bias.data_ptr() if bias is not None else None,
                                k, SCORING[scoring], int(renormalize), scale, n_group, topk_group, GROUP_SCORE[group_score], ids.data_ptr(), w.data_ptr(),
                                stream())
    L.check(rc, "fp8mi_moe_gate")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1
    assert guards_intact(ids_buf, T * k, SENT_I) and guards_intact(w_buf, T * k, SENT_F)
    ids, w = ids.reshape(T, k).cpu(), w.reshape(T, k).cpu()
    assert bool((bits(w) != bits(torch.tensor([SENT_F]))).all()), "a weight was not written"
    srt = ids.sort(dim=1).values
    assert bool((ids >= 0).all()) and bool((ids < G).all()) and bool((srt[:, 1:] != srt[:, :-1]).all()), "ids are not k distinct experts"
    return ids, w


def check_weights(w, scores, ids, scoring, renormalize, scale, what):
    want = weights_at(scores, ids.numpy(), renormalize, scale)
    err = np.abs(w.numpy().astype(np.float64) - want)
    tol = REL[scoring] * np.abs(want) + ABS
    assert bool((err <= tol).all()), (what, float((err / tol).max()))


def compare_scored(ids, w, r, kw, what, skip=True):
    """Device ids and weights of a scored-form run against its reference `r`: tolerances 1 and 2 of moe_gate_ref.py.  -> the share of
    tokens left out of the id comparison"""
    close = r.close if skip else np.zeros_like(r.close)
    share = float(close.mean())
    print(f"{what}: {100 * share:.2f} % of the tokens left out of the id comparison")
    assert share <= SKIP_CAP, (what, share)
    got, want = np.sort(ids.numpy().astype(np.int64), axis=1), np.sort(r.ids, axis=1)
    differ = (got != want).any(axis=1)
    assert not bool((differ & ~close).any()), (what, int((differ & ~close).sum()), np.nonzero(differ & ~close)[0][:8].tolist())
    check_weights(w, r.scores, ids, kw["scoring"], kw["renormalize"], kw["scale"], what)
    return share


def check_scored(lib, x, bias, kw, what, skip=True):
    """-> (device ids, the reference).  Tolerances 1 and 2 of moe_gate_ref.py."""
    r = gate_ref(x, bias=bias, **kw)
    bias_dev = None if bias is None else torch.from_numpy(bias).to(DEV)
    ids, w = run_gate(lib, torch.from_numpy(x).to(DEV), bias=bias_dev, **kw)
    compare_scored(ids, w, r, kw, what, skip)
    return ids, r
