"""References for the MoE routing ops, written from the definitions in include/fp8mi.h in torch on the CPU.

route_ref      the stable sort: torch.sort(stable=True) over the valid ids, bincount, cumsum
route_brute    the same outputs from the definitions' own counts, O(n^2): what route_ref is checked against
combine_ref    the sequential float32 loop acc = acc + w[:, j] * y[row]
combine_f64    the exact sum and the sum of magnitudes, in float64: the independent bound"""
import torch


def route_ref(ids: torch.Tensor, G: int):
    """ids: any integer tensor of n assignments (flattened row-major).  -> (offs [G], row_of [n], src_of_row [n]), int32, CPU."""
    flat = ids.detach().cpu().reshape(-1).to(torch.int64)
    n = flat.numel()
    valid = (flat >= 0) & (flat < G)
    idx = torch.nonzero(valid).reshape(-1)
    order = torch.sort(flat[idx], stable=True).indices
    counts = torch.bincount(flat[idx], minlength=G)[:G]
    offs = torch.cumsum(counts, 0).to(torch.int32)
    src_of_row = torch.full((n,), -1, dtype=torch.int32)
    src_of_row[: idx.numel()] = idx[order].to(torch.int32)
    row_of = torch.full((n,), -1, dtype=torch.int32)
    row_of[idx[order]] = torch.arange(idx.numel(), dtype=torch.int32)
    return offs, row_of, src_of_row


def route_brute(ids, G: int):
    """The definitions, count by count: offs[g] = #{valid i : ids[i] <= g}; row_of[i] = (g ? offs[g-1] : 0) + #{i' < i : ids[i'] = ids[i]}."""
    flat = [int(v) for v in ids]
    n = len(flat)
    ok = [0 <= v < G for v in flat]
    offs = [sum(1 for i in range(n) if ok[i] and flat[i] <= g) for g in range(G)]
    row_of = [-1] * n
    src_of_row = [-1] * n
    for i in range(n):
        if ok[i]:
            g = flat[i]
            row_of[i] = (offs[g - 1] if g else 0) + sum(1 for j in range(i) if flat[j] == g)
            src_of_row[row_of[i]] = i
    return offs, row_of, src_of_row


def combine_ref(y: torch.Tensor, row_of: torch.Tensor, weights, out_dtype):
    """y (rows, N), row_of (T, k) int, weights (T, k) float32 or None -> (T, N) out_dtype: two rounded float32 operations per assignment,
    j = 0 .. k-1 in order; an assignment whose row is outside [0, rows) is skipped."""
    y = y.detach().cpu()
    row_of = row_of.detach().cpu().to(torch.int64)
    T, k = row_of.shape
    rows = y.shape[0]
    acc = torch.zeros((T, y.shape[1]), dtype=torch.float32)
    yf = y.float()
    for j in range(k):
        r = row_of[:, j]
        ok = (r >= 0) & (r < rows)
        rows_j = yf[torch.where(ok, r, torch.zeros_like(r))] if rows > 0 else torch.zeros_like(acc)
        w = weights.detach().cpu().float()[:, j:j + 1] if weights is not None else torch.ones((T, 1), dtype=torch.float32)
        prod = w * rows_j
        acc = torch.where(ok[:, None], acc + prod, acc)
    return acc.to(out_dtype)


def combine_f64(y: torch.Tensor, row_of: torch.Tensor, weights):
    """-> (sum, sum of |w y|), float64 (T, N)"""
    y = y.detach().cpu().double()
    row_of = row_of.detach().cpu().to(torch.int64)
    T, k = row_of.shape
    rows = y.shape[0]
    total = torch.zeros((T, y.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(total)
    for j in range(k):
        r = row_of[:, j]
        ok = ((r >= 0) & (r < rows))[:, None]
        rows_j = y[torch.where(ok[:, 0], r, torch.zeros_like(r))] if rows > 0 else torch.zeros_like(total)
        w = weights.detach().cpu().double()[:, j:j + 1] if weights is not None else torch.ones((T, 1), dtype=torch.float64)
        total = total + torch.where(ok, w * rows_j, torch.zeros_like(total))
        mag = mag + torch.where(ok, (w * rows_j).abs(), torch.zeros_like(total))
    return total, mag
