"""reference trackers/utils/matching.py:20-61, on device tensors."""
import torch

from ...nn import _ops


def linear_assignment(cost_matrix, thresh):
    """cost_matrix: float32 (n, m) device tensor -> (matches (k, 2) int64 [row, column] by ascending row, unmatched_a (rows), unmatched_b
    (columns)), device tensors: the partial matching that minimises the sum of (cost - thresh), pairs above thresh excluded -- what the
    reference gets from lap.lapjv(cost, extend_cost=True, cost_limit=thresh).  Equal optima may be resolved differently."""
    n, m = int(cost_matrix.shape[0]), int(cost_matrix.shape[1])
    dev = cost_matrix.device
    if n == 0 or m == 0:
        return torch.empty((0, 2), dtype=torch.int64, device=dev), torch.arange(n, device=dev), torch.arange(m, device=dev)
    c = cost_matrix if cost_matrix.dtype == torch.float32 and cost_matrix.stride(1) == 1 else cost_matrix.float().contiguous()
    r2c, c2r = _ops.linear_assignment([c], thresh)
    r2c, c2r = r2c[0, :n].long(), c2r[0, :m].long()
    rows = torch.nonzero(r2c >= 0)[:, 0]
    return torch.stack([rows, r2c[rows]], 1), torch.nonzero(r2c < 0)[:, 0], torch.nonzero(c2r < 0)[:, 0]
