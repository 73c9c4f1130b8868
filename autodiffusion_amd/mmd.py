"""What the two MMD^2 metrics share: KID (kid.py, cubic polynomial kernel on pool3 features) and CMMD (cmmd.py, Gaussian RBF kernel on
CLIP embeddings).  Both take three float64 pair sums from one tile loop (csrc/adm_pairsum.h) and combine them here:

* sums        S_xy = sum_i sum_j k(x_i, y_j);   S_xx = sum_{i != j} k(x_i, x_j)  (the diagonal is left out);
* estimators  MMD^2_u = S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m),  n, m >= 2;
              MMD^2_v = S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)  (the full-matrix means; the diagonal must add nothing to the sums).

Host tensors raise ``AdmError``: there is no CPU fallback, as in fid.py.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import AdmError

TILE = 64            # csrc/adm_pairsum.h: a block owns one 64 x 64 tile of the Gram
FINAL_THREADS = 256  # ... and the last pass is one block of 256 threads


def pair_blocks(n: int, m: int, self_pairs: bool) -> int:
    """Blocks (= per-block partials in the workspace) of the tile pass of adm_poly3_sums / adm_rbf_sums: the tiles of the rectangle, or
    of the triangle on and above the diagonal."""
    ti, tj = -(-n // TILE), -(-m // TILE)
    return ti * (ti + 1) // 2 if self_pairs else ti * tj


def reduction_chain(n: int, m: int, self_pairs: bool) -> int:
    """The longest chain of rounding float64 additions behind a pair sum's out[0] (the L of the tests' error bounds): 16 per lane
    (2 x 2 MFMA tiles x 4 results), 6 xor shuffles across the wave, 3 across the block's 4 waves, then ceil(blocks / 256) per thread
    and an 8-level tree in the last pass -- and never more than the number of pairs summed: a masked entry enters as an exact 0.0,
    and adding zero does not round.  The doubling of a tile above the diagonal is exact."""
    pairs = n * (n - 1) if self_pairs else n * m
    return min(16 + 6 + 3 + -(-pair_blocks(n, m, self_pairs) // FINAL_THREADS) + 8, pairs)


def device_rows(t, name: str, metric: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise AdmError(f"{name}: expected fp32 device rows [n, d] (the {metric} kernel has no CPU fallback)")
    return t.to(torch.float32).contiguous()


def mmd2_from_sums(s_xx: float, n: int, s_yy: float, m: int, s_xy: float, unbiased: bool = False) -> float:
    """MMD^2_v (unbiased False) or MMD^2_u from the three sums.  The two self terms are added first, so swapping the sets changes
    nothing but S_xy's own summation order."""
    n, m = int(n), int(m)
    if unbiased:
        if n < 2 or m < 2:
            raise ValueError(f"the unbiased MMD^2 needs at least 2 rows in each set (n={n}, m={m})")
        return (s_xx / (n * (n - 1.0)) + s_yy / (m * (m - 1.0))) - 2.0 * s_xy / (float(n) * m)
    if n < 1 or m < 1:
        raise ValueError(f"MMD^2 needs at least 1 row in each set (n={n}, m={m})")
    return (s_xx / (float(n) * n) + s_yy / (float(m) * m)) - 2.0 * s_xy / (float(n) * m)


def load_ref_rows(path: str, key: str, writer: str) -> np.ndarray:
    """The array `key` (fp32 [m >= 2, d]) of an .npz; `writer` names the command line that writes such a file."""
    with np.load(path, allow_pickle=False) as z:
        if key not in z.files:
            raise KeyError(f"{path}: no array '{key}' (members: {sorted(z.files)}); write it with {writer}")
        feats = np.asarray(z[key], dtype=np.float32)
    if feats.ndim != 2 or feats.shape[0] < 2:
        raise ValueError(f"{path}: {key} must be [m >= 2, d], got {feats.shape}")
    return feats


class PairSumReference:
    """The reference rows on the device with their self sum S_yy, computed once by the subclass's self_sum: a candidate then costs
    two kernel sums."""

    def __init__(self, feats, device=None):
        if isinstance(feats, torch.Tensor) and device is None:
            device = feats.device
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.y = torch.as_tensor(feats).to(device=device, dtype=torch.float32).contiguous()
        if self.y.dim() != 2 or self.y.shape[0] < 2:
            raise ValueError(f"{type(self).__name__}: reference rows must be [m >= 2, d], got {tuple(self.y.shape)}")
        self.s_yy = self.self_sum()


def pooled_rows(rows: torch.Tensor, group=None, local: bool = False) -> torch.Tensor:
    """Every rank's rows, concatenated in rank order (local=True, or no collectives: this rank's rows as they are).  Ranks may
    hold different numbers of rows: the counts are gathered first (8 bytes per rank), then ONE all_gather moves each rank's block
    padded to the largest count.  RCCL gathers device tensors, gloo host copies, like ActivationAccumulator.pooled; the result
    lives where `rows` does."""
    import torch.distributed as dist
    from .dist_util import collectives_on
    if local or not collectives_on(group):
        return rows
    world = dist.get_world_size(group)
    comm_dev = rows.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    count = torch.tensor([rows.shape[0]], dtype=torch.int64, device=comm_dev)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count, group=group)
    counts = [int(c.item()) for c in counts]
    cap = max(max(counts), 1)
    mine = torch.zeros((cap,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=comm_dev)
    mine[:rows.shape[0]] = rows.to(comm_dev)
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], 0).to(rows.device)
