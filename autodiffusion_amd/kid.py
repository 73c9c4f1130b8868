"""Kernel Inception Distance on the device: the unbiased MMD^2 with the cubic polynomial kernel on the pool3 features.

Project-defined (the reference has no KID); the convention is Binkowski et al., "Demystifying MMD GANs" (2018), with
torch-fidelity's defaults:

* kernel      k(a, b) = (a . b / d + 1)^3, d the feature width;
* cross sum   S_xy = sum_i sum_j k(x_i, y_j);   self sum  S_xx = sum_{i != j} k(x_i, x_j)  (the diagonal is left out);
* estimator   MMD^2_u = S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m),  n, m >= 2  (the search fitness);
* reported    mean and np.std (ddof 0) of MMD^2_u over `subsets` draws of `subset_size` rows from each set without
              replacement, rows chosen by np.random.RandomState(seed), sample set first, then the reference set, per draw
              (defaults 100 x 1000, seed 0).

The Frechet distance is a biased estimator at the search's sizes (num_samples <= 1000, 64-image candidates), with a bias that
depends on n and on the candidate; MMD^2_u is unbiased at any n.  The three sums come from ``adm_poly3_sums``
(csrc/adm_kid.hip): an f64 matrix-core Gram of the fp32 rows with the cube and the reduction in its epilogue, so the n x m
matrix never exists in memory and every sum is float64 -- the estimator is a difference of three O(1) means whose result is
1e-5 .. 1e-3.  Host tensors raise ``AdmError``: there is no CPU fallback, as in fid.py.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import AdmError

TILE = 64            # csrc/adm_kid.hip: a block owns one 64 x 64 tile of the Gram
FINAL_THREADS = 256  # ... and the second pass is one block of 256 threads
FITNESS_SCALE = 1000.0   # KIDReference.fitness = 1000 * MMD^2_u: only makes log lines readable
SUBSET_FLAG = "--kid_subset_size"


def poly3_blocks(n: int, m: int, self_pairs: bool) -> int:
    """Blocks (= workspace elements) of adm_poly3_sums: the tiles of the rectangle, or of the triangle on and above the diagonal."""
    ti, tj = -(-n // TILE), -(-m // TILE)
    return ti * (ti + 1) // 2 if self_pairs else ti * tj


def reduction_chain(n: int, m: int, self_pairs: bool) -> int:
    """The longest chain of rounding float64 additions behind adm_poly3_sums's out[0] (the L of the tests' error bound): 16 per lane
    (2 x 2 MFMA tiles x 4 results), 6 xor shuffles across the wave, 3 across the block's 4 waves, then in the second pass
    ceil(blocks / 256) per thread and an 8-level tree -- and never more than the number of pairs summed: a masked entry enters as
    an exact 0.0, and adding zero does not round.  The doubling of a tile above the diagonal is exact."""
    pairs = n * (n - 1) if self_pairs else n * m
    return min(16 + 6 + 3 + -(-poly3_blocks(n, m, self_pairs) // FINAL_THREADS) + 8, pairs)


def _rows(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise AdmError(f"{name}: expected fp32 device rows [n, d] (the KID kernel has no CPU fallback)")
    return t.to(torch.float32).contiguous()


def poly3_sums(x: torch.Tensor, y: Optional[torch.Tensor] = None) -> float:
    """S_xy of fp32 device rows x [n, d], y [m, d]; with y None, S_xx (pairs i != j).  d % 4 == 0."""
    return float(ops.poly3_sums(_rows(x, "x"), None if y is None else _rows(y, "y")).item())


def mmd2_from_sums(s_xx: float, n: int, s_yy: float, m: int, s_xy: float) -> float:
    """MMD^2_u from the three sums.  The two self terms are added first, so swapping the sets changes nothing but S_xy's own
    summation order."""
    if n < 2 or m < 2:
        raise ValueError(f"the unbiased MMD^2 needs at least 2 rows in each set (n={n}, m={m})")
    return (s_xx / (n * (n - 1.0)) + s_yy / (m * (m - 1.0))) - 2.0 * s_xy / (float(n) * m)


def mmd2_unbiased(x: torch.Tensor, y: torch.Tensor, s_yy: Optional[float] = None) -> float:
    """MMD^2_u of the full sets; `s_yy` takes a cached self sum of y (KIDReference) and saves its kernel call."""
    n, m = int(x.shape[0]), int(y.shape[0])
    if n < 2 or m < 2:
        raise ValueError(f"the unbiased MMD^2 needs at least 2 rows in each set (n={n}, m={m})")
    if s_yy is None:
        s_yy = poly3_sums(y)
    return mmd2_from_sums(poly3_sums(x), n, s_yy, m, poly3_sums(x, y))


def draw_subsets(n: int, m: int, subsets: int, subset_size: int, seed: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The row indices of every draw: RandomState(seed).choice without replacement, sample set then reference set, draw by draw."""
    for name, rows in (("sample", n), ("reference", m)):
        if rows < subset_size:
            raise ValueError(f"KID: the {name} set has {rows} rows, fewer than {SUBSET_FLAG} {subset_size}; lower {SUBSET_FLAG} "
                             "(subsets are drawn without replacement and are not clipped)")
    if subset_size < 2 or subsets < 1:
        raise ValueError(f"KID: need {SUBSET_FLAG} >= 2 and at least one subset (got {subset_size}, {subsets})")
    rs = np.random.RandomState(seed)
    return [(rs.choice(n, subset_size, replace=False), rs.choice(m, subset_size, replace=False)) for _ in range(subsets)]


def kid_subsets(x: torch.Tensor, y: torch.Tensor, subsets: int = 100, subset_size: int = 1000, seed: int = 0) -> Tuple[float, float]:
    """(mean, std) of MMD^2_u over the draws of draw_subsets; the rows of a draw are gathered on the device (index_select) and
    scored by three kernel calls."""
    vals = []
    for ix, iy in draw_subsets(int(x.shape[0]), int(y.shape[0]), subsets, subset_size, seed):
        xs = x.index_select(0, torch.as_tensor(ix, dtype=torch.int64, device=x.device))
        ys = y.index_select(0, torch.as_tensor(iy, dtype=torch.int64, device=y.device))
        vals.append(mmd2_unbiased(xs, ys))
    vals = np.asarray(vals, dtype=np.float64)
    return float(np.mean(vals)), float(np.std(vals))


def load_ref_feats(path: str) -> np.ndarray:
    """The `feats` array (fp32 [m, d]) of the .npz that scripts/evaluator.py --save_ref_feats writes."""
    with np.load(path, allow_pickle=False) as z:
        if "feats" not in z.files:
            raise KeyError(f"{path}: no array 'feats' (members: {sorted(z.files)}); write it with scripts/evaluator.py --save_ref_feats")
        feats = np.asarray(z["feats"], dtype=np.float32)
    if feats.ndim != 2 or feats.shape[0] < 2:
        raise ValueError(f"{path}: feats must be [m >= 2, d], got {feats.shape}")
    return feats


class KIDReference:
    """The reference rows on the device with their self sum S_yy, computed once: a candidate then costs two kernel sums."""

    def __init__(self, feats, device=None):
        if isinstance(feats, torch.Tensor) and device is None:
            device = feats.device
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.y = torch.as_tensor(feats).to(device=device, dtype=torch.float32).contiguous()
        if self.y.dim() != 2 or self.y.shape[0] < 2:
            raise ValueError(f"KIDReference: reference rows must be [m >= 2, d], got {tuple(self.y.shape)}")
        self.s_yy = poly3_sums(self.y)

    def mmd2(self, rows: torch.Tensor) -> float:
        return mmd2_unbiased(rows, self.y, s_yy=self.s_yy)

    def fitness(self, rows: torch.Tensor) -> float:
        """1000 * MMD^2_u of `rows` against the reference."""
        return FITNESS_SCALE * self.mmd2(rows)


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
