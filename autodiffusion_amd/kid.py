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

from . import mmd, ops
from .mmd import pooled_rows, reduction_chain  # noqa: F401
from .mmd import pair_blocks as poly3_blocks  # noqa: F401  (blocks = workspace elements of adm_poly3_sums)

FITNESS_SCALE = 1000.0   # KIDReference.fitness = 1000 * MMD^2_u: only makes log lines readable
SUBSET_FLAG = "--kid_subset_size"


def poly3_sums(x: torch.Tensor, y: Optional[torch.Tensor] = None) -> float:
    """S_xy of fp32 device rows x [n, d], y [m, d]; with y None, S_xx (pairs i != j).  d % 4 == 0."""
    return float(ops.poly3_sums(mmd.device_rows(x, "x", "KID"), None if y is None else mmd.device_rows(y, "y", "KID")).item())


def mmd2_from_sums(s_xx: float, n: int, s_yy: float, m: int, s_xy: float) -> float:
    """MMD^2_u from the three sums."""
    return mmd.mmd2_from_sums(s_xx, n, s_yy, m, s_xy, unbiased=True)


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
    return mmd.load_ref_rows(path, "feats", "scripts/evaluator.py --save_ref_feats")


class KIDReference(mmd.PairSumReference):
    """The reference rows on the device with their self sum S_yy, computed once: a candidate then costs two kernel sums."""

    def self_sum(self) -> float:
        return poly3_sums(self.y)

    def mmd2(self, rows: torch.Tensor) -> float:
        return mmd2_unbiased(rows, self.y, s_yy=self.s_yy)

    def fitness(self, rows: torch.Tensor) -> float:
        """1000 * MMD^2_u of `rows` against the reference."""
        return FITNESS_SCALE * self.mmd2(rows)
