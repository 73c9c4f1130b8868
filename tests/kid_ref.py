"""float64 numpy restatement of the Kernel Inception Distance of autodiffusion_amd/kid.py (csrc/adm_kid.hip), the error bound the
kernel's sums are held to, and the defects the bound must catch.

Definitions (project-defined; the reference has no KID):
    k(a, b) = (a . b / d + 1)^3
    S_xy    = sum_i sum_j k(x_i, y_j)                 S_xx = sum_{i != j} k(x_i, x_j)       (the diagonal is left out)
    MMD2_u  = S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m)
    KID     = mean, np.std (ddof 0) of MMD2_u over `subsets` draws of `subset_size` rows of each set without replacement, the rows
              chosen by np.random.RandomState(seed).choice, sample set then reference set, draw by draw.

The error bound.  With u = 2^-53 (float64 round to nearest) the kernel's sum S_hip obeys

    |S_hip - S| <= (3 d + 4 + L) u sum |k|                                                     (first order in u)

    * the operands are fp32 widened to f64: every product x_ik y_jk is exact (24 + 24 bits fit in 53);
    * an entry's dot product g is a length-d f64 accumulation, in whatever order the matrix cores take:
      |g^ - g| <= d u sum_k |x_ik y_jk|;
    * t = g / d + 1 is two more roundings, (t t) t two more: t^3 (1 + e), |e| <= 4 u, on top of the dot product's error
      pushed through the cube, d(t^3) = 3 t^2 dt with |dt| <= d u sum_k |x_ik y_jk| / d.  For non-negative rows (pool3 features
      are post-ReLU averages) sum_k |x y| / d = g / d <= t, so 3 t^2 |dt| <= 3 d u t^3.  For mixed-sign rows an entry obeys the
      same while sum_k |x_ik y_jk| / d <= |g / d + 1| (0.6 randn rows: 0.23 against ~1); an entry with k < 0 cannot (g / d < -1
      means sum_k |x y| / d >= |g| / d = |t| + 1), so for such sets the 3 d term is held against the entry-wise form it stands for,
      bound_entrywise() = u sum (3 t^2 sum_k |x y| + (4 + L) |t|^3), which the host tests show to lie below it on the sets used;
    * the entries are then added along the kernel's reduction tree: an entry passes through at most L additions, each off by
      u times a partial sum of magnitude <= sum |k|.  L is the tree's depth (kid.reduction_chain: 16 in the lane, 6 across the
      wave, 3 across the block, ceil(blocks / 256) + 8 in the second pass), never more than the number of pairs (a masked entry
      enters as an exact 0.0, and adding zero does not round); the doubling of a tile above the diagonal is exact.
This restatement's own float64 error (numpy's blocked dot and pairwise sums) is of the same form and far inside it.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
TILE = 64
DEFECTS = ("padded_rows", "diagonal_kept", "offdiag_once", "fp32_running_sum", "fp16_inputs")


def kernel_matrix(x, y):
    """float64 [n, m]: (x_i . y_j / d + 1)^3."""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = x64 @ y64.T / x64.shape[1] + 1.0
    return (t * t) * t


def poly3_sum(x, y=None, defect=None):
    """(S, sum |k|) over the pairs the definition counts: all of them (y given), or i != j of x alone (y None).
    defect: one of DEFECTS -- the same sum as a kernel with that mistake would form it."""
    assert defect is None or defect in DEFECTS, defect
    self_pairs = y is None
    x = np.asarray(x, dtype=np.float32)
    y = x if self_pairs else np.asarray(y, dtype=np.float32)
    n, m = x.shape[0], y.shape[0]
    if defect == "fp16_inputs":                    # a half-precision Gram: the operands rounded to fp16 first
        k = kernel_matrix(x.astype(np.float16), y.astype(np.float16))
    else:
        k = kernel_matrix(x, y)
    live = np.ones((n, m), dtype=bool)
    if self_pairs and defect != "diagonal_kept":
        np.fill_diagonal(live, False)
    if defect == "offdiag_once":                   # self mode computes the tiles on and above the diagonal: the others never doubled
        assert self_pairs
        bi, bj = np.arange(n)[:, None] // TILE, np.arange(m)[None, :] // TILE
        live &= (bi == bj) | (bi < bj)
    vals = k[live]
    if defect == "fp32_running_sum":
        s = float(np.cumsum(vals.astype(np.float32), dtype=np.float32)[-1])
    else:
        s = float(vals.sum())
    if defect == "padded_rows":                    # the zero rows that fill the last 64-tiles: (0 + 1)^3 = 1 each
        s += float((-(-n // TILE) * TILE) * (-(-m // TILE) * TILE) - n * m)
    return s, float(np.abs(k[live]).sum())


def poly3_sum_loops(x, y=None):
    """The definition as an explicit double loop (python floats: float64), for tiny shapes."""
    self_pairs = y is None
    x = [[float(v) for v in row] for row in np.asarray(x, dtype=np.float32)]
    y = x if self_pairs else [[float(v) for v in row] for row in np.asarray(y, dtype=np.float32)]
    d = len(x[0])
    s = 0.0
    for i, a in enumerate(x):
        for j, b in enumerate(y):
            if self_pairs and i == j:
                continue
            t = sum(p * q for p, q in zip(a, b)) / d + 1.0
            s += t * t * t
    return s


def bound(sum_abs: float, d: int, chain: int) -> float:
    return (3 * d + 4 + chain) * U * sum_abs


def bound_entrywise(x, y, chain: int, self_pairs=False) -> float:
    """The derivation's first-order bound without the step sum_k |x y| / d <= |t|: u sum (3 t^2 sum_k |x_ik y_jk| + (4 + L) |t|^3)."""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = x64 @ y64.T / x64.shape[1] + 1.0
    e = 3.0 * t * t * (np.abs(x64) @ np.abs(y64).T) + (4 + chain) * np.abs(t) ** 3
    if self_pairs:
        np.fill_diagonal(e, 0.0)
    return U * float(e.sum())


def mmd2_unbiased(x, y):
    n, m = len(x), len(y)
    assert n >= 2 and m >= 2
    return poly3_sum(x)[0] / (n * (n - 1.0)) + poly3_sum(y)[0] / (m * (m - 1.0)) - 2.0 * poly3_sum(x, y)[0] / (float(n) * m)


def mmd2_loops(x, y):
    n, m = len(x), len(y)
    return poly3_sum_loops(x) / (n * (n - 1.0)) + poly3_sum_loops(y) / (m * (m - 1.0)) - 2.0 * poly3_sum_loops(x, y) / (float(n) * m)


def subset_draws(n, m, subsets, subset_size, seed):
    """The index draws of the reported KID, spelled out: one RandomState, sample set then reference set, draw by draw."""
    rs = np.random.RandomState(seed)
    draws = []
    for _ in range(subsets):
        ix = rs.choice(n, subset_size, replace=False)
        iy = rs.choice(m, subset_size, replace=False)
        draws.append((ix, iy))
    return draws


def kid_subsets(x, y, subsets=100, subset_size=1000, seed=0):
    x, y = np.asarray(x), np.asarray(y)
    vals = np.array([mmd2_unbiased(x[ix], y[iy]) for ix, iy in subset_draws(len(x), len(y), subsets, subset_size, seed)])
    return float(np.mean(vals)), float(np.std(vals)), vals


def features(n, d, seed, mixed_sign=False):
    """Seeded CPU rows: relu(randn) * 0.6 (Inception-like: non-negative), or 0.6 randn (mixed sign)."""
    import torch
    z = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return ((z if mixed_sign else torch.relu(z)) * 0.6).contiguous()


def oppose(x, y, i=0, j=0):
    """x with row i = -5 y_j: x_i . y_j / d = -5 |y_j|^2 / d ~ -1.8 for 0.6 randn rows, so k(x_i, y_j) < 0 and sum |k| != sum k."""
    x = x.clone()
    x[i] = -5.0 * y[j]
    return x
