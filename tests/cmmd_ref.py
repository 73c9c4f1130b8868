"""float64 numpy restatement of CMMD as autodiffusion_amd/cmmd.py defines it (csrc/adm_cmmd.hip), the error bound the kernel's sums
are held to, and the defects the bound must catch.

Definitions (project-defined, after Jayasumana et al. 2024; the reference has no CMMD).  Rows x [n, d], y [m, d] fp32, NOT normalised:
    r_i = |x_i|^2   s_j = |y_j|^2   G_ij = x_i . y_j   c_ij = G_ij / sqrt(r_i s_j)   D_ij = max(2 - 2 c_ij, 0)
    gamma = 1 / (2 sigma^2)          kappa_ij = expm1(-gamma D_ij) = k_ij - 1 <= 0
    S_xy   = sum_i sum_j kappa_ij                       S_xx = sum_{i != j} kappa_ij          (the diagonal is skipped by index)
    MMD2_v = S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)                    CMMD    = 1000 MMD2_v
    MMD2_u = S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m)    fitness = 1000 MMD2_u

The error bound.  With u = 2^-53 (float64 round to nearest) the kernel's sum S_hip obeys, to first order in u,

    |S_hip - S| <= pairs 2 gamma (d + c1) u + (L + E) u sum |kappa|,          c1 = norm_chain(d) + 6.5

    * the operands are fp32 widened to f64: every product x_ik y_jk, x_ik^2 is exact (24 + 24 bits fit in 53);
    * G is a length-d f64 accumulation in whatever order the matrix cores take: |G^ - G| <= d u sum_k |x_ik y_jk| <= d u sqrt(r s)
      (Cauchy-Schwarz), i.e. d u on the cosine;
    * r and s are sums of non-negative terms along a chain of at most R = cmmd.norm_chain(d) additions (4 ceil(d / 256) in the lane,
      6 shuffles): relative error <= R u each.  Their product rounds once (u), the square root halves the relative error of its
      argument, (2 R + 1) u / 2, and rounds once more (u); the division rounds once (u).  With |c| <= 1 the cosine is off by at most
      (d + R + 2.5) u;
    * 2 c is exact, 2 - 2 c rounds once: D u <= 4 u; the clamp only moves a negative value towards the true D >= 0.  So
      |D^ - D| <= 2 (d + R + 2.5) u + 4 u.  z = -gamma D^ rounds once more: gamma D u <= 4 gamma u.  gamma itself is the same
      double on both sides.  Together |z^ - z| <= 2 gamma (d + R + 2.5 + 2 + 2) u = 2 gamma (d + c1) u;
    * |d expm1 / dz| = e^z <= 1 on z <= 0, so an entry carries that error through, plus the device expm1's own E ulps of |kappa|;
    * the entries are then added along the kernel's reduction tree: an entry passes through at most L additions
      (cmmd.reduction_chain), each off by u times a partial sum of magnitude <= sum |kappa| (all kappa <= 0).
c1 is pinned by this count, not fitted.  E is measured, not assumed: tests/test_hip_cmmd.py::test_device_expm1_ulp_error drives
adm_rbf_sums with 1 x 1 row pairs of chosen cosine, whose argument z the host reproduces bit for bit, and compares with expm1 in
np.longdouble (64-bit mantissa).  MEASURED_E_ULP is the worst it found on the MI355X over sigma in {1, 10}; E is that rounded up to
the next integer, plus 1.
This restatement's own float64 error (numpy's blocked dot, fsum) is of the same form with shorter chains and lies inside it.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -53
TILE = 64
SIGMA = 10.0
MEASURED_E_ULP = 0.9913       # MI355X, rounded up: 0.99121 ulp at sigma = 1 (z = -0.4134); sigma = 10: 0.5029 ulp
E_ULP = math.ceil(MEASURED_E_ULP) + 1
DEFECTS = ("padded_rows", "diagonal_tile_twice", "offdiag_once", "fp32_running_sum", "fp32_gram")
SELF_ONLY = ("diagonal_tile_twice", "offdiag_once")


def gamma_of(sigma):
    return 1.0 / (2.0 * float(sigma) * float(sigma))


def norm_chain(d):
    return min(4 * -(-d // 256) + 6, d)


def kappa_matrix(x, y, sigma=SIGMA, fp32_gram=False):
    """float64 [n, m]: expm1(-gamma max(2 - 2 cos(x_i, y_j), 0))."""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    r, s = (x64 * x64).sum(1), (y64 * y64).sum(1)
    if fp32_gram:                                  # the Gram accumulated in fp32
        g = (np.asarray(x, dtype=np.float32) @ np.asarray(y, dtype=np.float32).T).astype(np.float64)
    else:
        g = x64 @ y64.T
    c = g / np.sqrt(r[:, None] * s[None, :])
    return np.expm1(-gamma_of(sigma) * np.maximum(2.0 - 2.0 * c, 0.0))


def rbf_sum(x, y=None, sigma=SIGMA, defect=None):
    """(S, sum |kappa|, pairs) over the pairs the definition counts: all of them (y given), or i != j of x alone (y None).
    defect: one of DEFECTS -- the same sum as a kernel with that mistake would form it."""
    assert defect is None or defect in DEFECTS, defect
    self_pairs = y is None
    assert self_pairs or defect not in SELF_ONLY, defect
    x = np.asarray(x, dtype=np.float32)
    y = x if self_pairs else np.asarray(y, dtype=np.float32)
    n, m = x.shape[0], y.shape[0]
    k = kappa_matrix(x, y, sigma, fp32_gram=defect == "fp32_gram")
    live = np.ones((n, m), dtype=bool)
    if self_pairs:
        np.fill_diagonal(live, False)
    weight = np.ones((n, m))
    bi, bj = np.arange(n)[:, None] // TILE, np.arange(m)[None, :] // TILE
    if defect == "offdiag_once":                   # self mode computes the tiles on and above the diagonal: the others never doubled
        live &= bi <= bj
    if defect == "diagonal_tile_twice":            # ... or every partial doubled, the diagonal tiles' too
        weight = np.where(bi == bj, 2.0, 1.0)
    vals = (k * weight)[live]
    if defect == "fp32_running_sum":
        s = float(np.cumsum(vals.astype(np.float32), dtype=np.float32)[-1])
    else:
        s = math.fsum(vals)
    if defect == "padded_rows":                    # the zero rows that fill the last 64-tiles, counted at cosine 0 (norm guarded to 1)
        pad = (-(-n // TILE) * TILE) * (-(-m // TILE) * TILE) - n * m
        s += pad * math.expm1(-2.0 * gamma_of(sigma))
    full = np.ones((n, m), dtype=bool)
    if self_pairs:
        np.fill_diagonal(full, False)
    return s, math.fsum(np.abs(k[full])), n * (n - 1) if self_pairs else n * m


def rbf_sum_loops(x, y=None, sigma=SIGMA):
    """The definition as an explicit double loop (python floats: float64), for tiny shapes."""
    self_pairs = y is None
    x = [[float(v) for v in row] for row in np.asarray(x, dtype=np.float32)]
    y = x if self_pairs else [[float(v) for v in row] for row in np.asarray(y, dtype=np.float32)]
    g = gamma_of(sigma)
    s = 0.0
    for i, a in enumerate(x):
        for j, b in enumerate(y):
            if self_pairs and i == j:
                continue
            r, q = sum(p * p for p in a), sum(p * p for p in b)
            c = sum(p * t for p, t in zip(a, b)) / math.sqrt(r * q)
            s += math.expm1(-g * max(2.0 - 2.0 * c, 0.0))
    return s


def bound(pairs: int, sum_abs: float, d: int, chain: int, sigma=SIGMA, e_ulp=None) -> float:
    e = E_ULP if e_ulp is None else e_ulp
    c1 = norm_chain(d) + 6.5
    return pairs * 2.0 * gamma_of(sigma) * (d + c1) * U + (chain + e) * U * sum_abs


def mmd2_from_sums(s_xx, n, s_yy, m, s_xy, unbiased):
    if unbiased:
        assert n >= 2 and m >= 2
        return (s_xx / (n * (n - 1.0)) + s_yy / (m * (m - 1.0))) - 2.0 * s_xy / (float(n) * m)
    return (s_xx / (float(n) * n) + s_yy / (float(m) * m)) - 2.0 * s_xy / (float(n) * m)


def mmd2(x, y, sigma=SIGMA, unbiased=False):
    n, m = len(x), len(y)
    sxx = rbf_sum(x, None, sigma)[0] if n >= 2 else 0.0
    syy = rbf_sum(y, None, sigma)[0] if m >= 2 else 0.0
    return mmd2_from_sums(sxx, n, syy, m, rbf_sum(x, y, sigma)[0], unbiased)


def mmd2_loops(x, y, sigma=SIGMA, unbiased=False):
    return mmd2_from_sums(rbf_sum_loops(x, None, sigma), len(x), rbf_sum_loops(y, None, sigma), len(y), rbf_sum_loops(x, y, sigma), unbiased)


def cmmd(x, y, sigma=SIGMA):
    return 1000.0 * mmd2(x, y, sigma)


def fitness(x, y, sigma=SIGMA):
    return 1000.0 * mmd2(x, y, sigma, unbiased=True)


def mmd2_naive_fp32(x, y, sigma=SIGMA):
    """What the kernel is built to avoid: rows normalised in fp32, an fp32 Gram, exp in fp32, each mean from ONE fp32 running sum
    (a single accumulator, as an atomicAdd or a serial loop has), the three means subtracted.  From 2^20 pairs on, the accumulator's
    spacing (2^-4 at 2^20) is larger than 1 - k ~ 0.006: every k is added as if it were 1 or 0.9375."""
    g = np.float32(gamma_of(sigma))

    def mean_k(a, b):
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
        dist = np.maximum(np.float32(2.0) - np.float32(2.0) * (a @ b.T), np.float32(0.0))
        k = np.exp(-g * dist)
        return np.cumsum(k.ravel(), dtype=np.float32)[-1] / np.float32(k.size)
    return float((mean_k(x, x) + mean_k(y, y)) - np.float32(2.0) * mean_k(x, y))


def features(n, d, seed, shift=0.0):
    """Seeded CPU rows shaped like CLIP embeddings: 10 (w mu + sqrt(1 - w^2) noise), mu a fixed unit direction (shared by every seed),
    noise a unit vector, w in [0.6, 0.95]: norms near 10, cosines between rows about 0.35 .. 0.9.  shift moves the set's mean along a
    second fixed direction (a different distribution)."""
    import torch
    g0 = torch.Generator().manual_seed(12345)
    mu, nu = torch.randn(d, generator=g0, dtype=torch.float64), torch.randn(d, generator=g0, dtype=torch.float64)
    mu, nu = mu / mu.norm(), nu / nu.norm()
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=g, dtype=torch.float64)
    z = z / z.norm(dim=1, keepdim=True)
    w = 0.6 + 0.35 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    scale = 10.0 * (1.0 + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64))
    return (scale * (w * mu + (1 - w * w).sqrt() * z + shift * nu)).to(torch.float32).contiguous()


def with_near_duplicates(x, seed=0):
    """Row 1 = row 0 + 1e-4 noise (where there are 2 rows): 2 - 2 c cancels to ~1e-10 and rounding may push it below 0 (the clamp)."""
    import torch
    x = x.clone()
    if x.shape[0] >= 2:
        x[1] = x[0] + 1e-4 * torch.randn(x.shape[1], generator=torch.Generator().manual_seed(seed))
    return x


def with_shared_row(x, y, i=2, j=0):
    """x with row i = y_j bit for bit (where x has such a row): cosine 1, kappa = 0."""
    x = x.clone()
    if x.shape[0] > i:
        x[i] = y[j]
    return x


def cross_inputs(n, m, d):
    y = with_near_duplicates(features(m, d, 300 + m + d), 1)
    x = with_shared_row(with_near_duplicates(features(n, d, 200 + n + d, shift=0.1), 2), y)
    return x, y


def self_inputs(n, d):
    x = with_near_duplicates(features(n, d, 100 + n + d), 3)
    if n > 3:
        x[3] = x[2]                                # an exact duplicate inside the set
    return x
