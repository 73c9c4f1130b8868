"""CMMD on the device: the MMD^2 with a Gaussian RBF kernel on L2-normalised CLIP image embeddings.

Project-defined (the reference has no CMMD), after Jayasumana et al., "Rethinking FID: Towards a Better Evaluation Metric for Image
Generation" (CVPR 2024):

* rows        x [n, d], y [m, d] fp32: the `encode_image` outputs (projected embeddings), NOT normalised -- the kernel normalises in f64;
* norms, Gram r_i = |x_i|^2, s_j = |y_j|^2 (sums of exact products in f64), G_ij = x_i . y_j in f64;
* cosine      c_ij = G_ij / sqrt(r_i s_j);        squared distance  D_ij = max(2 - 2 c_ij, 0);
* kernel      gamma = 1 / (2 sigma^2), sigma = 10 by default;   kappa_ij = expm1(-gamma D_ij) = k_ij - 1 <= 0;
* sums        S_xy = sum_i sum_j kappa_ij;   S_xx = sum_{i != j} kappa_ij  (the diagonal is skipped by index; it would add an exact 0);
* estimators  MMD^2_v = S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)   (the full-matrix means of the paper's public implementation: the
              +1 of every k cancels exactly, 1 + 1 - 2),
              MMD^2_u = S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m),  n, m >= 2  (likewise: the +1s cancel);
* reported    CMMD = 1000 MMD^2_v;        search fitness  1000 MMD^2_u -- the V-statistic's bias, about (1 - mean k) / n per set,
              depends on n, which a fitness compared across candidates must not.

On unit vectors with sigma = 10 every k lies in [exp(-0.02), 1], the three means are each about 0.99 and the result is 1e-4 .. 1e-3:
an fp32 Gram or a naive mean(k) loses it.  ``adm_rbf_sums`` (csrc/adm_cmmd.hip) sums k - 1 through expm1 on an f64 matrix-core
Gram, so the ones cancel algebraically, not numerically, and the n x m matrix never exists in memory.

The embeddings come from the ViT-L/14 224-pixel tower that Stable Diffusion's CLIP checkpoint holds (sd_clip.CLIPVisionTransformer):
values are comparable between runs of this project, not with the paper's tables, which use the 336-pixel tower.

A row of norm 0 has no direction: it is refused (ValueError) from the kernel's own norms before the sum is used.  Host tensors
raise ``AdmError``: there is no CPU fallback, as in kid.py.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import mmd, ops
from .mmd import mmd2_from_sums, pooled_rows, reduction_chain  # noqa: F401
from .mmd import pair_blocks as rbf_blocks  # blocks of adm_rbf_sums's tile pass

SIGMA = 10.0         # the paper's bandwidth
SCALE = 1000.0       # the paper's scaling of the reported value; the fitness uses the same
SAVE_FLAG = "scripts/sd_clip_score.py --save_clip_feats"


def gamma_of(sigma: float) -> float:
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"CMMD: the bandwidth sigma must be finite and positive, got {sigma}")
    return 1.0 / (2.0 * sigma * sigma)


def work_elems(n: int, m: int, self_pairs: bool) -> int:
    """Workspace doubles of adm_rbf_sums: one partial per block, then the n + m squared norms."""
    return rbf_blocks(n, m, self_pairs) + n + m


def norm_chain(d: int) -> int:
    """The longest chain of rounding float64 additions behind a squared norm of adm_rbf_sums (norm_kernel): a lane adds the 4 squares
    of each of its ceil(d / 256) float4s, then 6 xor shuffles; never more than the d terms there are."""
    return min(4 * -(-d // 256) + 6, d)


def rbf_sums(x: torch.Tensor, y: Optional[torch.Tensor] = None, sigma: float = SIGMA) -> float:
    """S_xy of fp32 device rows x [n, d], y [m, d] (not normalised); with y None, S_xx (pairs i != j).  d % 4 == 0.  A row whose
    squared norm is 0 (or not finite) raises ValueError."""
    g = gamma_of(sigma)
    out, norms = ops.rbf_sums(mmd.device_rows(x, "x", "CMMD"), None if y is None else mmd.device_rows(y, "y", "CMMD"), g,
                              return_norms=True)
    s, lo, hi = torch.stack([out[0], norms.min(), norms.max()]).tolist()
    if not (lo > 0.0 and math.isfinite(hi)):
        raise ValueError(f"CMMD: an embedding row has squared norm {lo if not lo > 0.0 else hi}: a row without a direction cannot be "
                         "normalised")
    return float(s)


def _self_sum(x: torch.Tensor, sigma: float) -> float:
    return rbf_sums(x, None, sigma) if x.shape[0] >= 2 else 0.0      # one row has no pair i != j


def mmd2(x: torch.Tensor, y: torch.Tensor, sigma: float = SIGMA, unbiased: bool = False, s_yy: Optional[float] = None) -> float:
    """MMD^2 of the two sets; `s_yy` takes a cached self sum of y (CMMDReference) and saves its kernel call."""
    n, m = int(x.shape[0]), int(y.shape[0])
    if unbiased and (n < 2 or m < 2):
        raise ValueError(f"the unbiased MMD^2 needs at least 2 rows in each set (n={n}, m={m})")
    if s_yy is None:
        s_yy = _self_sum(y, sigma)
    return mmd2_from_sums(_self_sum(x, sigma), n, s_yy, m, rbf_sums(x, y, sigma), unbiased)


def cmmd(x: torch.Tensor, y: torch.Tensor, sigma: float = SIGMA) -> float:
    """CMMD = 1000 MMD^2_v of embedding rows x against y."""
    return SCALE * mmd2(x, y, sigma)


def load_ref_clip_feats(path: str) -> np.ndarray:
    """The `clip_feats` array (fp32 [m >= 2, d]) of the .npz that scripts/sd_clip_score.py --save_clip_feats writes."""
    return mmd.load_ref_rows(path, "clip_feats", SAVE_FLAG)


class CMMDReference(mmd.PairSumReference):
    """The reference embeddings on the device with their self sum S_yy, computed once: a candidate then costs two kernel sums."""

    def __init__(self, feats, device=None, sigma: float = SIGMA):
        self.sigma = float(sigma)
        gamma_of(self.sigma)
        super().__init__(feats, device)

    def self_sum(self) -> float:
        return rbf_sums(self.y, None, self.sigma)

    def mmd2(self, rows: torch.Tensor, unbiased: bool = False) -> float:
        return mmd2(rows, self.y, self.sigma, unbiased, s_yy=self.s_yy)

    def cmmd(self, rows: torch.Tensor) -> float:
        """1000 * MMD^2_v of `rows` against the reference: the reported value."""
        return SCALE * self.mmd2(rows)

    def fitness(self, rows: torch.Tensor) -> float:
        """1000 * MMD^2_u of `rows` against the reference: the search fitness."""
        return SCALE * self.mmd2(rows, unbiased=True)
