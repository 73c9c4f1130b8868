"""The ADM evaluation suite on the MI355X: Inception Score, FID, sFID, precision and recall of a sample batch against a
reference batch -- what the reference's ``evaluations/evaluator.py`` (``main()`` :29-84) reports after sampling.

* Features: ``inception.InceptionV3.features_all`` (pool3 and the ``mixed_6/conv[..., :7]`` spatial tap of one pass),
  standing for the frozen TensorFlow graph (:665-671).  Its parity with that graph is unpinned.
* Statistics: ``fid.ActivationAccumulator`` (float64 Gram sums on the device) and ``fid.FIDStatistics`` (Frechet distance).
* Inception Score: logits = pool3 @ fc.weight^T through ``ops.linear_f32`` (the graph's bias-free ``softmax/logits/MatMul``,
  :674-685), softmax and the per-split KL on the device in float64 (:217-229).
* Precision / recall: ``ManifoldEstimator`` (:276-430) on the fused k-NN kernels of csrc/adm_knn.hip (``adm_knn_smallest``,
  ``adm_knn_cover``): one fp16 GEMM per call with the k-smallest selection / radius comparison in its epilogue, no N x N
  distance matrix in memory.  The distances are fp32 sums of fp16 products of the fp16-rounded features (the reference
  rounds each distance to fp16 as well: DESIGN.md section 10).
* KID (``Evaluator.compute_kid``; project-defined, the reference reports none): ``kid.kid_subsets`` on the cubic-kernel sums of
  csrc/adm_kid.hip.
"""
from __future__ import annotations

import math
import zipfile
from typing import Iterable, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import AdmError, check
from .fid import ActivationAccumulator, FIDStatistics

FP16_MAX = 65504.0
KNN_MAX = 8          # longest k-NN list / most neighbourhood sizes of the kernels
KNN_DSTEP = 64       # the kernels' d step: features are zero-padded to a multiple of it (zeros change no dot product or norm)


# ------------------------------------------------------------------ .npz batches
def iter_npz_batches(path: str, key: str = "arr_0", batch_size: int = 64) -> Iterator[np.ndarray]:
    """Rows of array `key` of an .npz file, `batch_size` at a time, without holding the whole array in host memory (a 50k x
    256 x 256 x 3 uint8 sample file is 9.8 GB): the member's .npy header is parsed and its data streamed from the zip entry
    (stored or deflated).  Fortran-ordered or object arrays are loaded whole and sliced."""
    with zipfile.ZipFile(path) as zf:
        name = key + ".npy"
        if name not in zf.namelist():
            raise KeyError(f"{path}: no array {key!r} (members: {sorted(n[:-4] for n in zf.namelist())})")
        with zf.open(name) as f:
            major, _ = np.lib.format.read_magic(f)
            if major == 1:
                shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
            else:
                shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
            if not (fortran or dtype.hasobject or len(shape) == 0):
                row = int(np.prod(shape[1:], dtype=np.int64)) * dtype.itemsize
                for start in range(0, shape[0], batch_size):
                    n = min(batch_size, shape[0] - start)
                    buf = bytearray(n * row)
                    view, got = memoryview(buf), 0
                    while got < len(buf):
                        r = f.readinto(view[got:])
                        if not r:
                            raise ValueError(f"{path}: {key} ends after {start * row + got} of {shape[0] * row} data bytes")
                        got += r
                    yield np.frombuffer(buf, dtype=dtype).reshape((n,) + tuple(shape[1:]))
                return
    arr = np.load(path, allow_pickle=False)[key]
    for start in range(0, arr.shape[0], batch_size):
        yield arr[start:start + batch_size]


# ------------------------------------------------------------------ k-NN precision / recall
def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _rows(features) -> torch.Tensor:
    t = torch.as_tensor(features)
    if t.dim() != 2:
        raise ValueError(f"features must be [N, D], got {tuple(t.shape)}")
    return t.to(device=_device(), dtype=torch.float32)


class _Prepared:
    """fp16 rows zero-padded to a multiple of KNN_DSTEP, their fp32 squared norms, and whether fp16 distances could overflow."""

    def __init__(self, x32: torch.Tensor):
        self.x32 = x32
        n, d = x32.shape
        dp = (d + KNN_DSTEP - 1) // KNN_DSTEP * KNN_DSTEP
        x16 = torch.zeros((n, dp), dtype=torch.float16, device=x32.device)
        x16[:, :d] = x32
        self.x16 = x16
        self.norm = torch.empty(n, dtype=torch.float32, device=x32.device)
        finite = torch.ones((), dtype=torch.bool, device=x32.device)
        for i in range(0, n, 8192):      # row chunks: no fp32 copy of the whole set
            blk = x16[i:i + 8192].float()
            self.norm[i:i + 8192] = blk.pow(2).sum(1)
            finite &= torch.isfinite(blk).all()
        self.finite = bool(finite)
        self.max_norm = float(self.norm.max()) if n else 0.0


def _fits_fp16(*sets: _Prepared) -> bool:
    """The fp16 GEMM is used when no distance can reach the fp16 range: dist <= (|u| + |v|)^2 <= 4 max|x|^2 < 65504 over
    both sets, and every feature is finite in fp16.  The reference decides per 10k x 10k block on the actual distances
    (a non-finite fp16 block is recomputed in fp32, evaluator.py:451-455); this bound is set-wide and conservative."""
    return all(s.finite for s in sets) and 4.0 * max(s.max_norm for s in sets) < FP16_MAX


def _dist32(u: torch.Tensor, un: torch.Tensor, v: torch.Tensor, vn: torch.Tensor) -> torch.Tensor:
    """fp32 fallback block: max(|u|^2 - 2 u v^T + |v|^2, 0) (_batch_pairwise_distances, evaluator.py:485-500)."""
    return torch.clamp_min(un[:, None] - 2.0 * (u @ v.T) + vn[None, :], 0.0)


def knn_splits(nq: int, nx: int) -> int:
    """Blocks per 128-query tile over the candidate rows: enough to put ~4 blocks on every CU at N = 5 000 .. 50 000."""
    qt, rt = (nq + 127) // 128, (nx + 127) // 128
    cus = torch.cuda.get_device_properties(_device()).multi_processor_count
    return max(1, min(rt, -(-4 * cus // qt)))


def knn_smallest(q16: torch.Tensor, qn: torch.Tensor, x16: torch.Tensor, xn: torch.Tensor, kk: int,
                 splits: Optional[int] = None) -> torch.Tensor:
    """fp32 [nq, kk]: the kk smallest distances of every row of q16 to the rows of x16, ascending (adm_knn_smallest)."""
    nq, nx, d = q16.shape[0], x16.shape[0], q16.shape[1]
    if x16.shape[1] != d:
        raise AdmError(f"knn_smallest: feature widths differ ({d} vs {x16.shape[1]})")
    splits = knn_splits(nq, nx) if splits is None else int(splits)
    out = torch.empty((nq, kk), dtype=torch.float32, device=q16.device)
    ws = torch.empty((splits, nq, kk), dtype=torch.float32, device=q16.device) if splits > 1 else None
    check(_lib.load().adm_knn_smallest(ops._ptr(q16, torch.float16, "q"), nq, ops._ptr(qn, torch.float32, "qnorm"),
                                       ops._ptr(x16, torch.float16, "x"), nx, ops._ptr(xn, torch.float32, "xnorm"), d, kk,
                                       ops._ptr(out), ops._ptr(ws), splits, ops._stream()), "adm_knn_smallest")
    return out


def knn_cover(a16, an, ra, b16, bn, rb) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a_in bool [na, K], b_in bool [nb, K]) of adm_knn_cover: a_in[i, k] = any_j dist(i, j) <= rb[j, k], b_in likewise."""
    na, nb, d, K = a16.shape[0], b16.shape[0], a16.shape[1], ra.shape[1]
    if rb.shape[1] != K or b16.shape[1] != d:
        raise AdmError(f"knn_cover: radii widths {ra.shape[1]} / {rb.shape[1]} or feature widths {d} / {b16.shape[1]} differ")
    a_in = torch.zeros((na, K), dtype=torch.uint8, device=a16.device)
    b_in = torch.zeros((nb, K), dtype=torch.uint8, device=a16.device)
    check(_lib.load().adm_knn_cover(ops._ptr(a16, torch.float16, "a"), na, ops._ptr(an, torch.float32, "anorm"),
                                    ops._ptr(ra, torch.float32, "ra"), ops._ptr(b16, torch.float16, "b"), nb,
                                    ops._ptr(bn, torch.float32, "bnorm"), ops._ptr(rb, torch.float32, "rb"), d, K,
                                    ops._ptr(a_in), ops._ptr(b_in), ops._stream()), "adm_knn_cover")
    return a_in.bool(), b_in.bool()


class ManifoldEstimator:
    """k-NN manifolds of feature sets (evaluations/evaluator.py:276-430, after kynkaat/improved-precision-and-recall-metric).

    Same constructor, ``manifold_radii`` and ``evaluate_pr`` semantics and return types as the reference (minus its TF
    session); features may be numpy arrays or device tensors.  ``row_batch_size`` / ``col_batch_size`` only size the
    blocks of the fp32 fallback (features whose fp16 distances could overflow); the fused kernels need no blocking.
    ``evaluate()`` (realism score, nearest indices) is not provided: ``main()`` never calls it."""

    def __init__(self, row_batch_size: int = 10000, col_batch_size: int = 10000, nhood_sizes: Sequence[int] = (3,),
                 clamp_to_percentile: Optional[float] = None, eps: float = 1e-5, splits: Optional[int] = None):
        self.row_batch_size = row_batch_size
        self.col_batch_size = col_batch_size
        self.nhood_sizes = list(nhood_sizes)
        self.num_nhoods = len(self.nhood_sizes)
        self.clamp_to_percentile = clamp_to_percentile
        self.eps = eps
        self.splits = splits
        self.last_path = None          # "fp16" (fused kernels) or "fp32" (fallback) of the last call
        if not 1 <= self.num_nhoods <= KNN_MAX or min(self.nhood_sizes) < 0 or max(self.nhood_sizes) + 1 > KNN_MAX:
            raise ValueError(f"nhood_sizes {tuple(nhood_sizes)}: 1..{KNN_MAX} sizes, each in [0, {KNN_MAX - 1}]")

    def warmup(self):
        z = np.zeros([KNN_MAX, 2048], dtype=np.float32)
        self.evaluate_pr(z, self.manifold_radii(z), z, self.manifold_radii(z))

    def manifold_radii(self, features) -> np.ndarray:
        """float32 [N, num_nhoods]: for every point the distance to its k-th nearest neighbour (itself included at 0) for each k
        of nhood_sizes; with clamp_to_percentile, radii above that percentile (per k) are set to 0."""
        x = _Prepared(_rows(features))
        n, kk = x.x32.shape[0], max(self.nhood_sizes) + 1
        if n < kk:
            raise ValueError(f"manifold_radii: {n} features, fewer than max(nhood_sizes) + 1 = {kk}")
        if _fits_fp16(x):
            self.last_path = "fp16"
            dist = knn_smallest(x.x16, x.norm, x.x16, x.norm, kk, self.splits)
        else:
            self.last_path = "fp32"
            xn = x.x32.pow(2).sum(1)
            parts = []
            for i in range(0, n, self.row_batch_size):
                blk = torch.cat([_dist32(x.x32[i:i + self.row_batch_size], xn[i:i + self.row_batch_size],
                                         x.x32[j:j + self.col_batch_size], xn[j:j + self.col_batch_size])
                                 for j in range(0, n, self.col_batch_size)], 1)
                parts.append(torch.topk(blk, kk, dim=1, largest=False, sorted=True).values)
            dist = torch.cat(parts, 0)
        radii = dist[:, self.nhood_sizes].cpu().numpy().astype(np.float32)
        if self.clamp_to_percentile is not None:
            max_distances = np.percentile(radii, self.clamp_to_percentile, axis=0)
            radii[radii > max_distances] = 0
        return radii

    def evaluate_pr(self, features_1, radii_1, features_2, radii_2) -> Tuple[np.ndarray, np.ndarray]:
        """(precision [K1], recall [K2]) float64: the fraction of features_2 inside some hypersphere of features_1 (radii_1),
        and of features_1 inside some hypersphere of features_2 (radii_2)."""
        a, b = _Prepared(_rows(features_1)), _Prepared(_rows(features_2))
        ra, rb = _rows(radii_1).contiguous(), _rows(radii_2).contiguous()
        if ra.shape[0] != a.x32.shape[0] or rb.shape[0] != b.x32.shape[0]:
            raise ValueError("evaluate_pr: one radius row per feature row")
        if _fits_fp16(a, b) and ra.shape[1] == rb.shape[1] and 1 <= ra.shape[1] <= KNN_MAX:
            self.last_path = "fp16"
            a_in, b_in = knn_cover(a.x16, a.norm, ra, b.x16, b.norm, rb)
        else:
            self.last_path = "fp32"
            an, bn = a.x32.pow(2).sum(1), b.x32.pow(2).sum(1)
            a_in = torch.zeros((a.x32.shape[0], rb.shape[1]), dtype=torch.bool, device=ra.device)
            b_in = torch.zeros((b.x32.shape[0], ra.shape[1]), dtype=torch.bool, device=ra.device)
            for i in range(0, a.x32.shape[0], self.row_batch_size):
                i1 = i + self.row_batch_size
                for j in range(0, b.x32.shape[0], self.col_batch_size):
                    j1 = j + self.col_batch_size
                    dist = _dist32(a.x32[i:i1], an[i:i1], b.x32[j:j1], bn[j:j1])[..., None]
                    a_in[i:i1] |= (dist <= rb[j:j1][None]).any(1)
                    b_in[j:j1] |= (dist <= ra[i:i1][:, None]).any(0)
        return (b_in.double().mean(0).cpu().numpy(), a_in.double().mean(0).cpu().numpy())


# ------------------------------------------------------------------ the evaluator
class Evaluator:
    """``Evaluator`` of evaluations/evaluator.py (:110-262) over the HIP Inception-v3: ``inception`` is an
    ``inception.InceptionV3`` on the GPU (its ``fc_weight`` serves the Inception Score)."""

    def __init__(self, inception, batch_size: int = 64, softmax_batch_size: int = 512, mode: str = "tf1",
                 manifold_estimator: Optional[ManifoldEstimator] = None):
        self.inception = inception
        self.batch_size = batch_size
        self.softmax_batch_size = softmax_batch_size
        self.mode = mode
        self.manifold_estimator = manifold_estimator or ManifoldEstimator()

    def warmup(self):
        self.compute_activations([np.zeros([8, 64, 64, 3], dtype=np.uint8)])

    def read_activations(self, npz_path: str) -> Tuple[np.ndarray, np.ndarray]:
        return self.compute_activations(iter_npz_batches(npz_path, "arr_0", self.batch_size))

    def compute_activations(self, batches: Iterable[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """uint8 NHWC batches in [0, 255] -> (pool_3 float32 [N, 2048], spatial float32 [N, 2023])."""
        preds, spatial = [], []
        for batch in batches:
            u8 = torch.as_tensor(np.ascontiguousarray(batch)).to(torch.uint8)
            p, s = self.inception.features_all(u8.to(self.inception.device), self.mode)
            preds.append(p.cpu().numpy())
            spatial.append(s.cpu().numpy())
        return np.concatenate(preds, 0), np.concatenate(spatial, 0)

    def read_statistics(self, npz_path: str, activations: Tuple[np.ndarray, np.ndarray]) -> Tuple[FIDStatistics, FIDStatistics]:
        """A reference batch may carry its statistics (keys mu, sigma, mu_s, sigma_s); otherwise they come from `activations`."""
        with np.load(npz_path, allow_pickle=False) as obj:
            if "mu" in obj.files:
                return FIDStatistics(obj["mu"], obj["sigma"]), FIDStatistics(obj["mu_s"], obj["sigma_s"])
        return tuple(self.compute_statistics(x) for x in activations)

    def compute_statistics(self, activations, rows_per_call: int = 4096) -> FIDStatistics:
        """mean / covariance (np.mean, np.cov rowvar=False) through the device float64 Gram sums.  adm_fid_accumulate takes
        d % 4 == 0: narrower widths (the spatial 2023) are padded with zero columns and the statistics sliced back."""
        acts = torch.as_tensor(activations)
        n, d = acts.shape
        dp = (d + 3) // 4 * 4
        acc = ActivationAccumulator(dp, _device())
        for i in range(0, n, rows_per_call):
            blk = acts[i:i + rows_per_call].to(device=_device(), dtype=torch.float32)
            if dp != d:
                blk = torch.nn.functional.pad(blk, (0, dp - d))
            acc.add(blk.contiguous())
        st = acc.statistics()
        return FIDStatistics(st.mu[:d], st.sigma[:d, :d])

    def compute_inception_score(self, activations, split_size: int = 5000) -> float:
        """exp(mean KL(p(y|x) || p(y))) per split of `split_size` rows, averaged over the splits (the last may be shorter)."""
        w = getattr(self.inception, "fc_weight", None)
        if w is None:
            raise AdmError("compute_inception_score: the Inception checkpoint has no fc.weight (the softmax head)")
        acts = torch.as_tensor(activations)
        probs = []
        for i in range(0, acts.shape[0], self.softmax_batch_size):
            x = acts[i:i + self.softmax_batch_size].to(device=w.device, dtype=torch.float32).contiguous()
            probs.append(torch.softmax(ops.linear_f32(x, w).double(), dim=1))
        preds = torch.cat(probs, 0)
        scores = []
        for i in range(0, preds.shape[0], split_size):
            part = preds[i:i + split_size]
            kl = part * (torch.log(part) - torch.log(part.mean(0, keepdim=True)))
            scores.append(torch.exp(kl.sum(1).mean()))
        return float(torch.stack(scores).mean())

    def compute_prec_recall(self, activations_ref, activations_sample) -> Tuple[float, float]:
        me = self.manifold_estimator
        radii_1 = me.manifold_radii(activations_ref)
        radii_2 = me.manifold_radii(activations_sample)
        pr = me.evaluate_pr(activations_ref, radii_1, activations_sample, radii_2)
        return float(pr[0][0]), float(pr[1][0])

    def compute_kid(self, activations_ref, activations_sample, subsets: int = 100, subset_size: int = 1000,
                    seed: int = 0) -> Tuple[float, float]:
        """(mean, std) of the unbiased cubic-kernel MMD^2 over `subsets` draws of `subset_size` rows from each set (kid.py;
        project-defined: the reference's evaluator has no KID).  A set smaller than `subset_size` raises ValueError."""
        from .kid import kid_subsets
        return kid_subsets(_rows(activations_sample).contiguous(), _rows(activations_ref).contiguous(), subsets, subset_size, seed)


def random_inception(device, dtype: torch.dtype = torch.float16, classes: int = 1008, seed: int = 0):
    """An InceptionV3 on random weights with a seeded random softmax head: throughput runs and tests only."""
    from .inception import InceptionV3
    net = InceptionV3(dtype=dtype).to(device)
    net.weights_loaded = True        # asked for: the CLI tags every line instead
    g = torch.Generator().manual_seed(seed)
    net.fc_weight = (torch.randn(classes, 2048, generator=g) / math.sqrt(2048.0)).to(device)
    return net
