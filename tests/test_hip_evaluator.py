"""The ADM evaluation suite on the MI355X against the float64 restatement of the reference (test_evaluator_host.py):
k-NN radii, precision / recall, the fp32 fallback, the Inception taps, the Inception Score and the CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_evaluator_host import fp16_rows, ref_distances, ref_inception_score, ref_pr, ref_radii

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clustered(n, d, seed, clusters=20, spread=0.35):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(clusters, d)).astype(np.float32)
    x = centers[rng.integers(0, clusters, n)] + spread * rng.normal(size=(n, d)).astype(np.float32)
    return np.abs(x).astype(np.float32)          # pool3-like: non-negative


def lattice(n, d, seed, centers):
    """Clustered features on multiples of 1/4 in [-1, 1]: exact in fp16, and every dot product / distance is exact in fp32."""
    rng = np.random.default_rng(seed)
    x = centers[rng.integers(0, len(centers), n)] + rng.integers(-1, 2, size=(n, d))
    return (np.clip(x, -4, 4) / 4.0).astype(np.float32)


def tol(x):
    return 1e-5 * float((np.asarray(x, np.float64) ** 2).sum(1).max())


@pytest.fixture(scope="module")
def ev():
    from autodiffusion_amd import _lib, evaluator
    _lib.load()
    torch.cuda.set_device(0)
    return evaluator


def test_radii_match_the_restatement(ev):
    x = clustered(3000, 2048, 0)
    me = ev.ManifoldEstimator(nhood_sizes=(1, 3, 5))
    got = me.manifold_radii(x)
    assert me.last_path == "fp16" and got.dtype == np.float32 and got.shape == (3000, 3)
    ref = ref_radii(fp16_rows(x), (1, 3, 5))
    assert np.abs(got - ref).max() <= tol(x)
    # device tensors in, the same numbers out
    assert np.array_equal(me.manifold_radii(torch.from_numpy(x).to(DEV)), got)
    # clamp_to_percentile on top of the same radii
    me_c = ev.ManifoldEstimator(nhood_sizes=(1, 3, 5), clamp_to_percentile=50)
    gc = me_c.manifold_radii(x)
    assert np.array_equal(gc, np.where(got > np.percentile(got, 50, axis=0), 0, got))


@pytest.mark.parametrize("nq,nx,kk", [(333, 1001, 8), (1, 130, 3), (200, 4, 4), (129, 8, 8)])
def test_ragged_shapes(ev, nq, nx, kk):
    q, x = clustered(nq, 2048, 1), clustered(nx, 2048, 2)
    pq, px = ev._Prepared(torch.from_numpy(q).to(DEV)), ev._Prepared(torch.from_numpy(x).to(DEV))
    got = ev.knn_smallest(pq.x16, pq.norm, px.x16, px.norm, kk).cpu().numpy()
    ref = np.sort(ref_distances(fp16_rows(q), fp16_rows(x)), axis=1)[:, :kk]
    assert np.abs(got - ref).max() <= tol(np.concatenate([q, x]))


def test_bitwise_independent_of_splits_and_runs(ev):
    x = clustered(2600, 2048, 3)
    p = ev._Prepared(torch.from_numpy(x).to(DEV))
    a = ev.knn_smallest(p.x16, p.norm, p.x16, p.norm, 6, splits=1)
    b = ev.knn_smallest(p.x16, p.norm, p.x16, p.norm, 6, splits=7)
    c = ev.knn_smallest(p.x16, p.norm, p.x16, p.norm, 6, splits=7)
    assert torch.equal(a, b) and torch.equal(b, c)


def test_precision_recall_exactly_the_restatement(ev):
    centers = np.random.default_rng(4).integers(-3, 4, size=(16, 2048))
    f1, f2 = lattice(900, 2048, 5, centers[:12]), lattice(700, 2048, 6, centers[4:])     # 8 shared clusters of 16
    r1, r2 = ref_radii(f1, (1, 3)), ref_radii(f2, (1, 3))
    # radii half a lattice step (1/32; distances are multiples of 1/16) off the distances: every decision has a margin
    r1, r2 = r1 + 1 / 32, r2 + 1 / 32
    d12 = ref_distances(f1, f2)[..., None]
    margin = min(np.abs(d12 - r1[:, None]).min(), np.abs(d12 - r2[None]).min())
    assert margin > tol(np.concatenate([f1, f2]))
    me = ev.ManifoldEstimator(nhood_sizes=(1, 3))
    prec, rec = me.evaluate_pr(f1, r1.astype(np.float32), f2, r2.astype(np.float32))
    assert me.last_path == "fp16"
    rp, rr = ref_pr(f1, r1.astype(np.float32), f2, r2.astype(np.float32))
    assert np.array_equal(prec, rp) and np.array_equal(rec, rr)
    assert 0 < prec[0] < 1 and 0 < rec[1] < 1, (prec, rec)
    # on the lattice the kernel's distances are exact: its radii and the whole chain equal the restatement's
    g1, g2 = me.manifold_radii(f1), me.manifold_radii(f2)
    assert np.array_equal(g1, ref_radii(f1, (1, 3)).astype(np.float32))
    assert all(np.array_equal(u, v) for u, v in zip(me.evaluate_pr(f1, g1, f2, g2), ref_pr(f1, g1, f2, g2)))


def test_radii_at_50k_stay_out_of_memory(ev):
    n = 50000
    x = torch.from_numpy(clustered(n, 2048, 6)).to(DEV)
    me = ev.ManifoldEstimator()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = me.manifold_radii(x)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    assert me.last_path == "fp16" and r.shape == (n, 1)
    assert grew < (1 << 30) // 2, grew         # the fp16 copy of the rows (200 MB) and its norms; an N x N fp32 matrix: 10 GB
    rows = np.random.default_rng(7).choice(n, 64, replace=False)
    xs = fp16_rows(x.cpu().numpy())
    ref = np.sort(ref_distances(xs[rows], xs), axis=1)[:, 3]
    assert np.abs(r[rows, 0] - ref).max() <= tol(xs)


def test_fp32_fallback_past_the_fp16_bound(ev):
    f1, f2 = clustered(500, 2048, 8) * 8.0, clustered(400, 2048, 9) * 8.0     # 4 max|x|^2 >> 65504
    me = ev.ManifoldEstimator(nhood_sizes=(2,), row_batch_size=128, col_batch_size=96)
    r1 = me.manifold_radii(f1)
    assert me.last_path == "fp32"
    assert np.abs(r1 - ref_radii(f1, (2,))).max() <= tol(f1)
    r2 = me.manifold_radii(f2)
    prec, rec = me.evaluate_pr(f1, r1, f2, r2)
    assert me.last_path == "fp32"
    rp, rr = ref_pr(f1, r1, f2, r2)
    assert abs(prec[0] - rp[0]) <= 2 / 400 and abs(rec[0] - rr[0]) <= 2 / 500


@pytest.fixture(scope="module")
def net():
    from autodiffusion_amd.inception import InceptionV3
    from oracle import inception as oinc
    p = oinc.fill_params()
    m = InceptionV3().to(DEV)
    m.load_state_dict(p)
    return m, p


def test_inception_taps(net):
    from oracle import inception as oi
    m, p = net
    u8 = torch.from_numpy(np.random.default_rng(10).integers(0, 256, size=(3, 64, 64, 3), dtype=np.uint8))
    pool, spatial = m.features_all(u8.to(DEV), "tf1")
    assert torch.equal(pool, m.features(u8.to(DEV), "tf1"))
    assert spatial.shape == (3, 2023) and spatial.dtype == torch.float32
    x = oi.prepare(u8, "tf1")
    x = oi._bc(p, "Conv2d_1a_3x3", x, stride=2)
    x = oi._bc(p, "Conv2d_2a_3x3", x)
    x = oi._bc(p, "Conv2d_2b_3x3", x, padding=1)
    x = torch.nn.functional.max_pool2d(x, 3, stride=2)
    x = oi._bc(p, "Conv2d_3b_1x1", x)
    x = oi._bc(p, "Conv2d_4a_3x3", x)
    x = torch.nn.functional.max_pool2d(x, 3, stride=2)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = oi._a(p, n, x)
    x = oi._b(p, "Mixed_6a", x)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d"):
        x = oi._cblk(p, n, x)
    ref = x[:, :7].permute(0, 2, 3, 1).reshape(3, -1)          # mixed_6/conv[..., :7], NHWC-flattened
    s = spatial.cpu()
    assert ((s - ref).norm() / ref.norm()).item() <= 5e-3


def test_inception_score_matches_the_restatement(ev, net):
    m, _ = net
    g = torch.Generator().manual_seed(11)
    w = torch.randn(1008, 2048, generator=g) * 0.05
    m.fc_weight = w.to(DEV)
    acts = np.abs(np.random.default_rng(12).normal(size=(1300, 2048))).astype(np.float32)
    e = ev.Evaluator(m, softmax_batch_size=512)
    got = e.compute_inception_score(acts, split_size=500)            # splits 500, 500, 300
    ref = ref_inception_score(acts.astype(np.float64) @ w.numpy().astype(np.float64).T, split_size=500)
    assert abs(got - ref) <= 1e-5 * ref, (got, ref)


def test_compute_statistics_pads_to_the_gram_kernel(ev, net):
    m, _ = net
    acts = np.random.default_rng(13).normal(size=(300, 2023)).astype(np.float32)
    st = ev.Evaluator(m).compute_statistics(acts)
    assert st.mu.shape == (2023,) and st.sigma.shape == (2023, 2023)
    np.testing.assert_allclose(st.mu, acts.astype(np.float64).mean(0), atol=1e-9)
    np.testing.assert_allclose(st.sigma, np.cov(acts.astype(np.float64), rowvar=False), atol=1e-8)


def test_cli_end_to_end(ev, tmp_path):
    rng = np.random.default_rng(14)
    ref_p, smp_p, stats_p = str(tmp_path / "ref.npz"), str(tmp_path / "samples.npz"), str(tmp_path / "ref_stats.npz")
    ref = rng.integers(0, 256, size=(400, 64, 64, 3), dtype=np.uint8)
    smp = np.clip(ref[:300].astype(np.int16) + rng.integers(-40, 41, size=(300, 64, 64, 3)), 0, 255).astype(np.uint8)
    np.savez(ref_p, ref)
    np.savez(smp_p, smp)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "evaluator.py"), ref_p, smp_p,
                        "--inception_random", "True", "--batch_size", "100", "--save_ref_stats", stats_p],
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    names = ["Inception Score: ", "FID: ", "sFID: ", "Precision:", "Recall:"]
    vals = {}
    for name in names:
        lines = [ln.split(" ", 3)[3] for ln in r.stdout.splitlines() if ln.count(" ") >= 3]     # "%m/%d %I:%M:%S %p" message
        lines = [ln for ln in lines if ln.startswith(name) and ln.endswith("[RANDOM Inception weights: not a quality metric]")]
        assert len(lines) == 1, (name, r.stdout)
        vals[name] = float(lines[0][len(name):].split(" [", 1)[0])
    log = open(str(tmp_path / "samples_eval.log")).read()
    assert all(name in log for name in names) and log.count("RANDOM Inception weights") == 5
    # the same numbers from the Python API in this process
    from autodiffusion_amd.fid import FIDStatistics
    e = ev.Evaluator(ev.random_inception(DEV), batch_size=100)
    ra, sa = e.read_activations(ref_p), e.read_activations(smp_p)
    rs, rss = e.read_statistics(ref_p, ra)
    ss, sss = e.read_statistics(smp_p, sa)
    prec, rec = e.compute_prec_recall(ra[0], sa[0])
    api = {"Inception Score: ": e.compute_inception_score(sa[0]), "FID: ": ss.frechet_distance(rs),
           "sFID: ": sss.frechet_distance(rss), "Precision:": prec, "Recall:": rec}
    for name in names:
        assert vals[name] == pytest.approx(api[name], rel=1e-9, abs=1e-12), name
    # --save_ref_stats loads in the search driver's reader (search.EvolutionSearcher, --ref_path)
    z = np.load(stats_p, allow_pickle=False)
    st = FIDStatistics(z["mu"], z["sigma"])
    assert st.mu.shape == (2048,) and st.sigma.shape == (2048, 2048) and z["mu_s"].shape == (2023,)
    assert np.array_equal(st.mu, rs.mu) and np.array_equal(z["sigma_s"], rss.sigma)
