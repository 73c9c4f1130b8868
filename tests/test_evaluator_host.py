"""The ADM evaluation suite without a GPU: the k-NN C ABI's argument checks, the float64 restatement of the reference's
ManifoldEstimator / Inception Score that the GPU tests (test_hip_evaluator.py) compare against, the .npz handling and the
CLI's argument handling.

The restatement (TensorFlow and the Inception graph are not installed, so no reference-captured fixture can exist):
  * distances        evaluations/evaluator.py:485-500  max(|u|^2 - 2 u v^T + |v|^2, 0)
  * manifold_radii   :319-352  k-th smallest distance of each point to the whole set (itself included) for k in nhood_sizes,
                     then radii above np.percentile(radii, clamp_to_percentile, axis=0) set to 0
  * evaluate_pr      :396-430 with DistanceBlock.less_thans :473-483  precision = mean_j any_i d(i, j) <= r1[i],
                     recall = mean_i any_j d(i, j) <= r2[j]
  * inception score  :217-229  exp(mean_x KL(p(y|x) || mean p(y))) per split of split_size rows, averaged over the splits
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the float64 restatement (imported by test_hip_evaluator.py)
def ref_distances(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    nu, nv = (u * u).sum(1), (v * v).sum(1)
    return np.maximum(nu[:, None] - 2.0 * u @ v.T + nv[None, :], 0.0)


def ref_radii(features, nhood_sizes=(3,), clamp_to_percentile=None):
    d = ref_distances(features, features)
    kk = max(nhood_sizes) + 1
    radii = np.sort(d, axis=1)[:, :kk][:, list(nhood_sizes)]
    if clamp_to_percentile is not None:
        radii = radii.copy()
        radii[radii > np.percentile(radii, clamp_to_percentile, axis=0)] = 0
    return radii


def ref_pr(f1, r1, f2, r2):
    d = ref_distances(f1, f2)[..., None]
    f1_status = (d <= np.asarray(r2, np.float64)[None]).any(1)           # [n1, K2]
    f2_status = (d <= np.asarray(r1, np.float64)[:, None]).any(0)        # [n2, K1]
    return f2_status.astype(np.float64).mean(0), f1_status.astype(np.float64).mean(0)


def ref_inception_score(logits, split_size=5000):
    z = np.asarray(logits, np.float64)
    z = z - z.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    scores = []
    for i in range(0, len(p), split_size):
        part = p[i:i + split_size]
        kl = part * (np.log(part) - np.log(part.mean(0, keepdims=True)))
        scores.append(np.exp(kl.sum(1).mean()))
    return float(np.mean(scores))


def fp16_rows(x):
    """The features the kernels see: the reference's tf.float16 cast (evaluator.py:447-450), back in float64."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------ the restatement against brute force
def _brute_radii(x, nhood_sizes, clamp):
    n = len(x)
    out = np.zeros((n, len(nhood_sizes)))
    for i in range(n):
        ds = sorted(sum((x[i][t] - x[j][t]) ** 2 for t in range(x.shape[1])) for j in range(n))
        out[i] = [ds[k] for k in nhood_sizes]
    if clamp is not None:
        for c in range(out.shape[1]):
            col = sorted(out[:, c])
            pos = (len(col) - 1) * clamp / 100.0          # numpy's default ("linear") percentile
            lo = int(np.floor(pos))
            hi = min(lo + 1, len(col) - 1)
            thr = col[lo] + (col[hi] - col[lo]) * (pos - lo)
            out[out[:, c] > thr, c] = 0
    return out


@pytest.mark.parametrize("nhood_sizes,clamp", [((3,), None), ((1, 2, 5), None), ((0, 3), 50.0), ((2,), 90.0)])
def test_restated_radii_match_brute_force(nhood_sizes, clamp):
    rng = np.random.default_rng(1)
    x = rng.integers(-4, 5, size=(23, 5)).astype(np.float64)
    np.testing.assert_allclose(ref_radii(x, nhood_sizes, clamp), _brute_radii(x, nhood_sizes, clamp), rtol=0, atol=1e-9)


def test_restated_pr_match_brute_force():
    rng = np.random.default_rng(2)
    f1, f2 = rng.normal(size=(17, 4)), rng.normal(size=(11, 4)) + 0.3
    r1, r2 = ref_radii(f1, (1, 3)), ref_radii(f2, (1, 3))
    prec, rec = ref_pr(f1, r1, f2, r2)
    d = lambda u, v: float(((u - v) ** 2).sum())
    for k in range(2):
        assert prec[k] == np.mean([any(d(f1[i], f2[j]) <= r1[i, k] for i in range(17)) for j in range(11)])
        assert rec[k] == np.mean([any(d(f1[i], f2[j]) <= r2[j, k] for j in range(11)) for i in range(17)])


def test_restated_inception_score_with_a_remainder_split():
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(23, 7)) * 2
    got = ref_inception_score(logits, split_size=10)          # splits of 10, 10, 3
    scores = []
    for s in (slice(0, 10), slice(10, 20), slice(20, 23)):
        p = [np.exp(r) / np.exp(r).sum() for r in logits[s]]
        py = np.mean(p, 0)
        scores.append(np.exp(np.mean([sum(pi[c] * np.log(pi[c] / py[c]) for c in range(7)) for pi in p])))
    assert abs(got - np.mean(scores)) <= 1e-12 * abs(got)
    assert ref_inception_score(np.zeros((5, 4))) == pytest.approx(1.0)


# ------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree_on_the_knn_entry_points():
    from autodiffusion_amd import _lib
    assert _lib.ABI_VERSION == 10
    for kind in ("bf16", "f16"):
        lib = _lib.load(kind)
        assert lib.adm_abi_version() == 10
        for name in ("adm_knn_smallest", "adm_knn_cover"):
            assert name in _lib.SIGNATURES and hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    assert "int adm_knn_smallest(" in text and "int adm_knn_cover(" in text and "#define ADM_ABI_VERSION 10" in text


def test_knn_argument_errors_without_a_gpu():
    from autodiffusion_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)         # never dereferenced: every call below fails its argument check
    ok = dict(q=fake, nq=256, qn=fake, x=fake, nx=256, xn=fake, d=2048, kk=4, out=fake, ws=fake, splits=2)

    def smallest(**kw):
        a = dict(ok, **kw)
        return lib.adm_knn_smallest(a["q"], a["nq"], a["qn"], a["x"], a["nx"], a["xn"], a["d"], a["kk"], a["out"], a["ws"],
                                    a["splits"], None)
    assert smallest(q=None) == -1 and b"null" in lib.adm_last_error()
    assert smallest(out=None) == -1
    assert smallest(kk=0) == -1 and b"kk" in lib.adm_last_error()
    assert smallest(kk=9) == -1 and b"kk" in lib.adm_last_error()
    assert smallest(nx=3) == -1 and b"nx" in lib.adm_last_error()
    assert smallest(nq=0) == -1
    assert smallest(d=2000) == -2 and b"multiple" in lib.adm_last_error()
    assert smallest(splits=3) == -1 and b"splits" in lib.adm_last_error()     # 256 rows = 2 tiles of 128
    assert smallest(ws=None) == -1 and b"workspace" in lib.adm_last_error()
    assert smallest(q=C.c_void_p(0x1008)) == -3

    def cover(**kw):
        a = dict(a=fake, na=100, an=fake, ra=fake, b=fake, nb=50, bn=fake, rb=fake, d=64, K=1, ai=fake, bi=fake)
        a.update(kw)
        return lib.adm_knn_cover(a["a"], a["na"], a["an"], a["ra"], a["b"], a["nb"], a["bn"], a["rb"], a["d"], a["K"], a["ai"],
                                 a["bi"], None)
    assert cover(rb=None) == -1 and b"null" in lib.adm_last_error()
    assert cover(bi=None) == -1
    assert cover(K=0) == -1 and cover(K=9) == -1
    assert cover(nb=0) == -1 and b"nb" in lib.adm_last_error()
    assert cover(d=48) == -2
    assert cover(b=C.c_void_p(0x1004)) == -3


def test_estimator_rejects_unsupported_neighbourhoods():
    from autodiffusion_amd.evaluator import ManifoldEstimator
    with pytest.raises(ValueError):
        ManifoldEstimator(nhood_sizes=(8,))
    with pytest.raises(ValueError):
        ManifoldEstimator(nhood_sizes=())
    assert ManifoldEstimator(nhood_sizes=(1, 3, 7)).num_nhoods == 3


# ------------------------------------------------------------------ .npz handling
def test_npz_batches_stream_stored_and_compressed(tmp_path):
    from autodiffusion_amd.evaluator import iter_npz_batches
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 256, size=(37, 8, 6, 3), dtype=np.uint8)
    for save in (np.savez, np.savez_compressed):
        p = str(tmp_path / f"{save.__name__}.npz")
        save(p, arr, labels=np.arange(37))
        parts = list(iter_npz_batches(p, "arr_0", 10))
        assert [len(b) for b in parts] == [10, 10, 10, 7]
        assert np.array_equal(np.concatenate(parts), arr)
    p = str(tmp_path / "f.npz")
    np.savez(p, np.asfortranarray(arr[:5, :, :, 0]))
    assert np.array_equal(np.concatenate(list(iter_npz_batches(p, "arr_0", 2))), arr[:5, :, :, 0])
    with pytest.raises(KeyError):
        next(iter_npz_batches(p, "mu", 2))


class _NoNet:
    fc_weight = None


def test_read_statistics_takes_stored_statistics_or_computes_them(tmp_path, monkeypatch):
    from autodiffusion_amd import evaluator as ev
    e = ev.Evaluator(_NoNet())
    d = 6
    mu, sigma, mu_s, sigma_s = np.arange(d) * 1.0, np.eye(d) * 2, np.arange(3) * 1.0, np.eye(3) * 3
    with_stats = str(tmp_path / "ref_stats.npz")
    np.savez(with_stats, np.zeros((2, 8, 8, 3), np.uint8), mu=mu, sigma=sigma, mu_s=mu_s, sigma_s=sigma_s)
    a, b = e.read_statistics(with_stats, (None, None))
    assert np.array_equal(a.mu, mu) and np.array_equal(a.sigma, sigma)
    assert np.array_equal(b.mu, mu_s) and np.array_equal(b.sigma, sigma_s)
    # arr-only: the statistics come from the activations (compute_statistics; its device form is tested on the GPU)
    arr_only = str(tmp_path / "ref.npz")
    np.savez(arr_only, np.zeros((2, 8, 8, 3), np.uint8))
    monkeypatch.setattr(ev.Evaluator, "compute_statistics", lambda self, x: ("stats", x.shape))
    acts = (np.ones((4, d)), np.ones((4, 3)))
    assert e.read_statistics(arr_only, acts) == (("stats", (4, d)), ("stats", (4, 3)))


def test_inception_score_needs_the_softmax_head():
    from autodiffusion_amd import evaluator as ev
    from autodiffusion_amd._lib import AdmError
    with pytest.raises(AdmError, match="fc.weight"):
        ev.Evaluator(_NoNet()).compute_inception_score(np.zeros((4, 2048), np.float32))


def test_load_state_dict_keeps_fc_weight_only():
    import torch
    from autodiffusion_amd.inception import InceptionV3
    from oracle import inception as oinc
    sd = dict(oinc.fill_params())
    w = torch.randn(1008, 2048)
    sd.update({"fc.weight": w, "fc.bias": torch.zeros(1008), "AuxLogits.fc.weight": torch.zeros(1000, 768)})
    net = InceptionV3()
    assert net.fc_weight is None
    missing, unexpected = net.load_state_dict(sd)
    assert not missing and not unexpected
    assert torch.equal(net.fc_weight, w) and net.fc_weight.dtype == torch.float32


# ------------------------------------------------------------------ CLI
def _cli(*args, **kw):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluator.py"), *args], capture_output=True, text=True,
                          env=env, timeout=120, **kw)


def test_cli_refuses_random_weights_unless_asked(tmp_path):
    r = _cli(str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz"))
    assert r.returncode != 0 and "--inception_path" in r.stderr and "--inception_random True" in r.stderr
    assert not os.path.exists(str(tmp_path / "sample_eval.log"))


def test_cli_argument_handling():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import evaluator as cli
    finally:
        sys.path.pop(0)
    a = cli.create_argparser().parse_args(["r.npz", "s.npz"])
    assert (a.ref_batch, a.sample_batch, a.batch_size, a.mode, a.inception_random, a.save_ref_stats) == \
        ("r.npz", "s.npz", 64, "tf1", False, "")
    a = cli.create_argparser().parse_args(["r.npz", "/x/s.npz", "--inception_random", "True", "--batch_size", "16", "--mode", "pt",
                                           "--save_ref_stats", "o.npz"])
    assert a.inception_random is True and a.batch_size == 16 and a.mode == "pt" and a.save_ref_stats == "o.npz"
    assert cli.log_path("/x/s.npz") == "/x/s_eval.log"
    with pytest.raises(SystemExit):
        cli.create_argparser().parse_args(["r.npz", "s.npz", "--mode", "tf2"])
    r = _cli("--help")
    assert r.returncode == 0 and "--save_ref_stats" in r.stdout
