"""CPU checks of CMMD: the float64 restatement (tests/cmmd_ref.py) against an explicit double loop, the two estimators from the same
sums, why the kernel sums k - 1 through expm1 in float64, the error bound against the defects it must catch, autodiffusion_amd/cmmd.py
and SDCandidateEvaluator(fitness="cmmd") with the restatement standing in for the kernel, the loaders' and the C ABI's refusals
(argument checks run before any launch) and the command lines' parsers."""
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cmmd_ref
from autodiffusion_amd import _lib, cmmd
from autodiffusion_amd._lib import AdmError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cmmd_host", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def host_sums(monkeypatch):
    """cmmd.rbf_sums answered by the restatement on host tensors: everything of cmmd.py but the kernel call runs here."""
    def sums(x, y=None, sigma=cmmd.SIGMA):
        for t in (x, y):
            if t is not None and not bool((t.double().pow(2).sum(1) > 0).all()):
                raise ValueError("CMMD: an embedding row has squared norm 0.0")
        return cmmd_ref.rbf_sum(x.numpy(), None if y is None else y.numpy(), sigma)[0]
    monkeypatch.setattr(cmmd, "rbf_sums", sums)


# ------------------------------------------------------------------ the restatement
def test_restatement_equals_the_double_loop():
    x, y = cmmd_ref.features(5, 8, 1, shift=0.2), cmmd_ref.features(7, 8, 2)
    x = cmmd_ref.with_shared_row(cmmd_ref.with_near_duplicates(x), y)
    for sigma in (1.0, 10.0):
        for a, b in ((x, y), (y, x), (x, None), (y, None)):
            s, sa, pairs = cmmd_ref.rbf_sum(a, b, sigma)
            # both sides are float64: the loop's own rounding is of the bound's form, with python's serial sums
            tol = cmmd_ref.bound(pairs, sa, 8, pairs, sigma, e_ulp=2)
            assert abs(s - cmmd_ref.rbf_sum_loops(a, b, sigma)) <= 2 * tol
            assert sa == pytest.approx(-s, rel=1e-15) and s < 0 and pairs == (len(a) * (len(a) - 1) if b is None else len(a) * len(b))
        assert cmmd_ref.rbf_sum(x, None, sigma)[0] == pytest.approx(cmmd_ref.rbf_sum(x, x, sigma)[0], rel=1e-12)   # the diagonal adds (about) 0
        for unbiased in (False, True):
            assert cmmd_ref.mmd2(x, y, sigma, unbiased) == pytest.approx(cmmd_ref.mmd2_loops(x, y, sigma, unbiased), rel=1e-9)
    k = cmmd_ref.kappa_matrix(x, y)
    assert k[2, 0] == pytest.approx(0.0, abs=1e-16) and np.all(k <= 0.0)        # the shared row: cosine 1
    assert -1e-9 < cmmd_ref.kappa_matrix(x, x)[0, 1] < 0.0                       # the near duplicate: 2 - 2 c ~ 1e-9


def test_v_and_u_forms_come_from_the_same_sums_and_the_ones_cancel():
    x, y = cmmd_ref.features(9, 12, 3, shift=0.3).numpy(), cmmd_ref.features(14, 12, 4).numpy()
    n, m = 9, 14
    sxx, syy, sxy = (cmmd_ref.rbf_sum(a, b)[0] for a, b in ((x, None), (y, None), (x, y)))
    v, u = cmmd.mmd2_from_sums(sxx, n, syy, m, sxy), cmmd.mmd2_from_sums(sxx, n, syy, m, sxy, unbiased=True)
    assert v == cmmd_ref.mmd2(x, y) and u == cmmd_ref.mmd2(x, y, unbiased=True)
    # the textbook forms on k = kappa + 1: full-matrix means (the diagonal's k = 1 included), and the means over i != j
    kxx, kyy, kxy = (cmmd_ref.kappa_matrix(a, b).astype(np.longdouble) + 1 for a, b in ((x, x), (y, y), (x, y)))
    np.fill_diagonal(kxx, 1.0)
    np.fill_diagonal(kyy, 1.0)
    v_text = kxx.mean() + kyy.mean() - 2 * kxy.mean()
    u_text = (kxx.sum() - n) / (n * (n - 1)) + (kyy.sum() - m) / (m * (m - 1)) - 2 * kxy.mean()
    assert v == pytest.approx(float(v_text), rel=1e-9) and u == pytest.approx(float(u_text), rel=1e-9)
    assert v > u and v - u == pytest.approx(-(sxx / (n * n * (n - 1.0)) + syy / (m * m * (m - 1.0))), rel=1e-9)   # the V-statistic's bias
    assert cmmd_ref.cmmd(x, y) == 1000.0 * v and cmmd_ref.fitness(x, y) == 1000.0 * u
    assert cmmd.mmd2_from_sums(sxx, n, syy, m, sxy) == cmmd.mmd2_from_sums(syy, m, sxx, n, sxy)
    with pytest.raises(ValueError, match="at least 2 rows"):
        cmmd.mmd2_from_sums(0.0, 1, syy, m, sxy, unbiased=True)
    assert cmmd.mmd2_from_sums(0.0, 1, 0.0, 1, -0.25) == 0.5


def test_fp32_mean_of_exp_loses_the_value_and_float64_expm1_does_not():
    """Why the kernel is built the way it is.  1024 x 1024 pairs at sigma = 10: each mean of k is ~0.994 and MMD^2 ~1e-4.  An fp32
    running sum of 2^20 values near 1 has a spacing of 2^-4 by its end -- more than ten times 1 - k."""
    x, y = cmmd_ref.features(1024, 16, 1, shift=0.1).numpy(), cmmd_ref.features(1024, 16, 2).numpy()
    want = cmmd_ref.mmd2(x, y)
    naive = cmmd_ref.mmd2_naive_fp32(x, y)
    assert 1e-5 < want < 1e-3
    print(f"MMD^2_v {want:.6g}; fp32 mean(exp) {naive:.6g} (relative error {abs(naive - want) / want:.3g})")
    assert abs(naive - want) / want > 0.10
    # the float64 expm1 form against 64-bit-mantissa arithmetic on a subset (the whole set in long double takes too long)
    xs, ys = x[:96], y[:80]
    kl = [np.expm1(-np.longdouble(cmmd_ref.gamma_of(10.0)) * np.maximum(2 - 2 * (
        (a.astype(np.longdouble) @ b.astype(np.longdouble).T) / np.sqrt((a.astype(np.longdouble) ** 2).sum(1)[:, None] * (b.astype(np.longdouble) ** 2).sum(1)[None, :])), 0))
        for a, b in ((xs, xs), (ys, ys), (xs, ys))]
    ext = (kl[0].sum() - np.trace(kl[0])) / (96 * 96) + (kl[1].sum() - np.trace(kl[1])) / (80 * 80) - 2 * kl[2].sum() / (96 * 80)
    assert cmmd_ref.mmd2(xs, ys) == pytest.approx(float(ext), rel=1e-9)


# ------------------------------------------------------------------ the bound and the planted defects
def test_chains_and_workspace_match_the_library():
    assert cmmd.rbf_blocks(64, 64, False) == 1 and cmmd.rbf_blocks(65, 129, False) == 6 and cmmd.rbf_blocks(257, 257, True) == 15
    assert cmmd.reduction_chain(64, 64, False) == 16 + 6 + 3 + 1 + 8
    assert cmmd.reduction_chain(1, 1, False) == 1 and cmmd.reduction_chain(2, 3, False) == 6 and cmmd.reduction_chain(2, 2, True) == 2
    assert cmmd.reduction_chain(30000, 30000, True) == 16 + 6 + 3 + -(-(469 * 470 // 2) // 256) + 8
    assert [cmmd.norm_chain(d) for d in (4, 8, 36, 256, 260, 768)] == [4, 8, 10, 10, 14, 18]
    assert all(cmmd.norm_chain(d) == cmmd_ref.norm_chain(d) for d in range(4, 2049, 4))
    lib = _lib.load()
    for n, m, sp in ((1, 1, 0), (64, 64, 0), (65, 129, 0), (65, 65, 1), (257, 257, 1), (30000, 30000, 1), (5000, 30000, 0)):
        assert lib.adm_rbf_work_elems(n, m, sp) == cmmd.work_elems(n, m, bool(sp)) == cmmd.rbf_blocks(n, m, bool(sp)) + n + m, (n, m, sp)
    assert lib.adm_rbf_work_elems(0, 5, 0) == -1 and lib.adm_rbf_work_elems(5, 6, 1) == -1
    assert cmmd.gamma_of(10.0) == cmmd_ref.gamma_of(10.0) == 0.005 and cmmd.gamma_of(1.0) == 0.5
    assert cmmd_ref.E_ULP == math.ceil(cmmd_ref.MEASURED_E_ULP) + 1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            cmmd.gamma_of(bad)


def test_kid_and_cmmd_share_one_tile_geometry():
    """adm_pairsum.h and mmd.py each define the block count once: the two libraries' entry points and the two modules agree on it."""
    from autodiffusion_amd import kid
    lib = _lib.load()
    for n, m, sp in ((1, 1, 0), (2, 2, 1), (64, 64, 0), (65, 129, 0), (130, 70, 0), (65, 65, 1), (257, 257, 1), (30000, 30000, 1)):
        blocks = lib.adm_poly3_work_elems(n, m, sp)
        assert blocks == lib.adm_rbf_work_elems(n, m, sp) - n - m == kid.poly3_blocks(n, m, bool(sp)) == cmmd.rbf_blocks(n, m, bool(sp)), (n, m, sp)
        assert blocks > 0


@pytest.mark.parametrize("sigma", [1.0, 10.0])
def test_every_planted_defect_falls_outside_the_bound(sigma):
    n, m, d = 65, 129, 36
    x, y = cmmd_ref.cross_inputs(n, m, d)
    cases = [(x.numpy(), y.numpy(), [f for f in cmmd_ref.DEFECTS if f not in cmmd_ref.SELF_ONLY]),
             (cmmd_ref.self_inputs(65, d).numpy(), None, list(cmmd_ref.DEFECTS))]
    for a, b, defects in cases:
        s, sa, pairs = cmmd_ref.rbf_sum(a, b, sigma)
        rows_b = len(a) if b is None else len(b)
        tol = cmmd_ref.bound(pairs, sa, d, cmmd.reduction_chain(len(a), rows_b, b is None), sigma)
        assert 0 < tol < 1e-9 * sa                                  # the bound is a float64 bound: ten digits of the sum
        for defect in defects:
            bad = cmmd_ref.rbf_sum(a, b, sigma, defect)[0]
            print(f"sigma {sigma:g} {'self' if b is None else 'cross'} {defect}: off by {abs(bad - s):.3g}, bound {tol:.3g}")
            assert abs(bad - s) > 100 * tol, defect
    pad = 128 * 192 - 65 * 129
    assert cmmd_ref.rbf_sum(x.numpy(), y.numpy(), sigma, "padded_rows")[0] - cmmd_ref.rbf_sum(x.numpy(), y.numpy(), sigma)[0] == pytest.approx(
        pad * math.expm1(-2 * cmmd_ref.gamma_of(sigma)), rel=1e-9)
    with pytest.raises(AssertionError):
        cmmd_ref.rbf_sum(x.numpy(), y.numpy(), sigma, "offdiag_once")       # a self-mode defect


def test_inputs_are_clip_like():
    x, y = cmmd_ref.cross_inputs(257, 130, 768)
    norms = x.double().norm(dim=1)
    assert 7.0 < float(norms.min()) and float(norms.max()) < 13.0
    k = cmmd_ref.kappa_matrix(x.numpy(), y.numpy())
    cos = 1.0 + np.log1p(k) / (2.0 * cmmd_ref.gamma_of(10.0))
    assert 0.3 < np.median(cos) < 0.9 and np.percentile(cos, 1) > 0.2
    assert torch.equal(x[2], y[0]) and 0 < float((x[1] - x[0]).norm()) < 1e-2


# ------------------------------------------------------------------ cmmd.py around the kernel call
def test_cmmd_reference_and_cmmd_with_the_restatement(host_sums):
    x, y = cmmd_ref.features(9, 12, 7, shift=0.2), cmmd_ref.features(14, 12, 8)
    assert cmmd.cmmd(x, y) == cmmd_ref.cmmd(x.numpy(), y.numpy()) and cmmd.cmmd(x, y, 1.0) == cmmd_ref.cmmd(x.numpy(), y.numpy(), 1.0)
    assert cmmd.mmd2(x, y, unbiased=True) == cmmd_ref.mmd2(x.numpy(), y.numpy(), unbiased=True)
    assert cmmd.mmd2(x, y) == pytest.approx(cmmd.mmd2(y, x), rel=1e-12)
    ref = cmmd.CMMDReference(y, device="cpu")
    assert ref.s_yy == cmmd_ref.rbf_sum(y.numpy())[0] and ref.sigma == 10.0
    assert ref.cmmd(x) == cmmd_ref.cmmd(x.numpy(), y.numpy()) and ref.fitness(x) == cmmd_ref.fitness(x.numpy(), y.numpy())
    assert ref.cmmd(x) > ref.fitness(x)
    assert cmmd.CMMDReference(y.numpy(), device="cpu", sigma=1.0).fitness(x) == cmmd_ref.fitness(x.numpy(), y.numpy(), 1.0)
    assert cmmd.cmmd(x[:1], y) == cmmd_ref.cmmd(x[:1].numpy(), y.numpy())          # the V form takes a single row
    with pytest.raises(ValueError, match="at least 2 rows"):
        ref.fitness(x[:1])
    with pytest.raises(ValueError, match="m >= 2"):
        cmmd.CMMDReference(y[:1], device="cpu")
    zero = x.clone()
    zero[3] = 0.0
    with pytest.raises(ValueError, match="squared norm"):
        ref.cmmd(zero)


def test_host_tensors_are_refused_without_a_fallback():
    from autodiffusion_amd import ops
    x = cmmd_ref.features(4, 8, 1)
    with pytest.raises(AdmError, match="no CPU fallback"):
        cmmd.rbf_sums(x)
    with pytest.raises(AdmError, match="no CPU fallback"):
        cmmd.cmmd(x, x)
    with pytest.raises(AdmError):
        ops.rbf_sums(x, x)


def test_loader_names_the_flag_that_writes_the_file(tmp_path):
    from autodiffusion_amd import sd_script_util
    p = str(tmp_path / "feats.npz")
    rows = cmmd_ref.features(6, 8, 1).numpy()
    assert sd_script_util.save_clip_feats(p, rows.astype(np.float64)) == p and os.path.exists(p)
    got = cmmd.load_ref_clip_feats(p)
    assert got.dtype == np.float32 and np.array_equal(got, rows)
    np.savez(str(tmp_path / "other.npz"), feats=rows)
    with pytest.raises(KeyError, match=r"sd_clip_score\.py --save_clip_feats"):
        cmmd.load_ref_clip_feats(str(tmp_path / "other.npz"))
    for bad in (rows[:1], rows[0]):
        with open(p, "wb") as f:
            np.savez(f, clip_feats=bad)
        with pytest.raises(ValueError, match="m >= 2"):
            cmmd.load_ref_clip_feats(p)
    with pytest.raises(SystemExit, match="at least 2 images"):
        sd_script_util.save_clip_feats(p, rows[:1])


def test_abi_refusals_come_before_any_launch():
    lib = _lib.load()
    a0 = dict(x=0x10000, n=65, y=0x20000, m=129, d=36, gamma=0.005, work=0x30000, we=200, out=0x40000, sp=0)

    def refused(status, text, **kw):
        a = dict(a0, **kw)
        rc = lib.adm_rbf_sums(a["x"], a["n"], a["y"], a["m"], a["d"], a["gamma"], a["work"], a["we"], a["out"], None, a["sp"])
        assert rc == status and text in lib.adm_last_error(), (kw, rc, lib.adm_last_error())
    refused(-1, b"null", x=None)
    refused(-1, b"null", y=None)
    refused(-1, b"null", work=None)
    refused(-1, b"null", out=None)
    refused(-1, b"neither 0 nor 1", sp=2)
    refused(-3, b"16-byte", x=0x10004)
    refused(-3, b"8-byte", out=0x40004)
    refused(-1, b"n >= 1", n=0)
    refused(-2, b"multiple of 4", d=34)
    refused(-1, b"work holds 199", we=199)
    refused(-1, b"m == n", sp=1, y=None)
    refused(-1, b"self_pairs needs", sp=1, m=65)
    for g in (0.0, -1.0, float("inf"), float("nan")):
        refused(-1, b"gamma", gamma=g)
    sig = _lib.SIGNATURES["adm_rbf_sums"][1]
    assert sig[-1] is _lib.C.c_int and sig[-2] is _lib.C.c_void_p      # the stream second to last: outside the replay census


# ------------------------------------------------------------------ SDCandidateEvaluator(fitness="cmmd")
class _Model:
    device = torch.device("cpu")

    def get_learned_conditioning(self, prompts):
        return torch.zeros(len(prompts), 1, 4)

    def decode_first_stage(self, z):
        return torch.tanh(z[:, :3])


class _Sampler:
    def sample(self, S, conditioning, batch_size, shape, x_T, sampled_timestep, **kw):
        return x_T * (1.0 + 0.001 * float(np.sum(sampled_timestep))), None


class _Scorer:
    def __init__(self):
        self.calls = 0

    def cosine_and_embeds(self, images, prompts):
        self.calls += 1
        return torch.full((images.shape[0],), 0.25), images.flatten(1)[:, :8].clone() + 0.5

    cosine = None

    @staticmethod
    def score_of(cos):
        return float(100.0 * torch.as_tensor(cos).double().mean())


def _evaluator(ref_rows, **kw):
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    scorer = _Scorer()
    e = SDCandidateEvaluator(_Model(), _Sampler(), prompts=[["a", "b"], ["c", "d"], ["e", "f"]], num_samples=3, fitness="cmmd",
                             ref_clip_feats=ref_rows, clip_scorer=scorer, device="cpu", seed=5,
                             image_out=lambda x, out: out.copy_(((x + 1) / 2).clamp(0, 1)), **kw)
    return e, scorer


def test_sd_evaluator_with_fitness_cmmd(host_sums, monkeypatch, tmp_path):
    from autodiffusion_amd import sd_evaluate
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator, batch_seed, candidate_seed
    lines = []
    monkeypatch.setattr(sd_evaluate.logger, "log", lambda msg: lines.append(msg))
    ref_rows = cmmd_ref.features(6, 8, 1).numpy()
    ref_p = str(tmp_path / "ref.npz")
    with open(ref_p, "wb") as f:
        np.savez(f, clip_feats=ref_rows)
    opt = SimpleNamespace(fixed_code=False, C=4, H=16, W=16, f=2, n_samples=2, scale=1.0, time_step=2, ddim_eta=0.0)
    e, scorer = _evaluator(ref_p)                                   # the .npz is read by the constructor
    note = " [fitness: CMMD x 1e3 (unbiased)]"
    assert e.fitness == "cmmd" and e.fid_note == note and e.features is None and e.ref_stats is None and e.cmmd_ref is None
    cand = [300, 800]
    fid = e.get_cand_fid(cand, opt)
    seed0 = candidate_seed(5, cand)
    assert e.last_plan == [(0, batch_seed(seed0, 0)), (1, batch_seed(seed0, 1))]            # 2, then 4 > 3: the third batch is not drawn
    assert e.last_times["images"] == 4 and e.last_times["batches"] == 2 and scorer.calls == 2
    rows = e.last_rows
    assert rows.shape == (4, 8) and rows.dtype == torch.float32
    want_rows = []
    for itr in range(2):
        x = _Sampler().sample(2, None, 2, None, e.start_code(opt, batch_seed(seed0, itr)), np.array(cand))[0]
        want_rows.append(((torch.tanh(x[:, :3]) + 1) / 2).clamp(0, 1).flatten(1)[:, :8] + 0.5)
    assert torch.equal(rows, torch.cat(want_rows))
    assert fid == cmmd_ref.fitness(rows.numpy(), ref_rows) == e.cmmd_ref.fitness(rows)
    assert lines.count("FID: " + str(fid) + note) == 1 and any(ln.startswith("sample_time: ") and ", fid_time: " in ln for ln in lines)
    assert e.last_clip["score"] == 25.0 and e.last_clip["cosines"].shape == (4,)
    assert e.get_cand_fid(cand, opt) == fid and e.get_cand_fid([100, 900], opt) != fid
    # image-sharded: rank 1 of 2 samples batch 1 alone, with batch 1's seed; the count runs over both
    e2, scorer2 = _evaluator(ref_rows, image_sharded=True)
    assert e2._shard() == (1, 0)                                     # no process group: every batch is this rank's
    e2._shard = lambda: (2, 1)
    e2.get_cand_fid(cand, opt)
    assert e2.last_plan == [(1, batch_seed(seed0, 1))] and scorer2.calls == 1 and torch.equal(e2.last_rows, rows[2:])
    assert e2.last_times["images"] == 4
    # what the fitness needs, said clearly
    kw = dict(prompts=[["a", "b"]], num_samples=3, device="cpu")
    with pytest.raises(ValueError, match="ref_clip_feats"):
        SDCandidateEvaluator(None, None, fitness="cmmd", clip_scorer=_Scorer(), **kw)
    with pytest.raises(ValueError, match="clip_scorer"):
        SDCandidateEvaluator(None, None, fitness="cmmd", ref_clip_feats=ref_rows, **kw)
    with pytest.raises(ValueError, match="'cmmd'"):
        SDCandidateEvaluator(None, None, fitness="mmd", **kw)
    with pytest.raises(KeyError, match="--save_clip_feats"):
        np.savez(str(tmp_path / "stats.npz"), mu=np.zeros(3))
        SDCandidateEvaluator(None, None, fitness="cmmd", clip_scorer=_Scorer(), ref_clip_feats=str(tmp_path / "stats.npz"), **kw)
    # the other fitnesses: nothing of the above exists for them
    e3 = SDCandidateEvaluator(None, None, conditioning=[], ref_mu=np.zeros(4), ref_sigma=np.eye(4), num_samples=4, features=lambda u: u,
                              device="cpu", image_sharded=True)
    assert e3.fitness == "fid" and e3.fid_note == "" and e3.image_sharded is False and e3._shard() == (1, 0) and e3.features is not None


# ------------------------------------------------------------------ the command lines
def test_parsers_take_the_new_flags_and_leave_the_namespace_alone():
    p = _script("sd_search_ea").create_argparser()
    a = p.parse_args([])
    assert a.fitness == "fid" and not hasattr(a, "ref_clip_feats")
    a = p.parse_args(["--fitness", "cmmd", "--ref_clip_feats", "clip.npz", "--clip_ckpt", "clip.pt"])
    assert (a.fitness, a.ref_clip_feats, a.clip_ckpt) == ("cmmd", "clip.npz", "clip.pt")
    with pytest.raises(SystemExit):
        p.parse_args(["--fitness", "mmd"])
    p = _script("sd_clip_score").create_argparser()
    a = p.parse_args(["s.npz"])
    assert not hasattr(a, "ref_clip_feats") and not hasattr(a, "save_clip_feats")
    a = p.parse_args(["s.npz", "--ref_clip_feats", "r.npz", "--save_clip_feats", "o.npz"])
    assert (a.ref_clip_feats, a.save_clip_feats) == ("r.npz", "o.npz")


def test_search_cli_asks_for_what_cmmd_needs(tmp_path):
    cli = _script("sd_search_ea")
    base = ["--fitness", "cmmd", "--outdir", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="--ref_clip_feats"):
        cli.main(base, evaluator=object())
    with pytest.raises(SystemExit, match="--clip_ckpt"):
        cli.main(base + ["--ref_clip_feats", "r.npz"], evaluator=object())
    # with both, no reference statistics and no Inception checkpoint are asked for: an injected evaluator scores the candidate
    ev = SimpleNamespace(get_cand_fid=lambda cand, opt: 1.5, fid_note=" [fitness: CMMD x 1e3 (unbiased)]")
    assert cli.main(base + ["--ref_clip_feats", "r.npz", "--clip_ckpt", "c.pt", "--time_step", "2", "--evaluate", "[3, 9]"], evaluator=ev) == 1.5
    log = open(str(tmp_path / "out" / "log.txt")).read()
    assert "cand: [3, 9], fid: 1.5 [fitness: CMMD x 1e3 (unbiased)]" in log and "ref_clip_feats='r.npz'" in log


def test_clip_score_cli_argument_rules(monkeypatch):
    cli = _script("sd_clip_score")
    with pytest.raises(SystemExit, match="exactly one of --prompt_ids"):
        cli.main(["s.npz", "--synthetic", "tiny"])                                  # as before: prompts are needed for the score
    with pytest.raises(SystemExit, match="exactly one of --prompt_ids"):
        cli.main(["s.npz", "--synthetic", "tiny", "--save_clip_feats", "o.npz", "--prompt_ids", "i.npy", "--captions", "c.txt"])
    monkeypatch.setattr(cli, "require_gpu", lambda prog: (_ for _ in ()).throw(SystemExit("reached the device")))
    with pytest.raises(SystemExit, match="reached the device"):                      # no prompts, a feature flag: not refused
        cli.main(["s.npz", "--synthetic", "tiny", "--save_clip_feats", "o.npz"])
    with pytest.raises(SystemExit, match="--clip_ckpt"):
        cli.main(["s.npz", "--save_clip_feats", "o.npz"])
