"""GPU: the RBF-kernel sums of CMMD (adm_rbf_sums, csrc/adm_cmmd.hip) against the float64 restatement of tests/cmmd_ref.py under its
bound  |S_hip - S_ref| <= pairs 2 gamma (d + c1) 2^-53 + (L + E) 2^-53 sum |kappa|  (L: cmmd.reduction_chain, E: the device expm1's
measured error), in guarded buffers; then cmmd.py, the CLIP score command line's CMMD line and the SD search's CMMD fitness end to end.

This file holds adm_rbf_sums's per-element float64 check: the symbol's stream is its second-to-last argument, so the replay census of
tests/launch_replay.py does not count it.

Measured on the MI355X (profiles/cmmd/test_hip_cmmd.log): the worst error over bound of any shape is 0.0185 (cross 2 x 3, d = 36,
sigma = 10: 6.9e-18 against 3.8e-16), most shapes are at exactly 0; the device expm1's worst error is 0.9913 ulp (sigma = 1), so
E = 2 (tests/cmmd_ref.py).
"""
import functools
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cmmd_ref
import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
POISON = -3.0
TAIL = 8            # poisoned doubles behind the workspace the library asks for
SIGMAS = (1.0, 10.0)

# (n, m, d): a single entry, a d that is no multiple of the 16-feature group or the 64-feature chunk, ragged row / column tiles on
# either side of 64, one full tile at CLIP's width, several tiles
CROSS = [(1, 1, 4), (2, 3, 36), (63, 65, 36), (64, 64, 768), (65, 129, 36), (257, 130, 768)]
SELF = [(n, d) for n in (2, 64, 65, 257) for d in (36, 768)]
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import _lib
    torch.cuda.set_device(0)
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _sets(n, m, d):
    """(x, y) host rows of a cross case, or (x, None) of a self case (m None)."""
    if m is None:
        return cmmd_ref.self_inputs(n, d), None
    return cmmd_ref.cross_inputs(n, m, d)


@functools.lru_cache(maxsize=None)
def _reference(n, m, d, sigma):
    x, y = _sets(n, m, d)
    return cmmd_ref.rbf_sum(x.numpy(), None if y is None else y.numpy(), sigma)


def _launch(lib, x, y, self_pairs, sigma=10.0, g=None, ptrs=None):
    """One adm_rbf_sums call on guarded operands -> (status, out view, work view, Guarded, elems).  ptrs: overrides of the raw
    pointers."""
    g = g or guarded.Guarded(DEV)
    xd = g.inp("x", x.to(DEV), guarded.margin_rows(x.shape[1]))
    yd = None if y is None else g.inp("y", y.to(DEV), guarded.margin_rows(y.shape[1]))
    n, d = x.shape
    m = n if y is None else y.shape[0]
    elems = lib.adm_rbf_work_elems(n, m, int(self_pairs))
    assert elems > 0
    work = g.out("work", (elems + TAIL,), F64, fill=POISON)
    out = g.out("out", (4,), F64, fill=POISON)
    p = dict(x=xd.data_ptr(), y=None if yd is None else yd.data_ptr(), work=work.data_ptr(), out=out.data_ptr())
    p.update(ptrs or {})
    rc = lib.adm_rbf_sums(p["x"], n, p["y"], m, d, cmmd_ref.gamma_of(sigma), p["work"], elems, p["out"],
                          torch.cuda.current_stream().cuda_stream, int(self_pairs))
    torch.cuda.synchronize()
    return rc, out, work, g, elems


def _check_sum(lib, n, m, d, sigma):
    from autodiffusion_amd import _lib, cmmd
    x, y = _sets(n, m, d)
    self_pairs = y is None
    mm = n if self_pairs else m
    ref, ref_abs, pairs = _reference(n, m, d, sigma)
    rc, out, work, g, elems = _launch(lib, x, y, self_pairs, sigma)
    _lib.check(rc, "adm_rbf_sums")
    g.check()                                                   # margins of every operand intact, nothing non-finite
    blocks = cmmd.rbf_blocks(n, mm, self_pairs)
    assert elems == cmmd.work_elems(n, mm, self_pairs) == blocks + n + mm
    assert bool((work[elems:] == POISON).all()), "the workspace was written past adm_rbf_work_elems"
    assert bool((out[1:] == POISON).all()), "out was written beyond out[0]"
    assert bool((work[:elems] != POISON).all()), "a block left its partial, or a row its norm, unwritten"
    # the norms the kernel used: r, then s
    norms = work[blocks:elems].cpu().numpy()
    want = np.array([math.fsum(row * row) for a in (x, x if self_pairs else y) for row in a.double().numpy()])   # exact squares, one rounding
    assert np.all(np.abs(norms - want) <= (cmmd.norm_chain(d) + 1) * cmmd_ref.U * want)
    got = float(out[0].item())
    chain = cmmd.reduction_chain(n, mm, self_pairs)
    tol = cmmd_ref.bound(pairs, ref_abs, d, chain, sigma)
    err = abs(got - ref)
    WORST["ratio"] = max(WORST["ratio"], err / tol)
    print(f"rbf {'self' if self_pairs else 'cross'} n {n} m {mm} d {d} sigma {sigma:g}: S {ref:.17g} err {err:.3g} bound {tol:.3g} "
          f"(err / bound {err / tol:.3g}, L {chain}, E {cmmd_ref.E_ULP}; worst so far {WORST['ratio']:.3g})")
    assert err <= tol, (got, ref, err, tol)
    # a second call on the same inputs: bitwise the same sum, partials and norms
    rc2, out2, work2, g2, _ = _launch(lib, x, y, self_pairs, sigma)
    _lib.check(rc2, "adm_rbf_sums")
    assert torch.equal(out2.view(torch.int64), out.view(torch.int64)) and torch.equal(work2.view(torch.int64), work.view(torch.int64))
    return got, tol


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("n,m,d", CROSS)
def test_cross_sum_within_the_bound(lib, n, m, d, sigma):
    _check_sum(lib, n, m, d, sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("n,d", SELF)
def test_self_sum_within_the_bound(lib, n, d, sigma):
    _check_sum(lib, n, None, d, sigma)


def test_swapped_sets_agree_within_the_bound(lib):
    """S_xy(x, y) against S_xy(y, x): other tiles, other summation order, the same pairs."""
    from autodiffusion_amd import _lib, cmmd
    x, y = _sets(65, 129, 36)
    ref, ref_abs, pairs = _reference(65, 129, 36, 10.0)
    vals = []
    for a, b in ((x, y), (y, x)):
        rc, out, _, g, _ = _launch(lib, a, b, False)
        _lib.check(rc, "adm_rbf_sums")
        g.check()
        vals.append(float(out[0].item()))
    tol = cmmd_ref.bound(pairs, ref_abs, 36, cmmd.reduction_chain(65, 129, False)) + cmmd_ref.bound(pairs, ref_abs, 36, cmmd.reduction_chain(129, 65, False))
    print(f"rbf swapped sets: {vals[0]:.17g} / {vals[1]:.17g}, |diff| {abs(vals[0] - vals[1]):.3g} allowed {tol:.3g}")
    assert abs(vals[0] - vals[1]) <= tol and abs(vals[1] - ref) <= tol


def test_self_sum_of_y_passed_twice_equals_the_null_form(lib):
    """self_pairs with y == x is the same call as with y NULL."""
    from autodiffusion_amd import _lib
    x, _ = _sets(65, None, 36)
    g = guarded.Guarded(DEV)
    rc, out, _, g, _ = _launch(lib, x, None, True, g=g)
    _lib.check(rc, "adm_rbf_sums")
    xd = g.carves[0].view
    rc, out2, _, g2, _ = _launch(lib, x, None, True, ptrs=dict(x=xd.data_ptr(), y=xd.data_ptr()))
    _lib.check(rc, "adm_rbf_sums")
    assert torch.equal(out[:1].view(torch.int64), out2[:1].view(torch.int64))


def test_refusals_leave_out_and_work_untouched(lib):
    x, y = _sets(65, 129, 36)
    need = lib.adm_rbf_work_elems(65, 129, 0)
    assert need == 6 + 65 + 129

    def refused(status, text, self_pairs=False, **kw):
        g = guarded.Guarded(DEV)
        xd = g.inp("x", x.to(DEV), guarded.margin_rows(36))
        yd = g.inp("y", y.to(DEV), guarded.margin_rows(36))
        work, out = g.out("work", (need + 8,), F64), g.out("out", (4,), F64)   # NaN interiors: guarded.untouched() wants them NaN still
        a = dict(x=xd.data_ptr(), n=65, y=yd.data_ptr(), m=129, d=36, gamma=0.005, work=work.data_ptr(), we=need, out=out.data_ptr())
        for k, v in kw.items():
            a[k] = a[k] + v[1] if isinstance(v, tuple) else v
        rc = lib.adm_rbf_sums(a["x"], a["n"], a["y"], a["m"], a["d"], a["gamma"], a["work"], a["we"], a["out"],
                              torch.cuda.current_stream().cuda_stream, int(self_pairs))
        torch.cuda.synchronize()
        assert rc == status and text in lib.adm_last_error(), (kw, rc, lib.adm_last_error())
        guarded.untouched(g)
    refused(-1, b"null", x=None)
    refused(-1, b"null", y=None)
    refused(-1, b"null", work=None)
    refused(-1, b"null", out=None)
    refused(-3, b"16-byte", x=("+", 4))
    refused(-3, b"16-byte", y=("+", 8))
    refused(-3, b"8-byte", work=("+", 4))
    refused(-3, b"8-byte", out=("+", 4))
    refused(-1, b"n >= 1", n=0)
    refused(-1, b"n >= 1", m=0)
    refused(-2, b"multiple of 4", d=0)
    refused(-2, b"multiple of 4", d=2)
    refused(-2, b"multiple of 4", d=34)
    refused(-1, b"work holds 199", we=need - 1)
    refused(-1, b"m == n", self_pairs=True, y=None)             # m = 129 against n = 65
    refused(-1, b"self_pairs needs", self_pairs=True, m=65)     # y is another set
    refused(-1, b"gamma", gamma=0.0)
    refused(-1, b"gamma", gamma=-0.005)
    refused(-1, b"gamma", gamma=float("inf"))
    refused(-1, b"gamma", gamma=float("nan"))
    assert lib.adm_rbf_work_elems(0, 5, 0) == -1 and lib.adm_rbf_work_elems(5, 6, 1) == -1


# ------------------------------------------------------------------ the device expm1, measured
def test_device_expm1_ulp_error(lib):
    """E of the bound.  A 1 x 1 call on x = (1, 0, 0, 0), y = (a, b, 0, 0) has r = 1, s = fl(a^2 + b^2) and G = a exactly, so the
    kernel's argument z = -gamma max(2 - 2 fl(a / sqrt(s)), 0) is reproduced here bit for bit by the same IEEE operations (correctly
    rounded product, square root, division); what is left between out[0] and expm1(z) in 64-bit-mantissa arithmetic is the device
    expm1's own error (plus, if the device's sqrt or division were not correctly rounded, theirs: the figure is an upper bound).
    Angles cover the half circle evenly, and geometrically towards 0 (z from -4 gamma up to -1e-10 gamma)."""
    from autodiffusion_amd import _lib
    if np.finfo(np.longdouble).nmant >= 63:
        def ulp_errors(got, z):
            want = np.expm1(z.astype(np.longdouble))
            ulp = np.spacing(np.abs(want.astype(np.float64))).astype(np.longdouble)
            return (np.abs(got.astype(np.longdouble) - want) / ulp).astype(np.float64)
    else:
        try:
            import mpmath
        except ImportError:
            pytest.skip("no extended precision here: np.longdouble has fewer than 63 mantissa bits and mpmath is not importable")
        mpmath.mp.prec = 100

        def ulp_errors(got, z):
            want = [mpmath.expm1(mpmath.mpf(float(v))) for v in z]
            return np.array([float(abs(mpmath.mpf(float(g)) - w) / mpmath.mpf(float(np.spacing(abs(float(w)))))) for g, w in zip(got, want)])
    theta = np.concatenate([np.linspace(0.0, np.pi, 1201), np.logspace(-5, 0, 400)])
    a32, b32 = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
    cnt = theta.size
    x = torch.zeros(1, 4)
    x[0, 0] = 1.0
    y = torch.zeros(cnt, 4)
    y[:, 0], y[:, 1] = torch.from_numpy(a32), torch.from_numpy(b32)
    xd, yd = x.to(DEV), y.to(DEV)
    elems = lib.adm_rbf_work_elems(1, 1, 0)
    assert elems == 3
    worst_all = 0.0
    for sigma in SIGMAS:
        gamma = cmmd_ref.gamma_of(sigma)
        out = torch.full((cnt,), POISON, dtype=F64, device=DEV)
        work = torch.empty(elems, dtype=F64, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(cnt):
            _lib.check(lib.adm_rbf_sums(xd.data_ptr(), 1, yd.data_ptr() + 16 * i, 1, 4, gamma, work.data_ptr(), elems,
                                        out.data_ptr() + 8 * i, stream, 0), "adm_rbf_sums")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        a, b = a32.astype(np.float64), b32.astype(np.float64)
        s = a * a + b * b
        z = -(gamma * np.maximum(2.0 - 2.0 * (a / np.sqrt(1.0 * s)), 0.0))
        assert z.min() >= -4.0 * gamma * (1 + 1e-6) and z.max() <= 0.0
        live = z < 0.0
        assert np.all(got[~live] == 0.0) and live.sum() > 1500
        ulps = ulp_errors(got[live], z[live])
        k = int(np.argmax(ulps))
        print(f"device expm1, sigma {sigma:g} (z in [{z.min():.4g}, 0]): worst error {ulps.max():.4f} ulp at z = {z[live][k]:.17g}, "
              f"mean {ulps.mean():.4f} ulp over {live.sum()} arguments")
        worst_all = max(worst_all, float(ulps.max()))
    print(f"device expm1: worst over sigma in {SIGMAS}: {worst_all:.4f} ulp; cmmd_ref.MEASURED_E_ULP = {cmmd_ref.MEASURED_E_ULP}, "
          f"E = {cmmd_ref.E_ULP}")
    assert worst_all <= cmmd_ref.MEASURED_E_ULP, "the device expm1 is worse than the recorded measurement: record the new figure"
    assert cmmd_ref.E_ULP == int(np.ceil(cmmd_ref.MEASURED_E_ULP)) + 1


# ------------------------------------------------------------------ cmmd.py on the device
def _mmd2_tolerance(x, y, sigma, unbiased):
    """The three sums' bounds pushed through the estimator, plus the roundings of its own few operations."""
    from autodiffusion_amd import cmmd
    n, m, d = len(x), len(y), x.shape[1]
    (sxx, axx, pxx), (syy, ayy, pyy), (sxy, axy, pxy) = cmmd_ref.rbf_sum(x, None, sigma), cmmd_ref.rbf_sum(y, None, sigma), cmmd_ref.rbf_sum(x, y, sigma)
    dn, dm = (n * (n - 1.0), m * (m - 1.0)) if unbiased else (float(n) * n, float(m) * m)
    t = (cmmd_ref.bound(pxx, axx, d, cmmd.reduction_chain(n, n, True), sigma) / dn + cmmd_ref.bound(pyy, ayy, d, cmmd.reduction_chain(m, m, True), sigma) / dm
         + 2.0 * cmmd_ref.bound(pxy, axy, d, cmmd.reduction_chain(n, m, False), sigma) / (float(n) * m))
    return t + 8 * cmmd_ref.U * (abs(sxx) / dn + abs(syy) / dm + 2.0 * abs(sxy) / (float(n) * m))


def test_cmmd_reference_equals_the_restatement(lib):
    from autodiffusion_amd import cmmd
    from autodiffusion_amd._lib import AdmError
    x, y = _sets(65, 129, 36)
    xn, yn = x.numpy(), y.numpy()
    for sigma in SIGMAS:
        ref = cmmd.CMMDReference(y.to(DEV), sigma=sigma)
        assert ref.s_yy == cmmd.rbf_sums(y.to(DEV), None, sigma)
        for unbiased, got, want in ((False, ref.cmmd(x.to(DEV)), cmmd_ref.cmmd(xn, yn, sigma)),
                                    (True, ref.fitness(x.to(DEV)), cmmd_ref.fitness(xn, yn, sigma))):
            tol = 1000.0 * _mmd2_tolerance(xn, yn, sigma, unbiased)
            print(f"CMMDReference sigma {sigma:g} {'fitness' if unbiased else 'cmmd'} {got:.12g} restatement {want:.12g} "
                  f"|diff| {abs(got - want):.3g} allowed {tol:.3g}")
            assert abs(got - want) <= tol and abs(want) > 1e3 * tol          # the difference of the three means is resolved
    assert cmmd.cmmd(x.to(DEV), y.to(DEV)) == cmmd.CMMDReference(yn, device=DEV).cmmd(x.to(DEV))    # host rows are uploaded; S_yy cached
    assert cmmd.cmmd(x.to(DEV), x.to(DEV)) == pytest.approx(0.0, abs=1e-9)
    with pytest.raises(AdmError, match="no CPU fallback"):
        cmmd.rbf_sums(x)
    zero = x.clone()
    zero[7] = 0.0
    with pytest.raises(ValueError, match="squared norm"):
        cmmd.rbf_sums(zero.to(DEV), y.to(DEV))
    with pytest.raises(ValueError, match="squared norm"):
        cmmd.rbf_sums(zero.to(DEV))


# ------------------------------------------------------------------ scripts/sd_clip_score.py
def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cmmd_cli", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clip_cli_inputs(folder):
    """The sample file and prompt ids of the recorded run (tests/golden/sd_clip_score_tiny.txt) -> the command line's arguments."""
    rs = np.random.RandomState(4)
    samples = os.path.join(str(folder), "samples_5x48x40x3.npz")
    np.savez(samples, rs.randint(0, 256, size=(5, 48, 40, 3)).astype(np.uint8))
    np.save(os.path.join(str(folder), "ids.npy"), rs.randint(0, 500, size=(6, 77)).astype(np.int64))
    return [samples, "--prompt_ids", os.path.join(str(folder), "ids.npy"), "--batch_size", "2", "--synthetic", "tiny"]


def _stable(text):
    return [re.sub(r"time: [0-9.]+ s", "time: T s", ln) for ln in text.splitlines()]


def test_clip_score_cli_saves_embeddings_and_appends_the_cmmd_line(lib, tmp_path, capsys):
    from autodiffusion_amd import cmmd
    args = clip_cli_inputs(tmp_path)
    # without the new flags: what the parent commit printed (captured there with these inputs), the time aside
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sd_clip_score.py")] + args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    recorded = open(os.path.join(ROOT, "tests", "golden", "sd_clip_score_tiny.txt")).read()
    assert _stable(res.stdout) == _stable(recorded)
    plain = _stable(res.stdout)
    # a second sample file as the "real" images: its embeddings, no prompts
    cli = _script("sd_clip_score")
    rs = np.random.RandomState(5)
    real = str(tmp_path / "real.npz")
    np.savez(real, rs.randint(0, 256, size=(7, 48, 40, 3)).astype(np.uint8))
    ref_p, rows_p = str(tmp_path / "ref_feats.npz"), str(tmp_path / "rows.npz")
    assert cli.main([real, "--synthetic", "tiny", "--batch_size", "3", "--save_clip_feats", ref_p]) is None
    out = capsys.readouterr().out
    assert "CLIP score:" not in out and "CMMD" not in out and "the CLIP score is skipped" in out
    ref_rows = cmmd.load_ref_clip_feats(ref_p)
    assert ref_rows.shape == (7, 64) and ref_rows.dtype == np.float32 and os.path.exists(ref_p)
    # the first file against it: the lines of the plain run, then the CMMD line
    value = cli.main(args + ["--ref_clip_feats", ref_p, "--save_clip_feats", rows_p])
    lines = _stable(capsys.readouterr().out)
    assert lines[:len(plain)] == plain and plain[-1].startswith("CLIP score: ")
    assert lines[len(plain)] == f"CMMD: {value}"                                        # right after the CLIP score line
    assert lines[len(plain) + 1].startswith("saved 5 image embeddings") and len(lines) == len(plain) + 2
    rows = cmmd.load_ref_clip_feats(rows_p)
    want = cmmd_ref.cmmd(rows, ref_rows)
    tol = 1000.0 * _mmd2_tolerance(rows, ref_rows, 10.0, False)
    print(f"sd_clip_score.py CMMD {value:.12g} restatement {want:.12g} |diff| {abs(value - want):.3g} allowed {tol:.3g}")
    assert rows.shape == (5, 64) and abs(value - want) <= tol
    with pytest.raises(KeyError, match="--save_clip_feats"):
        cli.main(args + ["--ref_clip_feats", args[0]])


# ------------------------------------------------------------------ scripts/sd_search_ea.py --fitness cmmd
SEARCH = ["--synthetic", "tiny", "--H", "128", "--W", "128", "--n_samples", "2", "--num_sample", "3", "--scale", "7.5", "--population_num", "3",
          "--select_num", "2", "--mutation_num", "1", "--crossover_num", "1", "--max_epochs", "1", "--seed", "7", "--time_step", "2"]
TAG = " [fitness: CMMD x 1e3 (unbiased)]"


def _tiny_clip_checkpoint(path):
    """Both tiny towers in one plain state dict, CLIPModel layout."""
    from autodiffusion_amd.sd_clip import CLIP_TINY_TEXT_PROJ, CLIP_TINY_VISION, CLIPTextTransformer, CLIPVisionTransformer
    vis = CLIPVisionTransformer(**CLIP_TINY_VISION).randomize_(11).state_dict()
    txt = CLIPTextTransformer(**CLIP_TINY_TEXT_PROJ).randomize_(12).state_dict()
    torch.save({k: v.clone() for k, v in dict(vis, **txt).items()}, path)
    return path


def _env(**kw):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", **kw)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "ADM_DIST_BACKEND", "ADM_FORCE_COLLECTIVES"):
        if k not in kw:
            env.pop(k, None)
    return env


def test_search_cli_ranks_by_cmmd_pools_rows_and_builds_no_extractor(lib, tmp_path):
    """One nccl rank with the collectives forced: every candidate's embedding rows go through pooled_rows' all_gather and come back
    unchanged; every logged fitness is CMMDReference.fitness of those rows and the ranking is the restatement's; no Inception
    extractor exists."""
    from autodiffusion_amd import cmmd
    ref_rows = cmmd_ref.features(24, 64, 77).numpy()                 # the tiny tower projects to 64
    ref_p = str(tmp_path / "clip_ref.npz")
    with open(ref_p, "wb") as f:
        np.savez(f, clip_feats=ref_rows)
    np.save(tmp_path / "ids.npy", torch.randint(0, 512, (6, 77), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64))
    flags = SEARCH + ["--fitness", "cmmd", "--ref_clip_feats", ref_p, "--clip_ckpt", _tiny_clip_checkpoint(str(tmp_path / "clip.pt")),
                      "--prompt_ids", str(tmp_path / "ids.npy"), "--outdir", str(tmp_path / "out")]
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "cmmd_search_child.py"), str(tmp_path / "seen.npz")] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT,
                       env=_env(PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_PORT="29643",
                                ADM_FORCE_COLLECTIVES="1", RANK="0", WORLD_SIZE="1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    log = open(str(tmp_path / "out" / "log.txt")).read()
    cands = re.findall(r"^cand: (\[.*?\]), fid: ([-0-9.e+]+)" + re.escape(TAG) + "$", log, flags=re.M)
    tops = re.findall(r"^No\.\d+ (\[.*?\]) fid = ([-0-9.e+]+)" + re.escape(TAG) + "$", log, flags=re.M)
    z = np.load(str(tmp_path / "seen.npz"))
    assert int(z["count"]) == len(cands) >= 3 and tops and bool(z["no_extractor"])
    fitness_lines = re.findall(r"^(?:cand: .*, fid: |No\.\d+ |FID: ).*$", log, flags=re.M)
    assert len(fitness_lines) == 2 * len(cands) + len(tops) and all(ln.endswith(TAG) for ln in fitness_lines)
    assert "Inception" not in log and len(re.findall(r"^CLIP score: ", log, flags=re.M)) == len(cands)
    assert dict(tops) == dict(cands)
    ref = cmmd.CMMDReference(ref_rows, device=DEV)
    restated = {}
    for i, (cand, logged) in enumerate(cands):
        rows, value = z[f"rows{i}"], float(z[f"value{i}"])
        assert rows.shape == (4, 64) and float(logged) == value              # 2, then 4 > 3 images
        assert value == ref.fitness(torch.from_numpy(rows).to(DEV))           # the same kernel on the same rows: bitwise
        restated[cand] = cmmd_ref.fitness(rows, ref_rows)
        tol = 1000.0 * _mmd2_tolerance(rows, ref_rows, 10.0, True)
        print(f"sd_search_ea.py cand {cand}: fitness {value:.12g} restatement {restated[cand]:.12g} allowed {tol:.3g}")
        assert abs(value - restated[cand]) <= tol
        through, backend, device = (str(v) for v in z[f"pool_how{i}"])
        assert (through, backend) == ("True", "nccl") and device.startswith("cuda")          # one rank: RCCL hands the rows back
        assert np.array_equal(z[f"pool_in{i}"], z[f"pool_out{i}"]) and np.array_equal(z[f"pool_out{i}"], rows)
    assert [c for c, _ in tops] == sorted(restated, key=restated.get)        # ranked as the restatement ranks the kept rows
    assert re.search(r"^sample_time: .*, fid_time: ", log, flags=re.M)


def test_search_cli_with_fitness_fid_logs_what_it_logged_before(lib, tmp_path, monkeypatch):
    """--fitness fid (the default, spelled out) leaves log.txt as a run without the flag writes it: the same argument line but for
    the directory, the same values, no tag.  The host Frechet formula sees the leading 64 features (tests/test_hip_sd_search.py says
    why); the device path runs as it is."""
    from autodiffusion_amd.fid import FIDStatistics
    full = FIDStatistics.frechet_distance
    monkeypatch.setattr(FIDStatistics, "frechet_distance", lambda self, other, eps=1e-6: full(
        FIDStatistics(self.mu[:64], self.sigma[:64, :64]), FIDStatistics(other.mu[:64], other.sigma[:64, :64]), eps))
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "ref.npz", mu=rs.randn(2048) * 0.05, sigma=0.25 * np.eye(2048))
    np.save(tmp_path / "ids.npy", torch.randint(0, 512, (6, 77), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64))
    cli = _script("sd_search_ea")
    logs = {}
    for tag, extra in (("plain", []), ("fid", ["--fitness", "fid"])):
        cli.main(SEARCH + ["--allow_random_inception", "--evaluate", "[300, 800]", "--ref_mu", str(tmp_path / "ref.npz"),
                           "--prompt_ids", str(tmp_path / "ids.npy"), "--outdir", str(tmp_path / tag)] + extra)
        lines = [ln.replace(str(tmp_path / tag), "DIR") for ln in open(str(tmp_path / tag / "log.txt")).read().splitlines()]
        logs[tag] = [re.sub(r"(sample_time|fid_time): [-0-9.e]+", r"\1: T", ln) for ln in lines if not ln.startswith("Logging to ")]
    assert logs["plain"] == logs["fid"] and any(ln.startswith("FID: ") for ln in logs["fid"])
    text = "\n".join(logs["fid"])
    assert "CMMD" not in text and "fitness=" not in text and "ref_clip_feats" not in text
