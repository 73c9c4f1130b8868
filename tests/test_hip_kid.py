"""GPU: the cubic-kernel sums of the Kernel Inception Distance (adm_poly3_sums, csrc/adm_kid.hip) against the float64 restatement of
tests/kid_ref.py under its bound  |S_hip - S_ref| <= (3 d + 4 + L) 2^-53 sum |k|  (L: kid.reduction_chain), in guarded buffers;
then kid.py, the evaluator's KID line and the search's KID fitness end to end.

This file holds adm_poly3_sums's per-element float64 check: the symbol's stream is its second-to-last argument, so the replay
census of tests/launch_replay.py (symbols whose LAST argument is the stream) does not count it."""
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded
import kid_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
POISON = -3.0
TAIL = 8            # poisoned doubles behind the workspace the library asks for

# (n, m, d): a single entry, a d that is no multiple of the 16-feature group or the 64-feature chunk, ragged row / column tiles on
# either side of 64, one full tile at the full width, several tiles, and the search's shape class (a few hundred rows against 1000)
CROSS = [(1, 1, 4), (2, 3, 36), (63, 65, 36), (64, 64, 2048), (65, 129, 36), (257, 130, 2048), (200, 1000, 2048)]
CROSS_MIXED = [(65, 129, 36), (257, 130, 2048)]
SELF = [(n, d) for n in (2, 64, 65, 257) for d in (36, 2048)]
SELF_MIXED = [(65, 36), (257, 2048)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import _lib
    torch.cuda.set_device(0)
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _sets(n, m, d, mixed):
    """(x, y) host rows of a cross case; y is also the self cases' set when m is None."""
    if m is None:
        x = kid_ref.features(n, d, 100 + n + d, mixed)
        return (kid_ref.oppose(x, x, 1, 0) if mixed else x), None
    x, y = kid_ref.features(n, d, 200 + n + d, mixed), kid_ref.features(m, d, 300 + m + d, mixed)
    return (kid_ref.oppose(x, y) if mixed else x), y


@functools.lru_cache(maxsize=None)
def _reference(n, m, d, mixed):
    x, y = _sets(n, m, d, mixed)
    return kid_ref.poly3_sum(x.numpy(), None if y is None else y.numpy())


def _launch(lib, x, y, self_pairs, g=None, work_elems=None, n=None, m=None, d=None, ptrs=None):
    """One adm_poly3_sums call on guarded operands -> (status, out view, work view, Guarded, elems).  ptrs: overrides of the raw
    pointers (refusal cases)."""
    g = g or guarded.Guarded(DEV)
    xd = g.inp("x", x.to(DEV), guarded.margin_rows(x.shape[1]))
    yd = None if y is None else g.inp("y", y.to(DEV), guarded.margin_rows(y.shape[1]))
    n = x.shape[0] if n is None else n
    m = (x.shape[0] if y is None else y.shape[0]) if m is None else m
    d = x.shape[1] if d is None else d
    elems = lib.adm_poly3_work_elems(x.shape[0], x.shape[0] if y is None else y.shape[0], int(self_pairs))
    assert elems > 0
    work = g.out("work", (elems + TAIL,), F64, fill=POISON)
    out = g.out("out", (4,), F64, fill=POISON)
    p = dict(x=xd.data_ptr(), y=None if yd is None else yd.data_ptr(), work=work.data_ptr(), out=out.data_ptr())
    p.update(ptrs or {})
    rc = lib.adm_poly3_sums(p["x"], n, p["y"], m, d, p["work"], elems if work_elems is None else work_elems, p["out"],
                            torch.cuda.current_stream().cuda_stream, int(self_pairs))
    torch.cuda.synchronize()
    return rc, out, work, g, elems


def _check_sum(lib, n, m, d, mixed):
    from autodiffusion_amd import _lib, kid
    x, y = _sets(n, m, d, mixed)
    self_pairs = y is None
    ref, ref_abs = _reference(n, m, d, mixed)
    rc, out, work, g, elems = _launch(lib, x, y, self_pairs)
    _lib.check(rc, "adm_poly3_sums")
    g.check()                                                   # margins of every operand intact, nothing non-finite
    assert elems == kid.poly3_blocks(n, n if self_pairs else m, self_pairs)
    assert bool((work[elems:] == POISON).all()), "the workspace was written past adm_poly3_work_elems"
    assert bool((out[1:] == POISON).all()), "out was written beyond out[0]"
    assert bool((work[:elems] != POISON).all()), "a block left its partial unwritten"
    got = float(out[0].item())
    chain = kid.reduction_chain(n, n if self_pairs else m, self_pairs)
    tol = kid_ref.bound(ref_abs, d, chain)
    err = abs(got - ref)
    print(f"poly3 {'self' if self_pairs else 'cross'} n {n} m {m} d {d}{' mixed' if mixed else ''}: S {ref:.17g} err {err:.3g} bound {tol:.3g} "
          f"(err / bound {err / tol:.3g}, L {chain}, sum|k| - S {ref_abs - ref:.3g})")
    assert err <= tol, (got, ref, err, tol)
    if mixed:
        assert ref_abs > ref + 0.1                              # some k < 0: the bound is in sum |k|, not in S
    # a second call on the same inputs: bitwise the same sum and the same partials
    rc2, out2, work2, g2, _ = _launch(lib, x, y, self_pairs)
    _lib.check(rc2, "adm_poly3_sums")
    assert torch.equal(out2.view(torch.int64), out.view(torch.int64)) and torch.equal(work2.view(torch.int64), work.view(torch.int64))
    return got


@pytest.mark.parametrize("n,m,d", CROSS)
def test_cross_sum_within_the_bound(lib, n, m, d):
    _check_sum(lib, n, m, d, False)


@pytest.mark.parametrize("n,d", SELF)
def test_self_sum_within_the_bound(lib, n, d):
    _check_sum(lib, n, None, d, False)


@pytest.mark.parametrize("n,m,d", CROSS_MIXED + [(n, None, d) for n, d in SELF_MIXED])
def test_mixed_sign_rows_within_the_bound(lib, n, m, d):
    _check_sum(lib, n, m, d, True)


def test_self_sum_of_y_passed_twice_equals_the_null_form(lib):
    """self_pairs with y == x is the same call as with y NULL."""
    from autodiffusion_amd import _lib
    x, _ = _sets(65, None, 36, False)
    g = guarded.Guarded(DEV)
    rc, out, _, g, _ = _launch(lib, x, None, True, g=g)
    _lib.check(rc, "adm_poly3_sums")
    xd = g.carves[0].view
    rc, out2, _, g2, _ = _launch(lib, x, None, True, ptrs=dict(x=xd.data_ptr(), y=xd.data_ptr()))
    _lib.check(rc, "adm_poly3_sums")
    assert torch.equal(out[:1].view(torch.int64), out2[:1].view(torch.int64))


def test_refusals_leave_out_and_work_untouched(lib):
    x, y = _sets(65, 129, 36, False)

    def refused(status, text, self_pairs=False, **kw):
        g = guarded.Guarded(DEV)
        xd = g.inp("x", x.to(DEV), guarded.margin_rows(36))
        yd = g.inp("y", y.to(DEV), guarded.margin_rows(36))
        work, out = g.out("work", (16,), F64), g.out("out", (4,), F64)      # NaN interiors: guarded.untouched() wants them NaN still
        a = dict(x=xd.data_ptr(), n=65, y=yd.data_ptr(), m=129, d=36, work=work.data_ptr(), we=6, out=out.data_ptr())
        for k, v in kw.items():
            a[k] = a[k] + v[1] if isinstance(v, tuple) else v
        rc = lib.adm_poly3_sums(a["x"], a["n"], a["y"], a["m"], a["d"], a["work"], a["we"], a["out"],
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
    refused(-1, b"work holds 5", we=5)
    refused(-1, b"m == n", self_pairs=True, y=None)             # m = 129 against n = 65
    refused(-1, b"self_pairs needs", self_pairs=True, m=65)     # y is another set


# ------------------------------------------------------------------ kid.py on the device
def _mmd2_tolerance(x, y):
    """What the three sums' bounds allow MMD^2_u to move, plus 8 roundings of the O(1) terms of the estimator's own arithmetic."""
    from autodiffusion_amd import kid
    n, m, d = len(x), len(y), x.shape[1]
    (sxx, axx), (syy, ayy), (sxy, axy) = kid_ref.poly3_sum(x), kid_ref.poly3_sum(y), kid_ref.poly3_sum(x, y)
    t = (kid_ref.bound(axx, d, kid.reduction_chain(n, n, True)) / (n * (n - 1.0)) + kid_ref.bound(ayy, d, kid.reduction_chain(m, m, True)) / (m * (m - 1.0))
         + 2.0 * kid_ref.bound(axy, d, kid.reduction_chain(n, m, False)) / (float(n) * m))
    return t + 8 * kid_ref.U * (abs(sxx) / (n * (n - 1.0)) + abs(syy) / (m * (m - 1.0)) + 2.0 * abs(sxy) / (float(n) * m))


def test_kid_reference_fitness_equals_the_restatement(lib):
    from autodiffusion_amd import kid
    x, y = kid_ref.features(64, 2048, 41), kid_ref.features(300, 2048, 42) * 1.02
    ref = kid.KIDReference(y.to(DEV))
    assert ref.s_yy == kid.poly3_sums(y.to(DEV)) and abs(ref.s_yy - kid_ref.poly3_sum(y.numpy())[0]) <= kid_ref.bound(
        kid_ref.poly3_sum(y.numpy())[1], 2048, kid.reduction_chain(300, 300, True))
    want = kid_ref.mmd2_unbiased(x.numpy(), y.numpy())
    tol = _mmd2_tolerance(x.numpy(), y.numpy())
    got = ref.fitness(x.to(DEV))
    print(f"KIDReference.fitness {got:.12g} restatement {1000 * want:.12g} |diff| {abs(got - 1000 * want):.3g} allowed {1000 * tol:.3g}")
    assert abs(got - 1000.0 * want) <= 1000.0 * tol and tol < 1e-9
    assert got == 1000.0 * kid.mmd2_unbiased(x.to(DEV), y.to(DEV))              # the cached S_yy is the computed one
    assert kid.KIDReference(y.numpy(), device=DEV).s_yy == ref.s_yy             # host rows are uploaded
    from autodiffusion_amd._lib import AdmError
    with pytest.raises(AdmError):
        ref.fitness(x)                                                          # host rows: no CPU fallback


def test_kid_subsets_equals_the_restatement_on_the_same_draws(lib):
    from autodiffusion_amd import kid
    x, y = kid_ref.features(120, 64, 51), kid_ref.features(90, 64, 52) * 1.05
    mean, std = kid.kid_subsets(x.to(DEV), y.to(DEV), subsets=4, subset_size=50, seed=7)
    rmean, rstd, vals = kid_ref.kid_subsets(x.numpy(), y.numpy(), 4, 50, 7)
    tol = max(_mmd2_tolerance(x.numpy()[ix], y.numpy()[iy]) for ix, iy in kid_ref.subset_draws(120, 90, 4, 50, 7))
    print(f"kid_subsets mean {mean:.12g} / {rmean:.12g} std {std:.12g} / {rstd:.12g} allowed {tol:.3g}")
    assert abs(mean - rmean) <= tol and abs(std - rstd) <= tol       # the mean moves by at most the largest move, the std by their rms
    with pytest.raises(ValueError, match="--kid_subset_size"):
        kid.kid_subsets(x.to(DEV), y.to(DEV), subsets=2, subset_size=100)


# ------------------------------------------------------------------ scripts/evaluator.py --kid
def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _messages(text):
    return [ln.split(" ", 3)[3] for ln in text.splitlines() if ln.count(" ") >= 3]     # "%m/%d %I:%M:%S %p" message


def test_evaluator_cli_appends_the_kid_line(lib, tmp_path, monkeypatch, capsys):
    from autodiffusion_amd import evaluator, kid
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 256, size=(40, 64, 64, 3), dtype=np.uint8)
    smp = np.clip(ref.astype(np.int16) + rng.integers(-60, 61, size=ref.shape), 0, 255).astype(np.uint8)
    paths = {}
    for tag in ("plain", "kid"):
        os.makedirs(tmp_path / tag)
        paths[tag] = (str(tmp_path / tag / "ref.npz"), str(tmp_path / tag / "samples.npz"))
        np.savez(paths[tag][0], ref)
        np.savez(paths[tag][1], smp)
    seen = {}
    kid0 = evaluator.Evaluator.compute_kid

    def spy(self, activations_ref, activations_sample, subsets, subset_size, seed):
        seen["args"] = (np.array(activations_ref), np.array(activations_sample), subsets, subset_size, seed)
        seen["value"] = kid0(self, activations_ref, activations_sample, subsets, subset_size, seed)
        return seen["value"]
    monkeypatch.setattr(evaluator.Evaluator, "compute_kid", spy)
    cli = _script("evaluator")
    feats_p = str(tmp_path / "ref_feats.npz")
    cli.main([*paths["plain"], "--inception_random", "True", "--batch_size", "40"])
    plain = _messages(capsys.readouterr().out)
    assert "args" not in seen
    cli.main([*paths["kid"], "--inception_random", "True", "--batch_size", "40", "--kid", "True", "--kid_subsets", "3",
              "--kid_subset_size", "16", "--save_ref_feats", feats_p])
    with_kid = _messages(capsys.readouterr().out)
    names = ("Inception Score: ", "FID: ", "sFID: ", "Precision:", "Recall:")
    old = [ln for ln in plain if ln.startswith(names)]
    assert len(old) == 5 and [ln for ln in with_kid if ln.startswith(names)] == old          # the five lines, unchanged
    assert not [ln for ln in plain if ln.startswith("KID")]
    line = [ln for ln in with_kid if ln.startswith("KID: ")]
    assert len(line) == 1 and with_kid.index(line[0]) == with_kid.index(old[-1]) + 1        # one line, right after Recall
    assert line[0].endswith(cli.RANDOM_TAG)
    mean, std = (float(v) for v in line[0][len("KID: "):-len(cli.RANDOM_TAG)].split(" +- "))
    assert (mean, std) == seen["value"]
    ra, sa, subsets, size, seed = seen["args"]
    assert (subsets, size, seed) == (3, 16, 0) and ra.shape == (40, 2048) and sa.shape == (40, 2048)
    assert (mean, std) == kid.kid_subsets(torch.from_numpy(sa).to(DEV), torch.from_numpy(ra).to(DEV), 3, 16, 0)   # sample set first
    rmean, rstd, _ = kid_ref.kid_subsets(sa, ra, 3, 16, 0)
    tol = max(_mmd2_tolerance(sa[ix], ra[iy]) for ix, iy in kid_ref.subset_draws(40, 40, 3, 16, 0))
    assert abs(mean - rmean) <= tol and abs(std - rstd) <= tol
    # the log file next to the sample batch: the plain run's has no sixth line
    log_plain = _messages(open(str(tmp_path / "plain" / "samples_eval.log")).read())
    log_kid = _messages(open(str(tmp_path / "kid" / "samples_eval.log")).read())
    assert [ln for ln in log_plain if not ln.endswith("samples.npz")] == [ln for ln in log_kid if not ln.endswith("samples.npz")][:-1]
    assert log_kid[-1] == line[0]
    # --save_ref_feats: the reference's pool3 rows, as the searchers read them
    feats = kid.load_ref_feats(feats_p)
    assert feats.dtype == np.float32 and np.array_equal(feats, ra)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--kid_subset_size"):      # a set smaller than the subset size is an error that names the flag
        evaluator.Evaluator(None).compute_kid(ra, sa, 3, 41, 0)


# ------------------------------------------------------------------ scripts/search_ea.py --fitness kid
FLAGS = ("--image_size 32 --num_channels 32 --num_res_blocks 1 --channel_mult 1,2,2 --attention_resolutions 16,8 "
         "--num_head_channels 32 --class_cond True --learn_sigma True --resblock_updown True --noise_schedule cosine "
         "--use_scale_shift_norm True --use_fp16 True --use_ddim True --classifier_width 64 --classifier_depth 1 "
         "--batch_size 4 --num_samples 8 --time_step 3 --max_epochs 1 --population_num 3 --select_num 2 "
         "--mutation_num 1 --crossover_num 1 --m_prob 0.25 --use_ddim_init_x True --seed 3 --without_classifier True "
         "--features tests.feat_stub:factory").split()      # the tiny synthetic model of tests/test_hip_rccl.py


def _env(**kw):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", **kw)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "ADM_DIST_BACKEND", "ADM_FORCE_COLLECTIVES"):
        if k not in kw:
            env.pop(k, None)
    return env


def _search(tmp_path, tag, extra, child=False, **env):
    save = str(tmp_path / tag)
    prog = [os.path.join(ROOT, "tests", "kid_search_child.py"), str(tmp_path / (tag + ".npz"))] if child else [os.path.join(ROOT, "scripts", "search_ea.py")]
    cmd = ["timeout", "-k", "10", "600", sys.executable] + prog + FLAGS + ["--save_dir", save] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=700, cwd=ROOT,
                       env=_env(PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_PORT="29641", **env))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return open(os.path.join(save, "log.txt")).read()


def test_search_cli_ranks_by_kid_and_pools_rows_through_rccl(lib, tmp_path):
    """One nccl rank with the collectives forced (as tests/test_hip_rccl.py does): the image-sharded mode gathers every candidate's
    rows through RCCL and gets them back unchanged; every logged fitness is KIDReference.fitness of those rows."""
    from autodiffusion_amd import kid
    feats = (torch.randn(40, 24, generator=torch.Generator().manual_seed(9)) * 40.0).numpy()   # the stub's features are of this size
    feats_p = str(tmp_path / "feats.npz")
    np.savez(feats_p, feats=feats)
    log = _search(tmp_path, "kid", ["--fitness", "kid", "--ref_feats", feats_p], child=True, ADM_FORCE_COLLECTIVES="1")
    cands = re.findall(r"^cand: (\[.*?\]), fid: ([-0-9.e+]+) \[fitness: KID x 1e3\]$", log, flags=re.M)
    tops = re.findall(r"^No\.\d+ (\[.*?\]) fid = ([-0-9.e+]+) \[fitness: KID x 1e3\]$", log, flags=re.M)
    z = np.load(str(tmp_path / "kid.npz"))
    count = int(z["count"])
    assert count == len(cands) >= 2 and tops
    fitness_lines = re.findall(r"^(?:cand: .*, fid: |No\.\d+ ).*$", log, flags=re.M)
    assert len(fitness_lines) == len(cands) + len(tops) and all(ln.endswith(" [fitness: KID x 1e3]") for ln in fitness_lines)
    assert dict(tops) == {c: v for c, v in cands if c in dict(tops)}
    assert [float(v) for _, v in tops] == sorted(float(v) for _, v in tops)                  # ranked by the KID fitness
    ref = kid.KIDReference(feats, device=DEV)
    for i, (_, logged) in enumerate(cands):
        rows, value = z[f"rows{i}"], float(z[f"value{i}"])
        assert rows.shape == (8, 24) and float(logged) == value
        assert value == ref.fitness(torch.from_numpy(rows).to(DEV))                           # the same kernel on the same rows: bitwise
        want = 1000.0 * kid_ref.mmd2_unbiased(rows, feats)
        assert value == pytest.approx(want, rel=1e-9), (value, want)
        through, backend, device = (str(v) for v in z[f"pool_how{i}"])
        assert (through, backend) == ("True", "nccl") and device.startswith("cuda")          # one rank: RCCL hands the rows back
        assert np.array_equal(z[f"pool_in{i}"], z[f"pool_out{i}"]) and np.array_equal(z[f"pool_out{i}"], rows)
    assert re.search(r"^reset_time: .*, sample_time: .*, fid_time: ", log, flags=re.M)


def test_search_cli_with_fitness_fid_logs_what_it_logged_before(lib, tmp_path):
    """--fitness fid (the default, spelled out) leaves log.txt as a run without the flag writes it: same argument line but for the
    directory, same candidates, same values, no KID tag."""
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, mu=np.zeros(24), sigma=np.eye(24))
    log0 = _search(tmp_path, "plain", ["--ref_path", ref])
    log1 = _search(tmp_path, "fid", ["--fitness", "fid", "--ref_path", ref])

    def stable(log, tag):
        lines = [ln.replace(str(tmp_path / tag), "DIR") for ln in log.splitlines()]
        return [ln for ln in lines if not re.match(r"^(reset_time: |total searching time|Logging to )", ln)]
    assert stable(log0, "plain") == stable(log1, "fid")
    assert "KID x 1e3" not in log1 and "fitness=" not in log1 and "ref_feats=" not in log1
    assert re.search(r"^No\.1 \[.*\] fid = [-0-9.e+]+$", log1, flags=re.M)
