"""CPU checks of the pixel-space DPM-Solver: the float64 restatements (tests/adm_dpm_ref.py) against the reference capture
(tests/golden/adm_dpm.npz, capture_adm_dpm.py), the host half of autodiffusion_amd/dpm_solver.py against the restatements, and
planted defects that the bounds must catch."""
import math

import numpy as np
import pytest
import torch

import adm_dpm_ref as R
from helpers import golden

MODES = {"eps": (False, False), "x0": (True, False), "thr": (True, True)}
EA_INT = [1000, 800, 600, 350, 120, 0]


def _ea_float(sched):
    return [0.2, 0.9 if sched == "cosine" else 1.0, 0.7, 0.45, 0.05, 0.004]


def _case(sched, tag, sc):
    """A fixture key -> (ts, order, predict_x0, thresholding, lower_order_final, denoise_to_zero)."""
    parts = tag.split("_")
    mode, order = parts[-1], int(parts[-2][1:])
    px0, thr = MODES[mode]
    t_T = 1.0 if sched == "linear" else 0.9
    if tag.startswith("ea_int"):
        full = sc.time_steps("time_uniform", t_T, 0.004, 1000)[::-1]
        return [full[i] for i in EA_INT], order, px0, thr, True, True
    if tag.startswith("ea_float"):
        return sorted(_ea_float(sched), reverse=True), order, px0, thr, True, True
    skip = "_".join(parts[:-2])
    return sc.time_steps(skip, t_T, 0.001, 5), order, px0, thr, order < 3, skip != "logSNR"


def _cases(g, sched):
    pre = f"a_{sched}_"
    return [k[len(pre):-len("_final")] for k in g.files if k.startswith(pre) and k.endswith("_final")]


@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_loop_restatement_matches_the_reference_capture(sched):
    """Every evaluation's x, every model value and the final output of all 29 runs per schedule, at 1e-5 (rtol and atol)."""
    g = golden("adm_dpm")
    np.testing.assert_array_equal(g[f"betas_{sched}"], R.named_betas(sched))
    sc = R.Schedule(g[f"betas_{sched}"])
    fn = R.analytic_eps_fn(sc)
    x_T = torch.from_numpy(g["a_x_T"])
    tags = _cases(g, sched)
    assert len(tags) == 29
    worst, both = 0.0, set()
    for tag in tags:
        ts, order, px0, thr, lof, d2z = _case(sched, tag, sc)
        final, xs, ms, ss = R.loop_restate(sc, fn, x_T, ts, order, px0, thr, 1.0, lof, d2z)
        key = f"a_{sched}_{tag}"
        assert len(xs) == g[key + "_xs"].shape[0] == 5 + int(d2z) and len(ms) == g[key + "_ms"].shape[0]
        for got, want in [(final, g[key + "_final"])] + list(zip(xs, g[key + "_xs"])) + list(zip(ms, g[key + "_ms"])):
            np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=1e-5, err_msg=key)
            worst = max(worst, float((got - torch.from_numpy(want).double()).abs().max()))
        if thr:
            q = g[key + "_q"]
            both |= {bool(v) for v in (q > 1.0).ravel()}
            for s, qq in zip(ss, q):   # the restatement's s is max(quantile, 1)
                np.testing.assert_allclose(s.numpy(), np.maximum(qq, 1.0), rtol=1e-5, atol=1e-5)
    assert both == {True, False}, "the thresholded fixtures hold quantiles on both sides of max_val"
    print(f"{sched}: worst |restatement - reference| {worst:.3g}")


def test_tiny_fixtures_hold_what_the_gpu_tests_need():
    g = golden("adm_dpm")
    assert g["t_cand"].max() <= 900 and len(set(g["t_cand"].tolist())) == 5
    for tag in ("o1", "o2", "o2_thr", "o3"):
        assert g[f"t_{tag}_sample"].shape == (2, 3, 64, 64) and g[f"t_{tag}_uint8"].shape == (2, 64, 64, 3)
    assert (g["t_o2_thr_q"] > 1.0).any()
    assert np.abs(g["t_o2_thr_sample"]).max() <= 1.0 + 1e-6     # the final evaluation is a thresholded data prediction


# ------------------------------------------------------------------ the host half of autodiffusion_amd/dpm_solver.py
@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_schedule_time_grids_and_inverse_lambda(sched):
    from autodiffusion_amd import dpm_solver as D
    betas = R.named_betas(sched)
    ns, sc = D.NoiseScheduleVP("discrete", betas=betas), R.Schedule(betas)
    for t in (0.001, 0.0015, 0.2504, 0.5, 0.9, 1.0):
        assert ns.marginal_lambda(t) == pytest.approx(sc.lam(t), rel=1e-12, abs=1e-12)
        assert ns.inverse_lambda(ns.marginal_lambda(t)) == pytest.approx(t, rel=1e-9)
    for lam in (-5.0, -1.0, 0.0, 2.5, 4.0):
        assert ns.inverse_lambda(lam) == pytest.approx(sc.inverse_lam(lam), rel=1e-12)
    for skip in ("time_uniform", "time_quadratic", "logSNR"):
        got = D.get_time_steps(ns, skip, 0.9, 0.001, 7)
        np.testing.assert_allclose(got, sc.time_steps(skip, 0.9, 0.001, 7, dtype=np.float32), rtol=1e-12)
        assert len(got) == 8 and all(a > b for a, b in zip(got, got[1:]))
    with pytest.raises(ValueError):
        D.get_time_steps(ns, "nope", 1.0, 0.001, 4)


def test_time_points_follow_the_reference_forms():
    from autodiffusion_amd import dpm_solver as D
    from autodiffusion_amd.script_util import create_gaussian_diffusion
    base = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule="linear")
    s = D.DPMSolver(base)
    sc = R.Schedule(R.named_betas("linear"))
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    assert s.time_points(5) == sc.time_steps("time_uniform", 1.0, 0.001, 5, dtype=np.float32)
    full = sc.time_steps("time_uniform", 0.9, 0.004, 1000, dtype=np.float32)[::-1]
    assert s.time_points(5, t_start=0.9, t_end=0.004, timesteps=EA_INT) == [f32(full[i]) for i in EA_INT]
    assert s.time_points(5, timesteps=_ea_float("linear")) == [f32(v) for v in sorted(_ea_float("linear"), reverse=True)]
    with pytest.raises(ValueError):
        s.time_points(4, timesteps=EA_INT)
    with pytest.raises(ValueError):
        D.DPMSolver(base, predict_x0=False, thresholding=True)
    with pytest.raises(NotImplementedError):
        s.sample(None, (1, 3, 8, 8), noise=torch.zeros(1, 3, 8, 8), method="singlestep")
    with pytest.raises(NotImplementedError):
        s.sample(None, (1, 3, 8, 8), noise=torch.zeros(1, 3, 8, 8), solver_type="taylor")


def test_candidate_mapping_and_its_errors():
    from autodiffusion_amd import dpm_solver as D
    idx, ts = D.candidate_times([153, 424, 926, 690], 1000, 2)
    assert idx == [926, 690, 424, 153] and ts == [0.927, 0.691, 0.425, 0.154]
    assert D.candidate_times([0, 999], 1000, 1) == ([999, 0], [1.0, 0.001])
    for bad, order in (([5, 5, 9], 1), ([1000, 3], 1), ([-1, 3], 1), ([7], 1), ([7, 9], 2), ([7, 9, 11], 3)):
        with pytest.raises(ValueError):
            D.candidate_times(bad, 1000, order)
    assert D.step_orders(5, 3, False) == [1, 2, 3, 3, 3] == R.orders_of(5, 3, False)
    assert D.step_orders(5, 3, True) == [1, 2, 3, 2, 1] == R.orders_of(5, 3, True)
    assert D.step_orders(4, 2, True) == [1, 2, 2, 1] and D.step_orders(20, 2, True) == [1] + [2] * 19
    assert D.step_orders(3, 1, True) == [1, 1, 1]


@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_coefficient_expansion_matches_the_references_updates(sched):
    """a x + b0 m0 + b1 m1 + b2 m2 with update_coefs' float64 scalars against the unexpanded D1 / D2 form."""
    from autodiffusion_amd import dpm_solver as D
    betas = R.named_betas(sched)
    ns, sc = D.NoiseScheduleVP("discrete", betas=betas), R.Schedule(betas)
    g = torch.Generator().manual_seed(3)
    x, m0, m1, m2 = (torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(4))
    for th in ([0.9, 0.72, 0.51], [0.31, 0.3, 0.12], [0.05, 0.021, 0.004]):
        for t in (th[-1] * 0.6, 0.001):
            for px0 in (True, False):
                for order in (1, 2, 3):
                    a, b = D.update_coefs(ns, th, t, order, px0)
                    assert b[order:] == [0.0] * (3 - order)
                    got = a * x + b[0] * m0 + b[1] * m1 + b[2] * m2
                    want = R.ref_update(sc, x, [m2, m1, m0], th, t, order, px0)
                    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-11)
    with pytest.raises(ValueError):
        D.update_coefs(ns, [0.5], 0.4, 4, True)


@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_order_one_data_prediction_is_ddim_eta_zero(sched):
    """x_t = (sigma_t / sigma_s) x - alpha_t expm1(-h) x0 is DDIM's sqrt(abar_prev) x0 + sqrt(1 - abar_prev) eps: the tables of a
    candidate's order-1 coefficients against SpacedDiffusion's, to 1e-12."""
    import copy
    from autodiffusion_amd import dpm_solver as D
    from autodiffusion_amd.schedule import apply_candidate
    from autodiffusion_amd.script_util import create_gaussian_diffusion
    base = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule=sched)
    ns = D.NoiseScheduleVP("discrete", betas=base.betas)
    cand = [153, 424, 900, 690, 12]
    act = copy.deepcopy(base)
    apply_candidate(act, base, cand)
    idx, ts = D.candidate_times(cand, 1000, 1)
    for j in range(len(idx) - 1):
        i = len(idx) - 1 - j            # the respaced step index of idx[j]
        assert act.timestep_map[i] == idx[j]
        a, b = D.update_coefs(ns, [ts[j]], ts[j + 1], 1, True)
        ac, ap = act.alphas_cumprod[i], act.alphas_cumprod_prev[i]
        # DDIM eta 0 in terms of (x, x0): eps = (x - sqrt(ac) x0) / sqrt(1 - ac)
        dir_ = math.sqrt(1 - ap) / math.sqrt(1 - ac)
        assert a == pytest.approx(dir_, rel=1e-12) and b[0] == pytest.approx(math.sqrt(ap) - dir_ * math.sqrt(ac), rel=1e-12, abs=1e-12)
        assert ns.marginal_alpha(ts[j]) == pytest.approx(math.sqrt(ac), rel=1e-12)
        assert ns.marginal_std(ts[j]) == pytest.approx(math.sqrt(1 - ac), rel=1e-12)


# ------------------------------------------------------------------ the quantile restatement
@pytest.mark.parametrize("per", [3, 12, 192, 201, 12288])
def test_quantile_restatement_matches_torch_quantile(per):
    g = torch.Generator().manual_seed(per)
    v = torch.randn(3, per, generator=g)
    v[1] = v[1].clamp(-1, 1)
    for q in (0.995, 0.5, 0.25):
        ref, bound, lo, hi = R.quantile_restate(v, q)
        want = torch.quantile(v.abs(), q, dim=1)
        assert ((want.double() - ref).abs() <= bound + 2.0 ** -149).all(), (per, q)
        assert (lo <= ref).all() and (ref <= hi).all()
    ref, bound, _, _ = R.quantile_restate(torch.full((2, per), -0.75), 0.995)
    assert (ref == 0.75).all() and (bound == 0).all()


def _emulate_step(x, mo, grad, xb, h1, h2, *, alpha, sigma, a, b0, b1, b2, thresholding, max_val=1.0, **defects):
    """The kernel's arithmetic in numpy fp32 (one rounding per operation), with the planted defects of the real thing."""
    f = np.float32
    c = x.shape[1]
    xv, out = x.numpy(), (mo[:, c:2 * c] if defects.get("variance_half") else mo[:, :c]).numpy()
    eps = out - (f(1.0) if defects.get("no_sigma") else f(sigma)) * grad.numpy()
    m = (xv - f(sigma) * eps) / f(alpha)
    s = None
    if thresholding:
        n, per = m.shape[0], m[0].size
        srt = np.sort(np.abs(m).reshape(n, -1), axis=1)
        pos = f(0.995) * f(per - 1)
        lo_i, hi_i = (min(per - 1, int(r) + defects.get("rank_shift", 0)) for r in (np.floor(pos), np.ceil(pos)))
        w = f(0.0) if defects.get("drop_weight") else f(pos - np.floor(pos))
        lo, hi = srt[:, lo_i], srt[:, hi_i]
        qv = np.where(w < 0.5, lo + w * (hi - lo), hi - (hi - lo) * (f(1.0) - w)).astype(f)
        s = qv if defects.get("no_floor") else np.maximum(qv, f(max_val))
        sv = s.reshape(n, 1, 1, 1)
        m = np.minimum(np.maximum(m, -sv), sv) / sv
    if defects.get("swap_hist"):
        h1, h2 = h2, h1
    xn = f(a) * xb.numpy() + f(b0) * m
    xn = xn + f(b1) * h1.numpy()
    xn = xn + f(b2) * h2.numpy()
    return torch.from_numpy(xn), torch.from_numpy(m), None if s is None else torch.from_numpy(s)


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


def test_step_restatement_holds_the_emulated_kernel_and_catches_planted_defects():
    from autodiffusion_amd import dpm_solver as D
    ns = D.NoiseScheduleVP("discrete", betas=R.named_betas("cosine"))
    th, t = [0.9, 0.72, 0.51], 0.3
    a, b = D.update_coefs(ns, th, t, 3, True)
    g = torch.Generator().manual_seed(9)
    x, grad, h1, h2 = (torch.randn(3, 3, 8, 8, generator=g) for _ in range(4))
    mo = torch.randn(3, 6, 8, 8, generator=g)
    x[0] *= 0.3          # image 0: |x0| stays below max_val = 2.5; the others exceed it
    mo[0] *= 0.3
    grad *= 0.2
    kw = dict(alpha=ns.marginal_alpha(th[-1]), sigma=ns.marginal_std(th[-1]), a=a, b0=b[0], b1=b[1], b2=b[2])
    for thr in (False, True):
        (rx, rm, rs), (bx, bm, bs) = R.step_restate(x, mo, grad, x, h1, h2, thresholding=thr, max_val=2.5, **kw)
        ex, em, es = _emulate_step(x, mo, grad, x, h1, h2, thresholding=thr, max_val=2.5, **kw)
        assert _ratio(ex, rx, bx) <= 1.0 and _ratio(em, rm, bm) <= 1.0
        if thr:
            assert _ratio(es, rs, bs) <= 1.0
            assert rs[0] == 2.5 and (rs[1:] > 2.5).all()       # both sides of max_val in one batch
        defects = ["swap_hist", "no_sigma", "variance_half"] + (["no_floor", "rank_shift", "drop_weight"] if thr else [])
        for name in defects:
            for shift in ((1, -1) if name == "rank_shift" else (True,)):
                ex, em, es = _emulate_step(x, mo, grad, x, h1, h2, thresholding=thr, max_val=2.5, **kw, **{name: shift})
                r = max(_ratio(ex, rx, bx), _ratio(em, rm, bm), _ratio(es, rs, bs) if thr else 0.0)
                assert r > 1.0, (thr, name, shift, r)
    # the same defects planted in the restatement leave the honest emulation outside its bounds
    ex, em, es = _emulate_step(x, mo, grad, x, h1, h2, thresholding=True, max_val=2.5, **kw)
    for name in ("swap_hist", "no_sigma", "variance_half", "no_floor"):
        (rx, rm, rs), (bx, bm, bs) = R.step_restate(x, mo, grad, x, h1, h2, thresholding=True, max_val=2.5, defect=name, **kw)
        assert max(_ratio(ex, rx, bx), _ratio(em, rm, bm), _ratio(es, rs, bs)) > 1.0, name
    v = torch.randn(2, 192, generator=g)      # rank 190.045: an interior weight (at per = 201 the fp32 rank is the integer 199)
    ref, bound, _, _ = R.quantile_restate(v, 0.995)
    for kwq in (dict(rank_shift=1), dict(rank_shift=-1), dict(drop_weight=True)):
        bad = R.quantile_restate(v, 0.995, **kwq)[0]
        assert ((bad - ref).abs() > bound).any(), kwq


def test_evaluator_and_cli_defaults_are_todays_behaviour():
    import inspect
    from autodiffusion_amd.evaluate import CandidateEvaluator
    p = inspect.signature(CandidateEvaluator.__init__).parameters
    assert p["sampler"].default is None and p["dpm_order"].default == 2
    assert p["dpm_predict_x0"].default is True and p["dpm_thresholding"].default is False
    with pytest.raises(ValueError):
        CandidateEvaluator(None, None, image_size=64, sampler="nope", device="cpu")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks run before any pointer is read: host placeholders stand in for the device buffers."""
    import ctypes as C
    from autodiffusion_amd import _lib
    lib = _lib.load()
    n, c, h, w = 2, 4, 64, 64
    need = lib.adm_abs_quantile_work_bytes(n, c * h * w)
    assert need == 16 + 4 * n * c * h * w and lib.adm_abs_quantile_work_bytes(3, 12288) == 16
    assert lib.adm_abs_quantile_work_bytes(0, 5) == -1 and lib.adm_abs_quantile_work_bytes(1 << 31, 1 << 31) == -1

    def args(**over):
        a = _lib.PixDpmArgs()
        for k in ("x_eval", "model_out", "grad", "x_base", "h1", "h2", "m_out", "x_next", "u8_nhwc", "s_out", "work"):
            setattr(a, k, 0x1000)
        a.work_bytes, a.n, a.c, a.h, a.w, a.model_channels = need, n, c, h, w, 2 * c
        a.start_x, a.predict_x0, a.thresholding = 0, 1, 1
        a.alpha_s, a.sigma_s, a.a, a.b0, a.q, a.max_val = 0.37, 0.929, 0.81, -0.55, 0.995, 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over, word in ((dict(x_eval=None), b"null"), (dict(model_out=None), b"null"), (dict(m_out=None), b"null"),
                       (dict(x_base=None), b"x_base"), (dict(predict_x0=0), b"predict_x0"), (dict(q=0.0), b"q="), (dict(q=1.0), b"q="),
                       (dict(q=float("nan")), b"q="), (dict(work_bytes=need - 4), b"work holds"), (dict(work=None), b"work buffer"),
                       (dict(max_val=0.0), b"max_val"), (dict(n=0), b"bad shape"), (dict(model_channels=5), b"channels"),
                       (dict(h=1 << 20, w=1 << 20), b"overflow"), (dict(n=1 << 30, h=1 << 15, w=1 << 15), b"overflow")):
        assert lib.adm_pix_dpm_step(C.byref(args(**over)), None, 0) == -1 and word in lib.adm_last_error(), over
    assert lib.adm_pix_dpm_step(None, None, 0) == -1 and lib.adm_pix_dpm_step(C.byref(args()), None, 1) == -1
    ok = dict(v=0x1000, n=n, per=c * h * w, q=0.995, work=0x1000, wb=need, out=0x1000)
    for over in (dict(v=None), dict(work=None), dict(out=None), dict(q=0.0), dict(q=1.0), dict(wb=need - 1), dict(n=0),
                 dict(n=1 << 40, per=1 << 40), dict(work=0x1008)):
        a = {**ok, **over}
        assert lib.adm_abs_quantile(a["v"], a["n"], a["per"], a["q"], a["work"], a["wb"], a["out"], None, 0) != 0, over
        assert lib.adm_last_error()
