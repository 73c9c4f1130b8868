"""CPU checks of UniPC: the host half of autodiffusion_amd/unipc.py against the unexpanded float64 algorithm of
tests/unipc_ref.py, its special cases against dpm_solver.update_coefs, polynomial exactness against Gauss-Legendre quadrature,
the loop's properties on the analytic model, the kernel restatements against an fp32 emulation with planted defects, the entry
points' refusals, and the command lines (ADM flags, the SD parser and the SD searcher's candidate space under opt.unipc)."""
import ctypes as C
import importlib.util
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adm_dpm_ref as R
import unipc_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTS = ([0.9, 0.72, 0.51], [0.31, 0.3, 0.12], [0.05, 0.021, 0.004])


def _rel(got, want):
    return float((got - want).abs().max() / (1e-300 + want.abs().max()))


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_coefficient_expansion_matches_the_unexpanded_update(sched):
    """a x + sum p_k m_k and a x + c_0 m_t + sum c_{k+1} m_k with unipc_coefs' float64 scalars against rks / R / b / solve / D1."""
    from autodiffusion_amd import dpm_solver as D, unipc as P
    betas = R.named_betas(sched)
    ns, sc = D.NoiseScheduleVP("discrete", betas=betas), R.Schedule(betas)
    g = torch.Generator().manual_seed(3)
    x, mt, m0, m1, m2 = (torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(5))
    worst = 0.0
    for th in HISTS:
        for t in (th[-1] * 0.6, 0.001):
            for px0 in (True, False):
                for variant in ("bh1", "bh2"):
                    for order in (1, 2, 3):
                        a, p, c = P.unipc_coefs(ns, th, t, order, variant, px0, True)
                        assert p[order:] == [0.0] * (3 - order) and c[order + 1:] == [0.0] * (3 - order)
                        want_p, want_c = U.ref_update(sc, x, [m2, m1, m0], th, t, order, variant, px0, m_t=mt)
                        got_p = a * x + p[0] * m0 + p[1] * m1 + p[2] * m2
                        got_c = a * x + c[0] * mt + c[1] * m0 + c[2] * m1 + c[3] * m2
                        worst = max(worst, _rel(got_p, want_p), _rel(got_c, want_c))
                        assert _rel(got_p, want_p) <= 1e-11 and _rel(got_c, want_c) <= 1e-11, (th, t, px0, variant, order)
                        a2, p2, c2 = P.unipc_coefs(ns, th, t, order, variant, px0, False)
                        assert (a2, p2) == (a, p) and c2 == [0.0] * 4      # the predictor does not depend on the corrector flag
    print(f"{sched}: worst relative |expanded - unexpanded| {worst:.3g}")
    for bad in (dict(order=4), dict(variant="bh3"), dict(t_hist=[0.5], order=2)):
        kw = dict(t_hist=[0.9, 0.7, 0.5], t=0.4, order=2, variant="bh2")
        kw.update(bad)
        with pytest.raises(ValueError):
            P.unipc_coefs(ns, kw["t_hist"], kw["t"], kw["order"], kw["variant"], True, True)


@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_special_cases_are_dpm_solvers_coefficients(sched):
    """Order 2, bh2, corrector off is DPM-Solver++(2M) / DPM-Solver-2 multistep; the order-1 predictor is DDIM in either variant."""
    from autodiffusion_amd import dpm_solver as D, unipc as P
    ns = D.NoiseScheduleVP("discrete", betas=R.named_betas(sched))
    for th in HISTS:
        for t in (th[-1] * 0.6, 0.001):
            for px0 in (True, False):
                a, p, c = P.unipc_coefs(ns, th, t, 2, "bh2", px0, False)
                a2, b2 = D.update_coefs(ns, th, t, 2, px0)
                assert a == pytest.approx(a2, rel=1e-12) and p == pytest.approx(b2, rel=1e-12, abs=1e-300) and c == [0.0] * 4
                for variant in ("bh1", "bh2"):
                    a, p, _ = P.unipc_coefs(ns, th, t, 1, variant, px0, True)
                    a1, b1 = D.update_coefs(ns, th, t, 1, px0)
                    assert a == pytest.approx(a1, rel=1e-12) and p == pytest.approx(b1, rel=1e-12, abs=1e-300)


# (what, order, degrees that are exact, the degree that is not | None)
POLY_CASES = [("corrector", 2, (0, 1, 2), None), ("corrector", 3, (0, 1, 2, 3), None), ("predictor", 3, (0, 1, 2), None),
              ("predictor", 1, (0,), 1), ("predictor", 2, (0,), 1), ("corrector", 1, (0,), 1)]


@pytest.mark.parametrize("variant", ["bh1", "bh2"])
@pytest.mark.parametrize("what,order,exact,inexact", POLY_CASES, ids=[f"{c[0]}{c[1]}" for c in POLY_CASES])
def test_polynomial_exactness(variant, what, order, exact, inexact):
    """m(lambda) a polynomial of degree d, independent of x: the exact update by 40-point Gauss-Legendre quadrature.  The corrector
    of order 2 and 3 is exact for d <= order, the order-3 predictor for d <= 2, every update for d = 0; the fixed 0.5 of the
    order-2 predictor and the order-1 corrector (and the order-1 predictor itself) miss d = 1 by far more than rounding."""
    from autodiffusion_amd import dpm_solver as D, unipc as P
    betas = R.named_betas("linear")
    ns, sc = D.NoiseScheduleVP("discrete", betas=betas), R.Schedule(betas)
    rng = np.random.default_rng(5)
    x = 0.7
    for th, t in (([0.9, 0.72, 0.51], 0.3), ([0.5, 0.41, 0.3], 0.22)):
        for d in exact + (() if inexact is None else (inexact,)):
            poly = rng.standard_normal(d + 1)
            poly[0] = 1.0 if d else poly[0]      # a leading coefficient of size 1: the degree is really d
            m = [float(np.polyval(poly, sc.lam(v))) for v in th[::-1]] + [0.0, 0.0]      # newest first
            mt = float(np.polyval(poly, sc.lam(t)))
            a, p, c = P.unipc_coefs(ns, th, t, order, variant, True, True)
            got = a * x + (p[0] * m[0] + p[1] * m[1] + p[2] * m[2] if what == "predictor"
                           else c[0] * mt + c[1] * m[0] + c[2] * m[1] + c[3] * m[2])
            want = U.exact_update(sc, x, th[-1], t, poly)
            err = abs(got - want) / max(1.0, abs(want))
            if d == inexact:
                assert err > 1e-4, (th, d, err)
            else:
                assert err <= 1e-12, (th, d, err)


# ------------------------------------------------------------------ the loop
def _expanded_loop(plan, ns, eps_fn, x, ts, predict_x0, denoise_to_zero):
    """unipc.plan_evaluations' coefficients applied as UniPC._run applies them, in float64 on the host."""
    hist, x_base, xcs, calls = [], None, [], 0
    x = x.double()
    for j, e in enumerate(plan):
        al, sg = ns.marginal_alpha(ts[j]), ns.marginal_std(ts[j])
        eps = eps_fn(x, ts[j])
        calls += 1
        m = (x - sg * eps) / al if predict_x0 else eps
        h = hist + [None] * 3
        xc = x
        if e["corr"] is not None:
            ac, c, pc = e["corr"]
            xc = ac * x_base + c[0] * m + sum(c[k + 1] * h[k] for k in range(pc))
        ap, p, pp = e["pred"]
        xp = ap * xc + p[0] * m + sum(p[k + 1] * h[k] for k in range(pp - 1))
        xcs.append(xc)
        hist = ([m] + hist)[:3]
        x_base, x = xc, xp
    if denoise_to_zero:
        j = len(plan)
        x = (x - ns.marginal_std(ts[j]) * eps_fn(x, ts[j])) / ns.marginal_alpha(ts[j])
        calls += 1
    return x, xcs, calls


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("variant", ["bh1", "bh2"])
def test_loop_spends_one_model_call_per_update_and_leaves_the_arrival_uncorrected(order, variant):
    from autodiffusion_amd import dpm_solver as D, unipc as P
    betas = R.named_betas("linear")
    ns, sc = D.NoiseScheduleVP("discrete", betas=betas), R.Schedule(betas)
    inner = R.analytic_eps_fn(sc)
    calls = []

    def fn(x, t):
        calls.append(t)
        return inner(x, t)
    x_T = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for K, lof in ((5, True), (6, False), (8, True)):
        ts = sc.time_steps("time_uniform", 1.0, 0.001, K, dtype=np.float32)
        for px0 in (True, False):
            for corrector in (True, False):
                calls.clear()
                final, xs, ms, xcs = U.loop_restate(sc, fn, x_T, ts, order, variant, px0, corrector, lower_order_final=lof)
                assert calls == ts[:K] and len(xs) == len(ms) == len(xcs) == K      # K model calls make K updates
                # the last arrival is the predictor's output from the last accepted state: no corrector touched it
                orders = R.orders_of(K, order, lof)
                want, _ = U.ref_update(sc, xcs[-1], ms[-3:], ts[K - 3:K] if K >= 3 else ts[:K], ts[K], orders[-1], variant, px0)
                assert torch.equal(final, want)
                assert all(torch.equal(a, b) for a, b in zip(xs, xcs)) == (not corrector)
                plan = P.plan_evaluations(ns, ts, order, lof, variant, px0, corrector)
                assert len(plan) == K and plan[0]["corr"] is None and [e["pred"][2] for e in plan] == orders
                assert [e["corr"] is not None for e in plan[1:]] == [corrector] * (K - 1)
                assert [e["corr"][2] for e in plan[1:] if e["corr"]] == (orders[:-1] if corrector else [])
                got, got_xcs, n_calls = _expanded_loop(plan, ns, inner, x_T, ts, px0, False)
                assert n_calls == K
                assert _rel(got, final) <= 1e-9, (K, px0, corrector)
                for a, b in zip(got_xcs, xcs):
                    assert _rel(a, b) <= 1e-9
    # the corrector changes the result, and both stay close to a fine-grid solution of the same ODE
    ts = sc.time_steps("time_uniform", 1.0, 0.001, 8, dtype=np.float32)
    fine, *_ = U.loop_restate(sc, inner, x_T, sc.time_steps("time_uniform", 1.0, 0.001, 400, dtype=np.float32), 3, "bh2", True, True)
    on, *_ = U.loop_restate(sc, inner, x_T, ts, order, variant, True, True)
    off, *_ = U.loop_restate(sc, inner, x_T, ts, order, variant, True, False)
    assert not torch.equal(on, off) and _rel(on, fine) < 0.5 and _rel(off, fine) < 0.5


def test_loop_errors_come_before_any_launch():
    from autodiffusion_amd import unipc as P
    from autodiffusion_amd.script_util import create_gaussian_diffusion
    base = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule="linear")
    s = P.UniPC(base)
    noise = torch.zeros(1, 3, 8, 8)      # a host tensor: reaching a launch would raise AdmError, not what is asserted
    for order, cand in ((3, [100, 500, 900]), (2, [7, 9]), (1, [7]), (2, [5, 5, 9]), (1, [1000, 3])):
        with pytest.raises(ValueError):
            s.sample_candidate(None, (1, 3, 8, 8), noise=noise, indices=cand, order=order)
    with pytest.raises(ZeroDivisionError):
        s.sample(None, (1, 3, 8, 8), noise=noise, steps=3, order=2, timesteps=[0.9, 0.5, 0.5, 0.1])
    with pytest.raises(ZeroDivisionError):
        P.plan_evaluations(s.ns, [0.9, 0.9, 0.5], 1)
    with pytest.raises(ValueError):
        s.sample(None, (1, 3, 8, 8), noise=noise, steps=4, order=2, timesteps=[0.9, 0.5, 0.1])
    with pytest.raises(NotImplementedError):
        s.sample(None, (1, 3, 8, 8), noise=noise, method="singlestep")
    with pytest.raises(ValueError):
        P.UniPC(base, predict_x0=False, thresholding=True)
    with pytest.raises(ValueError):
        P.UniPC(base, variant="vary_coeff")
    assert s.time_points(5) == R.Schedule(R.named_betas("linear")).time_steps("time_uniform", 1.0, 0.001, 5, dtype=np.float32)
    # one schedule, one grid, one order table, one candidate mapping: dpm_solver's own objects
    from autodiffusion_amd import dpm_solver as D
    for name in ("NoiseScheduleVP", "get_time_steps", "step_orders", "candidate_times", "QUANTILE"):
        assert getattr(P, name) is getattr(D, name), name


# ------------------------------------------------------------------ the kernel restatements
def _emulate_states(m, x, xb, hs, corr, pred, swap_hist=False, pred_from_eval=False):
    f = np.float32
    if swap_hist:
        hs = (hs[1], hs[0], hs[2])
    xc = x
    if corr is not None:
        xc = f(corr[0]) * xb + f(corr[1]) * m
        for ci, hi in zip(corr[2:], hs):
            if hi is not None:
                xc = xc + f(ci) * hi
    xp = None
    if pred is not None:
        xp = f(pred[0]) * (x if pred_from_eval else xc) + f(pred[1]) * m
        for pi, hi in zip(pred[2:], hs[:2]):
            if hi is not None:
                xp = xp + f(pi) * hi
    return (xc if corr is not None else None), xp


def _ratio(got, ref, bound):
    return float(((torch.from_numpy(got).double() - ref).abs() / bound).max())


def test_restatements_hold_the_emulated_kernels_and_catch_planted_defects():
    from autodiffusion_amd import dpm_solver as D, unipc as P
    f = np.float32
    ns = D.NoiseScheduleVP("discrete", betas=R.named_betas("cosine"))
    ts = [0.9, 0.72, 0.51, 0.3, 0.12]
    plan = P.plan_evaluations(ns, ts, 3, False)
    e = plan[3]
    assert e["corr"][2] == 3 and e["pred"][2] == 3
    corr, pred = (e["corr"][0], *e["corr"][1]), (e["pred"][0], *e["pred"][1])
    alpha, sigma = ns.marginal_alpha(ts[3]), ns.marginal_std(ts[3])
    g = torch.Generator().manual_seed(9)
    x, xb, grad, h1, h2, h3 = (torch.randn(3, 3, 8, 8, generator=g) for _ in range(6))
    mo = torch.randn(3, 6, 8, 8, generator=g)
    grad *= 0.2
    # pixel kernel, data prediction with guidance
    eps = mo[:, :3].numpy() - f(sigma) * grad.numpy()
    m = (x.numpy() - f(sigma) * eps) / f(alpha)
    hs = (h1.numpy(), h2.numpy(), h3.numpy())
    for c_, p_ in ((corr, pred), (None, pred), (corr, None)):
        (rm, rc, rp, _), (bm, bc, bp, _) = U.pix_step_restate(x, mo, grad, xb, h1, h2, h3, alpha=alpha, sigma=sigma, corr=c_, pred=p_)
        ec, ep = _emulate_states(m, x.numpy(), xb.numpy(), hs, c_, p_)
        assert _ratio(m, rm, bm) <= 1.0
        assert (rc is None) == (c_ is None) and (rp is None) == (p_ is None)
        if c_ is not None:
            assert _ratio(ec, rc, bc) <= 1.0
        if p_ is not None:
            assert _ratio(ep, rp, bp) <= 1.0
    (rm, rc, rp, _), (bm, bc, bp, _) = U.pix_step_restate(x, mo, grad, xb, h1, h2, h3, alpha=alpha, sigma=sigma, corr=corr, pred=pred)
    for defect in ("swap_hist", "pred_from_eval"):
        ec, ep = _emulate_states(m, x.numpy(), xb.numpy(), hs, corr, pred, **{defect: True})
        assert max(_ratio(ec, rc, bc), _ratio(ep, rp, bp)) > 1.0, defect
        (dm, dc, dp, _), (_, dbc, dbp, _) = U.pix_step_restate(x, mo, grad, xb, h1, h2, h3, alpha=alpha, sigma=sigma, corr=corr,
                                                               pred=pred, defect=defect)
        ec, ep = _emulate_states(m, x.numpy(), xb.numpy(), hs, corr, pred)
        assert max(_ratio(ec, dc, dbc), _ratio(ep, dp, dbp)) > 1.0, defect
    # latent kernel
    eu, ec_ = (torch.randn(3, 3, 8, 8, generator=g) for _ in range(2))
    cfg = 7.5
    for guided in (True, False):
        en = eu.numpy() + f(cfg) * (ec_.numpy() - eu.numpy()) if guided else ec_.numpy()
        m = (x.numpy() - f(sigma) * en) / f(alpha)
        (rm, rc, rp), (bm, bc, bp) = U.sd_step_restate(x, eu if guided else None, ec_, xb, (h1, h2, h3), cfg=cfg, sigma=sigma,
                                                       alpha=alpha, corr=corr, pred=pred)
        gc, gp = _emulate_states(m, x.numpy(), xb.numpy(), hs, corr, pred)
        assert max(_ratio(m, rm, bm), _ratio(gc, rc, bc), _ratio(gp, rp, bp)) <= 1.0
        bad = (x.numpy() - f(sigma) * ec_.numpy()) / f(alpha)      # the guidance dropped
        assert (_ratio(bad, rm, bm) > 1.0) == guided


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks run before any pointer is read: host placeholders stand in for the device buffers."""
    from autodiffusion_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.adm_abi_version() == 10      # additions only
    n, c, h, w = 2, 4, 64, 64
    need = lib.adm_abs_quantile_work_bytes(n, c * h * w)

    def args(**over):
        a = _lib.PixUnipcArgs()
        for k in ("x_eval", "model_out", "grad", "x_base", "h1", "h2", "h3", "m_out", "x_corr", "x_pred", "u8_nhwc", "s_out", "work"):
            setattr(a, k, 0x1000)
        a.work_bytes, a.n, a.c, a.h, a.w, a.model_channels = need, n, c, h, w, 2 * c
        a.start_x, a.predict_x0, a.thresholding = 0, 1, 1
        a.alpha_s, a.sigma_s, a.ac, a.c0, a.ap, a.p0, a.q, a.max_val = 0.37, 0.929, 0.81, -0.55, 0.7, 0.2, 0.995, 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over, word in ((dict(x_eval=None), b"null"), (dict(model_out=None), b"null"), (dict(m_out=None), b"null"),
                       (dict(x_base=None), b"x_base"), (dict(predict_x0=0), b"predict_x0"), (dict(q=0.0), b"q="), (dict(q=1.0), b"q="),
                       (dict(q=float("nan")), b"q="), (dict(work_bytes=need - 4), b"work holds"), (dict(work=None), b"work buffer"),
                       (dict(work=0x1008), b"aligned"), (dict(max_val=0.0), b"max_val"), (dict(n=0), b"bad shape"),
                       (dict(model_channels=5), b"channels"), (dict(h=1 << 20, w=1 << 20), b"overflow"),
                       (dict(n=1 << 30, h=1 << 15, w=1 << 15), b"overflow")):
        assert lib.adm_pix_unipc_step(C.byref(args(**over)), None, 0) != 0 and word in lib.adm_last_error(), over
    assert lib.adm_pix_unipc_step(None, None, 0) == -1 and lib.adm_pix_unipc_step(C.byref(args()), None, 1) == -1

    def sd_args(**over):
        a = _lib.UnipcArgs()
        for k in ("x_eval", "eps_uncond", "eps_cond", "x_base", "h1", "h2", "h3", "m_out", "x_corr", "x_pred"):
            setattr(a, k, 0x1000)
        a.numel, a.cfg_scale, a.sigma_s, a.alpha_s = 64, 7.5, 0.929, 0.37
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over, word in ((dict(x_eval=None), b"null"), (dict(eps_cond=None), b"null"), (dict(m_out=None), b"null"),
                       (dict(x_base=None), b"x_base"), (dict(numel=0), b"numel"), (dict(numel=-4), b"numel"), (dict(alpha_s=0.0), b"alpha_s")):
        assert lib.adm_unipc_step(C.byref(sd_args(**over)), None, 0) != 0 and word in lib.adm_last_error(), over
    assert lib.adm_unipc_step(None, None, 0) == -1 and lib.adm_unipc_step(C.byref(sd_args()), None, 1) == -1
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    assert "int adm_pix_unipc_step(" in header and "int adm_unipc_step(" in header


# ------------------------------------------------------------------ command lines
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["search_ea", "classifier_sample", "image_sample"])
def test_adm_flags_parse_are_off_by_default_and_refuse_two_samplers(name):
    from autodiffusion_amd import script_util as S
    parser = _script(name).create_argparser()
    args = parser.parse_args([])
    assert [getattr(args, k) for k in S.UNIPC_FLAGS] == [False, 2, "bh2", True, True, False]
    before = {k: v for k, v in vars(args).items() if k not in S.UNIPC_FLAGS}
    assert S.unipc_kwargs(args) == {} and vars(args) == before      # off: the flags leave no trace in str(args)
    args = parser.parse_args(["--unipc", "True", "--unipc_order", "3", "--unipc_variant", "bh1", "--unipc_corrector", "False",
                              "--unipc_predict_x0", "False", "--unipc_thresholding", "False"])
    kw = S.unipc_kwargs(args)
    assert kw == dict(sampler="unipc", unipc_order=3, unipc_variant="bh1", unipc_corrector=False, unipc_predict_x0=False,
                      unipc_thresholding=False)
    assert S.dpm_kwargs(args) == {} and args.unipc is True and not hasattr(args, "dpm_solver")
    with pytest.raises(SystemExit):
        S.unipc_kwargs(parser.parse_args(["--unipc", "True", "--dpm_solver", "True"]))
    for bad in (["--unipc_order", "4"], ["--unipc_variant", "vary_coeff"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)


def test_evaluator_takes_the_unipc_sampler_and_keeps_its_defaults():
    import inspect
    from autodiffusion_amd.evaluate import CandidateEvaluator
    p = inspect.signature(CandidateEvaluator.__init__).parameters
    assert p["sampler"].default is None
    assert [p[k].default for k in ("unipc_order", "unipc_variant", "unipc_corrector", "unipc_predict_x0", "unipc_thresholding")] == \
        [2, "bh2", True, True, False]
    from autodiffusion_amd.script_util import create_gaussian_diffusion
    base = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule="linear")
    ev = CandidateEvaluator(torch.nn.Identity(), base, image_size=64, sampler="unipc", unipc_order=3, device="cpu")
    assert ev.sampler == "unipc" and ev.unipc_order == 3 and ev.unipc_corrector is True


def test_sd_command_line_and_sampler_builder():
    from autodiffusion_amd import sd_script_util as S
    cli = _script("sd_search_ea")
    parser = cli.create_argparser()
    opt = parser.parse_args([])
    assert not any(k.startswith("unipc") for k in vars(opt)) and S.unipc_options(opt, "t") is None
    opt = parser.parse_args(["--unipc"])
    assert S.unipc_options(opt, "t") == dict(order=2, variant="bh2", corrector=True)
    opt = parser.parse_args(["--unipc", "--unipc_order", "3", "--unipc_variant", "bh1", "--unipc_corrector", "false"])
    assert S.unipc_options(opt, "t") == dict(order=3, variant="bh1", corrector=False)
    for argv in (["--unipc", "--dpm_solver"], ["--unipc", "--plms"], ["--unipc_order", "3"]):
        with pytest.raises(SystemExit):
            S.unipc_options(parser.parse_args(argv), "t")
    model = SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.999, 0.01, 1000))
    s = S.build_sampler(opt, model)
    assert type(s).__name__ == "UniPCSampler" and (s.order, s.variant, s.corrector) == (3, "bh1", False)
    assert type(S.build_sampler(parser.parse_args(["--dpm_solver"]), model)).__name__ == "DPMSolverSampler"
    assert type(S.build_sampler(parser.parse_args([]), model)).__name__ == "DDIMSampler"


@pytest.mark.parametrize("tag", ["dpm_random", "dpm_init"])
def test_sd_searcher_under_unipc_walks_the_captured_dpm_trajectories(tag, monkeypatch):
    """opt.unipc searches DPM-Solver's candidate space with the same operators and draws: under the synthetic fitness of the
    capture, every evaluated candidate and every epoch's top-50 equal the reference driver's --dpm_solver run value for value."""
    from autodiffusion_amd import logger
    from autodiffusion_amd.sd_search import EvolutionSearcher, dpm_search_params, parse_sd_candidate
    from test_sd_search_host import RUNS, _assert_matches_fixture, _Fitness
    monkeypatch.setattr(logger, "log", lambda *a: None)
    opt = SimpleNamespace(max_epochs=3, select_num=4, population_num=10, m_prob=0.25, crossover_num=3, mutation_num=4, max_fid=3.0,
                          num_sample=4, use_ddim_init_x=RUNS[tag][1], dpm_solver=False, unipc=True, seed=0)
    ev = _Fitness()
    with pytest.raises(ValueError):
        EvolutionSearcher(opt, None, 4, np.zeros(4), np.eye(4), SimpleNamespace(ddpm_num_timesteps=1000), {"validation_loader": []}, 2,
                          evaluator=ev)
    s = EvolutionSearcher(opt, None, 4, np.zeros(4), np.eye(4), SimpleNamespace(ddpm_num_timesteps=1000), {"validation_loader": []}, 2,
                          dpm_params=dpm_search_params(range(1000), 4), evaluator=ev)
    tops, inner = [], s.update_top_k

    def update_top_k(candidates, *, k, key, reverse=False):
        inner(candidates, k=k, key=key, reverse=reverse)
        if k == 50:
            tops.append(([parse_sd_candidate(c) for c in s.keep_top_k[50]], [s.vis_dict[c]["fid"] for c in s.keep_top_k[50]]))
    s.update_top_k = update_top_k
    random.seed(0)
    np.random.seed(0)
    s.search()
    _assert_matches_fixture(tag, ev, tops)
    assert all(len(c) == 5 and type(v) is float for c in ev.evaluated for v in c)


def test_sd_command_line_evaluates_one_candidate_of_time_step_plus_one_times(tmp_path, monkeypatch):
    from autodiffusion_amd import logger
    from test_sd_search_host import _Fitness, fitness_of
    monkeypatch.setattr(logger, "log", lambda *a: None)
    cli = _script("sd_search_ea")
    np.savez(tmp_path / "ref.npz", mu=np.zeros(4), sigma=np.eye(4))
    base = ["--ref_mu", str(tmp_path / "ref.npz"), "--outdir", str(tmp_path / "out"), "--time_step", "2", "--unipc"]
    ev = _Fitness()
    cand = [0.25, 0.5, 1.0]
    assert cli.main(base + ["--evaluate", str(cand)], evaluator=ev) == fitness_of(cand) and ev.evaluated == [cand]
    for argv in (base + ["--evaluate", "[100, 500]"], base + ["--dpm_solver", "--evaluate", str(cand)], base[:-1] + ["--unipc_order", "3"]):
        with pytest.raises(SystemExit):
            cli.main(argv, evaluator=_Fitness())
