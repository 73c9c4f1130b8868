"""float64 restatements of UniPC (Zhao et al., NeurIPS 2023) for tests/test_unipc_host.py (CPU), tests/test_hip_unipc.py and
tests/test_hip_sd_unipc.py (GPU): the update in its unexpanded form (rks, R, b, numpy's solve, D1 differences), the whole
predictor-corrector loop, the exact solution for a model value that is a polynomial in lambda, and the operation sequences of
adm_pix_unipc_step and adm_unipc_step with their per-element rounding bounds.  Nothing here imports the code under test; the
schedule, the model value's restatement and the analytic model are tests/adm_dpm_ref.py's.

Bounds, first order in e = 2^-24, built as tests/adm_dpm_ref.py builds adm_pix_dpm_step's (one fp32 operation rounds once,
relative to its result; the kernels compile with fp contract(off); an input's error is carried by the absolute value of its
coefficient):

  m        adm_dpm_ref.step_restate's m and E(m), thresholding included (the pixel kernel calls the same function);
           latent kernel: d = ec - eu, p = cfg d, e = eu + p:  E(e) = e (|d| |cfg| + |p| + |e|);  q = sigma e, r = x - q,
           m = r / alpha:  E(m) = (sigma E(e) + e |q| + e |r|) / alpha + e |m|.
  x_c      t0 = ac xb, t1 = c0 m, x_c = t0 + t1:  E = |c0| E(m) + e (|t0| + |t1| + |x_c|); per further term t = c_i h_i,
           x_c += t:  E += e (|t| + |x_c|).  Without a corrector x_c = x_eval, exactly.
  x_pred   u0 = ap x_c, u1 = p0 m, x_pred = u0 + u1:  E = |ap| E(x_c) + |p0| E(m) + e (|u0| + |u1| + |x_pred|); further terms
           as above.  (m enters twice, through x_c and through u1: the two first-order terms are added in absolute value.)
"""
from __future__ import annotations

import math

import numpy as np
import torch

import adm_dpm_ref as R

E24 = R.E24
F32_MIN = R.F32_MIN
f32c = R.f32c


# ------------------------------------------------------------------ one update, unexpanded
def rhos_of(rks, hh, variant, order):
    """(rhos_p, rhos_c, h_phi_1, B) of the B(h) form: R_i = rks^(i-1), b_i = i! phi_{i+1}(hh) / B."""
    h_phi_1 = math.expm1(hh)
    B = hh if variant == "bh1" else h_phi_1
    assert variant in ("bh1", "bh2")
    rks = np.asarray(rks, dtype=np.float64)
    Rm, b = [], []
    phi, f = h_phi_1 / hh - 1.0, 1.0
    for i in range(1, order + 1):
        Rm.append(rks ** (i - 1))
        b.append(phi * f / B)
        f *= i + 1
        phi = phi / hh - 1.0 / f
    Rm, b = np.stack(Rm), np.array(b)
    rhos_p = [] if order == 1 else ([0.5] if order == 2 else list(np.linalg.solve(Rm[:-1, :-1], b[:-1])))
    rhos_c = [0.5] if order == 1 else list(np.linalg.solve(Rm, b))
    return rhos_p, rhos_c, h_phi_1, B


def ref_update(sc: R.Schedule, x, m_list, t_list, t, order, variant, predict_x0, m_t=None):
    """One update of `order` from t_list[-1] to t on the newest `order` entries of the history (newest LAST, as
    adm_dpm_ref.ref_update takes them).  -> (x_pred, x_corr | None): x_corr with m_t, the model value at (x_pred, t)."""
    s = t_list[-1]
    lam_s = sc.lam(s)
    h = sc.lam(t) - lam_s
    hh = -h if predict_x0 else h
    m0 = m_list[-1]
    rks = [(sc.lam(t_list[-1 - i]) - lam_s) / h for i in range(1, order)] + [1.0]
    D1s = [(m_list[-1 - i] - m0) / rks[i - 1] for i in range(1, order)]
    rhos_p, rhos_c, h_phi_1, B = rhos_of(rks, hh, variant, order)
    if predict_x0:
        base = sc.std(t) / sc.std(s) * x - sc.alpha(t) * h_phi_1 * m0
        scale = sc.alpha(t)
    else:
        base = math.exp(sc.log_mean(t) - sc.log_mean(s)) * x - sc.std(t) * h_phi_1 * m0
        scale = sc.std(t)
    pred = sum((rho * d for rho, d in zip(rhos_p, D1s)), torch.zeros_like(m0))
    x_pred = base - scale * B * pred
    if m_t is None:
        return x_pred, None
    corr = sum((rho * d for rho, d in zip(rhos_c[:-1], D1s)), torch.zeros_like(m0))
    x_corr = base - scale * B * (corr + rhos_c[-1] * (m_t - m0))
    return x_pred, x_corr


def loop_restate(sc: R.Schedule, eps_fn, x, ts, order, variant="bh2", predict_x0=True, corrector=True, thresholding=False,
                 max_val=1.0, lower_order_final=True, denoise_to_zero=False):
    """The whole loop in float64.  eps_fn(x, t): the guided noise prediction at continuous time t.
    -> (final, xs: the x of every evaluation, ms: every model value, xcs: the accepted state at every evaluated time)."""
    steps = len(ts) - 1
    orders = R.orders_of(steps, order, lower_order_final)
    x = x.double()
    xs, ms, xcs, hist, thist = [], [], [], [], []
    x_prev = None
    for j in range(steps + 1):
        if j == steps and not denoise_to_zero:
            break
        eps = eps_fn(x, ts[j])
        xs.append(x)
        if j == steps:      # the arrival point: its data prediction, no corrector
            x, _ = R.model_value(sc, x, eps, ts[j], True, thresholding, max_val)
            ms.append(x)
            break
        m, _ = R.model_value(sc, x, eps, ts[j], predict_x0, thresholding, max_val)
        ms.append(m)
        x_c = x
        if corrector and j >= 1:      # update j - 1 again, now with the value it was waiting for
            _, x_c = ref_update(sc, x_prev, hist, thist, ts[j], orders[j - 1], variant, predict_x0, m_t=m)
        xcs.append(x_c)
        hist, thist = (hist + [m])[-3:], (thist + [ts[j]])[-3:]
        x_prev = x_c
        x, _ = ref_update(sc, x_c, hist, thist, ts[j + 1], orders[j], variant, predict_x0)
    return x, xs, ms, xcs


# ------------------------------------------------------------------ the exact update for m(lambda) a polynomial
_GL_X, _GL_W = np.polynomial.legendre.leggauss(40)


def exact_update(sc: R.Schedule, x, s, t, poly):
    """Data prediction, m = poly(lambda) independent of x:  x_t = sigma_t / sigma_s x + alpha_t int_{lam_s}^{lam_t} e^(lam - lam_t)
    m(lam) dlam, by 40-point Gauss-Legendre quadrature."""
    ls, lt = sc.lam(s), sc.lam(t)
    lam = 0.5 * (lt - ls) * _GL_X + 0.5 * (lt + ls)
    integral = 0.5 * (lt - ls) * float(np.sum(_GL_W * np.exp(lam - lt) * np.polyval(poly, lam)))
    return sc.std(t) / sc.std(s) * x + sc.alpha(t) * integral


# ------------------------------------------------------------------ the kernels' operation sequences
def _states(m, em, x_eval64, xb, hs, corr, pred, defect=None):
    """(x_c, x_pred) and their bounds from m and E(m): the tail both kernels share.  corr = (ac, c0, c1, c2, c3) | None,
    pred = (ap, p0, p1, p2) | None as the fp32 values the kernel is passed; hs = (h1, h2, h3), None where absent."""
    if defect == "swap_hist":
        hs = (hs[1], hs[0], hs[2])
    xc, exc = x_eval64, torch.zeros_like(x_eval64)
    out_c = out_p = bc = bp = None
    if corr is not None:
        ac, c0 = f32c(corr[0]), f32c(corr[1])
        t0, t1 = ac * xb.double(), c0 * m
        xc = t0 + t1
        exc = abs(c0) * em + E24 * (t0.abs() + t1.abs() + xc.abs())
        for ci, hi in zip(corr[2:], hs):
            if hi is not None:
                t = f32c(ci) * hi.double()
                xc = xc + t
                exc = exc + E24 * (t.abs() + xc.abs())
        out_c, bc = xc, exc + F32_MIN
    if pred is not None:
        ap, p0 = f32c(pred[0]), f32c(pred[1])
        base = x_eval64 if defect == "pred_from_eval" else xc
        u0, u1 = ap * base, p0 * m
        xp = u0 + u1
        exp_ = abs(ap) * exc + abs(p0) * em + E24 * (u0.abs() + u1.abs() + xp.abs())
        for pi, hi in zip(pred[2:], hs[:2]):
            if hi is not None:
                t = f32c(pi) * hi.double()
                xp = xp + t
                exp_ = exp_ + E24 * (t.abs() + xp.abs())
        out_p, bp = xp, exp_ + F32_MIN
    return (out_c, out_p), (bc, bp)


def pix_step_restate(x, mo, grad, xb, h1, h2, h3, *, alpha, sigma, corr=None, pred=None, start_x=False, predict_x0=True,
                     thresholding=False, q=R.QUANTILE, max_val=1.0, defect=None):
    """adm_pix_unipc_step on its operands (fp32 tensors) -> ((m, x_corr | None, x_pred | None, s | None), (bounds))."""
    (_, m, s), (_, bm, bs) = R.step_restate(x, mo, grad, None, None, None, alpha=alpha, sigma=sigma, start_x=start_x,
                                            predict_x0=predict_x0, thresholding=thresholding, q=q, max_val=max_val,
                                            want_next=False, defect=defect if defect in ("no_sigma", "variance_half") else None)
    (xc, xp), (bc, bp) = _states(m, bm - F32_MIN, x.double(), xb, (h1, h2, h3), corr, pred, defect)
    return (m, xc, xp, s), (bm, bc, bp, bs)


def sd_step_restate(x, eu, ec, xb, hs, *, cfg, sigma, alpha, corr=None, pred=None, defect=None):
    """adm_unipc_step on its operands -> ((m, x_corr | None, x_pred | None), (bounds)).  hs: up to three tensors, newest first."""
    cfg, sigma, alpha = f32c(cfg), f32c(sigma), f32c(alpha)
    e = ec.double()
    ee = torch.zeros_like(e)
    if eu is not None:
        u = eu.double()
        d = e - u
        p = cfg * d
        e = u + p
        ee = E24 * (abs(cfg) * d.abs() + p.abs() + e.abs())
    x64 = x.double()
    qv = sigma * e
    r = x64 - qv
    m = r / alpha
    em = (sigma * ee + E24 * qv.abs() + E24 * r.abs()) / alpha + E24 * m.abs()
    hs = tuple(hs) + (None,) * (3 - len(hs))
    (xc, xp), (bc, bp) = _states(m, em, x64, xb, hs, corr, pred, defect)
    return (m, xc, xp), (em + F32_MIN, bc, bp)
