"""float64 restatements and per-element error bounds of the pixel-space DPM-Solver: the exact quantile (adm_abs_quantile), the
fused step (adm_pix_dpm_step) and the whole multistep loop (autodiffusion_amd/dpm_solver.py), for tests/test_adm_dpm_host.py
(CPU) and tests/test_hip_adm_dpm.py (GPU).  Nothing here imports the code under test: the schedule, the updates (in the
reference's unexpanded D1 / D2 form, dpm_solver.py:504-549, :755-857) and the analytic model are stated again.

Bounds, first order in e = 2^-24, in the style of tests/f32_kernels.py (one fp32 operation rounds once, relative to its
result: the kernels compile with fp contract(off); a cancelling difference carries its operands' errors absolutely).

  quantile   pos = fp32(q) * fp32(per - 1) in fp32, lo = sorted[floor(pos)], hi = sorted[ceil(pos)] EXACTLY (selection, not
             arithmetic), w = pos - floor(pos) (exact: both below 2^24).  torch's lerp: w < 0.5: lo + w (hi - lo), else
             hi - (hi - lo)(1 - w): three roundings, |got - ref| <= e (|hi - lo| + |w (hi - lo)| + |ref|) + e |hi - lo| (the
             1 - w); lo == hi: exact.  The GPU test holds the kernel to 4 fp32 ulps of torch.quantile, which has the same
             three roundings in the other order of contraction.
  step       eps = out, or START_X: p = alpha out, d = x - p, eps = d / sigma:  E = (e |p| + e |d|) / sigma + e |eps|.
             guidance: t = sigma g, eps' = eps - t:  E(eps) + e |t| + e |eps'|.
             predict_x0: p = sigma eps, d = x - p, m = d / alpha:  E(m) = (sigma E(eps) + e |p| + e |d|) / alpha + e |m|.
             thresholding: s = max(quantile_q |m|, max_val).  An order statistic is 1-Lipschitz in the sup norm, so the
             kernel's s (of its own fp32 m) is within E(s) = max_i E(m_i) + (quantile bound) of the float64 one;
             m' = clamp(m, -s, s) / s:  E(m') = (E(m) + E(s) + |clamp| E(s) / s) / s + e |m'|  (the clamp is 1-Lipschitz in
             m and in s; the last term in the bracket is the relative error of s carried by the division).
             x_next = a xb + b0 m + b1 h1 + b2 h2, left to right:  |b0| E(m) + e (|a xb| + |b0 m| + |sum|) + per further
             term e (|b_i h_i| + |sum|).
"""
from __future__ import annotations

import math

import numpy as np
import torch

E24 = 2.0 ** -24
F32_MIN = 2.0 ** -126
QUANTILE = 0.995


def f32c(x: float) -> float:
    return float(np.float32(x))


# ------------------------------------------------------------------ schedule (dpm_solver.py:99-174, float64)
class Schedule:
    def __init__(self, betas):
        self.N = len(betas)
        self.log_alpha = 0.5 * np.cumsum(np.log(1.0 - np.asarray(betas, dtype=np.float64)))
        self.t = np.arange(1, self.N + 1, dtype=np.float64) / self.N

    def _interp(self, x, xp, yp):
        k = int(np.clip(np.searchsorted(xp, x), 1, len(xp) - 1))   # outside the knots: the outermost segment, extended
        return yp[k - 1] + (x - xp[k - 1]) * (yp[k] - yp[k - 1]) / (xp[k] - xp[k - 1])

    def log_mean(self, t):
        return float(self._interp(t, self.t, self.log_alpha))

    def alpha(self, t):
        return math.exp(self.log_mean(t))

    def std(self, t):
        return math.sqrt(1.0 - math.exp(2.0 * self.log_mean(t)))

    def lam(self, t):
        lm = self.log_mean(t)
        return lm - 0.5 * math.log(1.0 - math.exp(2.0 * lm))

    def inverse_lam(self, lam):
        la = -0.5 * float(np.logaddexp(0.0, -2.0 * lam))
        return float(self._interp(la, self.log_alpha[::-1], self.t[::-1]))

    def time_steps(self, skip_type, t_T, t_0, n, dtype=np.float64):
        """get_time_steps (:410-437); dtype: that of the reference's torch.linspace (float32 by default there)."""
        if skip_type == "logSNR":
            lam = np.linspace(dtype(self.lam(t_T)), dtype(self.lam(t_0)), n + 1, dtype=dtype)
            return [self.inverse_lam(float(v)) for v in lam]
        if skip_type == "time_uniform":
            return [float(v) for v in np.linspace(t_T, t_0, n + 1, dtype=dtype)]
        assert skip_type == "time_quadratic"
        return [float(v) for v in np.linspace(t_T ** 0.5, t_0 ** 0.5, n + 1, dtype=dtype) ** dtype(2)]


def named_betas(name):
    if name == "linear":
        return np.linspace(0.0001, 0.02, 1000, dtype=np.float64)
    f = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2   # noqa: E731
    return np.array([min(1 - f((i + 1) / 1000) / f(i / 1000), 0.999) for i in range(1000)])


# ------------------------------------------------------------------ quantile
def quantile_restate(v, q: float, rank_shift: int = 0, drop_weight: bool = False):
    """v [n, per] (any float dtype; |v| is taken exactly) -> (ref float64 [n], bound [n], lo, hi).  rank_shift / drop_weight
    plant the defects the host tests must catch."""
    a = v.detach().abs().double()
    per = a.shape[1]
    pos = np.float32(q) * np.float32(per - 1)
    k_lo, k_hi = int(np.floor(pos)), int(np.ceil(pos))
    w = 0.0 if drop_weight else float(pos - np.floor(pos))
    k_lo, k_hi = min(per - 1, max(0, k_lo + rank_shift)), min(per - 1, max(0, k_hi + rank_shift))
    srt = torch.sort(a, dim=1).values
    lo, hi = srt[:, k_lo], srt[:, k_hi]
    d = hi - lo
    ref = lo + w * d
    bound = E24 * (2 * d.abs() + (w * d).abs() + ref.abs()) + F32_MIN
    return ref, torch.where(d == 0, torch.zeros_like(bound), bound), lo, hi


# ------------------------------------------------------------------ the fused step
def step_restate(x, mo, grad, xb, h1, h2, *, alpha, sigma, a=0.0, b0=0.0, b1=0.0, b2=0.0, start_x=False, predict_x0=True,
                 thresholding=False, q=QUANTILE, max_val=1.0, want_next=True, defect=None):
    """The kernel's operands (fp32 tensors; the scalars as the fp32 values it is passed) -> ((x_next | None, m, s | None),
    (bounds)).  defect in {None, "swap_hist", "no_sigma", "variance_half", "no_floor"} plants one."""
    alpha, sigma, a, b0, b1, b2, max_val = (f32c(v_) for v_ in (alpha, sigma, a, b0, b1, b2, max_val))
    c = x.shape[1]
    x64 = x.double()
    out = (mo[:, c:2 * c] if defect == "variance_half" else mo[:, :c]).double()
    if start_x:
        p = alpha * out
        d = x64 - p
        eps = d / sigma
        ee = (E24 * p.abs() + E24 * d.abs()) / sigma + E24 * eps.abs()
    else:
        eps, ee = out, torch.zeros_like(out)
    if grad is not None:
        t = (1.0 if defect == "no_sigma" else sigma) * grad.double()
        eps = eps - t
        ee = ee + E24 * t.abs() + E24 * eps.abs()
    s = es = None
    if predict_x0:
        p = sigma * eps
        d = x64 - p
        m = d / alpha
        em = (sigma * ee + E24 * p.abs() + E24 * d.abs()) / alpha + E24 * m.abs()
        if thresholding:
            n = m.shape[0]
            qv, qb, _, _ = quantile_restate(m.reshape(n, -1), q)
            s = qv if defect == "no_floor" else qv.clamp_min(max_val)
            es = em.reshape(n, -1).max(1).values + qb
            sv, esv = s.view(n, 1, 1, 1), es.view(n, 1, 1, 1)
            cl = torch.minimum(torch.maximum(m, -sv), sv)
            m2 = cl / sv
            em = (em + esv + cl.abs() * esv / sv) / sv + E24 * m2.abs()
            m = m2
    else:
        m, em = eps, ee
    if not want_next:
        return (None, m, s), (None, em + F32_MIN, es)
    if defect == "swap_hist":
        h1, h2 = h2, h1
    p1, p2 = a * xb.double(), b0 * m
    xn = p1 + p2
    en = abs(b0) * em + E24 * (p1.abs() + p2.abs() + xn.abs())
    for bi, hi in ((b1, h1), (b2, h2)):
        if hi is not None:
            t = bi * hi.double()
            xn = xn + t
            en = en + E24 * t.abs() + E24 * xn.abs()
    return (xn, m, s), (en + F32_MIN, em + F32_MIN, es)


# ------------------------------------------------------------------ the reference's updates, unexpanded (float64 tensors)
def ref_update(sc: Schedule, x, m_list, t_list, t, order, predict_x0):
    """multistep_dpm_solver_update (:885-913) of `order` on the newest `order` entries of the history (newest last)."""
    t0 = t_list[-1]
    lam0, lam_t = sc.lam(t0), sc.lam(t)
    h = lam_t - lam0
    m0 = m_list[-1]
    if predict_x0:
        a, scale, eh = sc.std(t) / sc.std(t0), sc.alpha(t), math.exp(-h)
    else:
        a, scale, eh = math.exp(sc.log_mean(t) - sc.log_mean(t0)), sc.std(t), math.exp(h)
    phi = scale * (eh - 1.0)
    if order == 1:
        return a * x - phi * m0
    r0 = (lam0 - sc.lam(t_list[-2])) / h
    D1_0 = (1.0 / r0) * (m0 - m_list[-2])
    if order == 2:
        return a * x - phi * m0 - 0.5 * phi * D1_0
    r1 = (sc.lam(t_list[-2]) - sc.lam(t_list[-3])) / h
    D1_1 = (1.0 / r1) * (m_list[-2] - m_list[-3])
    D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
    D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
    if predict_x0:
        return a * x - phi * m0 + scale * ((eh - 1.0) / h + 1.0) * D1 - scale * ((eh - 1.0 + h) / h ** 2 - 0.5) * D2
    return a * x - phi * m0 - scale * ((eh - 1.0) / h - 1.0) * D1 - scale * ((eh - 1.0 - h) / h ** 2 - 0.5) * D2


def orders_of(steps, order, lower_order_final):
    return [s_ if s_ < order else (min(order, steps + 1 - s_) if lower_order_final and steps < 15 else order)
            for s_ in range(1, steps + 1)]


def model_value(sc, x, eps, t, predict_x0, thresholding, max_val=1.0):
    if not predict_x0:
        return eps, None
    m = (x - sc.std(t) * eps) / sc.alpha(t)
    if not thresholding:
        return m, None
    s = quantile_restate(m.reshape(m.shape[0], -1), QUANTILE)[0].clamp_min(max_val)
    sv = s.view(-1, 1, 1, 1)
    return torch.minimum(torch.maximum(m, -sv), sv) / sv, s


def loop_restate(sc: Schedule, eps_fn, x, ts, order, predict_x0, thresholding=False, max_val=1.0, lower_order_final=True,
                 denoise_to_zero=False):
    """The whole multistep loop in float64.  eps_fn(x, t) is the guided noise prediction at continuous time t.
    -> (final, xs: the x of every evaluation, ms: every model value, ss: every per-image threshold)."""
    steps = len(ts) - 1
    orders = orders_of(steps, order, lower_order_final)
    x = x.double()
    xs, ms, ss, hist, thist = [], [], [], [], []
    for j in range(steps + 1):
        if j == steps and not denoise_to_zero:
            break
        eps = eps_fn(x, ts[j])
        xs.append(x)
        if j == steps:
            x, s = model_value(sc, x, eps, ts[j], True, thresholding, max_val)
            ms.append(x)
            ss.append(s)
            break
        m, s = model_value(sc, x, eps, ts[j], predict_x0, thresholding, max_val)
        ms.append(m)
        ss.append(s)
        hist, thist = (hist + [m])[-3:], (thist + [ts[j]])[-3:]
        x = ref_update(sc, x, hist, thist, ts[j + 1], orders[j], predict_x0)
    return x, xs, ms, ss


# ------------------------------------------------------------------ the analytic model of the capture
MU = (0.3, -0.2, 0.5)
VAR = (0.25, 0.5, 0.4)
CENTER = (0.6, 0.1, -0.4)
CLF_W = 0.5
GUIDANCE_SCALE = 2.0


def _chan(vals, x):
    return torch.tensor(vals, dtype=x.dtype).view(1, -1, 1, 1)


def gauss_eps(x, alpha, sigma):
    """The exact noise prediction of per-channel Gaussian data N(MU, VAR): eps = sigma (x - alpha mu) / (alpha^2 v + sigma^2)."""
    return sigma * (x - alpha * _chan(MU, x)) / (alpha * alpha * _chan(VAR, x) + sigma * sigma)


def _posterior(x, alpha, sigma):
    """p(x0 | x_t) of that data: mean MU + g (x - alpha MU), variance vp -> (mean, g, vp)."""
    v, mu = _chan(VAR, x), _chan(MU, x)
    den = alpha * alpha * v + sigma * sigma
    g = alpha * v / den
    return mu + g * (x - alpha * mu), g, v * sigma * sigma / den


def quad_log_prob(x, alpha, sigma):
    """The quadratic log-probability 'classifier': an observation CENTER of x0 with Gaussian noise of variance CLF_W, seen
    through x_t -- log p_t(c | x_t) = -1/2 sum (c - E[x0 | x_t])^2 / (CLF_W + Var[x0 | x_t]) per image (up to a constant).  Its
    gradient vanishes like alpha at high noise, as a trained noisy classifier's does, so the guided x0 stays O(1)."""
    mean, _, vp = _posterior(x, alpha, sigma)
    return -0.5 * ((_chan(CENTER, x) - mean) ** 2 / (CLF_W + vp)).flatten(1).sum(1)


def quad_grad(x, alpha, sigma):
    mean, g, vp = _posterior(x, alpha, sigma)
    return g * (_chan(CENTER, x) - mean) / (CLF_W + vp)


def analytic_eps_fn(sc: Schedule, guided=True):
    def fn(x, t):
        al, sg = sc.alpha(t), sc.std(t)
        e = gauss_eps(x, al, sg)
        return e - GUIDANCE_SCALE * sg * quad_grad(x, al, sg) if guided else e
    return fn
