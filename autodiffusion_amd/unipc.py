"""UniPC (Zhao et al., "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models", NeurIPS 2023) on
the pixel (ADM) path: the multistep B(h) form of orders 1-3, both prediction types, classifier guidance, dynamic thresholding.

The reference tree has no UniPC; DESIGN.md section 11.1 is the specification this file follows.  The multistep predictor of order
p is wrapped in a corrector of the same order that reuses the model value the next update has to compute anyway: K evaluations
still make K updates, each but the last arrival corrected, one order of accuracy higher.  DPM-Solver++(2M) is the special case
order 2, variant 'bh2', corrector off.

As in dpm_solver.py the schedule, the time grids and every coefficient are host float64; one model evaluation is one launch of
``adm_pix_unipc_step`` (two with thresholding), which forms the model value once and writes both the corrected point of the update
that arrived here and the predicted point of the next one.  The schedule, grids, order table and candidate mapping are
dpm_solver.py's own, imported.

Out of scope: singlestep UniPC, ``vary_coeff``.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import ops
from .dpm_solver import (QUANTILE, DPMSolver, NoiseScheduleVP, candidate_times, get_time_steps,  # noqa: F401  (the grids: through
                         step_orders)                                                           # DPMSolver.time_points)
from .schedule import ModelMeanType

VARIANTS = ("bh1", "bh2")


def unipc_coefs(ns, t_hist: Sequence[float], t: float, order: int, variant: str = "bh2", predict_x0: bool = True,
                corrector: bool = True):
    """One update of `order` from s = t_hist[-1] to t on the model values m_0 (at s), m_1, ... (newest first; t_hist oldest first):
        x_pred = a x + sum_k p[k] m_k                       k < 3
        x_corr = a x + c[0] m_t + sum_k c[k + 1] m_k        m_t the model value at (x_pred, t)
    float64 -> (a, [p0, p1, p2], [c0, c1, c2, c3]); unused entries are 0, c is all 0 with the corrector off."""
    if order not in (1, 2, 3):
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
    if variant not in VARIANTS:
        raise ValueError(f"variant must be 'bh1' or 'bh2', got {variant!r}")
    if len(t_hist) < order:
        raise ValueError(f"an update of order {order} needs {order} history times, got {len(t_hist)}")
    s = t_hist[-1]
    lam_s = ns.marginal_lambda(s)
    h = ns.marginal_lambda(t) - lam_s
    hh = -h if predict_x0 else h
    if hh == 0.0:
        raise ZeroDivisionError(f"a zero-length update: lambda({t}) == lambda({s})")
    rks = [(ns.marginal_lambda(t_hist[-1 - i]) - lam_s) / h for i in range(1, order)] + [1.0]
    h_phi_1 = math.expm1(hh)
    B = hh if variant == "bh1" else h_phi_1
    phi, f = h_phi_1 / hh - 1.0, 1.0
    R, b = np.zeros((order, order)), np.zeros(order)
    for i in range(1, order + 1):
        R[i - 1] = np.power(rks, i - 1)
        b[i - 1] = phi * f / B
        f *= i + 1
        phi = phi / hh - 1.0 / f
    if order == 1:
        rhos_p = []
    elif order == 2:
        rhos_p = [0.5]
    else:
        rhos_p = list(np.linalg.solve(R[:-1, :-1], b[:-1]))
    if predict_x0:
        a, scale = ns.marginal_std(t) / ns.marginal_std(s), ns.marginal_alpha(t)
    else:
        a, scale = math.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(s)), ns.marginal_std(t)
    # D1_k = (m_k - m_0) / rk_k: its weight goes to m_k, minus it to m_0
    p = [-scale * h_phi_1, 0.0, 0.0]
    for k, rho in enumerate(rhos_p, start=1):
        w = -scale * B * rho / rks[k - 1]
        p[k] += w
        p[0] -= w
    c = [0.0, 0.0, 0.0, 0.0]
    if corrector:
        rhos_c = [0.5] if order == 1 else list(np.linalg.solve(R, b))
        c[1] = -scale * h_phi_1
        for k, rho in enumerate(rhos_c[:-1], start=1):
            w = -scale * B * rho / rks[k - 1]
            c[k + 1] += w
            c[1] -= w
        w = -scale * B * rhos_c[-1]     # (m_t - m_0), rk = 1
        c[0] += w
        c[1] -= w
    return float(a), [float(v) for v in p], [float(v) for v in c]


def plan_evaluations(ns, ts: Sequence[float], order: int, lower_order_final: bool = True, variant: str = "bh2",
                     predict_x0: bool = True, corrector: bool = True):
    """The coefficients of every evaluation of the loop over the descending times ts[0 .. K], before anything is launched.
    Evaluation j (0 <= j < K) runs the network at ts[j]; entry j is a dict
        corr   None, or (ac, [c0 .. c3], p): the corrector of update j - 1 (order p), which forms x_corr_j from x_{j-1}, this
               evaluation's m and the history h1 .. h_p
        pred   (ap, [p0 .. p2], p): the predictor of update j (order p) from x_corr_j (x_pred_j where corr is None), m, h1 .. h_{p-1}
    The arrival point ts[K] is not in the list: it is never corrected."""
    steps = len(ts) - 1
    if order not in (1, 2, 3):
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
    if steps < order:
        raise ValueError(f"steps={steps} is fewer than order {order}")
    orders = step_orders(steps, order, lower_order_final)
    plan = []
    for j in range(steps):
        corr = None
        if corrector and j >= 1:
            pc = orders[j - 1]
            ac, _, c = unipc_coefs(ns, ts[max(0, j - pc):j], ts[j], pc, variant, predict_x0, True)
            corr = (ac, c, pc)
        pp = orders[j]
        ap, p, _ = unipc_coefs(ns, ts[max(0, j + 1 - pp):j + 1], ts[j + 1], pp, variant, predict_x0, False)
        plan.append(dict(corr=corr, pred=(ap, p, pp)))
    return plan


class UniPC:
    """Multistep UniPC over a base (1000-step) ``SpacedDiffusion``, in ``DPMSolver``'s terms: its betas give the discrete schedule,
    its model types say what the network predicts, its ``_eval_networks`` evaluates eps and the guidance gradient."""

    def __init__(self, diffusion, *, predict_x0: bool = True, thresholding: bool = False, max_val: float = 1.0,
                 variant: str = "bh2", corrector: bool = True):
        if thresholding and not predict_x0:
            raise ValueError("thresholding is defined for the data-prediction solver only (predict_x0=True)")
        if variant not in VARIANTS:
            raise ValueError(f"variant must be 'bh1' or 'bh2', got {variant!r}")
        self.diffusion = diffusion
        self.ns = NoiseScheduleVP("discrete", betas=np.asarray(diffusion.betas, dtype=np.float64))
        self.predict_x0, self.thresholding, self.max_val = bool(predict_x0), bool(thresholding), float(max_val)
        self.variant, self.corrector = variant, bool(corrector)
        self.start_x = diffusion.model_mean_type == ModelMeanType.START_X
        self.last_uint8_nhwc = None
        self.last_s = None      # per-image thresholds of the last evaluation (thresholding only)

    # the time grids (skip types, t_start / t_end, both `timesteps` forms) and the networks' time input are DPMSolver's own
    time_points = DPMSolver.time_points
    _t_tensor = DPMSolver._t_tensor

    # ------------------------------------------------------------------ loops
    def sample(self, model, shape, noise=None, cond_fn=None, model_kwargs=None, device=None, *, steps=20, order=2,
               skip_type="time_uniform", method="multistep", lower_order_final=True, denoise_to_zero=False, t_start=None,
               t_end=None, timesteps=None, record=None):
        """``DPMSolver.sample``'s interface: continuous times, the networks receive (t - 1/N) * 1000."""
        if method != "multistep":
            raise NotImplementedError("the ADM path runs method='multistep' only")
        ts = self.time_points(steps, skip_type, t_start, t_end, timesteps)
        t_in = [(t - 1.0 / self.ns.total_N) * 1000.0 for t in ts]
        return self._run(model, shape, noise, cond_fn, model_kwargs, device, ts, t_in, order, lower_order_final,
                         denoise_to_zero, record)

    def sample_candidate(self, model, shape, noise=None, cond_fn=None, model_kwargs=None, device=None, *, indices, order=2,
                         lower_order_final=True, record=None):
        """A searched candidate, mapped as ``DPMSolver.sample_candidate`` maps it: the networks are evaluated at exactly its K
        integer timesteps, K - 1 updates between them (all but the last arrival corrected) and denoise_to_zero at the smallest."""
        idx, ts = candidate_times(indices, self.ns.total_N, order)
        return self._run(model, shape, noise, cond_fn, model_kwargs, device, ts, idx, order, lower_order_final, True, record)

    def _run(self, model, shape, noise, cond_fn, model_kwargs, device, ts, t_in, order, lower_order_final, denoise_to_zero,
             record):
        steps = len(ts) - 1
        ns = self.ns
        plan = plan_evaluations(ns, ts, order, lower_order_final, self.variant, self.predict_x0, self.corrector)   # raises first
        if model_kwargs is None:
            model_kwargs = {}
        if device is None:
            device = noise.device if noise is not None else next(model.parameters()).device
        x = noise if noise is not None else torch.randn(*shape, device=device)
        x = x.to(torch.float32).contiguous()
        n = x.shape[0]
        work = ops.abs_quantile_work(n, x[0].numel(), x.device) if self.thresholding else None
        hist = []          # model values, newest last
        x_base = None      # the accepted state at the previous time: what the corrector restarts from
        u8 = s = None
        with torch.no_grad():
            for j in range(steps + 1):
                last_eval = j == steps
                if last_eval and not denoise_to_zero:
                    break
                model_out, grad = self.diffusion._eval_networks(model, x, self._t_tensor(t_in[j], n, x.device), cond_fn, model_kwargs)
                model_out = model_out.contiguous()
                kw = dict(alpha_s=ns.marginal_alpha(ts[j]), sigma_s=ns.marginal_std(ts[j]), start_x=self.start_x,
                          thresholding=self.thresholding, q=QUANTILE, max_val=self.max_val, work=work, want_s=self.thresholding)
                if last_eval:   # the data prediction at the arrival point, which is not corrected
                    m, x_corr, x_pred, u8, s = ops.pix_unipc_step(x, model_out, grad, None, None, None, None, predict_x0=True,
                                                                  want_u8=True, **kw)
                    corr = pred = None
                    hs = (None, None, None)
                    out = m
                else:
                    e = plan[j]
                    depth = max(e["corr"][2] if e["corr"] else 0, e["pred"][2] - 1)
                    hs = tuple(hist[-1 - i] if i < depth else None for i in range(3))
                    corr = None if e["corr"] is None else (e["corr"][0], *e["corr"][1])
                    pred = (e["pred"][0], *e["pred"][1])
                    final_launch = j == steps - 1 and not denoise_to_zero
                    m, x_corr, x_pred, u8, s = ops.pix_unipc_step(x, model_out, grad, x_base if corr else None, *hs, corr=corr,
                                                                  pred=pred, predict_x0=self.predict_x0, want_u8=final_launch, **kw)
                    out = x_pred
                if record is not None:
                    record.append(dict(j=j, t=ts[j], x=x, model_out=model_out, grad=grad, x_base=x_base if corr else None,
                                       h1=hs[0], h2=hs[1], h3=hs[2], corr=corr, pred=pred, alpha=kw["alpha_s"],
                                       sigma=kw["sigma_s"], m=m, x_corr=x_corr, x_pred=x_pred, s=s,
                                       orders=None if last_eval else (plan[j]["corr"][2] if plan[j]["corr"] else None,
                                                                      plan[j]["pred"][2])))
                hist = (hist + [m])[-3:]
                x_base = x_corr if x_corr is not None else x
                x = out
        self.last_uint8_nhwc, self.last_s = u8, s
        return x


__all__ = ["UniPC", "VARIANTS", "plan_evaluations", "unipc_coefs"]
