"""DPM-Solver / DPM-Solver++ on the pixel (ADM) path: multistep orders 1-3, classifier guidance, dynamic thresholding.

Mirror of the reference's generic solver (ldm/models/diffusion/dpm_solver/dpm_solver.py: NoiseScheduleVP :11-174,
model_wrapper(guidance_type="classifier") :312-335, DPM_Solver :351-1141) for ``method='multistep'`` and
``solver_type='dpm_solver'``.  The schedule, the time grids and every update coefficient are host float64; one model
evaluation is one launch of ``adm_pix_dpm_step`` (two with thresholding: the per-image quantile of |x0|, then the update),
and the networks are evaluated exactly as ``SpacedDiffusion._step`` evaluates them (two streams, graph replay).

Out of scope: singlestep, adaptive, ``solver_type='taylor'``.

One deliberate difference: the reference cannot run order-3 multistep with ``lower_order_final=True`` and ``steps < 15``
(``multistep_dpm_solver_second_update`` unpacks the 3-long history, :773, ValueError).  Here a lower-order update uses the
newest entries of the history, the evident intent.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import ops
from .schedule import ModelMeanType
from .sd_sampler import NoiseScheduleVP as _DiscreteVP

QUANTILE = 0.995   # Imagen's dynamic-thresholding percentile (dpm_solver.py:395)


class NoiseScheduleVP(_DiscreteVP):
    """The discrete VP schedule of sd_sampler with ``inverse_lambda`` (dpm_solver.py:158-169)."""

    def inverse_lambda(self, lamb: float) -> float:
        log_alpha = -0.5 * float(np.logaddexp(0.0, -2.0 * lamb))
        xp, yp = self.log_alpha_array[::-1], self.t_array[::-1]       # ascending log(alpha)
        k = min(max(int(np.searchsorted(xp, log_alpha)), 1), self.total_N - 1)
        return float(yp[k - 1] + (log_alpha - xp[k - 1]) * (yp[k] - yp[k - 1]) / (xp[k] - xp[k - 1]))


def get_time_steps(ns: NoiseScheduleVP, skip_type: str, t_T: float, t_0: float, N: int):
    """dpm_solver.py:410-437 -> N + 1 descending times.  The grids are float32 there (torch.linspace); the same float32 values
    here, so that both walk the same points."""
    if skip_type == "logSNR":
        lam = np.linspace(np.float32(ns.marginal_lambda(t_T)), np.float32(ns.marginal_lambda(t_0)), N + 1, dtype=np.float32)
        return [ns.inverse_lambda(float(v)) for v in lam]
    if skip_type == "time_uniform":
        return [float(v) for v in np.linspace(t_T, t_0, N + 1, dtype=np.float32)]
    if skip_type == "time_quadratic":
        return [float(v) for v in np.linspace(t_T ** 0.5, t_0 ** 0.5, N + 1, dtype=np.float32) ** np.float32(2)]
    raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")


def candidate_times(indices: Sequence[int], total_N: int, order: int):
    """A searched candidate (K distinct integers of range(total_N)) -> (descending indices, their continuous times (i + 1) / N).
    K evaluations: K - 1 solver updates between consecutive points and denoise_to_zero at the smallest."""
    idx = [int(i) for i in indices]
    if len(set(idx)) != len(idx) or any(not 0 <= i < total_N for i in idx):
        raise ValueError(f"a DPM-Solver candidate is a list of distinct integers of range({total_N}), got {list(indices)}")
    if len(idx) - 1 < order:
        raise ValueError(f"a DPM-Solver candidate of {len(idx)} timesteps takes {len(idx) - 1} updates, fewer than order {order}")
    idx.sort(reverse=True)
    return idx, [(i + 1) / total_N for i in idx]


def step_orders(steps: int, order: int, lower_order_final: bool):
    """The order of update 1 .. steps (dpm_solver.py:1103-1115)."""
    out = []
    for step in range(1, steps + 1):
        if step < order:
            out.append(step)
        elif lower_order_final and steps < 15:
            out.append(min(order, steps + 1 - step))
        else:
            out.append(order)
    return out


def update_coefs(ns: NoiseScheduleVP, t_hist: Sequence[float], t: float, order: int, predict_x0: bool):
    """x_t = a x + b0 m0 + b1 m1 + b2 m2 for the multistep update of `order` from t_hist[-1] to t, m0 the newest model value
    (dpm_solver.py:504-549, :755-857 with solver_type='dpm_solver'; D1 / D2 expanded).  float64 -> (a, [b0, b1, b2])."""
    t0 = t_hist[-1]
    lam0, lam_t = ns.marginal_lambda(t0), ns.marginal_lambda(t)
    h = lam_t - lam0
    e = np.eye(3)
    if predict_x0:
        a = ns.marginal_std(t) / ns.marginal_std(t0)
        scale, eh = ns.marginal_alpha(t), math.exp(-h)
        phi = scale * (eh - 1.0)
        c1, c2 = scale * ((eh - 1.0) / h + 1.0), -scale * ((eh - 1.0 + h) / h ** 2 - 0.5)
    else:
        a = math.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(t0))
        scale, eh = ns.marginal_std(t), math.exp(h)
        phi = scale * (eh - 1.0)
        c1, c2 = -scale * ((eh - 1.0) / h - 1.0), -scale * ((eh - 1.0 - h) / h ** 2 - 0.5)
    if order == 1:
        b = -phi * e[0]
    elif order == 2:
        r0 = (lam0 - ns.marginal_lambda(t_hist[-2])) / h
        b = -phi * e[0] - 0.5 * phi * (e[0] - e[1]) / r0
    elif order == 3:
        lam1, lam2 = ns.marginal_lambda(t_hist[-2]), ns.marginal_lambda(t_hist[-3])
        r0, r1 = (lam0 - lam1) / h, (lam1 - lam2) / h
        d10, d11 = (e[0] - e[1]) / r0, (e[1] - e[2]) / r1
        d1 = d10 + r0 / (r0 + r1) * (d10 - d11)
        d2 = (d10 - d11) / (r0 + r1)
        b = -phi * e[0] + c1 * d1 + c2 * d2
    else:
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
    return float(a), [float(v) for v in b]


class DPMSolver:
    """Multistep DPM-Solver over a base (1000-step) ``SpacedDiffusion``: its betas give the discrete schedule, its model types
    say what the network predicts, its ``_eval_networks`` evaluates eps and the guidance gradient."""

    def __init__(self, diffusion, *, predict_x0: bool = True, thresholding: bool = False, max_val: float = 1.0):
        if thresholding and not predict_x0:
            raise ValueError("thresholding is defined for the data-prediction solver only (predict_x0=True)")
        self.diffusion = diffusion
        self.ns = NoiseScheduleVP("discrete", betas=np.asarray(diffusion.betas, dtype=np.float64))
        self.predict_x0, self.thresholding, self.max_val = bool(predict_x0), bool(thresholding), float(max_val)
        self.start_x = diffusion.model_mean_type == ModelMeanType.START_X
        self.last_uint8_nhwc = None
        self.last_s = None      # per-image thresholds of the last evaluation (thresholding only)

    # ------------------------------------------------------------------ time points
    def time_points(self, steps, skip_type="time_uniform", t_start=None, t_end=None, timesteps=None):
        """dpm_solver.py:1071-1097 -> the steps + 1 descending times.  `timesteps` are the reference's ea_timesteps: integers
        index the ascending 1000-point grid of `skip_type` in the given order, floats are times, sorted descending."""
        ns = self.ns
        t_0 = 1.0 / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
        if timesteps is None:
            ts = get_time_steps(ns, skip_type, t_T, t_0, steps)
        else:
            ea = [v.item() if hasattr(v, "item") else v for v in timesteps]
            if max(ea) > 1:
                full = get_time_steps(ns, skip_type, t_T, t_0, 1000)[::-1]
                ts = [float(np.float32(full[int(v)])) for v in ea]
            else:
                ts = [float(np.float32(v)) for v in sorted(ea, reverse=True)]
        if len(ts) - 1 != steps:
            raise ValueError(f"{len(ts)} time points make {len(ts) - 1} steps, not steps={steps}")
        return ts

    # ------------------------------------------------------------------ loops
    def sample(self, model, shape, noise=None, cond_fn=None, model_kwargs=None, device=None, *, steps=20, order=2,
               skip_type="time_uniform", method="multistep", lower_order_final=True, denoise_to_zero=False,
               solver_type="dpm_solver", t_start=None, t_end=None, timesteps=None, record=None):
        """``DPM_Solver.sample`` (:965-1141) with continuous times: the networks receive (t - 1/N) * 1000 as there."""
        if method != "multistep" or solver_type != "dpm_solver":
            raise NotImplementedError("the ADM path runs method='multistep' with solver_type='dpm_solver' only")
        ts = self.time_points(steps, skip_type, t_start, t_end, timesteps)
        t_in = [(t - 1.0 / self.ns.total_N) * 1000.0 for t in ts]
        return self._run(model, shape, noise, cond_fn, model_kwargs, device, ts, t_in, order, lower_order_final,
                         denoise_to_zero, record)

    def sample_candidate(self, model, shape, noise=None, cond_fn=None, model_kwargs=None, device=None, *, indices, order=2,
                         lower_order_final=True, record=None):
        """A searched candidate: the networks are evaluated at exactly its integer timesteps (they receive the integer), K - 1
        updates between them and denoise_to_zero at the smallest -- K evaluations, as DDIM spends on the same candidate."""
        idx, ts = candidate_times(indices, self.ns.total_N, order)
        return self._run(model, shape, noise, cond_fn, model_kwargs, device, ts, idx, order, lower_order_final, True, record)

    def _t_tensor(self, t_in, n, device):
        if isinstance(t_in, int):
            t = torch.full((n,), t_in, device=device, dtype=torch.long)
            return t.float() * (1000.0 / self.ns.total_N) if self.diffusion.rescale_timesteps else t
        return torch.full((n,), float(t_in), device=device, dtype=torch.float32)

    def _run(self, model, shape, noise, cond_fn, model_kwargs, device, ts, t_in, order, lower_order_final, denoise_to_zero,
             record):
        steps = len(ts) - 1
        if order not in (1, 2, 3):
            raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
        if steps < order:
            raise ValueError(f"steps={steps} is fewer than order {order}")
        if model_kwargs is None:
            model_kwargs = {}
        if device is None:
            device = noise.device if noise is not None else next(model.parameters()).device
        x = noise if noise is not None else torch.randn(*shape, device=device)
        x = x.to(torch.float32).contiguous()
        n = x.shape[0]
        ns, orders = self.ns, step_orders(steps, order, lower_order_final)
        work = ops.abs_quantile_work(n, x[0].numel(), x.device) if self.thresholding else None
        hist = []        # model values, newest last
        u8 = s = None
        with torch.no_grad():
            for j in range(steps + 1):
                last_eval = j == steps
                if last_eval and not denoise_to_zero:
                    break   # "We do not need to evaluate the final model value" (:1120)
                model_out, grad = self.diffusion._eval_networks(model, x, self._t_tensor(t_in[j], n, x.device), cond_fn, model_kwargs)
                model_out = model_out.contiguous()
                kw = dict(alpha_s=ns.marginal_alpha(ts[j]), sigma_s=ns.marginal_std(ts[j]), start_x=self.start_x,
                          thresholding=self.thresholding, q=QUANTILE, max_val=self.max_val, work=work, want_s=self.thresholding)
                if last_eval:   # denoise_to_zero_fn: the data prediction at the last point, whatever the solver predicts (:498-502)
                    m, x_next, u8, s = ops.pix_dpm_step(x, model_out, grad, None, None, None, predict_x0=True, want_next=False,
                                                        want_u8=True, **kw)
                    rec_coefs, out = None, m
                else:
                    p = orders[j]
                    a, b = update_coefs(ns, ts[max(0, j - 2):j + 1], ts[j + 1], p, self.predict_x0)
                    h1 = hist[-1] if p >= 2 else None
                    h2 = hist[-2] if p >= 3 else None
                    final_launch = j == steps - 1 and not denoise_to_zero
                    m, x_next, u8, s = ops.pix_dpm_step(x, model_out, grad, x, h1, h2, a=a, b0=b[0], b1=b[1], b2=b[2],
                                                        predict_x0=self.predict_x0, want_u8=final_launch, **kw)
                    rec_coefs, out = (a, b, p), x_next
                if record is not None:
                    record.append(dict(j=j, t=ts[j], x=x, model_out=model_out, grad=grad, h1=None if last_eval else h1,
                                       h2=None if last_eval else h2, coefs=rec_coefs, alpha=kw["alpha_s"], sigma=kw["sigma_s"],
                                       m=m, x_next=x_next, s=s))
                hist = (hist + [m])[-2:]
                x = out
        self.last_uint8_nhwc, self.last_s = u8, s
        return x


__all__ = ["DPMSolver", "NoiseScheduleVP", "QUANTILE", "candidate_times", "get_time_steps", "step_orders", "update_coefs"]
