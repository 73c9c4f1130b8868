#!/usr/bin/env python3
"""Capture golden vectors from the REFERENCE's own DPM-Solver ("Stable Diffusion"/ldm/models/diffusion/dpm_solver/
dpm_solver.py: NoiseScheduleVP, model_wrapper(guidance_type="classifier"), DPM_Solver.sample(method='multistep')) on the CPU.
Build container only (needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_adm_dpm.py     ->  tests/golden/adm_dpm.npz

(i)  An analytic model (tests/adm_dpm_ref.py: the exact eps of per-channel Gaussian data plus a quadratic log-probability
     'classifier', guidance scale 2): orders 1-3, noise / data prediction / data prediction with thresholding, linear and
     cosine betas, the three skip types, and the reference's two ea_timesteps forms.  Every evaluation's x and model value and
     the final output are stored (2 x 3 x 4 x 4 tensors).  A true denoiser keeps x0 O(1); an arbitrary function for eps does
     not (x0 scales with 1 / alpha).
     The cosine runs start at t = 0.9: at t = 1 that schedule has alpha = 4.9e-5, and the reference's fp32 x - sigma eps
     loses every digit of x0 = (x - sigma eps) / alpha there.  The linear runs start at t = 1 (alpha = 6.3e-3).
     These runs execute the reference's code with torch's default dtype set to float64 (its grids, schedule and updates then
     carry no fp32 rounding) and are stored rounded to fp32: the fixture pins the algorithm.  The same runs in the default
     fp32 differ from it by up to 1.9e-4 (order 3, and the logSNR grid): the reference's fp32 lambda = log(alpha) - log(sigma)
     cancels near t = 1 / N (sigma^2 = 1e-4 there), which the step ratios r0, r1 and the inverse_lambda grid inherit.
     Order 3 runs with lower_order_final=False: with it and steps < 15 the reference raises (it unpacks a 3-long history
     into two names, dpm_solver.py:773).
(ii) The tiny plan_m64 UNet and plan_c64 classifier (weights: oracle/fill.py), guided, on the integer-candidate form
     DPM_Solver.sample(x, steps=K-1, t_end=ts[-1], ea_timesteps=ts, denoise_to_zero=True) with ts = (i + 1) / 1000 of a
     candidate whose largest index is <= 900 (1 / alpha <= ~7 on the cosine schedule).

The one ``torch.Tensor(timesteps).to('cuda')`` in dpm_solver.py:1088/1091 is routed to the CPU (device placement only).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/examples/Stable Diffusion")
sys.path.insert(0, "/root/reference/examples/guided_diffusion")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adm_dpm_ref as R  # noqa: E402
from ldm.models.diffusion.dpm_solver import dpm_solver as _dpm  # noqa: E402
from oracle.fill import fill_array  # noqa: E402

torch.set_num_threads(8)


def _tensor_on_cpu(data):
    t = torch.tensor(data, dtype=torch.get_default_dtype())

    class _T:
        def to(self, *_a, **_k):
            return t
    return _T()


class _TorchShim:
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def Tensor(data):
        return _tensor_on_cpu(data)


def run(ns, model_fn, x, *, predict_x0, thresholding, **kw):
    """DPM_Solver.sample with every evaluation recorded -> (final, xs, ms, ss)."""
    solver = _dpm.DPM_Solver(model_fn, ns, predict_x0=predict_x0, thresholding=thresholding, max_val=1.0)
    xs, ms, ss = [], [], []

    def rec(orig, data_pred):
        def f(x_, t_):
            out = orig(x_, t_)
            xs.append(x_.numpy().copy())
            ms.append(out.numpy().copy())
            if thresholding and (predict_x0 or data_pred):
                noise = solver.noise_prediction_fn(x_, t_)
                d = x_.dim()
                x0 = (x_ - _dpm.expand_dims(ns.marginal_std(t_), d) * noise) / _dpm.expand_dims(ns.marginal_alpha(t_), d)
                ss.append(torch.quantile(x0.abs().reshape(x0.shape[0], -1), 0.995, dim=1).numpy().copy())
            return out
        return f
    solver.model_fn = rec(solver.model_fn, False)
    solver.denoise_to_zero_fn = rec(solver.denoise_to_zero_fn, True)
    with torch.no_grad():
        final = solver.sample(x, method="multistep", solver_type="dpm_solver", **kw)
    return final.numpy(), np.stack(xs), np.stack(ms), (np.stack(ss) if ss else None)


MODES = {"eps": (False, False), "x0": (True, False), "thr": (True, True)}


def analytic():
    out, quant = {}, []
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float32)
    out["a_x_T"] = x_T.numpy()
    x_T = x_T.double()
    for sched in ("linear", "cosine"):
        betas = torch.tensor(R.named_betas(sched), dtype=torch.float64)
        out[f"betas_{sched}"] = betas.numpy()
        ns = _dpm.NoiseScheduleVP("discrete", betas=betas)

        def model(x, t_input):
            t = t_input / 1000.0 + 1.0 / ns.total_N
            al, sg = (v.view(-1, 1, 1, 1) for v in (ns.marginal_alpha(t), ns.marginal_std(t)))
            return R.gauss_eps(x, al, sg)

        def classifier(x, t_input, cond):
            t = t_input / 1000.0 + 1.0 / ns.total_N
            return R.quad_log_prob(x, ns.marginal_alpha(t).view(-1, 1, 1, 1), ns.marginal_std(t).view(-1, 1, 1, 1))

        fn = _dpm.model_wrapper(model, ns, model_type="noise", guidance_type="classifier", condition=torch.zeros(2),
                                guidance_scale=R.GUIDANCE_SCALE, classifier_fn=classifier)
        t_start = None if sched == "linear" else 0.9
        cases = [(f"{skip}_o{order}_{mode}", dict(steps=5, order=order, skip_type=skip, lower_order_final=order < 3,
                                                  denoise_to_zero=skip != "logSNR", t_start=t_start), mode)
                 for skip in ("time_uniform", "time_quadratic", "logSNR") for order in (1, 2, 3) for mode in MODES]
        # the two ea_timesteps forms: integers index the ascending 1001-point grid, floats are times
        cases.append(("ea_int_o2_x0", dict(steps=5, order=2, skip_type="time_uniform", t_start=t_start, t_end=0.004,
                                           ea_timesteps=[1000, 800, 600, 350, 120, 0], denoise_to_zero=True), "x0"))
        cases.append(("ea_float_o2_thr", dict(steps=5, order=2, skip_type="time_uniform", t_end=0.004, denoise_to_zero=True,
                                              ea_timesteps=[0.2, 0.9 if sched == "cosine" else 1.0, 0.7, 0.45, 0.05, 0.004]), "thr"))
        for tag, kw, mode in cases:
            px0, thr = MODES[mode]
            final, xs, ms, ss = run(ns, fn, x_T, predict_x0=px0, thresholding=thr, **kw)
            key = f"a_{sched}_{tag}"
            out[key + "_final"], out[key + "_xs"], out[key + "_ms"] = (v.astype(np.float32) for v in (final, xs, ms))
            if ss is not None:
                out[key + "_q"] = ss.astype(np.float32)
                quant.append(ss.ravel())
    return out, np.concatenate(quant)


def tiny():
    from guided_diffusion.script_util import (classifier_defaults, create_classifier, create_model_and_diffusion,
                                              model_and_diffusion_defaults)
    d = model_and_diffusion_defaults()
    d.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="16",
             num_head_channels=32, class_cond=True, learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True,
             use_new_attention_order=True, use_dynamic_unet=True, noise_schedule="cosine")
    m, diff = create_model_and_diffusion(**d)
    c = classifier_defaults()
    c.update(image_size=64, classifier_width=64, classifier_depth=1)
    clf = create_classifier(**c)
    for mod in (m, clf):
        with torch.no_grad():
            for k, v in mod.state_dict().items():
                v.copy_(torch.from_numpy(fill_array(k, tuple(v.shape))))
        mod.eval()
    y = torch.tensor([3, 977])
    g = torch.Generator().manual_seed(51)
    x_T = torch.randn(2, 3, 64, 64, generator=g)
    ns = _dpm.NoiseScheduleVP("discrete", betas=torch.tensor(diff.betas, dtype=torch.float32))

    def model(x, t_input):
        return m(x, t_input, y)[:, :3]

    def classifier(x, t_input, cond):
        lp = F.log_softmax(clf(x, t_input), dim=-1)
        return lp[range(len(lp)), cond.view(-1)]

    fn = _dpm.model_wrapper(model, ns, model_type="noise", guidance_type="classifier", condition=y, guidance_scale=1.0,
                            classifier_fn=classifier)
    cand = [153, 424, 900, 690, 820]
    ts = [(i + 1) / 1000.0 for i in cand]
    out = {"t_x_T": x_T.numpy(), "t_y": y.numpy(), "t_cand": np.array(cand)}
    quant = []
    for tag, order, lof, thr in (("o2", 2, True, False), ("o2_thr", 2, True, True), ("o1", 1, True, False), ("o3", 3, False, False)):
        final, _, _, ss = run(ns, fn, x_T, predict_x0=True, thresholding=thr, steps=len(cand) - 1, order=order,
                              lower_order_final=lof, t_end=min(ts), ea_timesteps=ts, denoise_to_zero=True)
        smp = torch.from_numpy(final)
        out[f"t_{tag}_sample"] = final
        out[f"t_{tag}_uint8"] = ((smp + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
        if ss is not None:
            out[f"t_{tag}_q"] = ss
            quant.append(ss.ravel())
    return out, np.concatenate(quant)


if __name__ == "__main__":
    _dpm.torch = _TorchShim()
    torch.set_default_dtype(torch.float64)
    out, qa = analytic()
    torch.set_default_dtype(torch.float32)
    o2, qt = tiny()
    _dpm.torch = torch
    out.update(o2)
    q = np.concatenate([qa, qt])
    print(f"thresholded image-steps: {q.size}, quantile > 1: {(q > 1).sum()}, <= 1: {(q <= 1).sum()}; analytic {qa.min():.3f}..{qa.max():.3f}, "
          f"tiny {qt.min():.3f}..{qt.max():.3f}")
    assert (q > 1.0).any() and (q <= 1.0).any(), "the thresholded fixtures must hold both sides of max_val"
    assert (qa > 1.0).any() and (qa <= 1.0).any()
    path = os.path.join(HERE, "adm_dpm.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < 1024 * 1024
