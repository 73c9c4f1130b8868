#!/usr/bin/env python3
"""Capture golden latents from the REFERENCE's own DPM-Solver ("Stable Diffusion"/ldm/models/diffusion/dpm_solver/
dpm_solver.py) for models that do not predict eps: ``model_wrapper(model_type="v" | "x_start", guidance_type=
"classifier-free")`` (noise_pred_fn :289-310) under ``DPM_Solver(predict_x0=True).sample(method="multistep", order=2,
lower_order_final=True, ea_timesteps=...)`` -- what dpm_solver/sampler.py:68-81 runs with ``model_type="noise"``.  The model is
oracle/sd_sampler.py::toy_model, read as a v- or an x0-prediction.  Build container only (needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_param.py

As in capture_sd_samplers.py the one ``torch.Tensor(timesteps).to('cuda')`` of dpm_solver.py:1088/1091 is routed to the CPU
(device placement only).  Only arrays are stored: tests/golden/sd_param_dpm.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/examples/Stable Diffusion")
sys.path.insert(0, ROOT)

from ldm.models.diffusion.dpm_solver import dpm_solver as _dpm  # noqa: E402
from ldm.modules.diffusionmodules.util import make_beta_schedule  # noqa: E402
from oracle.sd_sampler import toy_model  # noqa: E402


def _tensor_on_cpu(data):
    t = torch.tensor(data, dtype=torch.float32)

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


if __name__ == "__main__":
    g = torch.Generator().manual_seed(11)
    b, shape, scale = 2, (4, 8, 8), 3.0
    x_T = torch.randn(b, *shape, generator=g)
    c = torch.randn(b, 5, 16, generator=g)
    uc = torch.randn(b, 5, 16, generator=g)
    betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120)
    ac = torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)
    cand = [980, 700, 433, 150, 3]       # 4 steps: indices into the 1000-point time grid, as search_ea.py hands them over
    out = dict(x_T=x_T.numpy(), c=c.numpy(), uc=uc.numpy(), alphas_cumprod=ac.numpy(), cand=np.array(cand, dtype=np.float64),
               scale=np.array(scale))
    _dpm.torch = _TorchShim()
    for tag, model_type in (("v", "v"), ("x0", "x_start")):
        for gtag, (s, ucond) in {"cfg": (scale, uc), "plain": (1.0, None)}.items():
            ns = _dpm.NoiseScheduleVP("discrete", alphas_cumprod=ac)
            fn = _dpm.model_wrapper(lambda x, t, cc: toy_model(x, t, cc), ns, model_type=model_type, guidance_type="classifier-free",
                                    condition=c, unconditional_condition=ucond, guidance_scale=s)
            solver = _dpm.DPM_Solver(fn, ns, predict_x0=True, thresholding=False)
            with torch.no_grad():
                x = solver.sample(x_T, steps=len(cand) - 1, skip_type="time_uniform", method="multistep", order=2,
                                  lower_order_final=True, ea_timesteps=cand)
            out[f"dpm_{tag}_{gtag}"] = x.numpy()
    _dpm.torch = torch
    path = os.path.join(HERE, "sd_param_dpm.npz")
    np.savez_compressed(path, **out)
    print(sorted(out), f"{os.path.getsize(path) / 1024:.1f} KiB")
