#!/usr/bin/env python3
"""Capture golden latents of the image-to-image path from the REFERENCE's own ``DDIMSampler.stochastic_encode`` / ``.decode``
("Stable Diffusion"/ldm/models/diffusion/ddim.py:219-254) as scripts/img2img.py drives them: ``make_schedule`` (uniform, or a
searched ``sampled_timestep`` list, sorted as ``sample`` sorts it), ``z_enc = stochastic_encode(x0, tensor([t_enc] * b), noise=...)``,
``decode(z_enc, c, t_enc, unconditional_guidance_scale, unconditional_conditioning)``, over the toy ``apply_model`` of
oracle/sd_sampler.py.  Build container only (needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_img2img.py

As in capture_sd_samplers.py the reference's ``register_buffer`` (which moves every table to "cuda") is overridden with a plain
``setattr``.  ``stochastic_encode`` reads entry ``t`` of a table of ``steps`` entries, so ``t = steps`` does not exist in the
reference (its img2img.py fails at strength 1.0); the ``t_enc = steps`` case therefore encodes at the last entry, ``steps - 1``, and
decodes all ``steps`` updates from there.  Stored: x0, noise, c, uc, and per case ``enc_<schedule>_<t>`` / ``dec_<schedule>_<t>_<cfg|plain>``.
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

from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.modules.diffusionmodules.util import make_beta_schedule  # noqa: E402
from oracle.sd_sampler import toy_model  # noqa: E402


class Model:  # the attributes of LatentDiffusion the sampler reads (ddpm.py:117-137)
    def __init__(self):
        betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120)
        ac = np.cumprod(1.0 - betas, axis=0)
        self.num_timesteps = 1000
        self.device = torch.device("cpu")
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)

    def apply_model(self, x, t, c):
        return toy_model(x, t, c)


class CpuDDIM(DDIMSampler):
    def register_buffer(self, name, attr):
        setattr(self, name, attr)


STEPS = 4
SCHEDULES = {"uniform4": None, "k4": [153, 424, 926, 690]}

if __name__ == "__main__":
    g = torch.Generator().manual_seed(29)
    b, shape = 3, (4, 8, 8)
    x0 = torch.randn(b, *shape, generator=g) * 0.8
    noise = torch.randn(b, *shape, generator=g)
    c = torch.randn(b, 5, 16, generator=g)
    uc = torch.randn(b, 5, 16, generator=g)
    m = Model()
    out = dict(x0=x0.numpy(), noise=noise.numpy(), c=c.numpy(), uc=uc.numpy(), steps=np.array(STEPS))
    for tag, cand in SCHEDULES.items():
        s = CpuDDIM(m)
        st = None if cand is None else np.array(sorted(cand))
        s.make_schedule(ddim_num_steps=STEPS, ddim_eta=0.0, verbose=False, sampled_timestep=st)
        out[f"timesteps_{tag}"] = np.asarray(s.ddim_timesteps)
        for t_enc in (1, 2, STEPS):
            t_idx = min(t_enc, STEPS - 1)
            z = s.stochastic_encode(x0, torch.tensor([t_idx] * b), noise=noise)
            out[f"enc_{tag}_{t_idx}"] = z.numpy()
            for gtag, (scale, ucond) in {"cfg": (7.5, uc), "plain": (1.0, None)}.items():
                out[f"dec_{tag}_{t_enc}_{gtag}"] = s.decode(z, c, t_enc, unconditional_guidance_scale=scale,
                                                            unconditional_conditioning=ucond).numpy()
    path = os.path.join(HERE, "sd_img2img.npz")
    np.savez_compressed(path, **out)
    print(sorted(out), f"{os.path.getsize(path) / 1024:.1f} KiB")
