#!/usr/bin/env python3
"""Capture golden latents of MASKED sampling and of ``prompt_mask`` from the REFERENCE's own DDIMSampler / PLMSSampler
("Stable Diffusion"/ldm/models/diffusion/ddim.py:157-160, plms.py:85,131,159-171), in the manner of capture_sd_samplers.py: the same
``Model``, ``Cpu*`` subclasses, toy ``apply_model`` (oracle/sd_sampler.py::toy_model) and shared inputs (x_T, c, uc of
sd_samplers.npz: the same generator, the same draws).  Build container only (needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_masked.py

``LatentDiffusion`` itself needs pytorch_lightning and cannot be imported, so the capture ``Model`` gains ``q_sample(x0, t)``: it
restates ddpm.py:274-277 from the float32 tables (the per-sample sqrt(abar_t) times x_start plus sqrt(1 - abar_t) times the noise, the
tables being float32 roundings of float64 roots, ddpm.py:141-142) and takes its noise from a pre-drawn list, one draw per call, which
the fixture stores as ``q_noise``.  The loop, the blend and the prompt-mask branch are the reference's own code.

mask: 1 keeps x0, 0 is generated.  All runs: eta = 0, candidates k4 = [153, 424, 926, 690] and k1 = [500] (PLMS is handed the sorted
list, as search_ea.py hands it).  The file is written with fixed zip timestamps: a second run reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import capture_sd_samplers as base  # noqa: E402  (puts the reference on sys.path; Model, CpuDDIM, CpuPLMS)


class Model(base.Model):
    def __init__(self, q_noise):
        super().__init__()
        # ddpm.py:131-132: float32 buffers of the float64 square roots
        from ldm.modules.diffusionmodules.util import make_beta_schedule
        ac = np.cumprod(1.0 - make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120), axis=0)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)
        self.q_noise, self.q_calls = q_noise, 0

    def q_sample(self, x_start, t, noise=None):
        assert noise is None
        noise = self.q_noise[self.q_calls]
        self.q_calls += 1
        per_sample = (-1,) + (1,) * (x_start.dim() - 1)
        signal, sigma = self.sqrt_alphas_cumprod[t].reshape(per_sample), self.sqrt_one_minus_alphas_cumprod[t].reshape(per_sample)
        return signal * x_start + sigma * noise


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def masks(b, c, h, w, g):
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    blocks = np.stack([(((ii + n) // 2 + (jj + 2 * n) // 2) % 2) for n in range(b)])[:, None]          # [b, 1, h, w], 2 x 2 blocks
    half = (jj < w // 2)[None, None]                                                                 # [1, 1, h, w], left half kept
    chan = (torch.rand(b, c, h, w, generator=g) < 0.5).numpy()                                       # [b, c, h, w]
    return {"blocks": blocks.astype(np.float32), "half": half.astype(np.float32), "chan": chan.astype(np.float32)}


if __name__ == "__main__":
    g = torch.Generator().manual_seed(7)
    b, shape = 3, (4, 8, 8)
    x_T = torch.randn(b, *shape, generator=g)
    c = torch.randn(b, 5, 16, generator=g)
    uc = torch.randn(b, 5, 16, generator=g)
    g2 = torch.Generator().manual_seed(71)   # its own generator: the three shared inputs above stay those of sd_samplers.npz
    x0 = torch.randn(b, *shape, generator=g2)
    q_noise = torch.randn(4, b, *shape, generator=g2)
    mk = masks(b, *shape, g2)
    m = Model(list(q_noise))
    out = dict(x_T=x_T.numpy(), c=c.numpy(), uc=uc.numpy(), x0=x0.numpy(), q_noise=q_noise.numpy(),
               alphas_cumprod=m.alphas_cumprod.numpy())
    out.update({f"mask_{k}": v for k, v in mk.items()})
    cands = {"k4": [153, 424, 926, 690], "k1": [500]}
    guid = {"cfg": (7.5, uc), "plain": (1.0, None)}

    def run(name, tag, gtag, mask=None, prompt_mask=None):
        cls = {"ddim": base.CpuDDIM, "plms": base.CpuPLMS}[name]
        cand = cands[tag]
        st = np.array(sorted(cand)) if name == "plms" else np.array(cand)
        scale, ucond = guid[gtag]
        m.q_calls = 0
        kw = {} if prompt_mask is None else {"prompt_mask": prompt_mask}
        if mask is not None:
            kw.update(mask=torch.from_numpy(mk[mask]), x0=x0)
        s, _ = cls(m).sample(S=len(cand), batch_size=b, shape=list(shape), conditioning=c, verbose=False, eta=0.0, x_T=x_T,
                             unconditional_guidance_scale=scale, unconditional_conditioning=ucond, sampled_timestep=st, **kw)
        assert m.q_calls == (len(cand) if mask is not None else 0)
        return s.numpy()

    for tag in cands:
        out[f"cand_{tag}"] = np.array(cands[tag])
        for name in ("ddim", "plms"):
            for gtag in guid:
                for mask in ("blocks", "half"):
                    out[f"{name}_{tag}_{gtag}_{mask}"] = run(name, tag, gtag, mask=mask)
    out["ddim_k4_cfg_chan"] = run("ddim", "k4", "cfg", mask="chan")
    for pm in ([1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 1, 1], [1, 1, 1, 1]):   # [0, 1, 1, 1]: the two-call first step runs unguided
        out["plms_k4_cfg_pm" + "".join(map(str, pm))] = run("plms", "k4", "cfg", prompt_mask=pm)
    out["plms_k1_cfg_pm0"] = run("plms", "k1", "cfg", prompt_mask=[0])
    out["plms_k4_cfg_half_pm1010"] = run("plms", "k4", "cfg", mask="half", prompt_mask=[1, 0, 1, 0])
    path = os.path.join(HERE, "sd_masked.npz")
    save_npz(path, out)
    print(sorted(out), f"{os.path.getsize(path) / 1024:.1f} KiB")
