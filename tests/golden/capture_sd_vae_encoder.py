#!/usr/bin/env python3
"""Capture golden vectors of the Stable-Diffusion first stage's encode path by importing the REFERENCE's own ``Encoder``
("Stable Diffusion"/ldm/modules/diffusionmodules/model.py:368-459) and ``DiagonalGaussianDistribution``
(ldm/modules/distributions/distributions.py:24-37).

Runs only in the build container (needs /root/reference); the GPU box never sees the reference.  Only inputs, expected
outputs and parameter names / shapes are stored -- weights are regenerated on both sides from ``oracle/fill.py`` under their
checkpoint names (``first_stage_model.encoder.*``, ``first_stage_model.quant_conv.*``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_vae_encoder.py

``ldm/models/autoencoder.py`` needs ``pytorch_lightning`` and is not imported: its encode path is
``moments = self.quant_conv(self.encoder(x)); posterior = DiagonalGaussianDistribution(moments)`` (autoencoder.py:321-326) with
``quant_conv = torch.nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)`` (:302), which is torch's own Conv2d below.
``sample()`` draws its noise inside (distributions.py:36); the stored sample is ``mean + std * noise`` with the stored noise, from
the distribution's own ``mean`` / ``std``.  Stored per config: the image ``x``, the ``moments`` after quant_conv, ``noise``, ``sample``
and the float64 network's distance from the fp32 one (printed; the issue's "benign moments" figures).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/examples/Stable Diffusion"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from oracle.fill import fill_array  # noqa: E402
from ldm.modules.diffusionmodules.model import Encoder  # noqa: E402
from ldm.modules.distributions.distributions import DiagonalGaussianDistribution  # noqa: E402

torch.set_num_threads(8)

V1 = dict(double_z=True, ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=[], dropout=0.0, in_channels=3,
          resolution=256, z_channels=4)
CONFIGS = {
    # mid width 128 (the existing attention kernel), nin_shortcut, two Downsamples: 32 -> 16 -> 8
    "sd_vae_enc_tiny": dict(cfg=dict(double_z=True, ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0,
                                     in_channels=3, resolution=32, z_channels=4), n=2, hw=32),
    # mid width 512 at T = 256: the single-head 512-wide attention kernel
    "sd_vae_enc_mid512": dict(cfg=dict(double_z=True, ch=128, out_ch=3, ch_mult=(1, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0,
                                       in_channels=3, resolution=32, z_channels=4), n=1, hw=32),
    # the v1 first stage at full width, one 128 x 128 image -> 16 x 16
    "full_sd_vae_enc": dict(cfg=V1, n=1, hw=128),
}
EMBED_DIM = 4
PREFIX = "first_stage_model."


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def build(cfg):
    enc = Encoder(**cfg).eval()
    qc = torch.nn.Conv2d(2 * cfg["z_channels"], 2 * EMBED_DIM, 1).eval()
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            v.copy_(torch.from_numpy(fill_array(PREFIX + "encoder." + k, tuple(v.shape))))
        for k, v in qc.state_dict().items():
            v.copy_(torch.from_numpy(fill_array(PREFIX + "quant_conv." + k, tuple(v.shape))))
    return enc, qc


if __name__ == "__main__":
    for name, c in CONFIGS.items():
        enc, qc = build(c["cfg"])
        x = torch.tanh(rnd((c["n"], 3, c["hw"], c["hw"]), 13) * 0.8)   # images in (-1, 1)
        with torch.no_grad():
            moments = qc(enc(x))
            post = DiagonalGaussianDistribution(moments)
            noise = rnd(tuple(post.mean.shape), 17)
            sample = post.mean + post.std * noise
            m64 = qc.double()(enc.double()(x.double()))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, x=x.numpy(), moments=moments.numpy(), noise=noise.numpy(), sample=sample.numpy(),
                            cfg=np.array(repr(c["cfg"])), embed_dim=np.array(EMBED_DIM))
        print(name, "params", sum(p.numel() for p in enc.parameters()), "mean rms", float(post.mean.pow(2).mean().sqrt()),
              "logvar in [%.3f, %.3f]" % (float(moments[:, EMBED_DIM:].min()), float(moments[:, EMBED_DIM:].max())),
              "fp32 vs float64 rel fro %.3g" % float((moments.double() - m64).norm() / m64.norm()),
              f"{os.path.getsize(path) / 1024:.1f} KiB")
    enc, qc = build(V1)
    keys = {"encoder." + k: list(v.shape) for k, v in enc.state_dict().items()}
    keys.update({"quant_conv." + k: list(v.shape) for k, v in qc.state_dict().items()})
    with open(os.path.join(HERE, "sd_vae_encoder_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("sd_vae_encoder_keys.json:", len(keys), "entries,", sum(p.numel() for p in enc.parameters()), "encoder parameters")
