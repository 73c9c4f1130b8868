#!/usr/bin/env python3
"""Capture golden vectors of the Stable-Diffusion first stage's decode path by importing the REFERENCE's own ``Decoder``
("Stable Diffusion"/ldm/modules/diffusionmodules/model.py:462-568).

Runs only in the build container (needs /root/reference); the GPU box never sees the reference.  Only inputs, expected
outputs and parameter names / shapes are stored -- weights are regenerated on both sides from ``oracle/fill.py`` under their
checkpoint names (``first_stage_model.decoder.*``, ``first_stage_model.post_quant_conv.*``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_vae.py

``ldm/models/autoencoder.py`` needs ``pytorch_lightning`` and is not imported: its decode path is
``dec = self.decoder(self.post_quant_conv(z))`` (autoencoder.py:329-332) with ``post_quant_conv = torch.nn.Conv2d(embed_dim,
ddconfig["z_channels"], 1)`` (:303), which is torch's own Conv2d below.
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
from ldm.modules.diffusionmodules.model import Decoder  # noqa: E402

torch.set_num_threads(8)

V1 = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=[], dropout=0.0, in_channels=3,
          resolution=256, z_channels=4)
CONFIGS = {
    # mid width 128 (the existing attention kernel), nin_shortcut, two Upsamples: 8 -> 16 (below the phase-conv threshold), 16 -> 32
    "sd_vae_tiny": dict(cfg=dict(ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0,
                                 in_channels=3, resolution=32, z_channels=4), n=2, hw=8),
    # mid width 512 at T = 256: the single-head 512-wide attention kernel
    "sd_vae_mid512": dict(cfg=dict(ch=128, out_ch=3, ch_mult=(1, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0,
                                   in_channels=3, resolution=32, z_channels=4), n=1, hw=16),
    # the v1 first stage at full width
    "full_sd_vae": dict(cfg=V1, n=1, hw=32),
}
EMBED_DIM = 4
PREFIX = "first_stage_model."


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def build(cfg):
    dec = Decoder(**cfg).eval()
    pqc = torch.nn.Conv2d(EMBED_DIM, cfg["z_channels"], 1).eval()
    with torch.no_grad():
        for k, v in dec.state_dict().items():
            v.copy_(torch.from_numpy(fill_array(PREFIX + "decoder." + k, tuple(v.shape))))
        for k, v in pqc.state_dict().items():
            v.copy_(torch.from_numpy(fill_array(PREFIX + "post_quant_conv." + k, tuple(v.shape))))
    return dec, pqc


if __name__ == "__main__":
    for name, c in CONFIGS.items():
        dec, pqc = build(c["cfg"])
        z = rnd((c["n"], EMBED_DIM, c["hw"], c["hw"]), 11)
        with torch.no_grad():
            out = dec(pqc(z))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, z=z.numpy(), out=out.numpy(), cfg=np.array(repr(c["cfg"])), embed_dim=np.array(EMBED_DIM))
        outside = float(((out < -1) | (out > 1)).float().mean())
        print(name, "params", sum(p.numel() for p in dec.parameters()), "out rms", float(out.pow(2).mean().sqrt()),
              f"outside [-1, 1]: {100 * outside:.1f} %", f"{os.path.getsize(path) / 1024:.1f} KiB")
    dec, pqc = build(V1)
    keys = {"decoder." + k: list(v.shape) for k, v in dec.state_dict().items()}
    keys.update({"post_quant_conv." + k: list(v.shape) for k, v in pqc.state_dict().items()})
    with open(os.path.join(HERE, "sd_vae_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("sd_vae_keys.json:", len(keys), "entries")
