#!/usr/bin/env python3
"""Image-to-image with Stable Diffusion on the HIP path -- the reference's "Stable Diffusion"/scripts/img2img.py: the init image is
encoded by the KL-f8 encoder (``encode_first_stage`` -> ``get_first_stage_encoding``), noised to step ``t_enc = int(strength *
ddim_steps)`` of the DDIM table (``DDIMSampler.stochastic_encode``), denoised from there under classifier-free guidance
(``DDIMSampler.decode``) and decoded (``decode_first_stage``).

The reference's flags keep their names and defaults: ``--init-img --strength --ddim_steps --ddim_eta --scale --n_samples --n_iter
--seed --ckpt --config --outdir --prompt``; ``--plms`` is refused as the reference refuses it.  Loading and prompts are those of
autodiffusion_amd/sd_script_util.py: ``--prompt`` needs the LOCAL ``--tokenizer_dir``; ``--prompt_ids FILE.npy`` holds int64 [num, T] token ids
instead (one row for every sample of a batch, or ``--n_samples`` rows); ``--torso {bf16,fp16}``; ``--synthetic {tiny,v1,tiny2,v2}`` (tiny2 / v2: the v-predicting SD 2.x family) builds the
networks with ``randomize_()`` instead of reading ``--ckpt``.  ``--use_timestep "[t0, t1, ...]"`` (read with ``ast.literal_eval``)
runs on a searched schedule of ``--ddim_steps`` timesteps, sorted as ``DDIMSampler.sample`` sorts it, instead of the uniform one.

``--init-img`` is an image file (read with PIL, resized down to a multiple of ``--side_multiple``, default 64: f = 8 times the 8-pixel
latent granularity of the v1 first stage) or a ``.npy`` / ``.npz`` (``arr_0``) uint8 NHWC batch of one image (repeated
``--n_samples`` times, as the reference repeats its image) or of ``--n_samples`` images.  Output:
``OUTDIR/samples_{N}x{H}x{W}x3.npz`` with ``arr_0`` = uint8 NHWC images, N = n_iter * n_samples.

As in the reference ``t_enc`` indexes a table of ``ddim_steps`` entries: ``strength`` must leave 1 <= t_enc <= ddim_steps - 1
(the reference fails with an index error at strength 1.0).

``--skip_layers "[[ids], ...]"`` gives per-step layer-skip lists beside ``--use_timestep``: list i belongs to entry i
of ``--use_timestep`` as written; every UNet evaluation at that timestep bypasses those layers.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autodiffusion_amd import logger, ops  # noqa: E402
from autodiffusion_amd.sd_script_util import (add_sd_sampling_flags, build_model, load_images, load_prompts, read_skip_layers, read_use_timestep,  # noqa: E402
                                              require_gpu, save_samples, seed_everything)


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # ---- the reference's flags (img2img.py:52-190)
    add_sd_sampling_flags(p, "--prompt", "--init-img")
    p.add_argument("--outdir", type=str, nargs="?", help="dir to write results to", default="outputs/img2img-samples")
    p.add_argument("--ddim_steps", type=int, default=50, help="number of ddim sampling steps")
    p.add_argument("--plms", action="store_true", help="refused, as in the reference: img2img runs on DDIM")
    add_sd_sampling_flags(p, "--ddim_eta", "--scale")
    p.add_argument("--strength", type=float, default=0.75,
                   help="strength for noising/unnoising. 1.0 corresponds to full destruction of information in init image")
    add_sd_sampling_flags(p, "--config", "--side_multiple")   # from --tokenizer_dir on: additions (scripts/sd_search_ea.py)
    add_sd_sampling_flags(p, "--skip_layers", "--skip_layers")
    return p


def main(argv=None):
    """Returns the uint8 NHWC array it wrote."""
    from autodiffusion_amd.sd_sampler import DDIMSampler
    opt = create_argparser().parse_args(argv)
    if opt.plms:
        raise NotImplementedError("PLMS sampler not (yet) supported")   # img2img.py:209-211
    if not 0.0 <= opt.strength <= 1.0:
        raise SystemExit("sd_img2img.py: can only work with strength in [0.0, 1.0]")
    t_enc = int(opt.strength * opt.ddim_steps)
    if not 1 <= t_enc <= opt.ddim_steps - 1:
        raise SystemExit(f"sd_img2img.py: --strength {opt.strength} of --ddim_steps {opt.ddim_steps} gives t_enc = {t_enc}; "
                         f"the DDIM table has entries 1 .. {opt.ddim_steps - 1} to encode at")
    sched = read_use_timestep(opt.use_timestep, opt.ddim_steps, "sd_img2img.py")
    skips = read_skip_layers(getattr(opt, "skip_layers", ""), opt.use_timestep, opt.ddim_steps, "sd_img2img.py")
    seed_everything(opt.seed)
    logger.configure(opt.outdir)
    device = require_gpu("sd_img2img.py")
    init_image = load_images(opt.init_img, opt.n_samples, opt.side_multiple, "sd_img2img.py").to(device)
    prompts, empty, prompt_len = load_prompts(opt, device, "sd_img2img.py")
    model = build_model(opt, device, prompt_len=prompt_len, with_encoder=True)
    sampler = DDIMSampler(model)
    init_latent = model.get_first_stage_encoding(model.encode_first_stage(init_image))   # move to latent space
    sampler.make_schedule(ddim_num_steps=opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False, sampled_timestep=sched)
    print(f"target t_enc is {t_enc} steps")
    out = []
    for _ in range(opt.n_iter):
        uc = model.get_learned_conditioning(empty) if opt.scale != 1.0 else None
        c = model.get_learned_conditioning(prompts)
        z_enc = sampler.stochastic_encode(init_latent, torch.tensor([t_enc] * opt.n_samples))   # encode (scaled latent)
        samples = sampler.decode(z_enc, c, t_enc, unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc,
                                 skip_layers=skips)
        _, u8 = ops.vae_image_out(model.decode_first_stage(samples), want_unit=False, want_u8=True)
        out.append(u8.cpu().numpy())
    return save_samples(opt.outdir, np.concatenate(out, axis=0))


if __name__ == "__main__":
    main()
