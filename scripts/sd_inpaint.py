#!/usr/bin/env python3
"""Text-guided latent inpainting with Stable Diffusion on the HIP path: masked DDIM / PLMS sampling ("Stable Diffusion"/ldm/models/
diffusion/ddim.py:157-160, plms.py:159-162) as the reference's ``log_images(inpaint=True)`` drives it (ddpm.py:1327-1342).  The init
image is encoded by the KL-f8 encoder (``encode_first_stage`` -> ``get_first_stage_encoding``) into ``x0``; sampling starts from fresh
noise and before every step the kept region of the latent is replaced by ``q_sample(x0, t)``; the result is decoded and, unless
``--no_composite``, the kept PIXELS are restored from the input (scripts/inpaint.py:96, an exact uint8 select).

``--mask`` is an image file (read as 8-bit grey, resized like the init image, nearest) or a ``.npy`` / ``.npz`` (``arr_0``) uint8
``[N or 1, H, W]`` of the image's size.  WHITE (>= 128) MEANS REPAINT, scripts/inpaint.py's convention; the samplers' ``mask=`` means the
opposite (1 keeps ``x0``), so the script inverts it: latent keep mask = 1 - repaint, binarised at 0.5 and sampled at ``[::8, ::8]``
(``F.interpolate``'s default nearest, inpaint.py:77-78; 8 is the KL-f8 first stage's pixels per latent: the stride is the loaded
first stage's, image side / latent side).

``--plms`` samples with PLMSSampler (``--ddim_eta`` must stay 0) and admits ``--prompt_mask "[1,1,0,...]"``: one entry per step,
noisiest first; a step whose entry is 0 runs one unguided evaluation on the empty prompt instead of the guided pair
(plms.py:164-171, scripts/txt2img_prompt_mask.py).  Everything else -- ``--init-img --ckpt --config --prompt --prompt_ids
--tokenizer_dir --scale --ddim_steps --ddim_eta --n_samples --n_iter --seed --torso --synthetic --use_timestep --outdir
--side_multiple --skip_layers`` -- is scripts/sd_img2img.py's; what the two share is autodiffusion_amd/sd_script_util.py's.  Output:
``OUTDIR/samples_{N}x{H}x{W}x3.npz`` with ``arr_0`` = uint8 NHWC images.
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autodiffusion_amd import logger, ops  # noqa: E402
from autodiffusion_amd.sd_script_util import (add_sd_sampling_flags, build_model, load_images, load_prompts, read_skip_layers, read_use_timestep,  # noqa: E402
                                              require_gpu, save_samples, seed_everything)

F8 = 8   # pixels per latent of the KL-f8 first stage (--synthetic tiny's has two downsamplings: 4)


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_sd_sampling_flags(p, "--prompt", "--init-img")
    p.add_argument("--mask", type=str, required=True,
                   help="image file, or uint8 [N or 1, H, W] .npy / .npz of the image's size: white (>= 128) means REPAINT (inpaint.py's "
                        "convention); the script inverts it into the samplers' keep mask (1 keeps the image)")
    p.add_argument("--outdir", type=str, nargs="?", help="dir to write results to", default="outputs/inpaint-samples")
    p.add_argument("--ddim_steps", type=int, default=50, help="number of sampling steps")
    p.add_argument("--plms", action="store_true", help="use plms sampling")
    p.add_argument("--prompt_mask", type=str, default="", help="'[1,1,0,...]', --plms only: one entry per step, noisiest first; 0 = that "
                                                               "step runs unguided on the empty prompt")
    p.add_argument("--no_composite", action="store_true", help="write the decoded images as they are: do not restore the kept pixels")
    add_sd_sampling_flags(p, "--ddim_eta", "--skip_layers")
    return p


def load_mask(path, n_samples, hw, side_multiple=64):
    """-> bool [1 or n_samples, H, W], True = REPAINT (>= 128, i.e. >= 0.5 of inpaint.py:18-21); hw: the image's (H, W)."""
    if path.endswith((".npy", ".npz")):
        arr = np.load(path, allow_pickle=False)
        arr = arr["arr_0"] if path.endswith(".npz") else arr
        if arr.dtype != np.uint8 or arr.ndim != 3:
            raise SystemExit(f"sd_inpaint.py: --mask must hold a uint8 [N or 1, H, W] array, got {arr.dtype} {arr.shape}")
    else:
        from PIL import Image
        m = Image.open(path).convert("L")
        w, h = (v - v % side_multiple for v in m.size)
        arr = np.asarray(m.resize((w, h), resample=Image.NEAREST), dtype=np.uint8)[None]
    if arr.shape[0] not in (1, n_samples):
        raise SystemExit(f"sd_inpaint.py: --mask holds {arr.shape[0]} masks; one or --n_samples {n_samples} expected")
    if tuple(arr.shape[1:]) != tuple(hw):
        raise SystemExit(f"sd_inpaint.py: --mask is {arr.shape[1]} x {arr.shape[2]}, the image {hw[0]} x {hw[1]}")
    return arr >= 128


def latent_keep_mask(repaint, f=F8):
    """bool [M, H, W] repaint -> fp32 [M, 1, H / f, W / f], 1 = keep x0: the samplers' ``mask=`` (nearest, inpaint.py:77-78);
    f: pixels per latent of the first stage."""
    return (~repaint[:, ::f, ::f])[:, None].astype(np.float32)


def composite(init_u8, pred_u8, repaint):
    """inpaint.py:96 ``(1 - mask) * image + mask * predicted`` on uint8 NHWC with a 0/1 mask: an exact select."""
    return np.where(repaint[..., None], pred_u8, init_u8)


def main(argv=None):
    """Returns the uint8 NHWC array it wrote."""
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler
    opt = create_argparser().parse_args(argv)
    prompt_mask = None
    if opt.prompt_mask:
        if not opt.plms:
            raise SystemExit("sd_inpaint.py: --prompt_mask needs --plms (the reference has it on PLMSSampler only)")
        prompt_mask = [int(v) for v in ast.literal_eval(opt.prompt_mask)]
        if len(prompt_mask) != opt.ddim_steps:
            raise SystemExit(f"sd_inpaint.py: --prompt_mask holds {len(prompt_mask)} entries; --ddim_steps is {opt.ddim_steps}")
        if opt.scale == 1.0 and 0 in prompt_mask:
            raise SystemExit("sd_inpaint.py: --prompt_mask with a 0 entry needs --scale != 1 (the empty prompt is encoded only then)")
    sched = read_use_timestep(opt.use_timestep, opt.ddim_steps, "sd_inpaint.py")
    skips = read_skip_layers(getattr(opt, "skip_layers", ""), opt.use_timestep, opt.ddim_steps, "sd_inpaint.py")
    seed_everything(opt.seed)
    logger.configure(opt.outdir)
    device = require_gpu("sd_inpaint.py")
    init_image = load_images(opt.init_img, opt.n_samples, opt.side_multiple, "sd_inpaint.py")
    n, _, height, width = init_image.shape
    init_u8 = np.rint((init_image.permute(0, 2, 3, 1).numpy() + 1.0) * 127.5).astype(np.uint8)   # load_images' 2 * (u8 / 255) - 1, undone
    repaint = load_mask(opt.mask, opt.n_samples, (height, width), opt.side_multiple)
    prompts, empty, prompt_len = load_prompts(opt, device, "sd_inpaint.py")
    model = build_model(opt, device, prompt_len=prompt_len, with_encoder=True)
    sampler = (PLMSSampler if opt.plms else DDIMSampler)(model)
    x0 = model.get_first_stage_encoding(model.encode_first_stage(init_image.to(device)))   # move to latent space
    f = height // x0.shape[2]
    if (height, width) != (f * x0.shape[2], f * x0.shape[3]):
        raise SystemExit(f"sd_inpaint.py: the image is {height} x {width}, its latent {x0.shape[2]} x {x0.shape[3]}: no whole factor")
    keep = torch.from_numpy(latent_keep_mask(repaint, f)).to(device)
    extra = {} if prompt_mask is None else {"prompt_mask": prompt_mask}
    if skips is not None:
        extra["skip_layers"] = skips   # in ascending timestep order, as sched is
    out = []
    for _ in range(opt.n_iter):
        uc = model.get_learned_conditioning(empty) if opt.scale != 1.0 else None
        c = model.get_learned_conditioning(prompts)
        samples, _ = sampler.sample(S=opt.ddim_steps, batch_size=n, shape=list(x0.shape[1:]), conditioning=c, verbose=False,
                                    eta=opt.ddim_eta, mask=keep, x0=x0, unconditional_guidance_scale=opt.scale,
                                    unconditional_conditioning=uc, sampled_timestep=sched, **extra)
        _, u8 = ops.vae_image_out(model.decode_first_stage(samples), want_unit=False, want_u8=True)
        u8 = u8.cpu().numpy()
        out.append(u8 if opt.no_composite else composite(init_u8, u8, repaint))
    return save_samples(opt.outdir, np.concatenate(out, axis=0))


if __name__ == "__main__":
    main()
