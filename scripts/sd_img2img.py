#!/usr/bin/env python3
"""Image-to-image with Stable Diffusion on the HIP path -- the reference's "Stable Diffusion"/scripts/img2img.py: the init image is
encoded by the KL-f8 encoder (``encode_first_stage`` -> ``get_first_stage_encoding``), noised to step ``t_enc = int(strength *
ddim_steps)`` of the DDIM table (``DDIMSampler.stochastic_encode``), denoised from there under classifier-free guidance
(``DDIMSampler.decode``) and decoded (``decode_first_stage``).

The reference's flags keep their names and defaults: ``--init-img --strength --ddim_steps --ddim_eta --scale --n_samples --n_iter
--seed --ckpt --config --outdir --prompt``; ``--plms`` is refused as the reference refuses it.  Loading and prompts are those of
scripts/sd_search_ea.py: ``--prompt`` needs the LOCAL ``--tokenizer_dir``; ``--prompt_ids FILE.npy`` holds int64 [num, T] token ids
instead (one row for every sample of a batch, or ``--n_samples`` rows); ``--torso {bf16,fp16}``; ``--synthetic {tiny,v1}`` builds the
networks with ``randomize_()`` instead of reading ``--ckpt``.  ``--use_timestep "[t0, t1, ...]"`` (read with ``ast.literal_eval``)
runs on a searched schedule of ``--ddim_steps`` timesteps, sorted as ``DDIMSampler.sample`` sorts it, instead of the uniform one.

``--init-img`` is an image file (read with PIL, resized down to a multiple of ``--side_multiple``, default 64: f = 8 times the 8-pixel
latent granularity of the v1 first stage) or a ``.npy`` / ``.npz`` (``arr_0``) uint8 NHWC batch of one image (repeated
``--n_samples`` times, as the reference repeats its image) or of ``--n_samples`` images.  Output:
``OUTDIR/samples_{N}x{H}x{W}x3.npz`` with ``arr_0`` = uint8 NHWC images, N = n_iter * n_samples.

As in the reference ``t_enc`` indexes a table of ``ddim_steps`` entries: ``strength`` must leave 1 <= t_enc <= ddim_steps - 1
(the reference fails with an index error at strength 1.0).
"""
import argparse
import ast
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autodiffusion_amd import dist_util, logger, ops  # noqa: E402
from sd_search_ea import build_model  # noqa: E402


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # ---- the reference's flags (img2img.py:52-190)
    p.add_argument("--prompt", type=str, nargs="?", default="a painting of a virus monster playing guitar", help="the prompt to render")
    p.add_argument("--init-img", type=str, nargs="?", required=True, help="path to the input image (image file, or uint8 NHWC .npy / .npz)")
    p.add_argument("--outdir", type=str, nargs="?", help="dir to write results to", default="outputs/img2img-samples")
    p.add_argument("--ddim_steps", type=int, default=50, help="number of ddim sampling steps")
    p.add_argument("--plms", action="store_true", help="refused, as in the reference: img2img runs on DDIM")
    p.add_argument("--ddim_eta", type=float, default=0.0, help="ddim eta (eta=0.0 corresponds to deterministic sampling)")
    p.add_argument("--n_iter", type=int, default=1, help="sample this often")
    p.add_argument("--n_samples", type=int, default=2, help="how many samples to produce for each given prompt. A.k.a batch size")
    p.add_argument("--scale", type=float, default=5.0,
                   help="unconditional guidance scale: eps = eps(x, empty) + scale * (eps(x, cond) - eps(x, empty))")
    p.add_argument("--strength", type=float, default=0.75,
                   help="strength for noising/unnoising. 1.0 corresponds to full destruction of information in init image")
    p.add_argument("--config", type=str, default="configs/stable-diffusion/v1-inference.yaml",
                   help="path to config which constructs model (read when the file exists; else the SD-v1 constants)")
    p.add_argument("--ckpt", type=str, default="models/ldm/stable-diffusion-v1/model.ckpt", help="path to checkpoint of model")
    p.add_argument("--seed", type=int, default=42, help="the seed (for reproducible sampling)")
    # ---- additions (scripts/sd_search_ea.py)
    p.add_argument("--tokenizer_dir", type=str, default="", help="LOCAL directory of the transformers CLIP tokenizer (nothing is fetched)")
    p.add_argument("--prompt_ids", type=str, default="", help=".npy int64 [num, T] token ids (num = 1 or --n_samples); replaces --prompt")
    p.add_argument("--torso", choices=["bf16", "fp16"], default="bf16", help="16-bit type of activations and weights between kernels")
    p.add_argument("--synthetic", choices=["tiny", "v1"], default="", help="build the networks with randomize_() instead of reading --ckpt")
    p.add_argument("--use_timestep", type=str, default="", help="'[t0, t1, ...]': a searched schedule of --ddim_steps timesteps")
    p.add_argument("--side_multiple", type=int, default=64, help="an image FILE is resized down to a multiple of this many pixels")
    return p


def load_images(path, n_samples, side_multiple):
    """-> fp32 NCHW [n_samples, 3, H, W] in [-1, 1] (host), as img2img.py:39-49 load_img builds it."""
    if path.endswith((".npy", ".npz")):
        arr = np.load(path, allow_pickle=False)
        arr = arr["arr_0"] if path.endswith(".npz") else arr
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
            raise SystemExit(f"sd_img2img.py: --init-img must hold a uint8 [N, H, W, 3] batch, got {arr.dtype} {arr.shape}")
    else:
        from PIL import Image
        image = Image.open(path).convert("RGB")
        w, h = (v - v % side_multiple for v in image.size)
        print(f"loaded input image of size {image.size} from {path}, resized to ({w}, {h})")
        arr = np.asarray(image.resize((w, h), resample=Image.LANCZOS), dtype=np.uint8)[None]
    if arr.shape[0] == 1:
        arr = np.repeat(arr, n_samples, axis=0)
    if arr.shape[0] != n_samples:
        raise SystemExit(f"sd_img2img.py: --init-img holds {arr.shape[0]} images; one or --n_samples {n_samples} expected")
    x = arr.astype(np.float32) / 255.0
    return torch.from_numpy(2.0 * x - 1.0).permute(0, 3, 1, 2).contiguous()


def load_prompts(opt, device):
    """-> (what get_learned_conditioning takes for the batch, for the empty prompt, T of --prompt_ids | None)."""
    if opt.prompt_ids:
        ids = np.load(opt.prompt_ids, allow_pickle=False)
        if ids.ndim != 2 or not np.issubdtype(ids.dtype, np.integer) or ids.shape[0] not in (1, opt.n_samples):
            raise SystemExit(f"sd_img2img.py: --prompt_ids must hold an integer [1 | n_samples, T] array, got {ids.dtype} {ids.shape}")
        ids = torch.from_numpy(np.repeat(ids, opt.n_samples, 0) if ids.shape[0] == 1 else ids).to(torch.int64).to(device)
        return ids, opt.n_samples * [""], ids.shape[1]
    if not opt.tokenizer_dir:
        raise SystemExit("sd_img2img.py: --prompt needs --tokenizer_dir (a local CLIP tokenizer directory); or pass token ids with --prompt_ids")
    return opt.n_samples * [opt.prompt], opt.n_samples * [""], None


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
    sched = None
    if opt.use_timestep:
        sched = np.array(sorted(int(t) for t in ast.literal_eval(opt.use_timestep)))
        if sched.shape[0] != opt.ddim_steps:
            raise SystemExit(f"sd_img2img.py: --use_timestep holds {sched.shape[0]} entries; --ddim_steps is {opt.ddim_steps}")
    random.seed(opt.seed)      # pytorch_lightning.seed_everything(opt.seed): random, numpy, torch
    np.random.seed(opt.seed)
    torch.manual_seed(opt.seed)
    logger.configure(opt.outdir)
    device = dist_util.dev()
    if device.type != "cuda":
        raise SystemExit("sd_img2img.py: no GPU is visible (the HIP path has no CPU fallback)")
    torch.cuda.set_device(device)
    init_image = load_images(opt.init_img, opt.n_samples, opt.side_multiple).to(device)
    prompts, empty, prompt_len = load_prompts(opt, device)
    opt.with_encoder = True
    model = build_model(opt, device, prompt_len=prompt_len)
    sampler = DDIMSampler(model)
    init_latent = model.get_first_stage_encoding(model.encode_first_stage(init_image))   # move to latent space
    sampler.make_schedule(ddim_num_steps=opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False, sampled_timestep=sched)
    print(f"target t_enc is {t_enc} steps")
    out = []
    for _ in range(opt.n_iter):
        uc = model.get_learned_conditioning(empty) if opt.scale != 1.0 else None
        c = model.get_learned_conditioning(prompts)
        z_enc = sampler.stochastic_encode(init_latent, torch.tensor([t_enc] * opt.n_samples))   # encode (scaled latent)
        samples = sampler.decode(z_enc, c, t_enc, unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc)
        _, u8 = ops.vae_image_out(model.decode_first_stage(samples), want_unit=False, want_u8=True)
        out.append(u8.cpu().numpy())
    arr = np.concatenate(out, axis=0)
    os.makedirs(opt.outdir, exist_ok=True)
    path = os.path.join(opt.outdir, "samples_%s.npz" % "x".join(str(v) for v in arr.shape))
    np.savez(path, arr)
    logger.log(f"saved {arr.shape[0]} images to {path}")
    return arr


if __name__ == "__main__":
    main()
