"""Factories with the reference's signatures (drop-in lower boundary).

Mirrors reference guided_diffusion/script_util.py:
``model_and_diffusion_defaults`` (:43-66), ``classifier_defaults`` (:27-40),
``create_model_and_diffusion`` (:75-130), ``create_model`` (:133-211),
``create_classifier`` (:257-295), ``create_gaussian_diffusion`` (:415-453) and the
argparse helpers (:456-481).  The returned model is the HIP engine
(``autodiffusion_amd.unet``), the diffusion is ``autodiffusion_amd.sampler.SpacedDiffusion``.
Super-resolution factories are out of scope (no search script uses them).
"""
from __future__ import annotations

import argparse

from . import dist_util, logger
from . import schedule as gd
from .evaluate import parse_int_list
from .arch import build_unet_plan
from .sampler import SpacedDiffusion
from .schedule import space_timesteps

NUM_CLASSES = 1000


def diffusion_defaults():
    return dict(
        learn_sigma=False, diffusion_steps=1000, noise_schedule="linear", timestep_respacing="",
        use_kl=False, predict_xstart=False, rescale_timesteps=False, rescale_learned_sigmas=False,
    )


def classifier_defaults():
    return dict(
        image_size=64, classifier_use_fp16=False, classifier_width=128, classifier_depth=2,
        classifier_attention_resolutions="32,16,8", classifier_use_scale_shift_norm=True,
        classifier_resblock_updown=True, classifier_pool="attention",
    )


def model_and_diffusion_defaults():
    res = dict(
        image_size=64, num_channels=128, num_res_blocks=2, num_heads=4, num_heads_upsample=-1,
        num_head_channels=-1, attention_resolutions="16,8", channel_mult="", dropout=0.0,
        class_cond=False, use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=False,
        use_fp16=False, use_new_attention_order=False, use_dynamic_unet=False,
    )
    res.update(diffusion_defaults())
    return res


def classifier_and_diffusion_defaults():
    res = classifier_defaults()
    res.update(diffusion_defaults())
    return res


def _default_channel_mult(image_size):
    table = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4),
             64: (1, 2, 3, 4), 32: (1, 2, 2, 2)}
    if image_size not in table:
        raise ValueError(f"unsupported image size: {image_size}")
    return table[image_size]


def create_model(image_size, num_channels, num_res_blocks, channel_mult="", learn_sigma=False,
                 class_cond=False, use_checkpoint=False, attention_resolutions="16", num_heads=1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, dropout=0,
                 resblock_updown=False, use_fp16=False, use_new_attention_order=False,
                 use_dynamic_unet=False):
    from .unet import UNetModel
    if channel_mult == "":
        channel_mult = _default_channel_mult(image_size)
    else:
        channel_mult = tuple(int(m) for m in channel_mult.split(","))
    attention_ds = tuple(image_size // int(res) for res in attention_resolutions.split(","))
    plan = build_unet_plan(
        image_size=image_size, in_channels=3, model_channels=num_channels,
        out_channels=(3 if not learn_sigma else 6), num_res_blocks=num_res_blocks,
        attention_resolutions=attention_ds, channel_mult=channel_mult,
        num_classes=(NUM_CLASSES if class_cond else None), num_heads=num_heads,
        num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
        use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
        use_new_attention_order=use_new_attention_order, dynamic=use_dynamic_unet)
    # dropout / use_checkpoint only matter for training; accepted and ignored at inference
    if not use_fp16:
        from .unet import warn_compute_dtype
        warn_compute_dtype("create_model", "use_fp16")
    return UNetModel(plan, use_fp16=use_fp16)


def create_gaussian_diffusion(*, steps=1000, learn_sigma=False, sigma_small=False, noise_schedule="linear",
                              use_kl=False, predict_xstart=False, rescale_timesteps=False,
                              rescale_learned_sigmas=False, timestep_respacing=""):
    betas = gd.get_named_beta_schedule(noise_schedule, steps)
    if use_kl:
        loss_type = gd.LossType.RESCALED_KL
    elif rescale_learned_sigmas:
        loss_type = gd.LossType.RESCALED_MSE
    else:
        loss_type = gd.LossType.MSE
    if not timestep_respacing:
        timestep_respacing = [steps]
    if learn_sigma:
        var_type = gd.ModelVarType.LEARNED_RANGE
    else:
        var_type = gd.ModelVarType.FIXED_SMALL if sigma_small else gd.ModelVarType.FIXED_LARGE
    return SpacedDiffusion(
        use_timesteps=space_timesteps(steps, timestep_respacing), betas=betas,
        model_mean_type=(gd.ModelMeanType.START_X if predict_xstart else gd.ModelMeanType.EPSILON),
        model_var_type=var_type, loss_type=loss_type, rescale_timesteps=rescale_timesteps)


def create_model_and_diffusion(image_size, class_cond, learn_sigma, num_channels, num_res_blocks,
                               channel_mult, num_heads, num_head_channels, num_heads_upsample,
                               attention_resolutions, dropout, diffusion_steps, noise_schedule,
                               timestep_respacing, use_kl, predict_xstart, rescale_timesteps,
                               rescale_learned_sigmas, use_checkpoint, use_scale_shift_norm,
                               resblock_updown, use_fp16, use_new_attention_order, use_dynamic_unet=False):
    model = create_model(
        image_size, num_channels, num_res_blocks, channel_mult=channel_mult, learn_sigma=learn_sigma,
        class_cond=class_cond, use_checkpoint=use_checkpoint, attention_resolutions=attention_resolutions,
        num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
        use_scale_shift_norm=use_scale_shift_norm, dropout=dropout, resblock_updown=resblock_updown,
        use_fp16=use_fp16, use_new_attention_order=use_new_attention_order,
        use_dynamic_unet=use_dynamic_unet)
    diffusion = create_gaussian_diffusion(
        steps=diffusion_steps, learn_sigma=learn_sigma, noise_schedule=noise_schedule, use_kl=use_kl,
        predict_xstart=predict_xstart, rescale_timesteps=rescale_timesteps,
        rescale_learned_sigmas=rescale_learned_sigmas, timestep_respacing=timestep_respacing)
    return model, diffusion


def create_classifier(image_size, classifier_use_fp16, classifier_width, classifier_depth,
                      classifier_attention_resolutions, classifier_use_scale_shift_norm,
                      classifier_resblock_updown, classifier_pool):
    from .classifier import EncoderUNetModel
    if image_size not in (64, 128, 256, 512):
        raise ValueError(f"unsupported image size: {image_size}")
    attention_ds = tuple(image_size // int(res) for res in classifier_attention_resolutions.split(","))
    plan = build_unet_plan(
        image_size=image_size, in_channels=3, model_channels=classifier_width, out_channels=1000,
        num_res_blocks=classifier_depth, attention_resolutions=attention_ds,
        channel_mult=_default_channel_mult(image_size), num_head_channels=64,
        use_scale_shift_norm=classifier_use_scale_shift_norm, resblock_updown=classifier_resblock_updown,
        encoder_only=True, pool=classifier_pool)
    if not classifier_use_fp16:  # the reference's default: every classifier runs fp32 (script_util.py:33)
        from .unet import warn_compute_dtype
        warn_compute_dtype("create_classifier", "classifier_use_fp16")
    return EncoderUNetModel(plan, use_fp16=classifier_use_fp16)


def load_model_and_diffusion(args, log_source=False):
    """What every script does with its parsed flags: build the UNet and the diffusion, place the model, load --model_path
    (synthetic weights without one: benchmarks, tests), fp16, eval."""
    logger.log("creating model and diffusion...")
    model, diffusion = create_model_and_diffusion(**args_to_dict(args, model_and_diffusion_defaults().keys()))
    model.to(dist_util.dev())
    if args.model_path:
        model.load_state_dict(dist_util.load_state_dict(args.model_path, map_location="cpu"))
        if log_source:
            logger.log('load from: ' + args.model_path)
    else:
        model.randomize_(1234)
    if args.use_fp16:
        model.convert_to_fp16()
    model.eval()
    return model, diffusion


def load_classifier(args, log_loading=False):
    """The guidance classifier from the parsed flags, as load_model_and_diffusion; None with --without_classifier."""
    if args.without_classifier:
        return None
    if log_loading:
        logger.log("loading classifier...")
    classifier = create_classifier(**args_to_dict(args, classifier_defaults().keys()))
    classifier.to(dist_util.dev())
    if args.classifier_path:
        classifier.load_state_dict(dist_util.load_state_dict(args.classifier_path, map_location="cpu"))
    else:
        classifier.randomize_(4321)
    classifier.eval()
    return classifier


def candidate_from_flags(args, diffusion):
    """The sampling CLIs' candidate: --use_timestep (default: the diffusion's own steps), sorted; with --skip_layers, a dict
    candidate with one skip list per step."""
    steps = sorted(diffusion.use_timesteps if args.use_timestep is None else parse_int_list(args.use_timestep, "--use_timestep"))
    if args.skip_layers is None:
        return steps
    return {"timesteps": steps, "skip_layers": parse_int_list(args.skip_layers, "--skip_layers", nested=True)}


def gather_batches(ev, args):
    """The sampling CLIs' use of CandidateEvaluator.sample_plan: every reference batch (seeded by --seed and its global index)
    all-gathered over the ranks, rank-major as the reference concatenates them -> (host image batches, host label batches);
    the caller keeps the first num_samples of their concatenation."""
    import torch as th
    import torch.distributed as dist
    world = dist_util.get_world_size()
    all_images, all_labels = [], []
    for sample, classes, _ in ev.sample_plan(args.num_samples, args.batch_size, lambda g: args.seed * 1000003 + g, world=world,
                                             rank=dist_util.get_rank(), merge_batches=int(getattr(args, "merge_batches", 0) or 0)):
        sample, classes = sample.contiguous(), classes.contiguous()
        if world > 1:
            gathered = [th.zeros_like(sample) for _ in range(world)]
            gathered_labels = [th.zeros_like(classes) for _ in range(world)]
            dist.all_gather(gathered, sample)
            dist.all_gather(gathered_labels, classes)
        else:
            gathered, gathered_labels = [sample], [classes]
        all_images.extend([s.cpu().numpy() for s in gathered])
        all_labels.extend([lab.cpu().numpy() for lab in gathered_labels])
    return all_images, all_labels


def add_dict_to_argparser(parser, default_dict):
    for k, v in default_dict.items():
        v_type = type(v)
        if v is None:
            v_type = str
        elif isinstance(v, bool):
            v_type = str2bool
        parser.add_argument(f"--{k}", default=v, type=v_type)


def args_to_dict(args, keys):
    return {k: getattr(args, k) for k in keys}


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("boolean value expected")


DPM_FLAGS = ("dpm_solver", "dpm_order", "dpm_predict_x0", "dpm_thresholding")


def add_dpm_flags(parser):
    """--dpm_solver True: a candidate's K timesteps are K evaluations of multistep DPM-Solver (autodiffusion_amd/dpm_solver.py)
    instead of DDIM / ancestral steps."""
    parser.add_argument("--dpm_solver", type=str2bool, default=False)
    parser.add_argument("--dpm_order", type=int, default=2, choices=[1, 2, 3])
    parser.add_argument("--dpm_predict_x0", type=str2bool, default=True)
    parser.add_argument("--dpm_thresholding", type=str2bool, default=False)


def dpm_kwargs(args):
    """The CandidateEvaluator keywords of the flags.  With --dpm_solver off the four attributes are removed from `args`: the
    argument line of log.txt (str(args)) stays what it was before the flags existed."""
    if getattr(args, "dpm_solver", False):
        return dict(sampler="dpm_solver", dpm_order=args.dpm_order, dpm_predict_x0=args.dpm_predict_x0,
                    dpm_thresholding=args.dpm_thresholding)
    for k in DPM_FLAGS:
        if hasattr(args, k):
            delattr(args, k)
    return {}


UNIPC_FLAGS = ("unipc", "unipc_order", "unipc_variant", "unipc_corrector", "unipc_predict_x0", "unipc_thresholding")


def add_unipc_flags(parser):
    """--unipc True: a candidate's K timesteps are K evaluations of multistep UniPC (autodiffusion_amd/unipc.py): DPM-Solver's
    candidate mapping, every update but the last arrival corrected with the model value the next update computes anyway."""
    parser.add_argument("--unipc", type=str2bool, default=False)
    parser.add_argument("--unipc_order", type=int, default=2, choices=[1, 2, 3])
    parser.add_argument("--unipc_variant", type=str, default="bh2", choices=["bh1", "bh2"])
    parser.add_argument("--unipc_corrector", type=str2bool, default=True)
    parser.add_argument("--unipc_predict_x0", type=str2bool, default=True)
    parser.add_argument("--unipc_thresholding", type=str2bool, default=False)


def unipc_kwargs(args):
    """The CandidateEvaluator keywords of the flags; with --unipc off the six attributes are removed from `args`, as dpm_kwargs
    removes its own.  Call it before dpm_kwargs: --unipc together with --dpm_solver is refused while both are still there."""
    if getattr(args, "unipc", False):
        if getattr(args, "dpm_solver", False):
            raise SystemExit("--unipc and --dpm_solver both name the sampler of a candidate: give one of them")
        return dict(sampler="unipc", unipc_order=args.unipc_order, unipc_variant=args.unipc_variant,
                    unipc_corrector=args.unipc_corrector, unipc_predict_x0=args.unipc_predict_x0,
                    unipc_thresholding=args.unipc_thresholding)
    for k in UNIPC_FLAGS:
        if hasattr(args, k):
            delattr(args, k)
    return {}
