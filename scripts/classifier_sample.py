#!/usr/bin/env python3
"""Sample an .npz image batch with a searched timestep schedule (and optional per-step layer skipping).

The on-disk format either side of the hot path, as the reference's samplers write it
(scripts/classifier_sample.py:82-205, classifier_sample_prunedUNET.py:151-213, image_sample.py:96-159):
``<save_dir>/samples_{N}x{H}x{W}x3.npz`` with ``arr_0`` = uint8 NHWC images and ``arr_1`` = int64 labels
(when class-conditional); the same flags (``--use_timestep '[153, 424, 926, 690]'``, ``--use_ddim``,
``--classifier_scale``, ``--without_classifier`` ...), plus ``--skip_layers '[[1],[],[0,5],[2,3]]'`` for
dynamic UNets.  Without ``--model_path`` / ``--classifier_path`` the networks keep synthetic weights
(benchmarks, tests).  One process per GPU: ``python -m torch.distributed.run --nproc-per-node N ...``.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autodiffusion_amd import dist_util, logger  # noqa: E402
from autodiffusion_amd.evaluate import CandidateEvaluator, parse_int_list  # noqa: E402
from autodiffusion_amd.script_util import (add_dict_to_argparser, add_dpm_flags, add_unipc_flags, candidate_from_flags,  # noqa: E402
                                           classifier_defaults, dpm_kwargs, gather_batches, load_classifier,
                                           load_model_and_diffusion, model_and_diffusion_defaults, unipc_kwargs)


def create_argparser():
    defaults = dict(
        clip_denoised=True, num_samples=10000, batch_size=16, use_ddim=False, model_path="", classifier_path="",
        save_dir="", classifier_scale=1.0, use_timestep=None, skip_layers=None, MASTER_PORT="12344", use_mean=False,
        without_classifier=False, seed=0, merge_batches=0,
    )
    defaults.update(model_and_diffusion_defaults())
    defaults.update(classifier_defaults())
    parser = argparse.ArgumentParser()
    add_dict_to_argparser(parser, defaults)
    add_dpm_flags(parser)
    add_unipc_flags(parser)
    return parser


def main(argv=None):
    t1 = time.time()
    args = create_argparser().parse_args(argv)
    dpm = {**unipc_kwargs(args), **dpm_kwargs(args)}   # one of the two at most: unipc_kwargs refuses both
    if args.use_mean and args.use_timestep is not None:   # an averaged schedule, space-separated floats: round it
        args.use_timestep = str(parse_int_list(args.use_timestep, "--use_timestep", use_mean=True))
    os.environ.setdefault("MASTER_PORT", args.MASTER_PORT)
    dist_util.setup_dist()
    logger.configure(args.save_dir or None)
    logger.log(str(args))

    model, diffusion = load_model_and_diffusion(args)
    classifier = load_classifier(args, log_loading=True)

    ev = CandidateEvaluator(model, diffusion, classifier, image_size=args.image_size, use_ddim=args.use_ddim,
                            clip_denoised=args.clip_denoised, class_cond=args.class_cond,
                            classifier_scale=args.classifier_scale, device=dist_util.dev(), **dpm)
    ev.set_candidate(candidate_from_flags(args, diffusion))

    logger.log("sampling...")
    world, rank = dist_util.get_world_size(), dist_util.get_rank()
    # --merge_batches K (0 = auto: evaluate.merge_policy -- 256 images per pass at 64x64, 128 at 128x128, 64 at 256x256): K of the reference's batches per pass over the networks -- bitwise the same
    # images (every sub-batch draws from its own generator; an image's result does not depend on the batch it rides in), with the
    # chip filled like a batch of 256 (ADM-G-128 at the launch script's batch 32: +33 % images/s)
    all_images, all_labels = gather_batches(ev, args)

    arr = np.concatenate(all_images, axis=0)[: args.num_samples]
    label_arr = np.concatenate(all_labels, axis=0)[: args.num_samples]
    out_path = None
    if rank == 0:
        shape_str = "x".join(str(x) for x in arr.shape)
        out_path = os.path.join(logger.get_dir() or ".", "samples_" + shape_str + ".npz")
        logger.log("saving to " + str(out_path))
        if args.class_cond:
            np.savez(out_path, arr, label_arr)
        else:
            np.savez(out_path, arr)
    if world > 1:
        dist.barrier()
    logger.log("sampling complete")
    logger.log("total time: " + str(time.time() - t1))
    return out_path


if __name__ == "__main__":
    main()
