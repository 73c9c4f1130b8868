#!/usr/bin/env python3
"""CLIP score of a sample file against its prompts, on the HIP path.

    sd_clip_score.py SAMPLES.npz --clip_ckpt CLIP.pt (--prompt_ids IDS.npy | --captions FILE --tokenizer_dir DIR)

``SAMPLES.npz`` holds uint8 images ``arr_0`` [N, H, W, 3] (what the sampling scripts write as ``samples_*.npz``); image i is scored
against prompt i: row i of the int64 [num >= N, T] array ``--prompt_ids``, or caption i of ``--captions`` (a COCO-style JSON or one
caption per line) tokenised by the ``transformers`` tokenizer in the LOCAL directory ``--tokenizer_dir``.  ``--clip_ckpt`` is ONE
plain state dict holding both CLIP ViT-L/14 towers, in transformers' ``CLIPModel`` layout or the OpenAI ``clip`` package's, read
with ``dist_util.load_state_dict``; nothing is fetched.

The score is this project's (``sd_clip.CLIPScorer``; the reference has no CLIP-score script): 100 * mean(max(cos_i, 0)) with
cos_i the cosine of ``encode_image`` of image i -- behind the reference embedder's bicubic resize to 224 -- and ``encode_text`` of
prompt i.  ``--synthetic tiny`` builds the tiny towers with random weights instead of reading ``--clip_ckpt``: tests.

CMMD (``autodiffusion_amd/cmmd.py``: 1000 x the RBF-kernel MMD^2 of L2-normalised CLIP image embeddings, Jayasumana et al. 2024, on the
224-pixel ViT-L/14 tower of this checkpoint -- comparable between runs of this project, not with the paper's 336-pixel tables):
``--save_clip_feats OUT.npz`` writes the file's image embeddings (``clip_feats`` fp32 [N, E]; run it on an .npz of real images to make
the reference), ``--ref_clip_feats REF.npz`` appends a ``CMMD: <value>`` line against such a file.  With either flag and no prompts
the CLIP score is skipped.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autodiffusion_amd import cmmd, dist_util, sd_clip  # noqa: E402
from autodiffusion_amd.evaluator import iter_npz_batches  # noqa: E402
from autodiffusion_amd.sd_script_util import read_captions, read_prompt_ids, require_gpu, save_clip_feats  # noqa: E402


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("samples", help="npz with uint8 images arr_0 [N, H, W, 3]")
    p.add_argument("--clip_ckpt", type=str, default="", help="a CLIP state dict holding both towers (CLIPModel or OpenAI layout)")
    p.add_argument("--prompt_ids", type=str, default="", help=".npy with an int64 [num, T] array of token ids")
    p.add_argument("--captions", type=str, default="", help="COCO-style annotations JSON, or a text file with one caption per line")
    p.add_argument("--tokenizer_dir", type=str, default="", help="LOCAL directory of the transformers CLIP tokenizer")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--torso", choices=["bf16", "fp16"], default="bf16")
    p.add_argument("--synthetic", choices=["tiny"], default="", help="random tiny towers instead of --clip_ckpt")
    # absent from the namespace unless given
    p.add_argument("--ref_clip_feats", type=str, default=argparse.SUPPRESS,
                   help=".npz with `clip_feats` fp32 [m, E] (--save_clip_feats of a file of real images): also print CMMD against it")
    p.add_argument("--save_clip_feats", type=str, default=argparse.SUPPRESS,
                   help="write this file's image embeddings as `clip_feats` fp32 [N, E] to this .npz")
    return p


def main(argv=None):
    """Returns the CLIP score; with --ref_clip_feats the CMMD; None where neither was computed."""
    opt = create_argparser().parse_args(argv)
    ref_path, save_path = getattr(opt, "ref_clip_feats", ""), getattr(opt, "save_clip_feats", "")
    want_feats = bool(ref_path or save_path)
    with_prompts = bool(opt.prompt_ids or opt.captions) or not want_feats
    if with_prompts and bool(opt.prompt_ids) == bool(opt.captions):
        raise SystemExit("sd_clip_score.py: give exactly one of --prompt_ids IDS.npy and --captions FILE")
    if opt.captions and not opt.tokenizer_dir:
        raise SystemExit("sd_clip_score.py: --captions needs --tokenizer_dir (a local CLIP tokenizer directory)")
    if not opt.synthetic and not opt.clip_ckpt:
        raise SystemExit("sd_clip_score.py: give --clip_ckpt (or --synthetic tiny)")
    device = require_gpu("sd_clip_score.py")
    ref_rows = cmmd.load_ref_clip_feats(ref_path) if ref_path else None
    if not with_prompts:
        prompts, max_length = None, 77
    elif opt.prompt_ids:
        prompts = read_prompt_ids(opt.prompt_ids, "sd_clip_score.py")
        max_length = int(prompts.shape[1])
    else:
        prompts, max_length = read_captions(opt.captions), 77
    tiny = opt.synthetic == "tiny"
    scorer = sd_clip.build_clip_scorer(None if tiny else dist_util.load_state_dict(opt.clip_ckpt),
                                       sd_clip.CLIP_TINY_VISION if tiny else None, sd_clip.CLIP_TINY_TEXT_PROJ if tiny else None,
                                       device=device, torso=opt.torso, tokenizer_dir=opt.tokenizer_dir or None, max_length=max_length)
    if tiny:
        print("--synthetic tiny: the towers hold RANDOM weights; the score below is not a quality metric")
    t0, done, cosines, embeds = time.time(), 0, [], []
    for batch in iter_npz_batches(opt.samples, "arr_0", opt.batch_size):
        if batch.ndim != 4 or batch.shape[3] != 3 or batch.dtype != np.uint8:
            raise SystemExit(f"sd_clip_score.py: arr_0 must hold uint8 [N, H, W, 3] images, got {batch.dtype} {batch.shape}")
        n = batch.shape[0]
        if with_prompts and done + n > len(prompts):
            raise SystemExit(f"sd_clip_score.py: {len(prompts)} prompts for more than {done + n - 1} images")
        images = torch.from_numpy(np.ascontiguousarray(batch)).to(device)
        if not want_feats:
            cosines.append(scorer.cosine(images, prompts[done:done + n]))
        elif with_prompts:                       # one tower pass for both
            cos, emb = scorer.cosine_and_embeds(images, prompts[done:done + n])
            cosines.append(cos)
            embeds.append(emb)
        else:
            embeds.append(scorer.embeds(images))
        done += n
    if not done:
        raise SystemExit("sd_clip_score.py: the sample file holds no image")
    score = None
    if with_prompts:
        cos = torch.cat(cosines)
        score = scorer.score_of(cos)
        print(f"images: {done}, mean cosine: {float(cos.double().mean()):.6f}, time: {time.time() - t0:.2f} s")
        print(f"CLIP score: {score}")
    else:
        print(f"images: {done}, no prompts given: the CLIP score is skipped, time: {time.time() - t0:.2f} s")
    if not want_feats:
        return score
    rows = torch.cat(embeds, 0)
    value = None
    if ref_rows is not None:
        value = cmmd.CMMDReference(ref_rows, device=device).cmmd(rows)
        print(f"CMMD: {value}")
    if save_path:
        save_clip_feats(save_path, rows.cpu().numpy())
        print(f"saved {rows.shape[0]} image embeddings [{rows.shape[0]}, {rows.shape[1]}] to {save_path}")
    return score if value is None else value


if __name__ == "__main__":
    main()
