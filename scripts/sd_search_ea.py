#!/usr/bin/env python3
"""Evolutionary search over Stable-Diffusion sampling schedules on the HIP evaluation path -- the reference's
"Stable Diffusion"/scripts/search_ea.py as a CLI over ``autodiffusion_amd.sd_search.EvolutionSearcher``.

The reference's flags keep their names and defaults (search_ea.py:636-848): ``--plms --dpm_solver --fixed_code --ddim_eta --H --W
--C --f --n_samples --scale --config --ckpt --seed --outdir --num_sample --max_epochs --select_num --population_num --m_prob
--crossover_num --mutation_num --max_fid --thres --ref_mu --ref_sigma --time_step --use_ddim_init_x``.  ``--use_ddim_init_x`` is
parsed by ``str2bool`` (the reference's ``type=bool`` turns the string ``False`` into True).  ``--precision --laion400m
--skip_grid --skip_save --n_iter --n_rows --prompt --ddim_steps --cal_fid --data_dir`` are accepted and ignored; one log line
names those that were given.

Additions.  Prompts: ``--captions FILE`` -- a COCO-style JSON whose ``annotations[i]['caption'].lower()`` are taken in file order,
or a text file with one caption per line -- batched ``--n_samples`` at a time with the last short batch dropped (what the
reference's ``CocoDataset`` + ``DataLoader(shuffle=False, drop_last=True)`` feed), tokenised by the ``transformers`` tokenizer in
the LOCAL directory ``--tokenizer_dir`` (nothing is fetched); or ``--prompt_ids FILE.npy``, an int64 [num, T] array of token ids,
when no tokenizer is at hand (the empty prompt of classifier-free guidance is then built from the vocabulary's last two ids,
CLIP's start- and end-of-text).  FID: ``--inception_path`` is the pytorch_fid checkpoint; without it the run needs
``--allow_random_inception``, and every FID line then carries the "RANDOM Inception weights" note.  ``--ref_mu`` / ``--ref_sigma``
take the reference's ``.npy`` pair; ``--ref_mu`` alone may name an ``.npz`` holding ``mu`` and ``sigma`` (what
``scripts/evaluator.py --save_ref_stats`` writes).  ``--fitness kid --ref_feats FILE.npz`` ranks candidates by 1000 x the unbiased
cubic-kernel MMD^2 (KID, autodiffusion_amd/kid.py) against the rows ``feats`` of FILE.npz (``scripts/evaluator.py --save_ref_feats``)
instead; the fitness lines then carry "[fitness: KID x 1e3]" and ``--ref_mu`` / ``--ref_sigma`` are not read.
``--fitness cmmd --ref_clip_feats FILE.npz --clip_ckpt CLIP.pt`` ranks them by 1000 x the unbiased RBF-kernel MMD^2 of their CLIP
image embeddings (CMMD, autodiffusion_amd/cmmd.py) against the rows ``clip_feats`` of FILE.npz (``scripts/sd_clip_score.py
--save_clip_feats``); the lines carry "[fitness: CMMD x 1e3 (unbiased)]", no Inception network is built, and ``--ref_mu`` /
``--ref_sigma`` / ``--inception_path`` are not read; without ``--population_parallel`` the batches of a candidate are sharded over
the ranks and the embedding rows pooled.  ``--torso {bf16,fp16}`` selects the 16-bit torso; ``--population_parallel``
shards whole candidates over ranks (candidate i on rank i % world, one all_gather of the FIDs per epoch).
``--clip_ckpt PATH`` also scores every candidate's images against their prompts (``sd_clip.CLIPScorer``, a ``CLIP score:`` log line
per candidate; the fitness stays the FID): PATH is ONE plain state dict holding both CLIP towers, in transformers' ``CLIPModel``
layout or the OpenAI layout, read with ``dist_util.load_state_dict`` (ViT-L/14; under ``--synthetic tiny`` the tiny towers).
``--evaluate "[t0, t1, ...]"`` scores that one candidate over ``--num_sample`` images, prints the FID and exits (the reference's
txt2img_fid.py use of a searched schedule).  ``--synthetic {tiny,v1,tiny2,v2}`` (tiny2 / v2: the v-predicting SD 2.x family) builds the networks with ``randomize_()`` instead of
reading ``--ckpt``: tests and throughput runs.
``--use_dynamic_unet True --max_prun F --min_prun F [--index_step N]`` (scripts/search_ea.py's names and meaning) runs the joint search
over timesteps and per-step layer-skip lists of the latent UNet (``sd_search.DynamicEvolutionSearcher``; DDIM / PLMS
only); its candidates are ``{'timesteps': [...], 'skip_layers': [[ids], ...]}``, which ``--evaluate`` takes too.

Loading: ``--ckpt`` is read with ``torch.load(map_location="cpu")`` and its ``"state_dict"`` (or the dict itself) goes through
``LatentDiffusion.load_state_dict``.  ``--config``, when given, is read with PyYAML and supplies ``model.params.{timesteps,
linear_start, linear_end, scale_factor}`` and the ``params`` of ``unet_config``, ``first_stage_config`` and ``cond_stage_config``;
without it the SD-v1 constants of the package are used.

``OUTDIR/log.txt`` gets the reference's lines: the ``population_num = ...`` header, ``epoch = e``, ``epoch = e : top n result``,
``No.i cand fid = v`` and ``total searching time = ... hours`` (ranks > 0 write ``log-rankNNN.txt``).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autodiffusion_amd import dist_util, logger  # noqa: E402
from autodiffusion_amd.script_util import str2bool  # noqa: E402
from autodiffusion_amd.sd_script_util import (TINY_CLIP, TINY_UNET, TINY_VAE, EmptyPromptTokenizer, add_unipc_flags,  # noqa: E402,F401
                                              add_skip_search_flags, build_clip_scorer, build_inception, build_model, build_sampler,
                                              read_captions, read_prompt_ids, require_cmmd_flags, require_gpu, seed_everything,
                                              skip_search_options, unipc_options)
from autodiffusion_amd.sd_search import DynamicEvolutionSearcher, EvolutionSearcher, dpm_search_params, parse_sd_candidate  # noqa: E402

IGNORED = ("precision", "laion400m", "skip_grid", "skip_save", "n_iter", "n_rows", "prompt", "ddim_steps", "cal_fid", "data_dir")


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # ---- the reference's flags (search_ea.py:636-848)
    p.add_argument("--outdir", type=str, nargs="?", help="dir to write results to", default="outputs/txt2img-samples")
    p.add_argument("--plms", action="store_true", help="use plms sampling")
    p.add_argument("--dpm_solver", action="store_true", help="use dpm_solver sampling")
    p.add_argument("--fixed_code", action="store_true", help="if enabled, uses the same starting code across samples")
    p.add_argument("--ddim_eta", type=float, default=0.0, help="ddim eta (eta=0.0 corresponds to deterministic sampling)")
    p.add_argument("--H", type=int, default=512, help="image height, in pixel space")
    p.add_argument("--W", type=int, default=512, help="image width, in pixel space")
    p.add_argument("--C", type=int, default=4, help="latent channels")
    p.add_argument("--f", type=int, default=8, help="downsampling factor")
    p.add_argument("--n_samples", type=int, default=3, help="how many samples to produce for each given prompt. A.k.a. batch size")
    p.add_argument("--scale", type=float, default=7.5,
                   help="unconditional guidance scale: eps = eps(x, empty) + scale * (eps(x, cond) - eps(x, empty))")
    p.add_argument("--config", type=str, default="configs/stable-diffusion/v1-inference.yaml",
                   help="path to config which constructs model (read when the file exists; else the SD-v1 constants)")
    p.add_argument("--ckpt", type=str, default="models/ldm/stable-diffusion-v1/model.ckpt", help="path to checkpoint of model")
    p.add_argument("--seed", type=int, default=42, help="the seed (for reproducible sampling)")
    p.add_argument("--num_sample", type=int, default=4, help="samples num")
    p.add_argument("--max_epochs", type=int, default=10)
    p.add_argument("--select_num", type=int, default=10)
    p.add_argument("--population_num", type=int, default=50)
    p.add_argument("--m_prob", type=float, default=0.1)
    p.add_argument("--crossover_num", type=int, default=25)
    p.add_argument("--mutation_num", type=int, default=25)
    p.add_argument("--max_fid", type=float, default=3.)
    p.add_argument("--thres", type=float, default=0.2)
    p.add_argument("--ref_mu", type=str, default="", help="reference mean (.npy), or an .npz holding mu and sigma")
    p.add_argument("--ref_sigma", type=str, default="", help="reference covariance (.npy)")
    p.add_argument("--fitness", default="fid", choices=["fid", "kid", "cmmd"],
                   help="what ranks a candidate: the Frechet distance, 1000 x the unbiased cubic-kernel MMD^2 (autodiffusion_amd/kid.py), "
                        "or 1000 x the unbiased RBF-kernel MMD^2 of the CLIP image embeddings (autodiffusion_amd/cmmd.py)")
    p.add_argument("--ref_feats", type=str, default="",
                   help="--fitness kid: .npz with `feats` fp32 [m, 2048] (scripts/evaluator.py --save_ref_feats)")
    # absent from the namespace unless given: log.txt's argument line of every other run stays what it was
    p.add_argument("--ref_clip_feats", type=str, default=argparse.SUPPRESS,
                   help="--fitness cmmd: .npz with `clip_feats` fp32 [m, E] (scripts/sd_clip_score.py --save_clip_feats)")
    p.add_argument("--time_step", type=int, default=50)
    p.add_argument("--use_ddim_init_x", type=str2bool, default=False,
                   help="seed the population with the evenly spaced schedule; parsed as a boolean word (true/false/1/0/...): "
                        "the reference's type=bool turns the string 'False' into True, this flag does not")
    # ---- accepted and ignored
    p.add_argument("--prompt", type=str, nargs="?", default=None, help="ignored (the prompts come from --captions / --prompt_ids)")
    p.add_argument("--skip_grid", action="store_true", default=None, help="ignored")
    p.add_argument("--skip_save", action="store_true", default=None, help="ignored")
    p.add_argument("--ddim_steps", type=int, default=None, help="ignored (--time_step is the number of steps)")
    p.add_argument("--laion400m", action="store_true", default=None, help="ignored")
    p.add_argument("--n_iter", type=int, default=None, help="ignored")
    p.add_argument("--n_rows", type=int, default=None, help="ignored")
    p.add_argument("--precision", type=str, choices=["full", "autocast"], default=None, help="ignored (see --torso)")
    p.add_argument("--data_dir", type=str, default=None, help="ignored (see --captions)")
    p.add_argument("--cal_fid", type=str, default=None, help="ignored")
    # ---- additions
    p.add_argument("--captions", type=str, default="", help="COCO-style annotations JSON, or a text file with one caption per line")
    p.add_argument("--tokenizer_dir", type=str, default="", help="LOCAL directory of the transformers CLIP tokenizer (nothing is fetched)")
    p.add_argument("--prompt_ids", type=str, default="",
                   help=".npy int64 [num, T] token ids; replaces --captions and --tokenizer_dir (the empty prompt of classifier-free "
                        "guidance is then T ids: start-of-text, then end-of-text, the last two ids of the vocabulary)")
    p.add_argument("--inception_path", type=str, default="", help="the pytorch_fid Inception checkpoint (pt_inception-2015-12-05)")
    p.add_argument("--allow_random_inception", action="store_true",
                   help="run without --inception_path: every FID line is then tagged as computed on RANDOM Inception weights")
    p.add_argument("--torso", choices=["bf16", "fp16"], default="bf16", help="16-bit type of activations and weights between kernels")
    p.add_argument("--population_parallel", action="store_true", help="evaluate candidate i on rank i %% world, one all_gather per epoch")
    p.add_argument("--clip_ckpt", type=str, default="",
                   help="a CLIP state dict (both towers, CLIPModel or OpenAI layout): also log every candidate's CLIP score")
    p.add_argument("--evaluate", type=str, default="", help="'[t0, t1, ...]': score this one candidate, print its FID and exit")
    p.add_argument("--synthetic", choices=["tiny", "v1", "tiny2", "v2"], default="",
                   help="build the networks with randomize_() instead of reading --ckpt (tiny2 / v2: the SD 2.x family, v-prediction)")
    add_unipc_flags(p)
    add_skip_search_flags(p)
    return p


# ------------------------------------------------------------------ prompts
def batch_captions(captions, n_samples):
    """DataLoader(batch_size=n_samples, shuffle=False, drop_last=True) (build_dataloader.py:66-73): batches of {'text': [...]}."""
    return [{"text": list(captions[i:i + n_samples])} for i in range(0, len(captions) - n_samples + 1, n_samples)]


def build_loader(opt, device):
    if opt.prompt_ids:
        ids = read_prompt_ids(opt.prompt_ids, "sd_search_ea.py").to(device)
        loader = [{"text": ids[i:i + opt.n_samples]} for i in range(0, ids.shape[0] - opt.n_samples + 1, opt.n_samples)]
    elif opt.captions:
        if not opt.tokenizer_dir:
            raise SystemExit("sd_search_ea.py: --captions needs --tokenizer_dir (a local CLIP tokenizer directory); "
                             "or pass token ids with --prompt_ids")
        loader = batch_captions(read_captions(opt.captions), opt.n_samples)
    else:
        raise SystemExit("sd_search_ea.py: give --captions FILE (with --tokenizer_dir DIR) or --prompt_ids FILE.npy")
    if not loader:
        raise SystemExit(f"sd_search_ea.py: fewer prompts than one batch of --n_samples {opt.n_samples}")
    return loader


# ------------------------------------------------------------------ reference statistics
def load_ref_stats(opt):
    if opt.ref_mu.endswith(".npz") and not opt.ref_sigma:
        z = np.load(opt.ref_mu, allow_pickle=False)
        return np.asarray(z["mu"], dtype=np.float64), np.asarray(z["sigma"], dtype=np.float64)
    if not opt.ref_mu or not opt.ref_sigma:
        raise SystemExit("sd_search_ea.py: give --ref_mu MU.npy --ref_sigma SIGMA.npy, or --ref_mu STATS.npz holding mu and sigma")
    return (np.asarray(np.load(opt.ref_mu, allow_pickle=False), dtype=np.float64),
            np.asarray(np.load(opt.ref_sigma, allow_pickle=False), dtype=np.float64))


def main(argv=None, *, evaluator=None):
    """Returns the searcher after a search, or the FID under --evaluate.  ``evaluator=`` injects a candidate evaluator (an
    object with ``get_cand_fid(cand, opt)``) in place of the networks: host tests of the command line."""
    opt = create_argparser().parse_args(argv)
    unipc = unipc_options(opt, "sd_search_ea.py") is not None   # refuses --unipc beside --dpm_solver / --plms
    continuous = opt.dpm_solver or unipc                        # a candidate is time_step + 1 continuous times
    joint = skip_search_options(opt, "sd_search_ea.py")         # (max_prun, min_prun, index_step): timesteps and layer-skip lists
    fitness, ref_feats = opt.fitness, opt.ref_feats
    if fitness == "kid" and not ref_feats:
        raise SystemExit("sd_search_ea.py: --fitness kid needs --ref_feats FILE.npz (scripts/evaluator.py --save_ref_feats writes it)")
    ref_clip_feats = getattr(opt, "ref_clip_feats", "")
    if fitness == "cmmd":
        require_cmmd_flags(opt, "sd_search_ea.py")
    if fitness == "fid" and not ref_feats:
        # the defaults leave no trace: log.txt's argument line (str(opt) below) stays what it was before the two flags existed
        del opt.fitness, opt.ref_feats
    ignored = [k for k in IGNORED if getattr(opt, k) is not None]
    seed_everything(opt.seed)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        dist_util.setup_dist()
    logger.configure(opt.outdir)
    logger.log(str(opt))
    if ignored:
        logger.log("ignored flags (accepted for the reference's command lines, unused on this path): "
                   + ", ".join("--" + k for k in ignored))
    ref_mu, ref_sigma = load_ref_stats(opt) if fitness == "fid" else (None, None)
    model = sampler = inception = clip_scorer = None
    dpm_params = None
    if evaluator is None:
        device = require_gpu("sd_search_ea.py")
        loader = build_loader(opt, device)
        ids = loader[0]["text"]
        model = build_model(opt, device, prompt_len=ids.shape[1] if torch.is_tensor(ids) else None)
        sampler = build_sampler(opt, model)
        inception = build_inception(opt, device) if fitness != "cmmd" else None
        if opt.clip_ckpt:
            clip_scorer = build_clip_scorer(opt, device, prompt_len=ids.shape[1] if torch.is_tensor(ids) else None)
        alphas_cumprod = model.alphas_cumprod
    else:
        loader = []
        sampler = type("Sampler", (), {"ddpm_num_timesteps": 1000})()
        alphas_cumprod = range(1000)
    if continuous:
        dpm_params = dpm_search_params(alphas_cumprod, opt.time_step)
    t = time.time()
    # the joint search: search.py's dynamic searcher over this path's evaluator (an injected evaluator names the UNet's layer count)
    extra = {} if joint is None else dict(index_step=joint[2], layer_num=getattr(evaluator, "layer_num", None))
    searcher_cls = EvolutionSearcher if joint is None else DynamicEvolutionSearcher
    searcher = searcher_cls(opt=opt, model=model, time_step=opt.time_step, ref_mu=ref_mu, ref_sigma=ref_sigma, sampler=sampler,
                                 dataloader_info={"validation_loader": loader}, batch_size=opt.n_samples, dpm_params=dpm_params,
                                 evaluator=evaluator, population_parallel=opt.population_parallel, inception=inception,
                                 allow_random_inception=opt.allow_random_inception, clip_scorer=clip_scorer, fitness=fitness,
                                 ref_feats=ref_feats or None, ref_clip_feats=ref_clip_feats or None, **extra)
    if opt.evaluate:
        try:
            cand = parse_sd_candidate(opt.evaluate, "--evaluate")
        except ValueError as e:
            raise SystemExit(f"sd_search_ea.py: {e}") from e
        want = opt.time_step + (1 if continuous else 0)
        if isinstance(cand, dict):
            if continuous:
                raise SystemExit("sd_search_ea.py: --evaluate: a {'timesteps', 'skip_layers'} candidate is for DDIM / PLMS, not "
                                 "--dpm_solver / --unipc")
        elif len(cand) != want:
            raise SystemExit(f"sd_search_ea.py: --evaluate holds {len(cand)} entries; --time_step {opt.time_step} "
                             f"{'with --dpm_solver / --unipc ' if continuous else ''}needs {want}")
        fid = searcher.get_cand_fid(cand=cand, opt=opt)
        logger.log('cand: {}, fid: {}'.format(cand, fid) + searcher.fid_note)
        return fid
    searcher.search()
    logger.log('total searching time = {:.2f} hours'.format((time.time() - t) / 3600))
    return searcher


if __name__ == "__main__":
    main()
