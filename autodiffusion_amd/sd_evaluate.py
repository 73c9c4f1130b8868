"""Score one Stable-Diffusion candidate on decoded images: sampler -> VAE decoder -> [0, 1] images -> extractor -> FID.

The body of the reference's ``EvolutionSearcher.get_cand_fid`` ("Stable Diffusion"/scripts/search_ea.py:504-566) on the HIP
parts: ``sd_sampler`` (UNet + sampler with ``sampled_timestep``), ``sd_vae`` (``decode_first_stage``), ``adm_vae_image_out``
(the clamp expression of :540), ``inception.InceptionV3`` (pytorch_fid's extractor) and ``fid.ActivationAccumulator``.
Between the sampler's output and the float64 statistics every step is a libadm_hip.so launch: no torch compute op, no host copy
of an image (the reference moves every batch to the host and back, :541-549).

Kept from the reference: one sampler call per batch of the conditioning iterable; batches are collected until
``len(samples) > num_samples`` (strict: :553) and ALL collected samples are scored; the extractor sees them 320 at a time
(``calculate_fid(..., batch_size=320)``, :561); with ``opt.fixed_code`` one start code is drawn per call and reused for every
batch (:506-508, :537); the ``sample_time`` / ``fid_time`` log line (:565).

The first line of the reference loop, ``c = model.get_learned_conditioning(prompts)`` (:520-526), runs here too when the evaluator
is fed ``prompts=`` (``sd_clip.FrozenCLIPEmbedder`` as the model's cond stage); ``conditioning=`` keeps taking precomputed
``(c, uc)`` embeddings.

Different by design: the empty prompt of classifier-free guidance is encoded once per evaluator, not once per batch (the encoder
is deterministic, so the value is the same), and the start noise always comes from a CPU generator seeded from (seed, candidate,
batch index) and is passed as ``x_T`` -- a candidate's score does not depend on what was evaluated before it.

A candidate is a timestep list or, with per-step layer skipping, ``{'timesteps': [...], 'skip_layers': [[ids], ...]}``
as ``evaluate.py`` / ``search.py`` carry it on the ADM path: ``skip_layers[i]`` names the UNet layers (``sd_arch`` ids) that every
evaluation at ``timesteps[i]`` bypasses.  Its start noise is seeded from its timesteps alone, so candidates that differ only in
their skip lists share their noise and a dict of empty lists scores bitwise what the plain list scores.
"""
from __future__ import annotations

import time
import zlib

import numpy as np
import torch

from . import logger, ops
from ._lib import AdmError
from .fid import ActivationAccumulator, FIDStatistics

FID_BATCH = 320   # the reference's calculate_fid(batch_size=320)


def candidate_seed(seed: int, cand) -> int:
    """Base seed of a candidate's start noise (search.py: seed * 1000003 + crc32(str(cand)))."""
    key = str([t.item() if hasattr(t, "item") else t for t in cand])
    return (int(seed) * 1000003 + zlib.crc32(key.encode())) & 0x7FFFFFFF


def batch_seed(seed0: int, batch: int) -> int:
    return seed0 + 7919 * int(batch)


def inception_features(net, dims: int = 2048, allow_random: bool = False):
    """The default extractor: ``InceptionV3.forward`` on float [N, 3, H, W] images in [0, 1] -> fp32 [N, dims]."""
    if not getattr(net, "weights_loaded", False) and not allow_random:
        raise ValueError("SDCandidateEvaluator: the Inception-v3 extractor has no checkpoint loaded: FID values on random weights "
                         "are meaningless; pass allow_random_inception=True for throughput runs and tests")

    def features(images):
        pred = net(images)[0]
        if pred.shape[2] != 1 or pred.shape[3] != 1:
            raise AdmError(f"SDCandidateEvaluator: the extractor's block returns {tuple(pred.shape[2:])} maps; use the pooled block")
        return pred.reshape(pred.shape[0], pred.shape[1])
    features.random_weights = not getattr(net, "weights_loaded", False)
    features.dims = dims
    return features


class SDCandidateEvaluator:
    def __init__(self, model, sampler, conditioning=None, ref_mu=None, ref_sigma=None, num_samples: int = None, *, prompts=None,
                 features=None, inception=None, dims: int = 2048, allow_random_inception: bool = False, seed: int = 0,
                 device=None, image_out=None, accumulator=None, clip_scorer=None, fitness: str = "fid", ref_feats=None,
                 ref_clip_feats=None, cmmd_sigma: float = 10.0, image_sharded: bool = False):
        """model: ``sd_sampler.LatentDiffusion`` with a first stage (``decode_first_stage``); sampler: one of the
        ``sd_sampler`` samplers around it; conditioning: iterable of per-batch ``(c, uc)`` device tensors (``uc`` may be None
        when ``opt.scale == 1``), re-iterated by every call; prompts (instead of conditioning; the model then needs a cond
        stage): iterable of per-batch prompts -- a list or tuple of strings, or an integer tensor [n_samples, T] of token ids --
        encoded by ``model.get_learned_conditioning``; features: callable float [N, 3, H, W] in [0, 1] -> [N, dims]
        (default: ``inception`` -- an ``InceptionV3`` -- through ``inception_features``).
        image_out / accumulator: the clamp launch and the statistics sink, replaceable for host-only tests of the batch plan.
        clip_scorer (with prompts= only): an ``sd_clip.CLIPScorer`` -- anything with ``cosine(images, prompts) -> [N]`` and
        ``score_of(cosines)``; every batch's clamped [0, 1] images, the ones the extractor sees, are also scored against that batch's
        prompts: ``last_clip`` = {"score", "cosines", "clip_time"} (clip_time: wall time inside the scorer's calls, which are part of
        sample_time and begin by waiting for the batch's images).  The FID does not change by a bit.
        fitness="kid" with ref_feats= (fp32 rows [m, dims], an array or the .npz of scripts/evaluator.py --save_ref_feats): the value
        returned is ``kid.KIDReference.fitness`` of the candidate's activation rows -- 1000 x the unbiased cubic-kernel MMD^2 -- and the
        log line says so; ref_mu / ref_sigma are then not needed.
        fitness="cmmd" with ref_clip_feats= (fp32 CLIP image embeddings [m, E], an array or the .npz of scripts/sd_clip_score.py
        --save_clip_feats) and clip_scorer= (it also needs ``cosine_and_embeds(images, prompts) -> ([N], [N, E])``): the value returned
        is ``cmmd.CMMDReference.fitness`` of the candidate's image embeddings -- 1000 x the unbiased RBF-kernel MMD^2 on the normalised
        embeddings -- kept on the device batch by batch from the scorer's one tower pass.  No extractor is built or run (``features``
        is None) and no statistics are accumulated; fid_time is the two kernel sums.  image_sharded (this fitness only): under a
        process group whose collectives are on, rank r samples the batches r, r + world, ... (the start noise is a function of the
        batch index, not of the rank) and the rows are pooled over the ranks (``kid.pooled_rows``); False -- the population-parallel
        search -- keeps every batch and every row on this rank."""
        if (conditioning is None) == (prompts is None):
            raise ValueError("SDCandidateEvaluator: pass exactly one of conditioning= (precomputed (c, uc) batches) and prompts=")
        if clip_scorer is not None and prompts is None:
            raise ValueError("SDCandidateEvaluator: clip_scorer= scores images against their prompts: pass prompts=, not conditioning=")
        self.clip_scorer, self.last_clip = clip_scorer, None
        if fitness not in ("fid", "kid", "cmmd"):
            raise ValueError(f"SDCandidateEvaluator: fitness {fitness!r}: expected 'fid' or 'kid', or 'cmmd'")
        self.fitness, self.kid_ref, self.last_rows = fitness, None, None
        self.cmmd_ref, self.cmmd_sigma, self.image_sharded = None, float(cmmd_sigma), bool(image_sharded) and fitness == "cmmd"
        if fitness == "kid":
            if ref_feats is None or (isinstance(ref_feats, str) and not ref_feats) or num_samples is None:
                raise ValueError("SDCandidateEvaluator: fitness='kid' needs ref_feats= (rows or an .npz with `feats`) and num_samples")
            if isinstance(ref_feats, str):
                from .kid import load_ref_feats
                ref_feats = load_ref_feats(ref_feats)
            self._ref_feats = ref_feats
        elif fitness == "cmmd":
            if ref_clip_feats is None or (isinstance(ref_clip_feats, str) and not ref_clip_feats) or num_samples is None:
                raise ValueError("SDCandidateEvaluator: fitness='cmmd' needs ref_clip_feats= (rows or an .npz with `clip_feats`) and "
                                 "num_samples")
            if clip_scorer is None or not hasattr(clip_scorer, "cosine_and_embeds"):
                raise ValueError("SDCandidateEvaluator: fitness='cmmd' needs clip_scorer= (an sd_clip.CLIPScorer: its image tower "
                                 "produces the embeddings CMMD is computed on)")
            if isinstance(ref_clip_feats, str):
                from .cmmd import load_ref_clip_feats
                ref_clip_feats = load_ref_clip_feats(ref_clip_feats)
            self._ref_clip_feats = ref_clip_feats
        elif ref_mu is None or ref_sigma is None or num_samples is None:
            raise ValueError("SDCandidateEvaluator: ref_mu, ref_sigma and num_samples are required")
        self.model, self.sampler, self.conditioning, self.prompts = model, sampler, conditioning, prompts
        self._uc = {}            # n_samples -> the encoded empty prompt
        self.ref_stats = (FIDStatistics(np.asarray(ref_mu, dtype=np.float64), np.asarray(ref_sigma, dtype=np.float64))
                          if ref_mu is not None and ref_sigma is not None else None)
        self.num_samples, self.seed, self.dims = int(num_samples), int(seed), int(dims)
        self.device = torch.device(device) if device is not None else getattr(model, "device", torch.device("cpu"))
        if fitness == "cmmd":
            features = None          # CMMD needs no Inception pass: no extractor is built, none runs
        elif features is None:
            if inception is None:
                raise ValueError("SDCandidateEvaluator: pass features= (a callable) or inception= (an InceptionV3)")
            features = inception_features(inception, dims, allow_random_inception)
        self.features = features
        self.fid_note = (" [FID on RANDOM Inception weights: not a quality metric]"
                         if getattr(features, "random_weights", False) else "")
        if fitness == "cmmd":
            self.fid_note += " [fitness: CMMD x 1e3 (unbiased)]"
        self._image_out = image_out or (lambda x, out: ops.vae_image_out(x, unit_out=out)[0])
        if fitness == "kid":
            self.fid_note += " [fitness: KID x 1e3]"
        # KID works from the rows themselves: keep every one (the last batch may carry the count past num_samples)
        keep = (1 << 30) if fitness == "kid" else 0
        self._accumulator = accumulator or (lambda: ActivationAccumulator(self.dims, self.device, keep_rows=keep))
        self.last_times = None
        self.last_plan = None    # [(batch index, noise seed)] of the last call

    # ------------------------------------------------------------------ start noise
    def start_code(self, opt, seed: int):
        """fp32 [n_samples, C, H / f, W / f] from a CPU generator (device-independent), moved to the evaluator's device."""
        g = torch.Generator().manual_seed(int(seed))
        x = torch.randn([opt.n_samples, opt.C, opt.H // opt.f, opt.W // opt.f], generator=g, dtype=torch.float32)
        return x.to(self.device)

    def _shard(self):
        """(world, rank) of the image-sharded CMMD evaluation; (1, 0) everywhere else: every batch is this rank's."""
        from . import dist_util
        if self.image_sharded and dist_util.collectives_on():
            return dist_util.get_world_size(), dist_util.get_rank()
        return 1, 0

    # ------------------------------------------------------------------ search_ea.py:520-526
    def _batches(self, opt):
        """Per-batch (c, uc, prompts | None): the conditioning iterable as it is, or the prompts through the model's cond stage."""
        if self.prompts is None:
            for c, uc in self.conditioning:
                yield c, uc, None
            return
        for prompts in self.prompts:
            uc = None
            if opt.scale != 1.0:
                uc = self._uc.get(opt.n_samples)
                if uc is None:
                    uc = self._uc[opt.n_samples] = self.model.get_learned_conditioning(opt.n_samples * [""])
            if isinstance(prompts, tuple):
                prompts = list(prompts)
            yield self.model.get_learned_conditioning(prompts), uc, prompts

    # ------------------------------------------------------------------ layer-skip candidates
    @property
    def layer_num(self) -> int:
        """Layers of the UNet a skip list may name (0: the model's UNet does not take skip lists)."""
        return int(getattr(getattr(self.model, "model", None), "layer_num", 0) or 0)

    def split_candidate(self, cand):
        """-> (timesteps, skip_layers | None).  A dict candidate is checked here, before anything is launched: as many lists as
        timesteps, every id an int in range(layer_num), no id twice in one list."""
        if not isinstance(cand, dict):
            return cand, None
        if set(cand) != {"timesteps", "skip_layers"}:
            raise ValueError(f"SDCandidateEvaluator: a dict candidate holds 'timesteps' and 'skip_layers', got {sorted(cand)}")
        ts, sk = list(cand["timesteps"]), [list(s) for s in cand["skip_layers"]]
        if len(ts) != len(sk):
            raise ValueError(f"SDCandidateEvaluator: {len(sk)} skip lists for {len(ts)} timesteps")
        L = self.layer_num
        if L <= 0:
            raise ValueError("SDCandidateEvaluator: the model's UNet has no layer_num: it does not take layer-skip lists")
        for i, lst in enumerate(sk):
            for v in lst:
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < L:
                    raise ValueError(f"SDCandidateEvaluator: skip_layers[{i}] holds {v!r}: layer ids are ints in range({L})")
            if len(set(int(v) for v in lst)) != len(lst):
                raise ValueError(f"SDCandidateEvaluator: skip_layers[{i}] = {lst} names a layer twice")
        return ts, [[int(v) for v in lst] for lst in sk]

    def candidate_cost(self, cand) -> int:
        """UNet layer evaluations per image (search.py's candidate_cost): every step costs layer_num minus its skipped layers."""
        if isinstance(cand, dict):
            return sum(self.layer_num - len(sk) for sk in cand["skip_layers"])
        return len(cand) * max(1, self.layer_num)

    def _announce(self, skips):
        """Tell the UNet how many captured launch sequences this candidate's skipped evaluations need, before sampling: one per
        distinct non-empty set and, under split guidance, per stream."""
        unet = getattr(self.model, "model", None)
        if hasattr(unet, "plan_graphs"):
            sets = {tuple(sorted(s)) for s in (skips or []) if len(s)}
            unet.plan_graphs(len(sets), streams=2 if getattr(self.sampler, "split_guidance", False) else 1)

    # ------------------------------------------------------------------ search_ea.py:504-566
    def get_cand_fid(self, cand=None, opt=None, device=None):
        t1 = time.time()
        cand, skips = self.split_candidate(cand)
        self._announce(skips)
        extra = {} if skips is None else {"skip_layers": skips}
        seed0 = candidate_seed(self.seed, cand)
        fixed = self.start_code(opt, batch_seed(seed0, 0)) if opt.fixed_code else None
        shape = [opt.C, opt.H // opt.f, opt.W // opt.f]
        sampled_timestep = np.array(cand)
        use_cmmd = self.fitness == "cmmd"
        acc = None if use_cmmd else self._accumulator()
        stage, fill, count, plan = None, 0, 0, []
        cosines, clip_time, embeds = [], 0.0, []
        world, rank = self._shard()
        with torch.no_grad():
            for itr, (c, uc, prompts) in enumerate(self._batches(opt)):
                if opt.scale == 1.0:
                    uc = None
                if itr % world != rank:      # image-sharded CMMD: another rank samples this batch; the count runs on
                    count += int(opt.n_samples)
                    if count > self.num_samples:
                        break
                    continue
                seed = batch_seed(seed0, 0 if opt.fixed_code else itr)
                x_T = fixed if opt.fixed_code else self.start_code(opt, seed)
                plan.append((itr, seed))
                samples, _ = self.sampler.sample(S=opt.time_step, conditioning=c, batch_size=opt.n_samples, shape=shape,
                                                 verbose=False, unconditional_guidance_scale=opt.scale,
                                                 unconditional_conditioning=uc, eta=opt.ddim_eta, x_T=x_T,
                                                 sampled_timestep=sampled_timestep, **extra)
                x = self.model.decode_first_stage(samples)
                # clamp((x + 1) / 2, 0, 1) straight into the extractor's staging batch of 320 images
                if stage is None:
                    stage = torch.empty((FID_BATCH,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
                done = 0
                while done < x.shape[0]:
                    take = min(x.shape[0] - done, FID_BATCH - fill)
                    self._image_out(x[done:done + take], stage[fill:fill + take])
                    if use_cmmd:
                        t0 = time.time()
                        cos, emb = self.clip_scorer.cosine_and_embeds(stage[fill:fill + take], prompts[done:done + take])
                        cosines.append(torch.as_tensor(cos).cpu())
                        embeds.append(emb)
                        clip_time += time.time() - t0
                        fill, done = 0, done + take      # nothing is staged for an extractor
                        continue
                    if self.clip_scorer is not None:
                        t0 = time.time()
                        cosines.append(torch.as_tensor(self.clip_scorer.cosine(stage[fill:fill + take], prompts[done:done + take])).cpu())
                        clip_time += time.time() - t0
                    fill, done = fill + take, done + take
                    if fill == FID_BATCH:
                        acc.add(self.features(stage))
                        fill = 0
                count += int(x.shape[0])
                logger.log('samples: ' + str(count))
                if count > self.num_samples:
                    logger.log('samples: ' + str(count))
                    break
            if fill:
                acc.add(self.features(stage[:fill]))
        if count == 0:
            raise AdmError("SDCandidateEvaluator: the conditioning / prompts iterable is empty")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        sample_time = time.time() - t1
        t1 = time.time()
        if use_cmmd:
            from . import cmmd
            if self.cmmd_ref is None:      # uploads the reference embeddings and computes S_yy once
                self.cmmd_ref = cmmd.CMMDReference(self._ref_clip_feats, device=self.device, sigma=self.cmmd_sigma)
            mine = torch.cat(embeds, 0) if embeds else torch.zeros((0, self.cmmd_ref.y.shape[1]), dtype=torch.float32, device=self.device)
            self.last_rows = cmmd.pooled_rows(mine, None, local=not self.image_sharded)
            fid = float(self.cmmd_ref.fitness(self.last_rows))                     # fid_time: the two kernel sums
        elif self.fitness == "kid":
            from .kid import KIDReference
            if self.kid_ref is None:
                self.kid_ref = KIDReference(self._ref_feats, device=self.device)   # uploads the rows and computes S_yy once
            acc.join()
            self.last_rows = torch.cat(acc.rows, 0)
            fid = float(self.kid_ref.fitness(self.last_rows))                      # fid_time: the two kernel sums
        else:
            fid = float(acc.statistics(None, local=True).frechet_distance(self.ref_stats))
        logger.log('FID: ' + str(fid) + self.fid_note)
        fid_time = time.time() - t1
        logger.log('sample_time: ' + str(sample_time) + ', fid_time: ' + str(fid_time))
        self.last_times = {"sample_time": sample_time, "fid_time": fid_time, "images": count, "batches": len(plan)}
        self.last_plan = plan
        if self.clip_scorer is not None and cosines:
            cos = torch.cat(cosines)
            self.last_clip = {"score": float(self.clip_scorer.score_of(cos)), "cosines": cos, "clip_time": clip_time}
            logger.log('CLIP score: ' + str(self.last_clip["score"]) + ', clip_time: ' + str(clip_time))
        return fid
