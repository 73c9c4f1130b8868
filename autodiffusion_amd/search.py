"""Evolutionary search over timestep subsets -- the reference's driver on the HIP evaluation path.

Drop-in mirror of ``EvolutionSearcher`` (reference search_imagenet64_classifier_guidance.py:155-584;
unconditional variant search_uncondition_model.py; dict candidates with per-step skip lists are
accepted by ``get_cand_fid`` as in search_dynamic_unet_imagenet64_classifier_guidance_progressive.py
:369-445).  The EA operators consume ``random`` / ``np.random`` in exactly the reference's order
(pinned by tests/golden/ea_trajectory.npz), the log lines keep the reference's text, and
``get_cand_fid(cand, args) -> float`` keeps its signature and side effects.

The EA itself -- bookkeeping, operators, the population-parallel queue and the ``search()`` loop -- is ``ea.EvolutionDriver``,
shared with sd_search.py; this module holds what is ADM's own: the constructor, the FID / KID plumbing and the timestep space.
``DynamicEvolutionSearcher`` is ``ea.JointSearch``'s operators over this module's searcher.

What changes underneath:
  * sampling runs on the HIP engine (evaluate.CandidateEvaluator); images never leave the GPU;
  * FID statistics are accumulated on the GPU and pooled over ranks with one all-gather per
    candidate (fid.ActivationAccumulator) instead of all-gathering every uint8 batch;
  * every batch is seeded by (seed, candidate, batch index, rank), so a candidate's FID does not depend
    on how the work was sharded;
  * the Inception feature extractor is a plug: ``features(uint8 NHWC device batch) -> [B, D]`` -- the bundled HIP
    Inception-v3 pool3 (``inception.InceptionV3(...).features``, parity unpinned: DESIGN.md section 9) or any other callable --
    or an ``Evaluator_v1``-style object (then the reference's host cal_fid path is used).
"""
from __future__ import annotations

import time
import zlib

import numpy as np
import torch

from . import dist_util, logger
from .ea import EvolutionDriver, JointSearch, choice  # noqa: F401  (choice: part of this module's interface)
from .evaluate import CandidateEvaluator
from .fid import ActivationAccumulator, FIDStatistics, cal_fid
from .schedule import space_timesteps

# the search's wording of evaluate.MERGE_LOG: log.txt shows the deviation from the reference's launch unit
MERGE_LOG = ("evaluating {merge} batches of {batch_size} per pass over the networks ({per_pass} images per pass; "
             "bitwise the images of separate passes; --merge_batches 1 restores the reference's launch unit)")


class EvolutionSearcher(EvolutionDriver):
    shuffle_space_in_place = True    # sample_active_subnet shuffles `search_space` itself, as the reference does

    def __init__(self, args, model, base_diffusion, time_step, classifier=None, search_space=None,
                 evaluator=None, ref_stats=None, features=None, feature_dim=2048, variant=None,
                 population_parallel=False, ref_feats=None):
        super().__init__(args, population_parallel)
        self.model = model
        self.base_diffusion = base_diffusion
        self.classifier = classifier
        self.time_step = time_step
        self.max_fid = getattr(args, "max_fid", 48.0)
        self.thres = getattr(args, "thres", 0.2)
        self.search_space = search_space
        # "guided" = search_imagenet64_classifier_guidance.py, "unconditional" = search_uncondition_model.py
        # (the latter seeds pop//2 random candidates instead of pop//2 + 1 and stops before the last
        # epoch's offspring, :509-532, :554-555)
        self.variant = variant or ("guided" if classifier is not None else "unconditional")
        self.break_at_last_epoch = self.variant == "unconditional"
        # FID plumbing: reference-style evaluator object, or a device feature function
        self.evaluator = evaluator
        self.features = features
        self.feature_dim = feature_dim
        self.ref_stats = ref_stats
        # an extractor that runs on random weights (inception.pool3_features(allow_random=True): throughput runs, tests) ranks
        # candidates on a meaningless metric: every FID line of log.txt says so, next to the value
        self.fid_note = (" [FID on RANDOM Inception weights: not a quality metric]"
                         if getattr(features, "random_weights", False) else "")
        self.last_times = None   # {'reset_time', 'sample_time', 'fid_time', 'images'} of the last get_cand_fid
        # --fitness kid: candidates are ranked by 1000 x the unbiased cubic-kernel MMD^2 of their kept activation rows against the
        # reference rows (kid.KIDReference; unbiased at the search's num_samples <= 1000, where the Frechet distance is not).  The
        # value still travels under info['fid'] -- the EA only sorts by it -- and every line that prints it says what it is.
        self.fitness = getattr(args, "fitness", "fid") or "fid"
        if self.fitness not in ("fid", "kid"):
            raise ValueError(f"fitness {self.fitness!r}: expected 'fid' or 'kid'")
        self.kid_ref = None
        self.last_rows = None    # the rows the last KID fitness was computed from (tests compare against them)
        if self.fitness == "kid":
            if features is None:
                raise ValueError("fitness 'kid' needs a device `features` function (the rows stay on the GPU)")
            self._ref_feats = ref_feats if ref_feats is not None else getattr(args, "ref_feats", "")
            if isinstance(self._ref_feats, str):
                if not self._ref_feats:
                    raise ValueError("fitness 'kid' needs --ref_feats FILE.npz (scripts/evaluator.py --save_ref_feats writes it)")
                from .kid import load_ref_feats
                self._ref_feats = load_ref_feats(self._ref_feats)
            self.fid_note += " [fitness: KID x 1e3]"
        if ref_stats is None and getattr(args, "ref_path", ""):
            # the reference pickles a FIDStatistics; this build reads the two arrays from an .npz
            # (mu, sigma) written from it -- unpickling foreign files is not done here
            z = np.load(args.ref_path, allow_pickle=False)
            self.ref_stats = FIDStatistics(z["mu"], z["sigma"])
        self._ref_dev = None    # (ref_stats, mu, sigma on the device): uploaded once, not once per candidate
        self._ev = None
        if model is not None:
            self._ev = CandidateEvaluator(
                model, base_diffusion, classifier, image_size=args.image_size, use_ddim=args.use_ddim,
                clip_denoised=args.clip_denoised, class_cond=args.class_cond,
                classifier_scale=getattr(args, "classifier_scale", 1.0), device=dist_util.dev(),
                use_graph=bool(getattr(args, "use_graph", False)), **(getattr(args, "dpm", None) or {}))
            self.active_diffusion = self._ev.active_diffusion

    # ------------------------------------------------------------------ evaluate-candidate interface
    def reset_diffusion(self, use_timesteps):
        self._ev.set_candidate(list(use_timesteps))

    def get_cand_fid(self, cand=None, args=None):
        if self.population_parallel:
            # whole candidate on this rank alone: its batches are seeded as a single-rank run would seed them, the
            # statistics stay local and there is no collective inside (ranks evaluate different candidates)
            return self._cand_fid(cand, args, world=1, rank=0, local=True)
        return self._cand_fid(cand, args, world=dist_util.get_world_size(), rank=dist_util.get_rank(), local=False)

    def _cand_fid(self, cand, args, *, world, rank, local):
        """`world` / `rank` = how this candidate's image batches are sharded (1 / 0: all of them here)."""
        args = args if args is not None else self.args
        t1 = time.time()
        self._ev.set_candidate(cand)
        reset_time = time.time() - t1
        t1 = time.time()
        logger.log("sampling...")
        seed0 = (int(getattr(args, "seed", 0)) * 1000003 + zlib.crc32(str(cand).encode())) & 0x7FFFFFFF
        # fewer samples than feature dimensions (the search's regime, `num_samples <= 1000` against 2048): the on-device Frechet
        # distance can work from the rows (an n x n eigenproblem instead of two 2048 x 2048 ones)
        rows = int(args.num_samples) if (getattr(args, "fid_on_device", False) and args.num_samples < self.feature_dim) else 0
        if self.fitness == "kid":
            rows = int(args.num_samples)       # the KID sums work from the rows themselves, whatever their number
        acc = ActivationAccumulator(self.feature_dim, self._ev.device, keep_rows=rows) if self.features is not None else None
        if acc is not None and self._ref_dev is not None and self._ref_dev[0] is self.ref_stats:
            acc._ref_dev = self._ref_dev       # the reference statistics stay on the device across candidates
        host_images = []
        batches = 0
        # rounds, merged passes, sharding over ranks: evaluate.batch_plan; the merge line is logged once per search
        for u8, _, keep in self._ev.sample_plan(args.num_samples, args.batch_size, lambda g: seed0 + 7919 * g, world=world, rank=rank,
                                                merge_batches=int(getattr(args, "merge_batches", 0) or 0), merge_log=MERGE_LOG):
            if acc is None:
                host_images.append(u8[:keep].cpu().numpy())
            elif keep > 0:
                acc.add_from(self.features, u8[:keep])   # on a side stream, next to the next pass's sampling
            batches += 1
        if world > 1 or (not local and dist_util.collectives_on()):
            import torch.distributed as dist
            dist.barrier()
        logger.log("sampling complete")
        sample_time = time.time() - t1
        t1 = time.time()
        if acc is not None and self.fitness == "kid":
            fid = self._kid_fitness(acc, local)   # fid_time: the two kernel sums (S_yy is cached), and the row gather with several ranks
        elif acc is not None:
            if getattr(args, "fid_on_device", False):
                fid = acc.frechet_distance_device(self.ref_stats, None, local=local)  # eigh on the GPU instead of the host sqrtm
                self._ref_dev = acc._ref_dev
            else:
                fid = float(acc.statistics(None, local=local).frechet_distance(self.ref_stats))
        else:
            if world > 1:
                raise NotImplementedError("host-evaluator FID with several ranks: pass a device `features` function "
                                          "so that statistics are pooled on the GPUs")
            arr = np.concatenate(host_images, axis=0)[: args.num_samples]
            fid = float(cal_fid(arr, 64, self.evaluator, ref_stats=self.ref_stats))
        fid_time = time.time() - t1
        if acc is not None and acc.last_collective and not getattr(self, "_coll_logged", False):   # once per search
            c = acc.last_collective
            logger.log(f"collective: all_gather of the pooled FID statistics, backend {c['backend']}, {c['world_size']} rank(s), "
                       f"{c['bytes_per_rank']} B per rank, on {c['device']}")
            self._coll_logged = True
        logger.log('reset_time: ' + str(reset_time) + ', sample_time: ' + str(sample_time) + ', fid_time: ' + str(fid_time))
        self.last_times = {"reset_time": reset_time, "sample_time": sample_time, "fid_time": fid_time,
                           "images": int(args.num_samples), "batches_this_rank": batches}
        return fid

    def _kid_fitness(self, acc, local):
        """1000 x MMD^2_u of the candidate's kept rows (pooled over the ranks of the image-sharded mode) against the reference rows."""
        from .kid import KIDReference, pooled_rows
        acc.join()
        if acc.rows is None:
            raise RuntimeError("fitness 'kid': the accumulator dropped the activation rows (more than num_samples were added)")
        if self.kid_ref is None:
            self.kid_ref = KIDReference(self._ref_feats, device=acc.device)   # uploads the rows and computes S_yy once per search
        mine = torch.cat(acc.rows, 0) if acc.rows else torch.zeros((0, self.feature_dim), dtype=torch.float32, device=acc.device)
        self.last_rows = pooled_rows(mine, None, local=local)
        return float(self.kid_ref.fitness(self.last_rows))

    # ------------------------------------------------------------------ the space the EA searches
    @property
    def num_timesteps(self):
        return self.base_diffusion.original_num_steps

    def space(self):
        return (self.search_space if self.search_space is not None else range(self.num_timesteps)), self.time_step

    def gather_device(self):
        return self._ev.device if self._ev is not None else None

    def initial_candidate(self):
        return list(space_timesteps(self.num_timesteps, ('ddim' if self.args.use_ddim else '') + str(self.args.time_step)))


class DynamicEvolutionSearcher(JointSearch, EvolutionSearcher):
    """The joint search over timesteps and per-step layer-skip lists on the dynamic UNet (ea.JointSearch) over ADM evaluation."""

    def __init__(self, args, model, base_diffusion, time_step, classifier=None, index_step=None, **kw):
        super().__init__(args, model, base_diffusion, time_step, classifier=classifier, **kw)
        self._init_joint(model.layer_num if model is not None else int(getattr(args, "layer_num")), time_step, index_step)
