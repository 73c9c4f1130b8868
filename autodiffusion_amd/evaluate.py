"""Candidate evaluation: sample an image batch with a searched schedule (and layer-skip mask).

The device-side half of ``EvolutionSearcher.get_cand_fid`` (reference
search_imagenet64_classifier_guidance.py:308-366; dict candidates with per-step skip lists:
search_dynamic_unet_imagenet64_classifier_guidance_progressive.py:369-445; unconditional:
search_uncondition_model.py:312-368): reset_diffusion(cand) -> sample loop -> uint8 NHWC batch.
Differences from the reference, by design: images stay on the producing GPU
(no per-batch all_gather / D2H), and every batch is seeded per (seed) so results do not depend on
how batches are sharded over ranks.
"""
from __future__ import annotations

import ast
import copy
from typing import Callable, Optional, Sequence, Union

import torch

from . import logger
from .schedule import apply_candidate

NUM_CLASSES = 1000

# Images evaluated per pass over the networks when several of the reference's (memory-driven) batches are merged: the cap scales
# with the image area -- 256 images at 64x64 (the headline batch), 128 at 128x128, 64 at 256x256 -- so the activation working set of
# a pass stays near the headline's whatever the model (a 128x128 ADM-G pass of 256 images would carry 4 x the headline's tape).
PASS_IMAGES = {64: 256, 128: 128, 256: 64}


def pass_cap(image_size: int) -> int:
    for size in sorted(PASS_IMAGES):
        if image_size <= size:
            return PASS_IMAGES[size]
    return max(1, PASS_IMAGES[256] * 256 * 256 // (image_size * image_size))


def merge_policy(image_size: int, batch_size: int, requested: int = 0, rounds: int = None):
    """-> (reference batches per pass, images per pass).  requested > 0 is taken as given (--merge_batches K); 0 = auto:
    pass_cap(image_size) // batch_size, at least 1, at most the `rounds` a rank still has to run."""
    merge = int(requested) if requested and requested > 0 else max(1, pass_cap(image_size) // max(1, batch_size))
    if rounds is not None:
        merge = max(1, min(merge, rounds))
    return merge, merge * batch_size


def graph_auto(image_size: int, images_per_pass: int) -> bool:
    """`--use_graph auto`: hipGraph replay when the pass that is actually launched (the MERGED batch, which is what gets captured)
    is small enough for the host's launch rate to be the floor: up to 256 64x64-equivalents per pass (measured: batch 100 x 2
    at 64x64 replayed 6.78 s per candidate against 7.61 s eager; above that the GPU is the slower side)."""
    return images_per_pass * (image_size / 64.0) ** 2 <= 256


# the sampling CLIs' wording of the merge line; the search passes its own (search.MERGE_LOG)
MERGE_LOG = "evaluating {merge} batches of {batch_size} per pass ({per_pass} images per pass; bitwise the images of separate passes)"


def batch_plan(num_samples: int, batch_size: int, world: int = 1, rank: int = 0, image_size: int = 64, merge_batches: int = 0):
    """How `num_samples` images are produced in rounds: -> the passes over the networks that `rank` runs, each a list of
    (global batch index, images kept) -- the one statement of this policy; no torch, no GPU.

    Every round, each of the `world` ranks samples one reference batch of `batch_size` images; the batch of round i on rank r has
    the global index g = i * world + r, which is also its place in the rank-major concatenation of which the reference keeps
    `arr[:num_samples]`: it contributes its first max(0, min(batch_size, num_samples - g * batch_size)) images.  A batch that
    contributes none is still sampled, so that the ranks stay in step (barrier, all_gather).  merge_policy decides how many
    of a rank's batches ride in one pass (`merge_batches` > 0 is taken as given); the first pass is never the smaller one."""
    rounds = -(-num_samples // (batch_size * world))
    merge = merge_policy(image_size, batch_size, int(merge_batches or 0), rounds)[0]
    plan = [(i * world + rank, max(0, min(batch_size, num_samples - (i * world + rank) * batch_size))) for i in range(rounds)]
    return [plan[i:i + merge] for i in range(0, rounds, merge)]


def _literal(text: str, flag: str):
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError, TypeError, MemoryError, RecursionError):
        raise ValueError(f"{flag}: expected a literal (numbers, lists, dicts; expressions and calls are not evaluated), got {text!r}") from None


def _is_ints(v) -> bool:
    return isinstance(v, (list, tuple)) and all(isinstance(i, int) and not isinstance(i, bool) for i in v)


def _is_int_lists(v) -> bool:
    return isinstance(v, (list, tuple)) and all(_is_ints(s_) for s_ in v)


def parse_int_list(text: str, flag: str, *, nested: bool = False, use_mean: bool = False):
    """A list flag (--use_timestep, --search_space; nested: --skip_layers, one list per step) -> list of ints (of lists of ints).
    `use_mean`: the space-separated averaged schedule '[153.2 424.7 ...]', parsed as numbers and rounded before the check."""
    v = _literal(text.replace(" ", ",") if use_mean else text, flag)
    if use_mean and isinstance(v, (list, tuple)) and all(isinstance(t, (int, float)) and not isinstance(t, bool) for t in v):
        v = [round(t) for t in v]
    if nested and _is_int_lists(v):
        return [list(s_) for s_ in v]
    if not nested and _is_ints(v):
        return list(v)
    raise ValueError(f"{flag}: expected a list of {'lists of ints' if nested else 'ints'}, got {text!r}")


def parse_candidate(text: str, flag: str = "candidate"):
    """A candidate as the search writes it (str(cand)) or as a flag gives it: a list of ints, or a dict with `timesteps` and
    one `skip_layers` list per timestep.  ast.literal_eval plus a shape check: command-line text is input from outside."""
    v = _literal(text, flag)
    if isinstance(v, dict):
        ts, sk = v.get("timesteps"), v.get("skip_layers")
        if not (_is_ints(ts) and _is_int_lists(sk) and len(ts) == len(sk)):
            raise ValueError(f"{flag}: a dict candidate needs 'timesteps' (ints) and 'skip_layers' (one list of ints per timestep), got {text!r}")
        return v
    if not _is_ints(v):
        raise ValueError(f"{flag}: expected a list of ints or a {{'timesteps', 'skip_layers'}} dict, got {text!r}")
    return list(v)


def parse_index_step(value, flag: str = "--index_step"):
    """--index_step: a number, or a numeric string.  Arithmetic ('4*58': pass the product) is refused, as any expression."""
    if not isinstance(value, str):
        return int(value)
    v = _literal(value, flag)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"{flag}: expected a number, got {value!r}")
    return v


class CandidateEvaluator:
    def __init__(self, model, base_diffusion, classifier=None, *, image_size: int, use_ddim: bool = True,
                 clip_denoised: bool = True, class_cond: bool = True, classifier_scale: float = 1.0,
                 device=None, use_graph: bool = False, sampler: Optional[str] = None, dpm_order: int = 2,
                 dpm_predict_x0: bool = True, dpm_thresholding: bool = False, unipc_order: int = 2, unipc_variant: str = "bh2",
                 unipc_corrector: bool = True, unipc_predict_x0: bool = True, unipc_thresholding: bool = False):
        if sampler not in (None, "dpm_solver", "unipc"):
            raise ValueError(f"sampler={sampler!r}: None (use_ddim decides between DDIM and ancestral sampling), 'dpm_solver' or 'unipc'")
        # sampler="unipc": the same K evaluations as multistep UniPC (unipc.py): every update but the last arrival corrected
        self.unipc_order, self.unipc_variant, self.unipc_corrector = int(unipc_order), str(unipc_variant), bool(unipc_corrector)
        self.unipc_predict_x0, self.unipc_thresholding = bool(unipc_predict_x0), bool(unipc_thresholding)
        # sampler="dpm_solver": the candidate's K timesteps are K evaluations of multistep DPM-Solver (dpm_solver.py), not of DDIM
        self.sampler, self.dpm_order = sampler, int(dpm_order)
        self.dpm_predict_x0, self.dpm_thresholding = bool(dpm_predict_x0), bool(dpm_thresholding)
        self.model = model
        self.classifier = classifier
        self.base_diffusion = base_diffusion
        self.active_diffusion = copy.deepcopy(base_diffusion)
        self.image_size = image_size
        self.use_ddim = use_ddim
        self.clip_denoised = clip_denoised
        self.class_cond = class_cond
        self.classifier_scale = classifier_scale
        self.device = device if device is not None else model.device
        self.skip_layers = None
        self._merge_logged = False   # sample_plan's merge line: once per evaluator
        if use_graph:  # hipGraph replay of the UNet evaluation and of the guidance gradient (batches <= ~100: the host's
            model.enable_graph(True)   # ~60 ms of launch work per guided step is otherwise the floor)
            if classifier is not None and hasattr(classifier, "enable_graph"):
                classifier.enable_graph(True)

    def set_candidate(self, cand: Union[Sequence[int], dict]):
        """reset_diffusion(cand); dict candidates also carry one skip-layer list per step."""
        if isinstance(cand, dict):
            assert len(cand["timesteps"]) == len(cand["skip_layers"])
            self.skip_layers = [list(s) for s in cand["skip_layers"]]
            steps = cand["timesteps"]
        else:
            self.skip_layers = None
            steps = cand
        apply_candidate(self.active_diffusion, self.base_diffusion, steps)
        if hasattr(self.model, "plan_graphs"):   # one captured launch sequence per distinct skip set of this candidate
            self.model.plan_graphs(len({tuple(sorted(s)) for s in self.skip_layers}) if self.skip_layers is not None else 1)
        return self

    # closures with the reference's calling convention ------------------------------------------
    def _model_fn(self, x, t, y=None, skip_layers=None):
        yy = y if self.class_cond else None
        if skip_layers is not None:
            # the search script indexes by position in the ASCENDING timestep_map
            sl = skip_layers[self.active_diffusion.timestep_map.index(int(t[0]))]
            return self.model(x, t, yy, skip_layer=sl)
        return self.model(x, t, yy)

    def _cond_fn(self, x, t, y=None, skip_layers=None):
        assert y is not None
        return self.classifier.log_prob_grad(x, t, y, self.classifier_scale)

    def _sample(self, batch_size: int, seeds: Sequence[Optional[int]]):
        """One pass over the networks for len(seeds) reference batches of `batch_size` images, each drawing its labels, x_T and
        per-step noise from its own generator (a seed of None: the global RNG) -> (uint8 NHWC of the whole pass, fp32 sample)."""
        dev = self.device
        gens = [None if s_ is None else torch.Generator(device=dev).manual_seed(int(s_) & 0x7FFFFFFFFFFFFFFF) for s_ in seeds]
        shape1 = (batch_size, 3, self.image_size, self.image_size)
        classes, noise = [], []
        for g_ in gens:
            classes.append(torch.randint(low=0, high=NUM_CLASSES, size=(batch_size,), device=dev, generator=g_))
            noise.append(torch.randn(*shape1, device=dev, generator=g_))
        one = len(gens) == 1
        classes, x_T = (classes[0], noise[0]) if one else (torch.cat(classes, 0), torch.cat(noise, 0))
        d = self.active_diffusion
        d.generator = gens[0] if one else [(g_, batch_size) for g_ in gens]
        kwargs = {"y": classes}
        if self.skip_layers is not None:
            kwargs["skip_layers"] = self.skip_layers
        cond_fn = self._cond_fn if self.classifier is not None else None
        if getattr(self, "sampler", None) == "dpm_solver":
            # the networks see the candidate's own integer timesteps, so _model_fn's skip-list lookup works as under DDIM; the
            # solver draws no per-step noise
            from .dpm_solver import DPMSolver
            solver = DPMSolver(self.base_diffusion, predict_x0=self.dpm_predict_x0, thresholding=self.dpm_thresholding)
            sample = solver.sample_candidate(self._model_fn, tuple(x_T.shape), noise=x_T, cond_fn=cond_fn, model_kwargs=kwargs,
                                             device=dev, indices=d.timestep_map, order=self.dpm_order)
            self.last_classes = classes
            return solver.last_uint8_nhwc, sample
        if getattr(self, "sampler", None) == "unipc":   # the same candidate mapping and integer timesteps
            from .unipc import UniPC
            solver = UniPC(self.base_diffusion, predict_x0=self.unipc_predict_x0, thresholding=self.unipc_thresholding,
                           variant=self.unipc_variant, corrector=self.unipc_corrector)
            sample = solver.sample_candidate(self._model_fn, tuple(x_T.shape), noise=x_T, cond_fn=cond_fn, model_kwargs=kwargs,
                                             device=dev, indices=d.timestep_map, order=self.unipc_order)
            self.last_classes = classes
            return solver.last_uint8_nhwc, sample
        fn = d.ddim_sample_loop if self.use_ddim else d.p_sample_loop
        try:
            sample = fn(self._model_fn, tuple(x_T.shape), noise=x_T, clip_denoised=self.clip_denoised, model_kwargs=kwargs,
                        cond_fn=cond_fn, device=dev)
        finally:
            d.generator = None    # a later direct call of the diffusion object must not draw from this pass's generators
        self.last_classes = classes
        return d.last_uint8_nhwc, sample

    def sample_batches(self, batch_size: int, seeds: Sequence[int]):
        """len(seeds) reference batches of `batch_size` images in ONE pass over the networks -> [uint8 NHWC [B, H, W, 3]] per seed.

        Bitwise the images of sample_batch(batch_size, seed) for every seed: each sub-batch draws its labels, x_T and per-step noise
        from its own generator, and an image's result does not depend on how many images ride along (tests/test_hip_bigbatch.py).
        The reference's search batch (100, a memory-driven flag) leaves the 16x16 / 8x8 levels with 200-300 tiles on 256 CUs; two
        batches per pass fill the chip like the headline's 256."""
        return list(self._sample(batch_size, seeds)[0].split(batch_size, 0))

    def sample_batch(self, batch_size: int, seed: Optional[int] = None, return_float: bool = False):
        """-> uint8 NHWC [B, H, W, 3] on the device (and the fp32 sample if return_float)."""
        u8, sample = self._sample(batch_size, [seed])
        return (u8, sample) if return_float else u8

    def sample_plan(self, num_samples: int, batch_size: int, seed_of: Callable[[int], int], *, world: int = 1, rank: int = 0,
                    merge_batches: int = 0, merge_log: str = MERGE_LOG):
        """Walk batch_plan(...) for this rank: one sampling call per pass, yielding per reference batch
        (uint8 NHWC batch, its classes, how many of its images count towards `num_samples`).  `seed_of(g)` is the seed of the
        batch with global index g.  `merge_log` is the wording of the line that tells log.txt about merged passes; it is written
        at most once per evaluator (one search, one CLI run)."""
        passes = batch_plan(num_samples, batch_size, world, rank, self.image_size, merge_batches)
        merge = len(passes[0]) if passes else 1
        if merge > 1 and not self._merge_logged:
            logger.log(merge_log.format(merge=merge, batch_size=batch_size, per_pass=merge * batch_size))
            self._merge_logged = True
        done = 0
        for batches in passes:
            u8s = self.sample_batches(batch_size, [seed_of(g) for g, _ in batches])
            for u8, classes, (_, keep) in zip(u8s, self.last_classes.split(batch_size, 0), batches):
                yield u8, classes, keep
                done += 1    # logged once the caller has consumed the batch (the CLIs: after its all_gather)
                logger.log('created ' + str(done * batch_size * world) + ' samples')
