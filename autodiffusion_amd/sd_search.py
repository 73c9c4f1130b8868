"""Evolutionary search over Stable-Diffusion sampling schedules -- the reference's SD driver on the HIP evaluation path.

Drop-in mirror of ``EvolutionSearcher`` of the reference's "Stable Diffusion"/scripts/search_ea.py:184-633.  Two candidate
spaces, as there: ``time_step`` integers out of ``range(sampler.ddpm_num_timesteps)`` for the DDIM / PLMS samplers, and
``time_step + 1`` continuous times out of ``dpm_params['full_timesteps']`` (the 1001-point uniform grid 1 .. 1/1000) under
``opt.dpm_solver`` or ``opt.unipc``.  Every operator consumes ``random`` / ``np.random`` in exactly the reference's order (pinned by
tests/golden/sd_ea_trajectory.npz, captured from the reference's own driver): candidates are sorted ascending and deduplicated
by ``str(sorted(cand))`` in ``vis_dict``, cross and mutation try ``10 x num`` times, ``keep_top_k = {select_num: [], 50: []}``,
the search stops before the last epoch's offspring (:613-614), ``use_ddim_init_x`` seeds the init candidate, ``population_num
// 2`` random ones and ``population_num - population_num // 2 - 1`` mutations of the init candidate at ``m_prob = 0.1``
(:574-588).  The log lines keep the reference's text, through ``logger``; ``get_cand_fid(cand, opt, device)`` keeps its signature.

What is underneath: ``get_cand_fid`` is a plain delegation to ``sd_evaluate.SDCandidateEvaluator.get_cand_fid`` -- CLIP encoder,
latent UNet + sampler, VAE decoder, clamp, Inception extractor and float64 statistics, every device-side step a libadm_hip.so
launch.  The driver itself puts no torch compute op and no host copy of an image or a latent between a candidate and its FID.

Different by design:
  * candidate strings are parsed with ``ast.literal_eval``, never ``eval``, and candidates hold plain Python ``int`` / ``float``.
    Under numpy 2 the reference's init candidate prints as ``[np.int64(1), ...]``; this driver's prints as ``[1, 251, 501, 751]``.
    Comparisons with the reference are therefore on values, not on strings;
  * start noise is seeded per (seed, candidate, batch) -- ``SDCandidateEvaluator``'s behaviour: a candidate's FID does not
    depend on what was evaluated before it or on which rank evaluated it;
  * ``population_parallel=True`` is the driver's scheme, as in ``search.py``.  Candidate generation never looks at FID values
    (legality is only the visited-set dedupe; parents are the top-k frozen at epoch start), so ``is_legal*`` queues the candidate
    and ``flush_pending()`` assigns the queue by cost -- a flat candidate costs ``len(cand)``, all of one search the same, which
    puts candidate i on rank ``i % world`` -- runs ONE ``all_gather`` of the float64 FIDs and writes them back in order.  With one
    rank the trajectory is the sequential one.

The EA itself -- bookkeeping, operators, queue and the ``search()`` loop -- is ``ea.EvolutionDriver``, shared with search.py; this
module holds what is SD's own: the constructor (evaluator, ``dpm_params``, ``fid_note``), ``get_cand_fid``, the init candidate, the
two spaces and the sorted canonical form.  ``DynamicEvolutionSearcher`` below is the joint search over timesteps AND per-step
layer-skip lists in the integer timestep space: ``ea.JointSearch``'s operators over this module's searcher.
"""
from __future__ import annotations

import ast
import os

import numpy as np
import torch

from .ea import EvolutionDriver, JointSearch
from .evaluate import parse_candidate
from .schedule import space_timesteps
from .sd_sampler import make_ddim_timesteps


def dpm_search_params(alphas_cumprod, time_step):
    """search_ea.py:888-902: the DPM-Solver candidate space.  ``DPM_Solver.get_time_steps('time_uniform')`` is
    ``torch.linspace(t_T, t_0, N + 1)`` in float32 (dpm_solver.py:430-431) with t_T = 1 and t_0 = 1 / len(alphas_cumprod);
    ``full_timesteps`` is that grid for N = 1000, ``init_timesteps`` for N = time_step, both as Python floats (descending)."""
    t_T, t_0 = 1.0, 1.0 / len(alphas_cumprod)
    grid = lambda n: [v.item() for v in torch.linspace(t_T, t_0, n + 1, dtype=torch.float32)]  # noqa: E731
    return {'full_timesteps': grid(1000), 'init_timesteps': grid(int(time_step))}


def parse_sd_candidate(text, flag="candidate"):
    """A candidate as the search writes it (``str(cand)``) or as ``--evaluate`` gives it: a flat list of ints (a timestep
    list) or of floats (DPM-Solver times), or the joint search's ``{'timesteps': [ints], 'skip_layers': [[ints], ...]}`` with one
    list per timestep.  ``ast.literal_eval`` plus a shape check: command-line text is input from outside."""
    try:
        v = ast.literal_eval(text)
    except (ValueError, SyntaxError) as e:
        raise ValueError(f"{flag}: expected a list of numbers, got {text!r}") from e
    if isinstance(v, dict):
        return parse_candidate(text, flag)   # evaluate.py's shape check of the dict form
    if not isinstance(v, (list, tuple)) or not v or not all(isinstance(t, (int, float)) and not isinstance(t, bool) for t in v):
        raise ValueError(f"{flag}: expected a non-empty list of ints or floats, got {text!r}")
    return list(v)


def _plain(v):
    """numpy scalars -> the Python number of the same value, so that str(cand) reads back through literal_eval."""
    return v.item() if hasattr(v, "item") else v


class _Texts:
    """``batch['text']`` of every batch of a re-iterable loader, read lazily: the evaluator stops at num_sample images."""

    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        for batch in self.loader:
            yield batch['text']


class EvolutionSearcher(EvolutionDriver):
    parse = staticmethod(parse_sd_candidate)
    fid_keyword = "opt"

    def __init__(self, opt, model, time_step, ref_mu, ref_sigma, sampler, dataloader_info, batch_size, dpm_params=None, *,
                 evaluator=None, population_parallel=False, inception=None, features=None, allow_random_inception=False,
                 clip_scorer=None, fitness="fid", ref_feats=None, ref_clip_feats=None):
        super().__init__(opt, population_parallel)
        self.opt = opt
        self.model = model
        self.sampler = sampler
        self.time_step = time_step
        self.dataloader_info = dataloader_info
        self.batch_size = batch_size
        self.num_samples = getattr(opt, "num_sample", None)
        self.ddim_discretize = "uniform"
        self.max_fid = getattr(opt, "max_fid", 3.0)
        # search() as the reference's SD script runs it: no --init_x branch, population_num // 2 random candidates next to the
        # init candidate, a stop before the last epoch's offspring (:574-588, :613-614)
        self.x0, self.variant, self.break_at_last_epoch = '', "unconditional", True
        # opt.unipc searches the same space: time_step + 1 continuous times, the same operators and draws
        self.dpm_solver = bool(getattr(opt, "dpm_solver", False) or getattr(opt, "unipc", False))
        self.dpm_params = dpm_params
        if self.dpm_solver and dpm_params is None:
            raise ValueError("EvolutionSearcher: opt.dpm_solver / opt.unipc needs dpm_params (dpm_search_params(alphas_cumprod, time_step))")
        self.ref_mu = np.load(ref_mu) if isinstance(ref_mu, (str, os.PathLike)) else ref_mu
        self.ref_sigma = np.load(ref_sigma) if isinstance(ref_sigma, (str, os.PathLike)) else ref_sigma
        if evaluator is None:
            from .sd_evaluate import SDCandidateEvaluator
            evaluator = SDCandidateEvaluator(
                model, sampler, ref_mu=self.ref_mu, ref_sigma=self.ref_sigma, num_samples=opt.num_sample,
                prompts=_Texts(dataloader_info['validation_loader']), features=features, inception=inception,
                allow_random_inception=allow_random_inception, seed=int(getattr(opt, "seed", 0)), clip_scorer=clip_scorer,
                fitness=fitness, ref_feats=ref_feats,   # 'kid': 1000 x the unbiased cubic-kernel MMD^2 against the rows ref_feats
                # 'cmmd': 1000 x the unbiased RBF-kernel MMD^2 of the CLIP image embeddings against ref_clip_feats; the batches
                # are sharded over the ranks and the rows pooled unless whole candidates are (population_parallel)
                ref_clip_feats=ref_clip_feats, image_sharded=not population_parallel)
        self.evaluator = evaluator
        # an extractor on random weights ranks candidates on a meaningless metric: every FID line of log.txt says so
        self.fid_note = getattr(evaluator, "fid_note", "")

    # ------------------------------------------------------------------ evaluate-candidate interface
    def get_cand_fid(self, cand=None, opt=None, device='cuda'):
        return self.evaluator.get_cand_fid(cand, opt if opt is not None else self.opt)

    def gather_device(self):
        return getattr(self.evaluator, "device", None)

    # ------------------------------------------------------------------ the space the EA searches
    @property
    def num_timesteps(self):
        return self.sampler.ddpm_num_timesteps

    def space(self):
        if self.dpm_solver:
            return self.dpm_params['full_timesteps'], self.time_step + 1
        return range(self.num_timesteps), self.time_step

    def canonical(self, cand):
        """Flat candidates are stored sorted ascending: two orders of the same steps are one candidate."""
        return str(cand) if isinstance(cand, dict) else str(sorted(cand))

    def _key(self, text):
        return self.canonical(self.parse(text))

    def initial_candidate(self):
        """The evenly spaced schedule that ``use_ddim_init_x`` seeds the population with, sorted, as plain Python numbers."""
        if self.dpm_solver:
            init_x = self.dpm_params['init_timesteps']
        else:
            init_x = make_ddim_timesteps(ddim_discr_method=self.ddim_discretize, num_ddim_timesteps=self.time_step,
                                         num_ddpm_timesteps=self.num_timesteps, verbose=False)
        return sorted(_plain(v) for v in init_x)


class DynamicEvolutionSearcher(JointSearch, EvolutionSearcher):
    """Joint search over timesteps and per-step layer-skip lists of the latent UNet, DDIM / PLMS (integer timesteps).  The
    operators, the order of RNG draws, the budget (``max_index_number = time_step * layer_num``, or ``index_step``), the
    progressive ``skip_layer_range`` and the log lines are ``ea.JointSearch``'s, the ones ``search.DynamicEvolutionSearcher`` runs;
    what is set here is the space (``sampler.ddpm_num_timesteps`` steps, ``model_layers = unet.layer_num``) and the evaluation,
    which goes through ``SDCandidateEvaluator``.  With ``population_parallel`` the queued dict candidates are assigned by the
    driver's cost-aware rule (``flush_pending``: longest first to the least-loaded rank)."""
    fid_keyword = "args"

    def __init__(self, opt, model, time_step, ref_mu, ref_sigma, sampler, dataloader_info, batch_size, dpm_params=None, *,
                 index_step=None, layer_num=None, **kw):
        if getattr(opt, "dpm_solver", False) or getattr(opt, "unipc", False) or dpm_params is not None:
            raise ValueError("the joint timestep / layer-skip search is built for the integer timestep space (DDIM / PLMS): "
                             "not together with opt.dpm_solver / opt.unipc")
        super().__init__(opt, model, time_step, ref_mu, ref_sigma, sampler, dataloader_info, batch_size, **kw)
        if layer_num is None:
            layer_num = getattr(getattr(model, "model", None), "layer_num", None) or getattr(self.evaluator, "layer_num", None)
        if not layer_num:
            raise ValueError("the joint search needs the UNet's layer_num (model.model.layer_num, the evaluator's, or layer_num=)")
        self._init_joint(layer_num, time_step, index_step)

    def initial_candidate(self):
        """The init candidate of search.py's joint search: 'ddim<time_step>' spacing, which starts at step 0."""
        return list(space_timesteps(self.num_timesteps, 'ddim' + str(self.time_step)))

    def candidate_cost(self, cand) -> int:
        return self.evaluator.candidate_cost(cand) if hasattr(self.evaluator, "candidate_cost") else super().candidate_cost(cand)

    def get_cand_fid(self, cand=None, args=None, opt=None, device='cuda'):
        """The candidate's steps go to the evaluator in ascending timestep order, each list with its timestep: the order in which
        both samplers are driven on this path (search_ea.py:480 sorts before PLMS sees a list; DDIM sorts itself)."""
        if isinstance(cand, dict):
            order = sorted(range(len(cand['timesteps'])), key=lambda i: cand['timesteps'][i])
            cand = {'timesteps': [_plain(cand['timesteps'][i]) for i in order],
                    'skip_layers': [list(cand['skip_layers'][i]) for i in order]}
        return self.evaluator.get_cand_fid(cand, opt if opt is not None else self.opt)
