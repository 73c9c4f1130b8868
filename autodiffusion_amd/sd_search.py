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
  * ``population_parallel=True`` follows ``search.py``'s scheme.  Candidate generation never looks at FID values (legality is
    only the visited-set dedupe; parents are the top-k frozen at epoch start), so ``is_legal*`` queues the candidate and
    ``flush_pending()`` evaluates candidate i on rank ``i % world`` (all SD candidates of one search cost the same: no cost
    model), runs ONE ``all_gather`` of the float64 FIDs and writes them back in order; ``search()`` flushes where ``search.py``
    does.  With one rank the trajectory is the sequential one.

``DynamicEvolutionSearcher`` below is the joint search over timesteps AND per-step layer-skip lists in the integer
timestep space: ``search.DynamicEvolutionSearcher``'s own operators, draws, budget and bookkeeping over this module's evaluator.
"""
from __future__ import annotations

import ast
import copy
import os
import random
import time

import numpy as np
import torch

from . import dist_util, logger, search as adm_search
from .evaluate import parse_candidate
from .sd_sampler import make_ddim_timesteps

choice = lambda x: x[np.random.randint(len(x))] if isinstance(x, tuple) else choice(tuple(x))  # noqa: E731


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


class EvolutionSearcher(object):

    def __init__(self, opt, model, time_step, ref_mu, ref_sigma, sampler, dataloader_info, batch_size, dpm_params=None, *,
                 evaluator=None, population_parallel=False, inception=None, features=None, allow_random_inception=False,
                 clip_scorer=None, fitness="fid", ref_feats=None, ref_clip_feats=None):
        self.opt = opt
        self.model = model
        self.sampler = sampler
        self.time_step = time_step
        self.dataloader_info = dataloader_info
        self.batch_size = batch_size
        # EA hyperparameters
        self.max_epochs = opt.max_epochs
        self.select_num = opt.select_num
        self.population_num = opt.population_num
        self.m_prob = opt.m_prob
        self.crossover_num = opt.crossover_num
        self.mutation_num = opt.mutation_num
        self.num_samples = getattr(opt, "num_sample", None)
        self.ddim_discretize = "uniform"
        # tracking variables
        self.keep_top_k = {self.select_num: [], 50: []}
        self.epoch = 0
        self.candidates = []
        self.vis_dict = {}
        self.max_fid = getattr(opt, "max_fid", 3.0)
        self.use_ddim_init_x = opt.use_ddim_init_x
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
        # population parallelism: candidates are generated first -- with the reference's exact random / np.random draw order,
        # on every rank identically -- queued, then evaluated rank r -> candidates r, r + W, ... and the FIDs all-gathered
        self.population_parallel = population_parallel
        self._pending = []
        self.last_flush = None

    # ------------------------------------------------------------------ evaluate-candidate interface
    def get_cand_fid(self, cand=None, opt=None, device='cuda'):
        return self.evaluator.get_cand_fid(cand, opt if opt is not None else self.opt)

    # ------------------------------------------------------------------ EA bookkeeping (reference order of RNG draws)
    def update_top_k(self, candidates, *, k, key, reverse=False):
        assert k in self.keep_top_k
        logger.log('select ......')
        t = self.keep_top_k[k]
        t += candidates
        t.sort(key=key, reverse=reverse)
        self.keep_top_k[k] = t[:k]

    def _visit(self, cand):
        cand = str(sorted(parse_sd_candidate(cand)))
        if cand not in self.vis_dict:
            self.vis_dict[cand] = {}
        info = self.vis_dict[cand]
        if 'visited' in info:
            logger.log('cand: {} has visited!'.format(cand))
            return False
        if self.population_parallel:
            self._pending.append(cand)   # evaluated by flush_pending(), sharded over ranks
        else:
            info['fid'] = self.get_cand_fid(opt=self.opt, cand=parse_sd_candidate(cand))
            logger.log('cand: {}, fid: {}'.format(cand, info['fid']) + self.fid_note)
        info['visited'] = True
        return True

    def is_legal_before_search(self, cand):
        return self._visit(cand)

    def is_legal(self, cand):
        return self._visit(cand)

    def flush_pending(self):
        """Evaluate every queued candidate, candidate i on rank i % world; one all_gather of the float64 FIDs."""
        if not self._pending:
            return
        import torch.distributed as dist
        multi = dist_util.collectives_on()
        world = dist.get_world_size() if multi else 1
        rank = dist.get_rank() if multi else 0
        pending, self._pending = self._pending, []
        fids = np.zeros(len(pending), dtype=np.float64)
        t0 = time.time()
        for i, cand in enumerate(pending):
            if i % world == rank:
                fids[i] = self.get_cand_fid(opt=self.opt, cand=parse_sd_candidate(cand))
        mine_s = time.time() - t0
        coll = None
        if multi:
            dev = getattr(self.evaluator, "device", None) if dist.get_backend() == "nccl" else None
            mine = torch.from_numpy(fids).to(dev if dev is not None else torch.device("cpu"))
            parts = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            coll = {"op": "all_gather", "backend": dist.get_backend(), "world_size": world, "bytes_per_rank": int(mine.numel() * 8),
                    "device": str(mine.device)}
            for i in range(len(pending)):
                fids[i] = float(parts[i % world][i])
            logger.log(f"collective: all_gather of {len(pending)} candidate FIDs, backend {coll['backend']}, {world} rank(s), on {coll['device']}")
        self.last_flush = {"candidates": len(pending), "assigned": len(range(rank, len(pending), world)), "evaluate_s": mine_s,
                           "collective": coll}
        for cand, fid in zip(pending, fids):
            self.vis_dict[cand]['fid'] = float(fid)
            logger.log('cand: {}, fid: {}'.format(cand, float(fid)) + self.fid_note)

    def sample_active_subnet(self):
        use_timestep = [i for i in range(self.sampler.ddpm_num_timesteps)]
        random.shuffle(use_timestep)
        return use_timestep[:self.time_step]

    def sample_active_subnet_dpm(self):
        use_timestep = copy.deepcopy(self.dpm_params['full_timesteps'])
        random.shuffle(use_timestep)
        return use_timestep[:self.time_step + 1]

    def _fill_random(self, num, legal):
        logger.log('random select ........')
        while len(self.candidates) < num:
            cand = self.sample_active_subnet_dpm() if self.dpm_solver else self.sample_active_subnet()
            cand = str(sorted(cand))
            if not legal(cand):
                continue
            self.candidates.append(cand)
            logger.log('random {}/{}'.format(len(self.candidates), num))
        logger.log('random_num = {}'.format(len(self.candidates)))

    def get_random_before_search(self, num):
        self._fill_random(num, self.is_legal_before_search)

    def get_random(self, num):
        self._fill_random(num, self.is_legal)

    def _collect(self, what, num, make, legal):
        """The retry loop of every operator: up to 10 * num tries of `make()`, keeping the candidates that are `legal`."""
        logger.log(what + ' ......')
        res = []
        max_iters = num * 10
        while len(res) < num and max_iters > 0:
            max_iters -= 1
            cand = str(sorted(make()))
            if not legal(cand):
                continue
            res.append(cand)
            logger.log('{} {}/{}'.format(what, len(res), num))
        logger.log('{}_num = {}'.format(what.split()[0], len(res)))   # 'mutation x0' counts as mutation_num, as in the reference
        return res

    def get_cross(self, k, cross_num):
        assert k in self.keep_top_k

        def random_cross():
            cand1 = parse_sd_candidate(choice(self.keep_top_k[k]))
            cand2 = parse_sd_candidate(choice(self.keep_top_k[k]))
            return [cand1[i] if np.random.random_sample() < 0.5 else cand2[i] for i in range(len(cand1))]
        return self._collect('cross', cross_num, random_cross, self.is_legal)

    @staticmethod
    def _mutate(cand, pool, m_prob):
        candidates = [i for i in pool if i not in cand]
        for i in range(len(cand)):
            if np.random.random_sample() < m_prob:
                new_c = random.choice(candidates)
                del candidates[candidates.index(new_c)]
                cand[i] = new_c
                if len(candidates) == 0:
                    break
        return cand

    def get_mutation(self, k, mutation_num, m_prob):
        assert k in self.keep_top_k
        return self._collect('mutation', mutation_num, lambda: self._mutate(
            parse_sd_candidate(choice(self.keep_top_k[k])), range(self.sampler.ddpm_num_timesteps), m_prob), self.is_legal)

    def get_mutation_dpm(self, k, mutation_num, m_prob):
        assert k in self.keep_top_k
        return self._collect('mutation', mutation_num, lambda: self._mutate(
            parse_sd_candidate(choice(self.keep_top_k[k])), self.dpm_params['full_timesteps'], m_prob), self.is_legal)

    def mutate_init_x(self, x0, mutation_num, m_prob):
        return self._collect('mutation x0', mutation_num, lambda: self._mutate(
            parse_sd_candidate(x0), range(self.sampler.ddpm_num_timesteps), m_prob), self.is_legal_before_search)

    def mutate_init_x_dpm(self, x0, mutation_num, m_prob):
        return self._collect('mutation x0', mutation_num, lambda: self._mutate(
            parse_sd_candidate(x0), self.dpm_params['full_timesteps'], m_prob), self.is_legal_before_search)

    def initial_candidate(self):
        """The evenly spaced schedule that ``use_ddim_init_x`` seeds the population with, sorted, as plain Python numbers."""
        if self.dpm_solver:
            init_x = self.dpm_params['init_timesteps']
        else:
            init_x = make_ddim_timesteps(ddim_discr_method=self.ddim_discretize, num_ddim_timesteps=self.time_step,
                                         num_ddpm_timesteps=self.sampler.ddpm_num_timesteps, verbose=False)
        return sorted(_plain(v) for v in init_x)

    def search(self):
        logger.log('population_num = {} select_num = {} mutation_num = {} crossover_num = {} random_num = {} max_epochs = {}'.format(
            self.population_num, self.select_num, self.mutation_num, self.crossover_num,
            self.population_num - self.mutation_num - self.crossover_num, self.max_epochs))
        if self.use_ddim_init_x is False:
            self.get_random_before_search(self.population_num)
        else:
            init_x = str(self.initial_candidate())
            self.is_legal_before_search(init_x)
            self.candidates.append(init_x)
            self.get_random_before_search(self.population_num // 2)
            mutate = self.mutate_init_x_dpm if self.dpm_solver else self.mutate_init_x
            self.candidates += mutate(x0=init_x, mutation_num=self.population_num - self.population_num // 2 - 1, m_prob=0.1)
        while self.epoch < self.max_epochs:
            logger.log('epoch = {}'.format(self.epoch))
            self.flush_pending()
            self.update_top_k(self.candidates, k=self.select_num, key=lambda x: self.vis_dict[x]['fid'])
            self.update_top_k(self.candidates, k=50, key=lambda x: self.vis_dict[x]['fid'])
            logger.log('epoch = {} : top {} result'.format(self.epoch, len(self.keep_top_k[50])))
            for i, cand in enumerate(self.keep_top_k[50]):
                logger.log('No.{} {} fid = {}'.format(i + 1, cand, self.vis_dict[cand]['fid']) + self.fid_note)
            if self.epoch + 1 == self.max_epochs:
                break
            mutate = self.get_mutation_dpm if self.dpm_solver else self.get_mutation
            self.candidates = mutate(self.select_num, self.mutation_num, self.m_prob)
            self.candidates += self.get_cross(self.select_num, self.crossover_num)
            self.get_random(self.population_num)
            self.epoch += 1
        self.flush_pending()


class _Steps:
    """What search.py's operators read from the diffusion they search over."""

    def __init__(self, original_num_steps):
        self.original_num_steps = int(original_num_steps)


class DynamicEvolutionSearcher(adm_search.DynamicEvolutionSearcher):
    """Joint search over timesteps and per-step layer-skip lists of the latent UNet, DDIM / PLMS (integer timesteps).  The
    operators, the order of RNG draws, the budget (``max_index_number = time_step * layer_num``, or ``index_step``), the
    progressive ``skip_layer_range``, the bookkeeping and the log lines are ``search.DynamicEvolutionSearcher``'s, inherited; what
    is set here is the space (``original_num_steps = sampler.ddpm_num_timesteps``, ``model_layers = unet.layer_num``) and the
    evaluation, which goes through ``SDCandidateEvaluator``.  With ``population_parallel`` the queued dict candidates are assigned
    by search.py's cost-aware rule (``flush_pending``: longest first to the least-loaded rank)."""

    def __init__(self, opt, model, time_step, ref_mu, ref_sigma, sampler, dataloader_info, batch_size, dpm_params=None, *,
                 evaluator=None, population_parallel=False, inception=None, features=None, allow_random_inception=False,
                 clip_scorer=None, fitness="fid", ref_feats=None, ref_clip_feats=None, index_step=None, layer_num=None):
        if getattr(opt, "dpm_solver", False) or getattr(opt, "unipc", False) or dpm_params is not None:
            raise ValueError("the joint timestep / layer-skip search is built for the integer timestep space (DDIM / PLMS): "
                             "not together with opt.dpm_solver / opt.unipc")
        if evaluator is None:
            from .sd_evaluate import SDCandidateEvaluator
            evaluator = SDCandidateEvaluator(
                model, sampler, ref_mu=np.load(ref_mu) if isinstance(ref_mu, (str, os.PathLike)) else ref_mu,
                ref_sigma=np.load(ref_sigma) if isinstance(ref_sigma, (str, os.PathLike)) else ref_sigma, num_samples=opt.num_sample,
                prompts=_Texts(dataloader_info['validation_loader']), features=features, inception=inception,
                allow_random_inception=allow_random_inception, seed=int(getattr(opt, "seed", 0)), clip_scorer=clip_scorer,
                fitness=fitness, ref_feats=ref_feats, ref_clip_feats=ref_clip_feats, image_sharded=not population_parallel)
        if layer_num is None:
            layer_num = getattr(getattr(model, "model", None), "layer_num", None) or getattr(evaluator, "layer_num", None)
        if not layer_num:
            raise ValueError("the joint search needs the UNet's layer_num (model.model.layer_num, the evaluator's, or layer_num=)")
        args = copy.copy(opt)               # search.py's names for what it reads from the argument namespace
        args.layer_num = int(layer_num)
        args.time_step = time_step
        args.use_ddim = True
        args.fitness = "fid"                # the evaluator owns the fitness; search.py only sorts by the value
        # model=None: search.py builds no ADM evaluator; base_diffusion: only its original_num_steps is read
        super().__init__(args, None, _Steps(sampler.ddpm_num_timesteps), time_step, index_step=index_step,
                         population_parallel=population_parallel)
        self.opt, self.model, self.sampler = opt, model, sampler
        self.dataloader_info, self.batch_size = dataloader_info, batch_size
        self.evaluator = self._ev = evaluator      # _ev: flush_pending reads its .device for the all_gather
        self.fid_note = getattr(evaluator, "fid_note", "")

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
