"""The evolutionary-algorithm driver shared by the ADM searches (search.py) and the Stable-Diffusion ones (sd_search.py).

``EvolutionDriver`` owns the EA and knows nothing about how a candidate is scored: the visited-set dedupe, the top-k lists, the
population-parallel queue with its cost-aware assignment and single ``all_gather``, the operators and the ``search()`` loop.  The
order in which the operators consume ``random`` / ``np.random`` and the text of the log lines are the data contract with the
reference's drivers (search_imagenet64_classifier_guidance.py:155-584, search_uncondition_model.py, "Stable Diffusion"/scripts/
search_ea.py:184-633); tests/golden/{ea_trajectory,ea_dynamic_trajectory,sd_ea_trajectory}.npz pin them, and this is their one copy.

A searcher derives from it and supplies
  * ``parse``: candidate text -> candidate;
  * ``canonical(cand)``: the string a candidate is stored and deduplicated under, and ``_key(text)``: the same for text handed to
    ``is_legal*`` from outside;
  * ``space()``: ``(pool, n)`` -- an individual is ``n`` members of ``pool``; ``shuffle_space_in_place`` says whether drawing one
    shuffles a list pool itself (the reference's ADM scripts do, and later ``random.choice`` results depend on it) or a copy;
  * ``num_timesteps``, ``initial_candidate()`` (the evenly spaced schedule of ``use_ddim_init_x``), ``gather_device()``;
  * ``get_cand_fid``, called as ``self.get_cand_fid(cand=..., <fid_keyword>=self.args)``, looked up on the instance at every call.

``JointSearch`` holds the operators of the joint timestep / layer-skip search (search_dynamic_unet_imagenet64_classifier_guidance_
progressive.py:155-715) as a mixin over either package's flat searcher.
"""
from __future__ import annotations

import random
import time

import numpy as np
import torch

from . import dist_util, logger
from .evaluate import parse_candidate, parse_index_step

choice = lambda x: x[np.random.randint(len(x))] if isinstance(x, tuple) else choice(tuple(x))  # noqa: E731


class EvolutionDriver(object):
    parse = staticmethod(parse_candidate)
    fid_keyword = "args"             # the keyword get_cand_fid receives the argument namespace under
    shuffle_space_in_place = False

    def __init__(self, args, population_parallel=False):
        self.args = args
        self.max_epochs = args.max_epochs
        self.select_num = args.select_num
        self.population_num = args.population_num
        self.m_prob = args.m_prob
        self.crossover_num = args.crossover_num
        self.mutation_num = args.mutation_num
        self.use_ddim_init_x = getattr(args, "use_ddim_init_x", False)
        self.keep_top_k = {self.select_num: [], 50: []}
        self.epoch = 0
        self.candidates = []
        self.vis_dict = {}
        self.x0 = getattr(args, "init_x", "")
        # "guided" seeds pop//2 + 1 random candidates next to the init candidate and breeds after the last epoch too;
        # "unconditional" seeds pop//2 and stops before the last epoch's offspring (search_uncondition_model.py:509-532, :554-555)
        self.variant = "guided"
        self.break_at_last_epoch = False
        self.fid_note = ""
        # population parallelism: within an epoch candidate GENERATION never looks at
        # FID values (legality is only the visited-set dedupe; parents are the top-k frozen at epoch start),
        # so candidates are generated first -- with the reference's exact random / np.random draw order, on
        # every rank identically -- queued, then evaluated each on ONE rank (whole-candidate
        # FID local to one GPU) and the FIDs are all-gathered back in order.
        self.population_parallel = population_parallel
        self._pending = []
        self.last_flush = None

    # ------------------------------------------------------------------ what a searcher supplies
    def canonical(self, cand):
        return str(cand)

    def _key(self, text):
        return text

    def space(self):
        return range(self.num_timesteps), self.time_step

    def gather_device(self):
        """The device flush_pending's all_gather buffer lives on under the nccl backend (None: the host)."""
        return None

    def _fitness(self, cand):
        return self.get_cand_fid(**{self.fid_keyword: self.args, "cand": cand})

    # ------------------------------------------------------------------ EA bookkeeping (reference order of RNG draws)
    def update_top_k(self, candidates, *, k, key, reverse=False):
        assert k in self.keep_top_k
        logger.log('select ......')
        t = self.keep_top_k[k]
        t += candidates
        t.sort(key=key, reverse=reverse)
        self.keep_top_k[k] = t[:k]

    def _visit(self, cand):
        cand = self._key(cand)
        if cand not in self.vis_dict:
            self.vis_dict[cand] = {}
        info = self.vis_dict[cand]
        if 'visited' in info:
            logger.log('cand: {} has visited!'.format(cand))
            return False
        if self.population_parallel:
            self._pending.append(cand)  # evaluated by flush_pending(), sharded over ranks
        else:
            info['fid'] = self._fitness(self.parse(cand))
            logger.log('cand: {}, fid: {}'.format(cand, info['fid']) + self.fid_note)
        info['visited'] = True
        return True

    def is_legal_before_search(self, cand):
        return self._visit(cand)

    def is_legal(self, cand):
        return self._visit(cand)

    def candidate_cost(self, cand) -> int:
        """Relative cost of evaluating a candidate = UNet layer evaluations per image: every step costs `layer_num`
        minus its skipped layers (a plain timestep list: one unit per step)."""
        if isinstance(cand, dict):
            L = int(getattr(self, "model_layers", 0) or getattr(getattr(self, "model", None), "layer_num", 0)
                    or getattr(self.args, "layer_num", 0) or 1)
            return sum(max(1, L - len(sk)) for sk in cand["skip_layers"])
        return len(cand)

    @staticmethod
    def assign_candidates(costs, world):
        """Longest-processing-time-first: candidates sorted by cost (descending, ties by index) go one by one to the
        least-loaded rank (ties: lowest rank).  Deterministic, so every rank derives the same owner list with no
        communication; layer-skip candidates are cheaper, and round-robin left ranks finishing unevenly.  With equal
        costs (every flat candidate of one search) the owner of candidate i is i % world."""
        owner = [0] * len(costs)
        load = [0] * world
        for i in sorted(range(len(costs)), key=lambda j: (-costs[j], j)):
            r = min(range(world), key=lambda q: (load[q], q))
            owner[i] = r
            load[r] += costs[i]
        return owner

    def flush_pending(self):
        """Evaluate every queued candidate, each on ONE rank (cost-aware assignment); one all_gather of the FIDs."""
        if not self._pending:
            return
        import torch.distributed as dist
        multi = dist_util.collectives_on()   # > 1 rank (or a forced world-size-1 group: the same calls through RCCL on one GPU)
        world = dist.get_world_size() if multi else 1
        rank = dist.get_rank() if multi else 0
        pending, self._pending = self._pending, []
        cands = [self.parse(c) for c in pending]
        costs = [self.candidate_cost(c) for c in cands]
        owner = self.assign_candidates(costs, world)
        fids = np.zeros(len(pending), dtype=np.float64)
        t0 = time.time()
        for i, c in enumerate(cands):
            if owner[i] == rank:
                fids[i] = self._fitness(c)
        mine_s = time.time() - t0
        coll = None
        if multi:
            dev = self.gather_device() if dist.get_backend() == "nccl" else None
            mine = torch.from_numpy(fids).to(dev if dev is not None else torch.device("cpu"))
            parts = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            coll = {"op": "all_gather", "backend": dist.get_backend(), "world_size": world, "bytes_per_rank": int(mine.numel() * 8),
                    "device": str(mine.device)}
            for i in range(len(pending)):
                fids[i] = float(parts[owner[i]][i])
            logger.log(f"collective: all_gather of {len(pending)} candidate FIDs, backend {coll['backend']}, {world} rank(s), on {coll['device']}")
        # what this epoch's evaluation looked like from this rank (bench.py --workload population reports it per rank)
        self.last_flush = {"candidates": len(pending), "owner": owner, "costs": costs,
                           "assigned": sum(1 for o in owner if o == rank), "assigned_cost": sum(c for c, o in zip(costs, owner) if o == rank),
                           "evaluate_s": mine_s, "collective": coll}
        for cand, fid in zip(pending, fids):
            self.vis_dict[cand]['fid'] = float(fid)
            logger.log('cand: {}, fid: {}'.format(cand, float(fid)) + self.fid_note)

    # ------------------------------------------------------------------ operators (reference order of RNG draws)
    def sample_active_subnet(self):
        pool, n = self.space()
        if not (self.shuffle_space_in_place and isinstance(pool, list)):
            pool = list(pool)
        random.shuffle(pool)
        return pool[:n]

    def _fill_random(self, num, legal):
        logger.log('random select ........')
        while len(self.candidates) < num:
            cand = self.canonical(self.sample_active_subnet())
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
            cand = self.canonical(make())
            if not legal(cand):
                continue
            res.append(cand)
            logger.log('{} {}/{}'.format(what, len(res), num))
        logger.log('{}_num = {}'.format(what.split()[0], len(res)))   # 'mutation x0' counts as mutation_num, as in the reference
        return res

    def _cross(self, cand1, cand2):
        return [cand1[i] if np.random.random_sample() < 0.5 else cand2[i] for i in range(len(cand1))]

    def get_cross(self, k, cross_num):
        assert k in self.keep_top_k

        def make():
            cand1 = self.parse(choice(self.keep_top_k[k]))
            cand2 = self.parse(choice(self.keep_top_k[k]))
            return self._cross(cand1, cand2)
        return self._collect('cross', cross_num, make, self.is_legal)

    def _mutate(self, cand, m_prob):
        candidates = [i for i in self.space()[0] if i not in cand]
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
        return self._collect('mutation', mutation_num, lambda: self._mutate(self.parse(choice(self.keep_top_k[k])), m_prob), self.is_legal)

    def mutate_init_x(self, x0, mutation_num, m_prob):
        return self._collect('mutation x0', mutation_num, lambda: self._mutate(self.parse(x0), m_prob), self.is_legal_before_search)

    # ------------------------------------------------------------------ the loop
    def _initial_candidate(self, steps):
        """The candidate of the evenly spaced schedule that --use_ddim_init_x seeds the population with."""
        return steps

    def _after_selection(self):
        """Hook between an epoch's top list and its offspring (the joint search opens its skip range here)."""

    def search(self):
        logger.log('population_num = {} select_num = {} mutation_num = {} crossover_num = {} random_num = {} max_epochs = {}'.format(
            self.population_num, self.select_num, self.mutation_num, self.crossover_num,
            self.population_num - self.mutation_num - self.crossover_num, self.max_epochs))
        if self.x0 != '':  # search_uncondition_model.py:509-512
            self.get_random_before_search(self.population_num // 2)
            self.candidates += self.mutate_init_x(x0=self.x0, mutation_num=self.population_num - self.population_num // 2,
                                                  m_prob=0.05)
        elif self.use_ddim_init_x is False:
            self.get_random_before_search(self.population_num)
        else:
            init_x = self.canonical(self._initial_candidate(self.initial_candidate()))
            self.is_legal_before_search(init_x)
            self.candidates.append(init_x)
            # the guided script seeds pop//2 + 1 random candidates, the unconditional and the SD one pop//2
            extra = 0 if self.variant == "unconditional" else 1
            self.get_random_before_search(self.population_num // 2 + extra)
            self.candidates += self.mutate_init_x(x0=init_x, mutation_num=self.population_num - self.population_num // 2 - 1,
                                                  m_prob=0.1)
        while self.epoch < self.max_epochs:
            logger.log('epoch = {}'.format(self.epoch))
            self.flush_pending()
            self.update_top_k(self.candidates, k=self.select_num, key=lambda x: self.vis_dict[x]['fid'])
            self.update_top_k(self.candidates, k=50, key=lambda x: self.vis_dict[x]['fid'])
            logger.log('epoch = {} : top {} result'.format(self.epoch, len(self.keep_top_k[50])))
            for i, cand in enumerate(self.keep_top_k[50]):
                logger.log('No.{} {} fid = {}'.format(i + 1, cand, self.vis_dict[cand]['fid']) + self.fid_note)
            self._after_selection()
            if self.break_at_last_epoch and self.epoch + 1 == self.max_epochs:
                break
            self.candidates = self.get_mutation(self.select_num, self.mutation_num, self.m_prob)
            self.candidates += self.get_cross(self.select_num, self.crossover_num)
            self.get_random(self.population_num)
            self.epoch += 1
        self.flush_pending()


class JointSearch(object):
    """Joint search over timesteps AND per-step layer-skip lists of a dynamic UNet: the operators of the reference's
    search_dynamic_unet_imagenet64_classifier_guidance_progressive.py (EvolutionSearcher, :155-715), as a mixin in front of a
    flat searcher built on ``EvolutionDriver``.  They read ``model_layers``, ``num_timesteps`` and the driver, nothing else.

    A candidate is ``{'timesteps': [t_0, ...], 'skip_layers': [[layer ids skipped at t_0], ...]}``; its budget is
    ``max_index_number`` = time_step * layer_num evaluated layers (or ``index_step``).  The fraction of layers a step may
    skip is drawn from ``skip_layer_range``, which the search opens progressively: [0, 0] until the best candidate
    stalls (or epoch 5), then the upper end grows by max_prun / 5 per epoch up to max_prun, and from epoch 6 the lower end
    is min_prun (:684-692).  Every operator consumes ``random`` / ``np.random`` in the reference's order, including its
    quirks -- the list comparison that decides whether a crossover child is padded from a parent (:494-500) and the
    skip-list mutation that draws its replacement but leaves the list unchanged (``==`` at :568, :632) -- because the
    candidate sequence is the data contract (pinned by tests/golden/ea_dynamic_trajectory.npz).
    """

    def _init_joint(self, model_layers, time_step, index_step=None):
        """After the flat searcher's constructor: the budget, the closed skip range, and search() as the dynamic script runs it."""
        self.init_time_step = time_step
        self.model_layers = int(model_layers)
        self.max_index_number = time_step * self.model_layers
        if index_step is not None:
            self.max_index_number = parse_index_step(index_step)
        self.max_prun = self.args.max_prun
        self.min_prun = self.args.min_prun
        self.skip_layer_range = [0, 0]
        self.last_best_cand = None
        self.variant = "guided"            # pop//2 + 1 random candidates next to init_x,
        self.x0 = ''                       # no --init_x branch,
        self.break_at_last_epoch = True    # and always a stop before the last epoch's offspring (:701)

    def cand2gen(self, cand):
        """Flat index encoding (layer + layer_num * timestep of every evaluated layer), zero-padded (:207-217)."""
        ret = []
        for t, skipped in zip(cand['timesteps'], cand['skip_layers']):
            kept = [k for k in range(self.model_layers) if k not in skipped]
            ret += [k + self.model_layers * t for k in kept]
        return ret + [0] * max(0, self.max_index_number - len(ret))

    # ------------------------------------------------------------------ operators (reference order of RNG draws)
    def _draw_skips(self, count):
        layers = [i for i in range(self.model_layers)]
        random.shuffle(layers)
        return layers[:count]

    def sample_active_subnet(self):
        lo, hi = self.skip_layer_range
        L, budget = self.model_layers, self.max_index_number
        use_timestep = [i for i in range(self.num_timesteps)]
        random.shuffle(use_timestep)
        used, timesteps, skips = 0, [], []
        while True:
            n_skip = None
            tries = 0
            while n_skip is None or used + L - n_skip > budget:   # redraw until this step fits the budget
                n_skip = int((np.random.random_sample() * (hi - lo) + lo) * L)
                tries += 1
                if tries > 10 ** 6:
                    raise RuntimeError("sample_active_subnet: no skip count fits the index budget")
            skips.append(self._draw_skips(n_skip))
            timesteps.append(use_timestep[len(timesteps)])
            used += L - n_skip
            least = L - int(L * hi)                                # the cheapest step still allowed
            if used + least > budget:
                break
            if used + least == budget:                             # exactly one maximally pruned step fits
                skips.append(self._draw_skips(int(L * hi)))
                timesteps.append(use_timestep[len(timesteps)])
                break
        return {'timesteps': timesteps, 'skip_layers': skips}

    def _mutate_timesteps(self, cand, m_prob):
        pool = [i for i in range(self.num_timesteps) if i not in cand['timesteps']]
        for i in range(len(cand['timesteps'])):
            if np.random.random_sample() < m_prob:
                new_c = random.choice(pool)
                del pool[pool.index(new_c)]
                cand['timesteps'][i] = new_c
                if len(pool) == 0:
                    break

    def _touch_skips(self, skipped, m_prob):
        """The reference draws a replacement layer per mutated entry but never stores it: RNG draws only."""
        pool = [j for j in range(self.model_layers) if j not in skipped]
        for _ in range(len(skipped)):
            if np.random.random_sample() < m_prob:
                new_c = random.choice(pool)
                del pool[pool.index(new_c)]
                if len(pool) == 0:
                    break

    def _mutate(self, cand, m_prob, fill_empty=True):
        self._mutate_timesteps(cand, m_prob)
        if self.skip_layer_range[1] == 0:
            return cand
        lo, hi = self.skip_layer_range
        for i in range(len(cand['skip_layers'])):
            if fill_empty and len(cand['skip_layers'][i]) == 0:
                if np.random.random_sample() < m_prob:             # an unpruned step gets a fresh skip list
                    n_skip = int((np.random.random_sample() * (hi - lo) + lo) * self.model_layers)
                    cand['skip_layers'][i] = self._draw_skips(n_skip)
            else:
                self._touch_skips(cand['skip_layers'][i], m_prob)
        return cand

    def _cross(self, cand1, cand2):
        child = {'timesteps': [], 'skip_layers': []}
        for i in range(min(len(cand1['timesteps']), len(cand2['timesteps']))):
            src = cand1 if np.random.random_sample() < 0.5 else cand2
            child['timesteps'].append(src['timesteps'][i])
            child['skip_layers'].append(src['skip_layers'][i])
        for parent in (cand1, cand2):                          # list (lexicographic) comparison, as in the reference
            if child['timesteps'] < parent['timesteps']:
                child['timesteps'] += parent['timesteps'][len(child['timesteps']):]
                child['skip_layers'] += parent['skip_layers'][len(child['skip_layers']):]
        return child

    def mutate_init_x(self, x0, mutation_num, m_prob):
        return self._collect('mutation x0', mutation_num, lambda: self._mutate(self.parse(x0), m_prob, fill_empty=False),
                             self.is_legal_before_search)

    def _initial_candidate(self, steps):
        return {'timesteps': steps, 'skip_layers': [[] for _ in steps]}

    def _after_selection(self):
        """The progressive skip-layer range (:684-692), from this epoch's best candidate."""
        best = self.keep_top_k[50][0]
        if self.skip_layer_range[1] == 0 and (self.last_best_cand == best or self.epoch > 4):
            self.skip_layer_range[1] = self.max_prun / 5
        elif 0 < self.skip_layer_range[1] < self.max_prun:
            self.skip_layer_range[1] += self.max_prun / 5
        if self.skip_layer_range[0] == 0 and self.epoch > 5:
            self.skip_layer_range[0] = self.min_prun
        self.last_best_cand = best
        logger.log('skip_layer_range_left = {} , skip_layer_range_right {}'.format(*self.skip_layer_range))
