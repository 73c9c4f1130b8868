"""CPU: the one statement of "how a candidate's images are produced in rounds" (evaluate.batch_plan), the loop that walks it
(CandidateEvaluator.sample_plan) under its two users' seed formulas, the single sampling body, and the literal parsers that
replaced eval() on candidate strings and list flags.  Expected values are worked out from the formulas, not from a run."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from autodiffusion_amd import evaluate, logger, search
from autodiffusion_amd.evaluate import (CandidateEvaluator, batch_plan, parse_candidate, parse_index_step,
                                        parse_int_list)
from autodiffusion_amd.fid import FIDStatistics
from autodiffusion_amd.script_util import candidate_from_flags, create_gaussian_diffusion, gather_batches


def test_batch_plan_rounds_merging_sharding_and_keep_counts():
    assert batch_plan(10, 4, 1, 0) == [[(0, 4), (1, 4), (2, 2)]]
    assert batch_plan(10, 4, 2, 0) == [[(0, 4), (2, 2)]]
    assert batch_plan(10, 4, 2, 1) == [[(1, 4), (3, 0)]]            # a batch that keeps nothing is still sampled
    assert batch_plan(6, 4, 1, 0, 64, merge_batches=1) == [[(0, 4)], [(1, 2)]]
    p = batch_plan(5000, 100, 1, 0)
    assert [len(x) for x in p] == [2] * 25 and p[-1] == [(48, 100), (49, 100)]
    p = batch_plan(5000, 100, 8, 3)
    assert [len(x) for x in p] == [2, 2, 2, 1] and p[0] == [(3, 100), (11, 100)] and p[-1] == [(51, 0)]
    p = batch_plan(1000, 32, 1, 0, 128)
    assert [len(x) for x in p] == [4] * 8 and p[-1][-1] == (31, 8)
    # over all ranks the kept images are exactly num_samples, every global index once
    for n, b, w in ((10, 4, 2), (5000, 100, 8), (7, 3, 4)):
        flat = [gk for r in range(w) for x in batch_plan(n, b, w, r) for gk in x]
        assert sorted(g for g, _ in flat) == list(range(-(-n // (b * w)) * w)) and sum(k for _, k in flat) == n


class _Stub(CandidateEvaluator):
    """Records every sampling call; the images of the batch seeded s are all (s % 251)."""

    def __init__(self, image_size=64):
        self.image_size, self.device, self.calls, self._merge_logged = image_size, torch.device("cpu"), [], False

    def set_candidate(self, cand):
        return self

    def sample_batches(self, batch_size, seeds):
        self.calls.append((batch_size, list(seeds)))
        self.last_classes = torch.cat([torch.full((batch_size,), s_ % 1000, dtype=torch.int64) for s_ in seeds])
        return [torch.full((batch_size, self.image_size, self.image_size, 3), s_ % 251, dtype=torch.uint8) for s_ in seeds]

    def sample_batch(self, batch_size, seed=None, return_float=False):
        return self.sample_batches(batch_size, [seed])[0]


def test_sampling_cli_loop_asks_for_the_cli_seeds_one_call_per_pass(monkeypatch):
    lines = []
    monkeypatch.setattr(logger, "log", lambda *a: lines.append(" ".join(map(str, a))))
    ev = _Stub()
    args = SimpleNamespace(num_samples=10, batch_size=4, seed=3, merge_batches=0)
    images, labels = gather_batches(ev, args)
    assert ev.calls == [(4, [3 * 1000003 + g for g in (0, 1, 2)])]
    assert [int(i[0, 0, 0, 0]) for i in images] == [(3 * 1000003 + g) % 251 for g in (0, 1, 2)] and len(labels) == 3
    assert lines == ["evaluating 3 batches of 4 per pass (12 images per pass; bitwise the images of separate passes)",
                     "created 4 samples", "created 8 samples", "created 12 samples"]
    ev.calls, args.merge_batches = [], 2
    del lines[:]
    gather_batches(ev, args)
    assert ev.calls == [(4, [3000009, 3000010]), (4, [3000011])]
    assert lines == ["created 4 samples", "created 8 samples", "created 12 samples"]     # the merge line: once per evaluator
    # a rank of a sharded run: the keep counts of the plan ride along with the batches
    got = list(_Stub().sample_plan(10, 4, lambda g: 100 + g, world=2, rank=1, merge_log="{merge}/{batch_size}/{per_pass}"))
    assert [k for _, _, k in got] == [4, 0] and [int(u[0, 0, 0, 0]) for u, _, _ in got] == [101, 103]
    assert [c.tolist() for _, c, _ in got] == [[101] * 4, [103] * 4]
    assert lines[-3:] == ["2/4/8", "created 8 samples", "created 16 samples"]


def test_get_cand_fid_asks_for_the_search_seeds_and_keeps_arr_num_samples(monkeypatch):
    lines = []
    monkeypatch.setattr(logger, "log", lambda *a: lines.append(" ".join(map(str, a))))
    seen = []

    class HostEvaluator:
        def compute_activations(self, batches, batch_size):
            seen.append(batches[:, 0, 0, 0].tolist())
            pool = np.random.RandomState(0).randn(batches.shape[0], 8)
            return pool, pool[:, :3]

    args = SimpleNamespace(max_epochs=1, select_num=2, population_num=3, m_prob=0.25, crossover_num=1, mutation_num=1,
                           batch_size=4, num_samples=10, image_size=64, use_ddim=True, clip_denoised=True, class_cond=True,
                           seed=5, time_step=4, merge_batches=2)
    s = search.EvolutionSearcher(args, None, create_gaussian_diffusion(steps=1000), 4, evaluator=HostEvaluator(),
                                 ref_stats=FIDStatistics(np.zeros(8), np.eye(8)))
    s._ev = _Stub()
    cand = [153, 424, 926, 690]
    seed0 = (5 * 1000003 + zlib.crc32(str(cand).encode())) & 0x7FFFFFFF
    for _ in range(2):
        assert np.isfinite(s.get_cand_fid(cand=cand, args=args))
    want = [seed0 + 7919 * g for g in range(3)]
    assert s._ev.calls == [(4, want[:2]), (4, want[2:])] * 2 and s.last_times["batches_this_rank"] == 3
    assert seen[0] == [want[0] % 251] * 4 + [want[1] % 251] * 4 + [want[2] % 251] * 2       # arr[:num_samples]
    assert lines[:6] == ["sampling...", search.MERGE_LOG.format(merge=2, batch_size=4, per_pass=8), "created 4 samples",
                         "created 8 samples", "created 12 samples", "sampling complete"]
    assert "restores the reference's launch unit" in lines[1] and sum("per pass" in l for l in lines) == 1   # once per search


def test_one_sampling_body_draw_order_and_generator_reset():
    """sample_batch / sample_batches on a recording diffusion object: labels then x_T per generator, the per-step generators handed
    to the loop (one generator; a list of (generator, images) when merged; None for the global RNG) and taken back afterwards,
    also when the loop raises."""
    seen = {}

    def loop(model_fn, shape, noise=None, clip_denoised=True, model_kwargs=None, cond_fn=None, device=None):
        seen.update(shape=shape, noise=noise, y=model_kwargs["y"], generator=d.generator, cond_fn=cond_fn)
        if seen.get("fail"):
            raise RuntimeError("loop failed")
        d.last_uint8_nhwc = torch.zeros(shape[0], 8, 8, 3, dtype=torch.uint8)
        return noise * 2

    d = SimpleNamespace(generator=None, ddim_sample_loop=loop)
    ev = CandidateEvaluator.__new__(CandidateEvaluator)
    ev.device, ev.image_size, ev.active_diffusion, ev.skip_layers = torch.device("cpu"), 8, d, None
    ev.use_ddim, ev.clip_denoised, ev.classifier = True, True, None

    def draws(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, 1000, (2,), generator=g), torch.randn(2, 3, 8, 8, generator=g)

    u8, sample = ev.sample_batch(2, seed=7, return_float=True)
    y7, x7 = draws(7)
    assert torch.equal(seen["y"], y7) and torch.equal(seen["noise"], x7) and torch.equal(sample, x7 * 2) and u8.shape == (2, 8, 8, 3)
    assert isinstance(seen["generator"], torch.Generator) and d.generator is None and torch.equal(ev.last_classes, y7)
    outs = ev.sample_batches(2, [7, 9])
    y9, x9 = draws(9)
    assert len(outs) == 2 and seen["shape"] == (4, 3, 8, 8) and torch.equal(seen["y"], torch.cat([y7, y9]))
    assert torch.equal(seen["noise"], torch.cat([x7, x9])) and [n for _, n in seen["generator"]] == [2, 2] and d.generator is None
    torch.manual_seed(3)
    ev.sample_batch(2)                                    # seed=None: the global RNG, no generator for the loop
    torch.manual_seed(3)
    assert torch.equal(seen["y"], torch.randint(0, 1000, (2,))) and seen["generator"] is None
    seen["fail"] = True
    with pytest.raises(RuntimeError):
        ev.sample_batch(2, seed=7)
    assert isinstance(seen["generator"], torch.Generator) and d.generator is None


def test_candidates_and_list_flags_are_parsed_as_literals():
    assert parse_candidate("[153, 424, 926, 690]") == [153, 424, 926, 690]
    dcand = {"timesteps": [94, 217], "skip_layers": [[1], []]}
    assert parse_candidate(str(dcand)) == dcand
    assert parse_int_list("[153.2 424.7 926.1 689.5]", "--use_timestep", use_mean=True) == [153, 425, 926, 690]
    assert parse_int_list("[[1],[],[0,5],[2,3]]", "--skip_layers", nested=True) == [[1], [], [0, 5], [2, 3]]
    assert parse_index_step("232") == 232 and parse_index_step(232) == 232 and parse_index_step(None or 5.0) == 5
    with pytest.raises(ValueError, match="--use_timestep"):
        parse_candidate("__import__('os').system('true')", "--use_timestep")
    with pytest.raises(ValueError, match="candidate"):
        parse_candidate("{'timesteps': [1, 2, 3], 'skip_layers': [[], []]}")
    with pytest.raises(ValueError, match="--index_step.*not evaluated"):
        parse_index_step("4*58")
    for bad in ("[1, 2.5]", "{'timesteps': [1]}", "7", "[[1], 2]", "[True]"):
        with pytest.raises(ValueError):
            parse_candidate(bad)
    with pytest.raises(ValueError, match="--skip_layers"):
        parse_int_list("[1, 2]", "--skip_layers", nested=True)
    with pytest.raises(ValueError, match="--search_space"):
        parse_int_list("{'timesteps': [1], 'skip_layers': [[]]}", "--search_space")
    # the CLIs' candidate: sorted steps, a dict once --skip_layers is given, the diffusion's own steps by default
    diffusion = create_gaussian_diffusion(steps=1000, timestep_respacing="ddim4")
    flags = SimpleNamespace(use_timestep="[926, 153, 690, 424]", skip_layers=None)
    assert candidate_from_flags(flags, diffusion) == [153, 424, 690, 926]
    flags.skip_layers = "[[1],[],[0,5],[2,3]]"
    assert candidate_from_flags(flags, diffusion) == {"timesteps": [153, 424, 690, 926], "skip_layers": [[1], [], [0, 5], [2, 3]]}
    assert candidate_from_flags(SimpleNamespace(use_timestep=None, skip_layers=None), diffusion) == [0, 250, 500, 750]
    assert evaluate.MERGE_LOG != search.MERGE_LOG
