"""Host: per-step layer skipping on the Stable-Diffusion path -- the layer ids of the plan, the float reference the
GPU tests compare to, the joint searcher against search.py's, the command-line forms, the evaluator's checks and the cost-aware
assignment.  Nothing here needs a device; the samplers do (their first act is to ask for one), so their routing is tested in
test_hip_sd_skip.py."""
import importlib.util
import os
import random
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from autodiffusion_amd import ea, logger, sd_script_util, sd_search, search
from autodiffusion_amd.sd_arch import (SD_V1, SD_V2, SDDownSpec, SDResBlockSpec, SDStemSpec, SDTransformerSpec, SDUpSpec,
                                       sd_unet_plan)
from oracle import sd_nets
from sd_skip_ref import sd_unet_forward_skip, tiny_sets
from test_sd_oracle import sd_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name, folder="scripts"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ layer ids
@pytest.mark.parametrize("cfg", [SD_V1, SD_V2], ids=["v1", "v2"])
def test_sd_plans_number_38_layers_in_construction_order(cfg):
    plan = sd_unet_plan(**cfg)
    assert plan.layer_num == 38
    ids = lambda seqs: [b.layer_id for seq in seqs for b in seq if isinstance(b, (SDResBlockSpec, SDTransformerSpec))]  # noqa: E731
    assert ids(plan.input_blocks) == list(range(14))
    assert ids([plan.middle_block]) == [14, 15, 16]
    assert ids(plan.output_blocks) == list(range(17, 38))
    plain = [b for b in plan.all_blocks() if isinstance(b, (SDStemSpec, SDDownSpec, SDUpSpec))]
    assert len(plain) == 1 + 3 + 3 and not any(hasattr(b, "layer_id") for b in plain)
    # ids are metadata only: the tensors and their names are what they were
    assert [b.prefix for b in plan.all_blocks() if getattr(b, "layer_id", -1) == 15] == ["middle_block.1"]
    assert not any("layer_id" in k for k in plan.param_shapes())


def test_tiny_plan_layer_count_and_the_sets_the_gpu_test_runs():
    plan = sd_unet_plan(**sd_script_util.TINY_UNET)
    assert plan.layer_num == 15       # 2 + 2 input, 3 middle, 4 x 2 output (every level has transformers)
    assert [b.layer_id for b in plan.all_blocks() if hasattr(b, "layer_id")] == list(range(15))
    sets = tiny_sets(plan)
    by_id = {b.layer_id: b for b in plan.all_blocks() if hasattr(b, "layer_id")}
    a, b, c = (by_id[sets[k][0]] for k in ("identity ResBlock of the input path", "input ResBlock with a skip conv",
                                          "output ResBlock (two-source 1x1)"))
    assert not a.has_skip_conv and b.has_skip_conv and b.prefix.startswith("input_blocks.")
    assert c.has_skip_conv and c.prefix.startswith("output_blocks.")
    assert isinstance(by_id[sets["one transformer"][0]], SDTransformerSpec)
    assert sorted(sets["every layer"]) == list(range(15)) and sets["the middle block"] == [4, 5, 6]


# ------------------------------------------------------------------ the float reference
def test_skip_reference_with_an_empty_set_is_the_oracle():
    g, plan, P = sd_case("sd_unet_tiny")
    x, t, ctx = (torch.from_numpy(g[k]) for k in ("x", "t", "context"))
    assert torch.equal(sd_unet_forward_skip(P, plan, x, t, ctx, ()), sd_nets.sd_unet_forward(P, plan, x, t, ctx))
    with pytest.raises(AssertionError):
        sd_unet_forward_skip(P, plan, x, t, ctx, [plan.layer_num])


W320_MIXED = [2, 6, 7]   # test_hip_sd_skip.py's set on the w320 plan


@pytest.mark.parametrize("name", ["sd_unet_tiny", "sd_unet_w320"])
def test_every_set_of_the_gpu_test_moves_the_float_reference_tenfold_its_bound(name):
    """The GPU test holds the skipped network to relative Frobenius 2e-2 of the skipped reference.  That shows nothing unless the
    skipped and the unskipped reference are far apart: for every set, more than ten times the bound, with fill_state_dict's weights."""
    g, plan, P = sd_case(name)
    x, t, ctx = (torch.from_numpy(g[k]) for k in ("x", "t", "context"))
    full = sd_nets.sd_unet_forward(P, plan, x, t, ctx)
    sets = tiny_sets(plan) if name == "sd_unet_tiny" else {"mixed": W320_MIXED}
    for what, skip in sets.items():
        moved = float((sd_unet_forward_skip(P, plan, x, t, ctx, skip) - full).norm() / full.norm())
        print(f"{name} {what} {skip}: fro {moved:.3f}")
        assert moved > 10 * 2e-2, (what, moved)


# ------------------------------------------------------------------ the joint searcher is search.py's
def _fitness_of(cand):
    return (zlib.crc32(str(cand).encode()) % 100003) / 1000.0


def _opt(**over):
    o = SimpleNamespace(max_epochs=8, select_num=4, population_num=10, m_prob=0.25, crossover_num=3, mutation_num=5, max_fid=48.0,
                        max_prun=0.5, min_prun=0.1, use_ddim_init_x=False, num_sample=4, seed=0, n_samples=2)
    for k, v in over.items():
        setattr(o, k, v)
    return o


class _Evaluator:
    """Stands in for SDCandidateEvaluator: records what it is handed."""
    device = torch.device("cpu")
    fid_note = ""
    layer_num = 14

    def __init__(self):
        self.seen = []

    def get_cand_fid(self, cand, opt):
        self.seen.append(cand)
        return _fitness_of(cand)

    def candidate_cost(self, cand):
        return sum(self.layer_num - len(s) for s in cand["skip_layers"])


def _sd_joint(opt, **kw):
    sampler = SimpleNamespace(ddpm_num_timesteps=1000)
    return sd_search.DynamicEvolutionSearcher(opt, None, 4, None, None, sampler, {"validation_loader": []}, opt.n_samples,
                                              evaluator=_Evaluator(), **kw)


@pytest.mark.parametrize("init,seed,epochs", [(False, 3, 8), (True, 0, 9)])
def test_joint_searcher_reproduces_search_py_value_for_value(monkeypatch, init, seed, epochs):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    runs = []
    for which in ("adm", "sd"):
        if which == "adm":
            args = SimpleNamespace(**vars(_opt(max_epochs=epochs, use_ddim_init_x=init)), use_ddim=True, time_step=4, init_x="", layer_num=14)
            s = search.DynamicEvolutionSearcher(args, model=None, base_diffusion=SimpleNamespace(original_num_steps=1000), time_step=4)
        else:
            s = _sd_joint(_opt(max_epochs=epochs, use_ddim_init_x=init))
            assert isinstance(s, ea.JointSearch) and s.model_layers == 14 and s.max_index_number == 4 * 14
        evaluated, ranges = [], []

        def fitness(cand=None, args=None, s=s, evaluated=evaluated, ranges=ranges):
            evaluated.append(str(cand))
            ranges.append(list(s.skip_layer_range))
            return _fitness_of(cand)
        s.get_cand_fid = fitness
        random.seed(seed)
        np.random.seed(seed)
        s.search()
        runs.append((evaluated, ranges, list(s.candidates), list(s.keep_top_k[50]), [s.vis_dict[c]["fid"] for c in s.keep_top_k[50]],
                     list(s.keep_top_k[4]), list(s.skip_layer_range)))
    assert runs[0] == runs[1]
    assert len(runs[0][0]) > 20 and any("skip_layers': [[]" not in c for c in runs[0][0])   # the skip range did open


def test_joint_searcher_hands_the_evaluator_sorted_steps_and_refuses_the_continuous_space(monkeypatch):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    s = _sd_joint(_opt(), index_step="40")
    assert s.max_index_number == 40
    cand = {"timesteps": [700, 20, 300], "skip_layers": [[1], [], [5, 2]]}
    assert s.get_cand_fid(cand=cand, args=s.args) == _fitness_of({"timesteps": [20, 300, 700], "skip_layers": [[], [5, 2], [1]]})
    assert s.evaluator.seen == [{"timesteps": [20, 300, 700], "skip_layers": [[], [5, 2], [1]]}]
    assert cand["timesteps"] == [700, 20, 300]       # the searcher's own candidate is not reordered
    for bad in (dict(dpm_solver=True), dict(unipc=True)):
        with pytest.raises(ValueError, match="dpm_solver / opt.unipc"):
            _sd_joint(_opt(**bad))


def test_dict_candidates_are_assigned_by_cost(monkeypatch):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    s = _sd_joint(_opt(), population_parallel=True)
    heavy = {"timesteps": [1, 2, 3, 4], "skip_layers": [[], [], [], []]}
    light = {"timesteps": [5, 6, 7, 8], "skip_layers": [list(range(7))] * 4}
    assert s.candidate_cost(heavy) == 56 and s.candidate_cost(light) == 28
    # i % world would put candidates 0 and 2 (the two heavy ones) on rank 0; the cost-aware rule separates them
    cands = [heavy, light, dict(heavy, timesteps=[9, 10, 11, 12]), dict(light, timesteps=[13, 14, 15, 16])]
    owner = s.assign_candidates([s.candidate_cost(c) for c in cands], 2)
    assert owner == [0, 0, 1, 1] and [i % 2 for i in range(4)] != owner
    assert s.assign_candidates([s.candidate_cost(heavy), s.candidate_cost(light)], 2) == [0, 1]   # a heavy and a light one: two ranks
    for c in cands:
        assert s.is_legal(str(c))
    assert s.evaluator.seen == []                     # queued, not evaluated
    s.flush_pending()
    assert s.last_flush["costs"] == [56, 28, 56, 28] and s.last_flush["owner"] == [0, 0, 0, 0]     # one rank here
    assert [s.vis_dict[str(c)]["fid"] for c in cands] == [_fitness_of(c) for c in cands]


# ------------------------------------------------------------------ command lines
def test_dict_forms_of_evaluate_and_skip_layers_parse_and_malformed_ones_name_the_flag(tmp_path, monkeypatch):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    parse = sd_search.parse_sd_candidate
    text = "{'timesteps': [10, 500], 'skip_layers': [[], [3, 1]]}"
    assert parse(text, "--evaluate") == {"timesteps": [10, 500], "skip_layers": [[], [3, 1]]}
    assert parse("[10, 500]", "--evaluate") == [10, 500] and parse("[0.5, 0.25]") == [0.5, 0.25]
    for bad in ("{'timesteps': [10, 500], 'skip_layers': [[]]}", "{'timesteps': [10, 500]}", "{'timesteps': [10], 'skip_layers': [3]}",
                "{'timesteps': [0.5], 'skip_layers': [[]]}", "{'timesteps': [1], 'skip_layers': [['a']]}", "__import__('os')"):
        with pytest.raises(ValueError, match="--evaluate"):
            parse(bad, "--evaluate")
    # --skip_layers beside --use_timestep: list i belongs to entry i as written and is returned in ascending timestep order
    read = sd_script_util.read_skip_layers
    assert read("", "", 3, "p") is None
    assert read("[[1], [], [2, 3]]", "[900, 100, 500]", 3, "p") == [[], [2, 3], [1]]
    assert read("[[1], [], [2, 3]]", "", 3, "p") == [[1], [], [2, 3]]
    for bad, steps in (("[[1], []]", 3), ("[1, 2, 3]", 3), ("[[1.5], [], []]", 3), ("[[1], [], [", 3), ("[[True], [], []]", 3)):
        with pytest.raises(SystemExit, match="--skip_layers"):
            read(bad, "[900, 100, 500]", steps, "p")
    # the scripts: the flag is absent from the namespace unless given, in all three
    for name, req in (("sd_img2img", ["--init-img", "i.npy"]), ("sd_inpaint", ["--init-img", "i.npy", "--mask", "m.npy"])):
        ap = _script(name).create_argparser()
        assert not hasattr(ap.parse_args(req), "skip_layers")
        assert ap.parse_args(req + ["--skip_layers", "[[1]]"]).skip_layers == "[[1]]"
    cli = _script("sd_search_ea")
    ap = cli.create_argparser()
    base = ap.parse_args([])
    assert not any(hasattr(base, k) for k in ("use_dynamic_unet", "max_prun", "min_prun", "index_step"))
    opt = ap.parse_args(["--use_dynamic_unet", "True", "--max_prun", "0.5", "--min_prun", "0.1", "--index_step", "120"])
    assert sd_script_util.skip_search_options(opt, "p") == (0.5, 0.1, 120)
    assert sd_script_util.skip_search_options(base, "p") is None
    for argv, word in ((["--max_prun", "0.5"], "--max_prun needs"), (["--use_dynamic_unet", "True"], "needs --max_prun"),
                       (["--use_dynamic_unet", "True", "--max_prun", "0.5", "--min_prun", "0.1", "--dpm_solver"], "not with --dpm_solver"),
                       (["--use_dynamic_unet", "True", "--max_prun", "0.5", "--min_prun", "0.1", "--index_step", "4*58"], "--index_step"),
                       (["--use_dynamic_unet", "True", "--max_prun", "0.1", "--min_prun", "0.5"], "--min_prun <= --max_prun")):
        with pytest.raises(SystemExit, match=word):
            sd_script_util.skip_search_options(ap.parse_args(argv), "p")
    # through main(): a dict --evaluate reaches the (injected) evaluator as parsed; a malformed one is refused with the flag named
    np.savez(tmp_path / "ref.npz", mu=np.zeros(4), sigma=np.eye(4))
    flags = ["--ref_mu", str(tmp_path / "ref.npz"), "--outdir", str(tmp_path / "out"), "--time_step", "2"]
    ev = _Evaluator()
    want = {"timesteps": [10, 500], "skip_layers": [[], [3, 1]]}
    assert cli.main(flags + ["--evaluate", text], evaluator=ev) == _fitness_of(want) and ev.seen == [want]
    with pytest.raises(SystemExit, match="--evaluate"):
        cli.main(flags + ["--evaluate", "{'timesteps': [10, 500], 'skip_layers': [[]]}"], evaluator=_Evaluator())
    with pytest.raises(SystemExit, match="DDIM / PLMS"):
        cli.main(flags + ["--dpm_solver", "--evaluate", text], evaluator=_Evaluator())
    # ... and --use_dynamic_unet True runs the joint searcher to its top list of dict candidates
    ev = _Evaluator()
    random.seed(1)
    np.random.seed(1)
    s = cli.main(flags + ["--use_dynamic_unet", "True", "--max_prun", "0.5", "--min_prun", "0.1", "--max_epochs", "2", "--population_num", "4",
                          "--select_num", "2", "--mutation_num", "1", "--crossover_num", "1"], evaluator=ev)
    assert isinstance(s, sd_search.DynamicEvolutionSearcher) and s.model_layers == 14
    assert s.keep_top_k[50] and all(isinstance(sd_search.parse_sd_candidate(c), dict) for c in s.keep_top_k[50])
    named = _script("sd_bench", "tools").named_skip_set
    v1 = sd_unet_plan(**SD_V1)
    assert len(named(v1, "transformers")) == 16 and named(v1, "level0") == [0, 1, 2, 3, 32, 33, 34, 35, 36, 37] and named(v1, "[5, 2]") == [2, 5]


# ------------------------------------------------------------------ the evaluator's checks, before any launch
def test_evaluator_checks_dict_candidates_and_seeds_them_by_their_timesteps():
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator, candidate_seed
    model = SimpleNamespace(model=SimpleNamespace(layer_num=15), device=torch.device("cpu"))
    ev = SDCandidateEvaluator(model, sampler=None, conditioning=[], ref_mu=np.zeros(4), ref_sigma=np.eye(4), num_samples=2,
                              features=lambda x: x, dims=4, device="cpu")
    assert ev.layer_num == 15
    assert ev.split_candidate([3, 9]) == ([3, 9], None)
    assert ev.split_candidate({"timesteps": [3, 9], "skip_layers": [[], [14, 0]]}) == ([3, 9], [[], [14, 0]])
    for bad in ({"timesteps": [3, 9], "skip_layers": [[]]}, {"timesteps": [3], "skip_layers": [[15]]}, {"timesteps": [3], "skip_layers": [[-1]]},
                {"timesteps": [3], "skip_layers": [[2, 2]]}, {"timesteps": [3], "skip_layers": [[1.0]]}, {"timesteps": [3], "skip_layers": [[True]]},
                {"timesteps": [3]}):
        with pytest.raises(ValueError):
            ev.split_candidate(bad)
        with pytest.raises(ValueError):        # get_cand_fid refuses it before it touches opt, the sampler or the device
            ev.get_cand_fid(bad, opt=None)
    assert ev.candidate_cost({"timesteps": [3, 9], "skip_layers": [[], [14, 0]]}) == 15 + 13
    assert ev.candidate_cost([3, 9]) == ev.candidate_cost({"timesteps": [3, 9], "skip_layers": [[], []]})
    # candidates that differ only in their skip lists share their start noise; the plain list has the same
    assert candidate_seed(5, ev.split_candidate({"timesteps": [3, 9], "skip_layers": [[1], []]})[0]) == candidate_seed(5, [3, 9])


# ------------------------------------------------------------------ the samplers' host-side part
def test_sampler_ordering_moves_each_list_with_its_timestep_and_refuses_a_wrong_length():
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler, _LatentSampler
    model = SimpleNamespace(num_timesteps=1000)
    assert DDIMSampler(model)._order(np.array([690, 153, 424]), [[1], [2], [3]]) == ([153, 424, 690], [[2], [3], [1]])
    assert DDIMSampler(model)._order([690, 153]) == [153, 690] and DDIMSampler(model)._order(None) is None
    assert PLMSSampler(model)._order([690, 153], [[1], [2]]) == ([690, 153], [[1], [2]])
    assert _LatentSampler._check_skip_layers(None, 3, "s", "timesteps") is None
    assert _LatentSampler._check_skip_layers([[1], (), np.array([2])], 3, "s", "timesteps") == [[1], [], [2]]
    with pytest.raises(ValueError, match="2 lists for 3"):
        _LatentSampler._check_skip_layers([[1], []], 3, "s", "timesteps")
