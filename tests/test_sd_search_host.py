"""Host tests of the Stable-Diffusion evolutionary driver (autodiffusion_amd/sd_search.py) and its command line
(scripts/sd_search_ea.py): the four trajectories captured from the reference's own driver (tests/golden/capture_sd_ea.py ->
sd_ea_trajectory.npz) value for value, the DPM-Solver candidate space, the visited-set dedupe and the log text, the
population-parallel mode on one rank and on two gloo ranks, and the command line's parsing, prompt batching and statistics loading.
"""
import importlib.util
import json
import os
import random
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from autodiffusion_amd import logger
from autodiffusion_amd.sd_search import EvolutionSearcher, dpm_search_params, parse_sd_candidate

from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = {"int_random": (False, False), "int_init": (False, True), "dpm_random": (True, False), "dpm_init": (True, True)}
EVALUATIONS = {"int_random": 30, "int_init": 29, "dpm_random": 30, "dpm_init": 29}


def fitness_of(cand):
    """Same synthetic fitness as tests/golden/capture_sd_ea.py::fitness_of."""
    key = ",".join(repr(float(v)) for v in sorted(cand))
    return zlib.crc32(key.encode()) / 2.0 ** 32 * 100.0


class _Fitness:
    """Stands in for SDCandidateEvaluator: records what it was asked to score."""
    fid_note = ""

    def __init__(self):
        self.evaluated = []

    def get_cand_fid(self, cand=None, opt=None, device=None):
        self.evaluated.append(list(cand))
        return fitness_of(cand)


def _searcher(dpm=False, use_ddim_init_x=False, max_epochs=3, time_step=4, **kw):
    opt = SimpleNamespace(max_epochs=max_epochs, select_num=4, population_num=10, m_prob=0.25, crossover_num=3, mutation_num=4,
                          max_fid=3.0, num_sample=4, use_ddim_init_x=use_ddim_init_x, dpm_solver=dpm, seed=0)
    ev = _Fitness()
    s = EvolutionSearcher(opt, None, time_step, np.zeros(4), np.eye(4), SimpleNamespace(ddpm_num_timesteps=1000),
                          {"validation_loader": []}, 2, dpm_params=dpm_search_params(range(1000), time_step) if dpm else None,
                          evaluator=ev, **kw)
    return s, ev


def _run(tag, **kw):
    dpm, init = RUNS[tag]
    s, ev = _searcher(dpm, init, **kw)
    tops = []
    inner = s.update_top_k

    def update_top_k(candidates, *, k, key, reverse=False):
        inner(candidates, k=k, key=key, reverse=reverse)
        if k == 50:
            tops.append(([parse_sd_candidate(c) for c in s.keep_top_k[50]], [s.vis_dict[c]["fid"] for c in s.keep_top_k[50]]))
    s.update_top_k = update_top_k
    random.seed(0)
    np.random.seed(0)
    s.search()
    return s, ev, tops


def _assert_matches_fixture(tag, ev, tops, ordered=True):
    g = golden("sd_ea_trajectory")
    want = g[f"{tag}_evaluated"]
    assert len(want) == EVALUATIONS[tag]
    got = np.array(ev.evaluated, dtype=np.float64)
    if ordered:
        np.testing.assert_array_equal(got, want)
    else:
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist()))
    assert len(tops) == int(g[f"{tag}_epochs"]) == 3
    for e, (cands, fids) in enumerate(tops):
        np.testing.assert_array_equal(np.array(cands, dtype=np.float64), g[f"{tag}_top50_e{e}"])
        np.testing.assert_array_equal(np.array(fids, dtype=np.float64), g[f"{tag}_top50_fid_e{e}"])


# ------------------------------------------------------------------ 1. the reference's trajectories
@pytest.mark.parametrize("tag", list(RUNS))
def test_trajectory_matches_the_reference_driver(tag, monkeypatch):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    s, ev, tops = _run(tag)
    _assert_matches_fixture(tag, ev, tops)
    # plain Python numbers all the way: every candidate string reads back through literal_eval to what was evaluated
    assert all(type(v) is (float if RUNS[tag][0] else int) for c in ev.evaluated for v in c)
    assert [parse_sd_candidate(c) for c in s.vis_dict] == ev.evaluated
    assert s.keep_top_k[50] == sorted(s.keep_top_k[50], key=lambda c: s.vis_dict[c]["fid"])
    assert list(s.keep_top_k) == [4, 50] and s.epoch == 2   # stopped before the last epoch's offspring


# ------------------------------------------------------------------ 2. the DPM-Solver candidate space
def test_dpm_search_params_reproduce_the_reference_grids_bit_for_bit():
    g = golden("sd_ea_trajectory")
    p = dpm_search_params(np.zeros(1000), 4)
    assert len(p["full_timesteps"]) == 1001 and len(p["init_timesteps"]) == 5
    assert all(type(v) is float for v in p["full_timesteps"] + p["init_timesteps"])
    np.testing.assert_array_equal(np.array(p["full_timesteps"], dtype=np.float64), g["full_timesteps"])
    np.testing.assert_array_equal(np.array(p["init_timesteps"], dtype=np.float64), g["init_timesteps"])
    assert p["full_timesteps"][0] == 1.0 and p["full_timesteps"][-1] == float(np.float32(1.0 / 1000))
    assert len(set(p["full_timesteps"])) == 1001


@pytest.mark.parametrize("tag", ["dpm_random", "dpm_init"])
def test_dpm_candidates_are_members_of_the_full_grid(tag, monkeypatch):
    """time_step + 1 members of full_timesteps, ascending.  Members are distinct wherever an operator draws without replacement
    (random candidates, mutations, the init candidate); a crossover child takes position i from either parent and may repeat a
    time, in the reference as here (its dpm_init run holds such a child), so children are held to membership only."""
    monkeypatch.setattr(logger, "log", lambda *a: None)
    dpm, init = RUNS[tag]
    s, ev = _searcher(dpm, init)
    children = []
    cross = s.get_cross

    def get_cross(k, cross_num):
        res = cross(k, cross_num)
        children.extend(res)
        return res
    s.get_cross = get_cross
    random.seed(0)
    np.random.seed(0)
    s.search()
    full = set(s.dpm_params["full_timesteps"])
    assert len(ev.evaluated) == EVALUATIONS[tag] and children
    for text in s.vis_dict:
        cand = parse_sd_candidate(text)
        assert len(cand) == 5 and all(v in full for v in cand) and cand == sorted(cand)
        if text not in children:
            assert len(set(cand)) == 5, text


def test_init_candidate_is_the_uniform_ddim_grid():
    s, _ = _searcher(False, True)
    assert s.initial_candidate() == [1, 251, 501, 751] and str(s.initial_candidate()) == "[1, 251, 501, 751]"
    assert all(type(v) is int for v in s.initial_candidate())
    d, _ = _searcher(True, True)
    assert d.initial_candidate() == sorted(d.dpm_params["init_timesteps"]) and d.initial_candidate()[-1] == 1.0


def test_candidate_text_is_parsed_as_a_literal():
    assert parse_sd_candidate("[1, 251, 501, 751]") == [1, 251, 501, 751]
    assert parse_sd_candidate("[0.0010000000474974513, 1.0]") == [0.0010000000474974513, 1.0]
    for bad in ("__import__('os').getcwd()", "[np.int64(1)]", "[[1, 2]]", "[]", "[True]", "{'timesteps': [1]}", "1"):
        with pytest.raises(ValueError):
            parse_sd_candidate(bad)


# ------------------------------------------------------------------ 3. dedupe and log text
def test_visited_candidates_are_not_re_evaluated_and_log_format(monkeypatch):
    lines = []
    monkeypatch.setattr(logger, "log", lambda *a: lines.append(" ".join(str(x) for x in a)))
    s, ev = _searcher(False, True, max_epochs=2)
    random.seed(1)
    np.random.seed(1)
    s.search()
    keys = [str(sorted(c)) for c in ev.evaluated]
    assert len(keys) == len(set(keys)) == len(s.vis_dict)
    n = len(ev.evaluated)
    assert s.is_legal(str(ev.evaluated[0][::-1])) is False and s.is_legal_before_search(keys[3]) is False   # order does not matter
    assert len(ev.evaluated) == n and lines[-1] == "cand: {} has visited!".format(keys[3])
    assert lines[0] == "population_num = 10 select_num = 4 mutation_num = 4 crossover_num = 3 random_num = 3 max_epochs = 2"
    assert lines[1] == "cand: [1, 251, 501, 751], fid: {}".format(fitness_of([1, 251, 501, 751]))
    for want in ("random select ........", "random 2/5", "random_num = 5", "mutation x0 ......", "mutation x0 1/4",
                 "epoch = 0", "select ......", "mutation ......", "cross ......", "cross_num = 3",
                 "random_num = 10", "epoch = 1"):
        assert want in lines, want
    best = s.keep_top_k[50][0]
    assert "No.1 {} fid = {}".format(best, s.vis_dict[best]["fid"]) in lines
    tops = [l for l in lines if " : top " in l]     # the mutations of the init candidate at m_prob 0.1 often repeat it: < 10 seeds
    assert len(tops) == 2 and tops[0].startswith("epoch = 0 : top ") and tops[0].endswith(" result")
    assert tops[1] == "epoch = 1 : top {} result".format(len(s.keep_top_k[50]))
    assert sum(l.startswith("No.") for l in lines) == int(tops[0].split()[5]) + len(s.keep_top_k[50])
    assert any(l.startswith("mutation_num = ") for l in lines)
    assert sum(l.startswith("epoch = 1 : top ") for l in lines) == 1 and not any(l.startswith("epoch = 2") for l in lines)


def test_get_cand_fid_is_a_plain_delegation():
    s, ev = _searcher()
    assert s.get_cand_fid(cand=[5, 6, 7, 8], opt=s.opt, device="cuda") == fitness_of([5, 6, 7, 8]) and ev.evaluated == [[5, 6, 7, 8]]
    assert s.get_cand_fid([1, 2, 3, 4]) == fitness_of([1, 2, 3, 4]) and len(ev.evaluated) == 2   # opt defaults to the searcher's


# ------------------------------------------------------------------ 4. / 5. population parallelism
@pytest.mark.parametrize("tag", list(RUNS))
def test_population_parallel_one_rank_reproduces_the_sequential_trajectory(tag, monkeypatch):
    """Deferring evaluation to the epoch boundary must not change a single random / np.random draw, and with one rank the
    queue is evaluated in generation order: the evaluation order, every epoch's top list and the FIDs are the fixture's."""
    monkeypatch.setattr(logger, "log", lambda *a: None)
    s, ev, tops = _run(tag, population_parallel=True)
    _assert_matches_fixture(tag, ev, tops)
    assert s._pending == [] and s.last_flush["collective"] is None


class _RankFitness(_Fitness):
    def __init__(self, rank):
        super().__init__()
        self.rank, self.calls = rank, []

    def get_cand_fid(self, cand=None, opt=None, device=None):
        self.calls.append(self.rank)
        return super().get_cand_fid(cand, opt)


def _pp_rank(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    logger.log = lambda *a: None
    for tag in ("int_init", "dpm_random"):
        dpm, init = RUNS[tag]
        s, _ = _searcher(dpm, init, population_parallel=True)
        ev = s.evaluator = _RankFitness(rank)
        flushed = []            # (index within its flush) of every candidate this rank evaluated
        flush = s.flush_pending

        def flush_pending():
            queue, before = list(s._pending), len(ev.evaluated)
            flush()
            mine = ev.evaluated[before:]
            flushed.extend(i for i, c in enumerate(queue) if parse_sd_candidate(c) in mine)
            assert len(mine) == len(range(rank, len(queue), world))
        s.flush_pending = flush_pending
        random.seed(0)
        np.random.seed(0)
        s.search()
        np.savez(out + f".{tag}.{rank}.npz", evaluated=np.array(ev.evaluated, dtype=np.float64), flushed=np.array(flushed),
                 top=np.array([parse_sd_candidate(c) for c in s.keep_top_k[50]], dtype=np.float64),
                 fid=np.array([s.vis_dict[c]["fid"] for c in s.keep_top_k[50]]), visited=len(s.vis_dict))
    dist.barrier()
    dist.destroy_process_group()


def test_population_parallel_two_ranks_gloo(tmp_path):
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    out = str(tmp_path / "pp")
    mp.spawn(_pp_rank, args=(2, port, out), nprocs=2, join=True)
    g = golden("sd_ea_trajectory")
    for tag in ("int_init", "dpm_random"):
        z = [np.load(out + f".{tag}.{r}.npz") for r in (0, 1)]
        both = z[0]["evaluated"].tolist() + z[1]["evaluated"].tolist()
        assert len(both) == EVALUATIONS[tag]                                   # candidates were split, none twice
        assert sorted(map(tuple, both)) == sorted(map(tuple, g[f"{tag}_evaluated"].tolist()))
        for r in (0, 1):
            assert len(z[r]["flushed"]) == len(z[r]["evaluated"]) and bool((z[r]["flushed"] % 2 == r).all())   # only i % 2 == rank
            assert int(z[r]["visited"]) == EVALUATIONS[tag]
            np.testing.assert_array_equal(z[r]["top"], g[f"{tag}_top50_e2"])   # every rank ends with the sequential result
            np.testing.assert_array_equal(z[r]["fid"], g[f"{tag}_top50_fid_e2"])


# ------------------------------------------------------------------ 5b. one driver under both packages' searchers
def test_equal_costs_are_assigned_round_robin():
    """What lets the SD searchers use the cost-aware flush: with one cost for all, longest-first is exactly i % world."""
    for world in range(1, 9):
        for n in range(41):
            assert EvolutionSearcher.assign_candidates([5] * n, world) == [i % world for i in range(n)], (n, world)


def test_the_loops_and_the_joint_operators_exist_once():
    from autodiffusion_amd import ea, sd_search, search
    for name in ("search", "flush_pending", "_collect", "_fill_random", "update_top_k", "_visit", "is_legal", "is_legal_before_search",
                 "get_random", "get_random_before_search", "get_cross", "get_mutation", "mutate_init_x", "_mutate", "_cross",
                 "sample_active_subnet", "assign_candidates", "candidate_cost"):
        assert getattr(search.EvolutionSearcher, name) is getattr(sd_search.EvolutionSearcher, name), name
        assert getattr(search.EvolutionSearcher, name) is getattr(ea.EvolutionDriver, name), name
    for name in ("_mutate", "_cross", "sample_active_subnet", "_after_selection", "_mutate_timesteps", "_touch_skips", "_draw_skips",
                 "mutate_init_x", "_initial_candidate", "cand2gen", "_init_joint"):
        assert getattr(search.DynamicEvolutionSearcher, name) is getattr(sd_search.DynamicEvolutionSearcher, name), name
        assert getattr(search.DynamicEvolutionSearcher, name) is getattr(ea.JointSearch, name), name
    for name in ("search", "flush_pending", "_collect", "_fill_random", "update_top_k", "_visit"):   # the loops stay the driver's
        assert getattr(sd_search.DynamicEvolutionSearcher, name) is getattr(ea.EvolutionDriver, name), name
    assert not hasattr(sd_search, "_Steps")


def test_last_flush_of_flat_candidates_is_a_superset(monkeypatch):
    monkeypatch.setattr(logger, "log", lambda *a: None)
    s, ev = _searcher(population_parallel=True)
    cands = [[1, 2, 3, 4], [8, 7, 6, 5], [9, 10, 11, 12], [13, 14, 15, 16]]
    assert all(s.is_legal(str(c)) for c in cands) and ev.evaluated == []
    s.flush_pending()
    f = s.last_flush
    assert f["owner"] == [0, 0, 0, 0] and f["costs"] == [4, 4, 4, 4] and f["assigned_cost"] == 16
    assert f["candidates"] == 4 and f["assigned"] == 4 and f["evaluate_s"] >= 0 and f["collective"] is None
    assert ev.evaluated == [sorted(c) for c in cands] and [s.vis_dict[str(sorted(c))]["fid"] for c in cands] == [fitness_of(c) for c in cands]


# ------------------------------------------------------------------ 6. the command line
def _cli():
    spec = importlib.util.spec_from_file_location("sd_search_ea", os.path.join(ROOT, "scripts", "sd_search_ea.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_defaults_are_the_reference_defaults():
    opt = _cli().create_argparser().parse_args([])
    want = dict(outdir="outputs/txt2img-samples", plms=False, dpm_solver=False, fixed_code=False, ddim_eta=0.0, H=512, W=512, C=4, f=8,
                n_samples=3, scale=7.5, config="configs/stable-diffusion/v1-inference.yaml",
                ckpt="models/ldm/stable-diffusion-v1/model.ckpt", seed=42, num_sample=4, max_epochs=10, select_num=10,
                population_num=50, m_prob=0.1, crossover_num=25, mutation_num=25, max_fid=3.0, thres=0.2, ref_mu="", ref_sigma="",
                time_step=50, use_ddim_init_x=False)
    assert {k: getattr(opt, k) for k in want} == want
    assert opt.torso == "bf16" and not opt.population_parallel and not opt.allow_random_inception and opt.synthetic == ""


def test_cli_use_ddim_init_x_is_a_boolean_word():
    cli = _cli()
    parse = cli.create_argparser().parse_args
    assert parse(["--use_ddim_init_x", "False"]).use_ddim_init_x is False
    assert parse(["--use_ddim_init_x", "True"]).use_ddim_init_x is True
    assert parse(["--use_ddim_init_x", "0"]).use_ddim_init_x is False
    with pytest.raises(SystemExit):
        parse(["--use_ddim_init_x", "maybe"])
    assert "turns the string 'False' into True" in " ".join(cli.create_argparser().format_help().split())


def test_cli_batches_captions_like_the_reference_loader(tmp_path):
    cli = _cli()
    caps = ["A Cat on a mat", "Two DOGS", "a red bus", "The Sea", "one more"]
    js = tmp_path / "captions.json"
    js.write_text(json.dumps({"images": [], "annotations": [{"image_id": i, "id": 9 - i, "caption": c} for i, c in enumerate(caps)]}))
    want = [{"text": ["a cat on a mat", "two dogs"]}, {"text": ["a red bus", "the sea"]}]
    assert cli.batch_captions(cli.read_captions(str(js)), 2) == want          # lower-cased, file order, last short batch dropped
    txt = tmp_path / "captions.txt"
    txt.write_text("\n".join(c.lower() for c in caps) + "\n\n")
    assert cli.batch_captions(cli.read_captions(str(txt)), 2) == want
    assert cli.batch_captions(caps, 5) == [{"text": caps}] and cli.batch_captions(caps, 6) == []
    opt = cli.create_argparser().parse_args(["--captions", str(txt), "--tokenizer_dir", str(tmp_path), "--n_samples", "2"])
    assert cli.build_loader(opt, "cpu") == want
    ids = np.arange(5 * 7, dtype=np.int64).reshape(5, 7)
    np.save(tmp_path / "ids.npy", ids)
    loader = cli.build_loader(cli.create_argparser().parse_args(["--prompt_ids", str(tmp_path / "ids.npy"), "--n_samples", "2"]), "cpu")
    assert len(loader) == 2 and np.array_equal(loader[1]["text"].numpy(), ids[2:4]) and loader[0]["text"].dtype.is_floating_point is False
    with pytest.raises(SystemExit):
        cli.build_loader(cli.create_argparser().parse_args(["--captions", str(txt)]), "cpu")   # strings need a tokenizer


def _stats(tmp_path):
    a = np.random.RandomState(3).randn(40, 6)
    mu, sigma = a.mean(0), np.cov(a, rowvar=False)
    np.save(tmp_path / "mu.npy", mu)
    np.save(tmp_path / "sigma.npy", sigma)
    np.savez(tmp_path / "ref.npz", mu=mu, sigma=sigma, mu_s=mu, sigma_s=sigma)   # what scripts/evaluator.py --save_ref_stats writes
    return mu, sigma


def test_cli_reference_statistics_npz_and_npy_pair_agree(tmp_path):
    cli = _cli()
    mu, sigma = _stats(tmp_path)
    parse = cli.create_argparser().parse_args
    a = cli.load_ref_stats(parse(["--ref_mu", str(tmp_path / "ref.npz")]))
    b = cli.load_ref_stats(parse(["--ref_mu", str(tmp_path / "mu.npy"), "--ref_sigma", str(tmp_path / "sigma.npy")]))
    for x, y, z in zip(a, b, (mu, sigma)):
        assert x.dtype == np.float64 and np.array_equal(x, y) and np.array_equal(x, z)
    with pytest.raises(SystemExit):
        cli.load_ref_stats(parse(["--ref_mu", str(tmp_path / "mu.npy")]))


def test_cli_evaluate_scores_one_candidate_and_ignored_flags_are_logged(tmp_path, monkeypatch, capsys):
    cli = _cli()
    _stats(tmp_path)
    lines = []
    monkeypatch.setattr(logger, "configure", lambda *a, **k: None)
    monkeypatch.setattr(logger, "log", lambda *a: lines.append(" ".join(str(x) for x in a)))
    ev = _Fitness()
    base = ["--ref_mu", str(tmp_path / "ref.npz"), "--outdir", str(tmp_path / "out"), "--time_step", "3"]
    fid = cli.main(base + ["--evaluate", "[100, 500, 900]", "--precision", "full", "--skip_grid", "--ddim_steps", "20", "--n_iter", "1",
                           "--prompt", "a cat", "--data_dir", "/nowhere"], evaluator=ev)
    assert fid == fitness_of([100, 500, 900]) and ev.evaluated == [[100, 500, 900]]          # once, and no search
    assert "cand: [100, 500, 900], fid: {}".format(fid) in lines and not any(l.startswith("epoch") for l in lines)
    ign = [l for l in lines if l.startswith("ignored flags")]
    assert len(ign) == 1 and all("--" + k in ign[0] for k in ("precision", "skip_grid", "ddim_steps", "n_iter", "prompt", "data_dir"))
    assert "--laion400m" not in ign[0] and "--cal_fid" not in ign[0]
    with pytest.raises(SystemExit):
        cli.main(base + ["--evaluate", "[100, 500]"], evaluator=_Fitness())                   # --time_step 3 needs three entries
    # a search through the same entry point: the reference's lines, a DPM candidate space of time_step + 1 floats
    lines.clear()
    ev = _Fitness()
    s = cli.main(base + ["--dpm_solver", "--population_num", "4", "--select_num", "2", "--mutation_num", "1", "--crossover_num", "1",
                         "--max_epochs", "2", "--use_ddim_init_x", "True"], evaluator=ev)
    assert not any(l.startswith("ignored flags") for l in lines)
    assert ev.evaluated[0] == sorted(dpm_search_params(range(1000), 3)["init_timesteps"]) and all(len(c) == 4 for c in ev.evaluated)
    assert "population_num = 4 select_num = 2 mutation_num = 1 crossover_num = 1 random_num = 2 max_epochs = 2" in lines
    assert lines[-1].startswith("total searching time = ") and lines[-1].endswith(" hours")
    assert len(s.vis_dict) == len(ev.evaluated)


def test_cli_empty_prompt_of_a_prompt_ids_run():
    """CLIP tokenises "" as start-of-text, then end-of-text (its pad token) up to max_length: the last two ids of its vocabulary."""
    cli = _cli()
    tok = cli.EmptyPromptTokenizer(49408)
    ids = tok(["", ""], max_length=77, truncation=True, padding="max_length", return_tensors="pt")["input_ids"]
    assert tuple(ids.shape) == (2, 77) and ids.dtype.is_floating_point is False
    assert ids[:, 0].tolist() == [49406, 49406] and bool((ids[:, 1:] == 49407).all())
    with pytest.raises(SystemExit):
        tok(["a cat"], max_length=77)
