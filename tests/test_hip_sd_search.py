"""GPU: the Stable-Diffusion evolutionary driver end to end on the smallest networks the suite runs -- the 64-wide two-level latent
UNet, the three-level ``sd_vae_tiny`` decoder configuration, a one-layer CLIP of the UNet's context width fed token ids, the HIP
Inception-v3 with random weights (``allow_random_inception``), synthetic reference statistics -- through
``sd_search.EvolutionSearcher`` and ``scripts/sd_search_ea.main``.

Settings: ``n_samples = 2`` and ``num_sample = 3`` (two batches through the reference's strict ``>``), ``scale = 7.5``,
``time_step = 3`` (2 under ``--dpm_solver``, the smallest the order-2 solver takes), population 4, select 2, mutation 1,
crossover 1, ``max_epochs = 2``.

Latents are 4 x 16 x 16 (``--H 128 --W 128 --f 8``), which the tiny decoder turns into 64 x 64 images: the two-level UNet halves the
map once and ``adm_conv`` takes 3x3 convs on maps of 8 x 8 and up, so 16 x 16 is the smallest latent this UNet evaluates (8 x 8
latents would put a 4 x 4 map in front of it: ``AdmError``, tests/test_hip_kernels.py::test_conv_rejects_bad_shapes).

Host FID cost.  ``FIDStatistics.frechet_distance`` is the reference's float64 scipy ``sqrtm`` formula; at 2048 dimensions it takes
4 - 6 s per candidate on the host (measured: 3.9 - 5.8 s with 16 threads), and a search of 8 candidates, its 8 direct re-evaluations
and a second run would make every test here minutes long.  The device path is not touched: the extractor, the 2048 x 2048 float64
accumulation and the statistics' copy to the host run as they are.  Only the host formula is handed the leading 64 features'
statistics (``_leading_fid``), in every test but the ``--evaluate`` one, which scores its single candidate with the full
2048-dimensional formula.  The formula itself is held to its references in tests/test_fid.py.
"""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from autodiffusion_amd.fid import FIDStatistics
from autodiffusion_amd.sd_search import EvolutionSearcher, dpm_search_params, parse_sd_candidate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NOTE = " [FID on RANDOM Inception weights: not a quality metric]"
BASE = ["--synthetic", "tiny", "--allow_random_inception", "--H", "128", "--W", "128", "--n_samples", "2", "--num_sample", "3",
        "--scale", "7.5", "--population_num", "4", "--select_num", "2", "--mutation_num", "1", "--crossover_num", "1",
        "--max_epochs", "2", "--seed", "7"]
LEADING = 64


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture
def _leading_fid(monkeypatch):
    """The host Frechet formula on the statistics of the leading 64 features (module docstring: host FID cost)."""
    full = FIDStatistics.frechet_distance
    k = LEADING

    def frechet_distance(self, other, eps=1e-6):
        return full(FIDStatistics(self.mu[:k], self.sigma[:k, :k]), FIDStatistics(other.mu[:k], other.sigma[:k, :k]), eps)
    monkeypatch.setattr(FIDStatistics, "frechet_distance", frechet_distance)


_SHARED = {}


def _cli():
    if "cli" not in _SHARED:
        spec = importlib.util.spec_from_file_location("sd_search_ea", os.path.join(ROOT, "scripts", "sd_search_ea.py"))
        _SHARED["cli"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_SHARED["cli"])
    return _SHARED["cli"]


def _ref_stats():
    """Synthetic 2048-d reference statistics: a full-rank covariance (a Gram matrix of 96 rows in the leading block, a ridge)."""
    if "ref" not in _SHARED:
        rs = np.random.RandomState(11)
        sigma = 0.25 * np.eye(2048)
        b = rs.randn(96, LEADING)
        sigma[:LEADING, :LEADING] += b.T @ b / 96
        _SHARED["ref"] = (rs.randn(2048) * 0.05, sigma)
    return _SHARED["ref"]


def _prompt_ids():
    return torch.randint(0, 512, (6, 77), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64)


def _networks():
    """One set of tiny networks for the module, built by the command line's own builders."""
    if "net" not in _SHARED:
        cli = _cli()
        opt = cli.create_argparser().parse_args(BASE)
        ids = torch.from_numpy(_prompt_ids()).to(DEV)
        loader = [{"text": ids[i:i + 2]} for i in range(0, 6, 2)]
        _SHARED["net"] = (cli.build_model(opt, torch.device(DEV), prompt_len=77), cli.build_inception(opt, torch.device(DEV)), loader)
    return _SHARED["net"]


def _searcher(extra, time_step):
    cli = _cli()
    opt = cli.create_argparser().parse_args(BASE + ["--time_step", str(time_step)] + extra)
    model, inception, loader = _networks()
    sampler = cli.build_sampler(opt, model)
    mu, sigma = _ref_stats()
    dpm = dpm_search_params(model.alphas_cumprod, time_step) if opt.dpm_solver else None
    s = EvolutionSearcher(opt, model, time_step, mu, sigma, sampler, {"validation_loader": loader}, opt.n_samples, dpm,
                          inception=inception, allow_random_inception=True)
    return s, opt


def _search(extra, time_step):
    s, opt = _searcher(extra, time_step)
    random.seed(0)
    np.random.seed(0)
    s.search()
    return s, opt


def _check_search(extra, time_step, members):
    s, opt = _search(extra, time_step)
    assert type(s.evaluator).__name__ == "SDCandidateEvaluator" and s.fid_note == NOTE
    assert 8 >= len(s.vis_dict) >= 4 and all(len(parse_sd_candidate(c)) == members for c in s.vis_dict)
    fids = {c: info["fid"] for c, info in s.vis_dict.items()}
    print({c: f for c, f in fids.items()})
    assert all(isinstance(f, float) and np.isfinite(f) for f in fids.values())
    assert len(set(fids.values())) > 1                                       # the candidates are told apart
    assert s.evaluator.last_times["images"] == 4 and s.evaluator.last_times["batches"] == 2   # 2, then 4 > 3
    top = s.keep_top_k[50]
    assert sorted(top) == sorted(fids) and [fids[c] for c in top] == sorted(fids.values())
    assert s.keep_top_k[2] == top[:2]
    # the driver adds nothing to the numbers: the evaluator alone, asked afterwards and in another order, returns the same bits
    for c in reversed(list(fids)):
        assert s.evaluator.get_cand_fid(parse_sd_candidate(c), opt) == fids[c], c
    again, _ = _search(extra, time_step)
    assert again.vis_dict == s.vis_dict and again.keep_top_k == s.keep_top_k and list(again.vis_dict) == list(s.vis_dict)
    return s


# ------------------------------------------------------------------ 1. - 3. a search per sampler
def test_ddim_search_runs_to_the_end(_leading_fid):
    s = _check_search([], 3, 3)
    assert all(isinstance(v, int) and 0 <= v < 1000 for c in s.vis_dict for v in parse_sd_candidate(c))


def test_plms_search_runs_to_the_end(_leading_fid):
    s = _check_search(["--plms"], 3, 3)
    assert type(s.sampler).__name__ == "PLMSSampler"


def test_dpm_solver_search_hands_its_candidates_to_the_sampler(_leading_fid, monkeypatch):
    from autodiffusion_amd.sd_sampler import DPMSolverSampler
    seen = []
    sample = DPMSolverSampler.sample

    def recording(self, *a, **kw):
        seen.append([float(v) for v in kw["sampled_timestep"]])
        assert kw["S"] == 2
        return sample(self, *a, **kw)
    monkeypatch.setattr(DPMSolverSampler, "sample", recording)
    s = _check_search(["--dpm_solver"], 2, 3)
    assert type(s.sampler) is DPMSolverSampler
    full = set(s.dpm_params["full_timesteps"])
    cands = [parse_sd_candidate(c) for c in s.vis_dict]
    assert all(isinstance(v, float) and v in full for c in cands for v in c)
    # two batches per evaluation; first the search's evaluations in order, as sampled_timestep
    n = len(cands)
    assert seen[:2 * n] == [c for c in cands for _ in range(2)]


# ------------------------------------------------------------------ 4. the command line, in-process
def _cli_flags(tmp_path):
    mu, sigma = _ref_stats()
    np.savez(tmp_path / "ref.npz", mu=mu, sigma=sigma)
    np.save(tmp_path / "ids.npy", _prompt_ids())
    return BASE + ["--time_step", "3", "--prompt_ids", str(tmp_path / "ids.npy"), "--ref_mu", str(tmp_path / "ref.npz"),
                   "--outdir", str(tmp_path / "out")]


def test_cli_search_writes_the_reference_log(_leading_fid, tmp_path):
    s = _cli().main(_cli_flags(tmp_path))
    lines = (tmp_path / "out" / "log.txt").read_text().splitlines()
    assert "population_num = 4 select_num = 2 mutation_num = 1 crossover_num = 1 random_num = 2 max_epochs = 2" in lines
    e0, e1 = lines.index("epoch = 0"), lines.index("epoch = 1")
    assert e0 < e1 and "epoch = 0 : top 4 result" in lines[e0:e1]
    final = lines.index("epoch = 1 : top {} result".format(len(s.keep_top_k[50])))
    assert final > e1
    for i, c in enumerate(s.keep_top_k[50]):
        assert lines[final + 1 + i] == "No.{} {} fid = {}".format(i + 1, c, s.vis_dict[c]["fid"]) + NOTE
    assert lines[-1].startswith("total searching time = ") and lines[-1].endswith(" hours")
    fid_lines = [l for l in lines if l.startswith(("FID: ", "No.")) or (l.startswith("cand: ") and ", fid: " in l)]
    assert len(fid_lines) >= 3 * len(s.vis_dict) and all(l.endswith(NOTE) for l in fid_lines)
    assert any("RANDOM weights" in l for l in lines if l.startswith("WARNING"))
    # the same networks (randomize_() is seeded) in the module's evaluator give the same numbers
    mine, opt = _searcher([], 3)
    best = s.keep_top_k[50][0]
    assert mine.evaluator.get_cand_fid(parse_sd_candidate(best), opt) == s.vis_dict[best]["fid"]


def test_cli_evaluate_prints_one_fid_equal_to_the_evaluators(tmp_path, capsys, monkeypatch):
    """The one full 2048-dimensional host FID of this module."""
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    returned = []
    inner = SDCandidateEvaluator.get_cand_fid

    def recording(self, cand=None, opt=None, device=None):
        returned.append((list(cand), inner(self, cand, opt, device)))
        return returned[-1][1]
    monkeypatch.setattr(SDCandidateEvaluator, "get_cand_fid", recording)
    fid = _cli().main(_cli_flags(tmp_path) + ["--evaluate", "[100, 500, 900]"])
    out = capsys.readouterr().out.splitlines()
    assert returned == [([100, 500, 900], fid)] and np.isfinite(fid)
    assert out.count("cand: [100, 500, 900], fid: {}".format(fid) + NOTE) == 1
    assert not any(l.startswith("epoch") or l.startswith("population_num") for l in out)


# ------------------------------------------------------------------ 5. nothing but the statistics leaves the device
def test_driver_moves_no_image_or_latent_to_the_host(_leading_fid, monkeypatch):
    """Two checks.  (a) ``get_cand_fid`` is a plain delegation: the evaluator is called once, with the candidate and opt objects it
    was given, and its return value is handed back as it is.  (b) Every device-to-host transfer torch makes during one
    ``get_cand_fid`` through the driver (``.cpu()``, ``.to(cpu)``, ``.numpy()``, ``.item()``, ``.tolist()``, ``bool()`` / ``int()`` /
    ``float()`` of a device tensor) is recorded: they are the transfers of a direct ``SDCandidateEvaluator.get_cand_fid`` -- the
    float64 sums (2048,) and (2048, 2048), per batch the sampler's read of the 1000-entry alphas_cumprod table and the text encoder's
    range check of the [2, 77] token ids, and scalars -- and none is an image or a latent (4-D) or an embedding (3-D)."""
    s, opt = _searcher([], 3)
    s.evaluator.get_cand_fid([100, 500, 900], opt)     # the empty prompt is encoded once per evaluator: not part of either record
    moved = []

    def watch(name):
        inner = getattr(torch.Tensor, name)

        def wrapper(self, *a, **kw):
            out = inner(self, *a, **kw)
            if self.is_cuda and not (torch.is_tensor(out) and out.is_cuda):
                moved.append(tuple(self.shape))
            return out
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    for name in ("cpu", "to", "numpy", "item", "tolist", "__bool__", "__int__", "__float__", "__index__"):
        watch(name)
    cand = [120, 480, 870]
    direct = s.evaluator.get_cand_fid(cand, opt)
    direct_moves, moved[:] = list(moved), []
    calls = []
    inner = s.evaluator.get_cand_fid
    s.evaluator.get_cand_fid = lambda c, o, *a: calls.append((c, o, a)) or inner(c, o, *a)
    fid = s.get_cand_fid(cand=cand, opt=opt)
    assert fid == direct and len(calls) == 1 and calls[0][0] is cand and calls[0][1] is opt and calls[0][2] == ()
    print("device-to-host transfers of one candidate:", moved)
    assert moved == direct_moves
    big = [m for m in moved if len(m) > 0]
    assert set(big) == {(2, 77), (1000,), (2048,), (2048, 2048)} and big.count((2048,)) == 1 and big.count((2048, 2048)) == 1
    assert big.count((2, 77)) == 2 and big.count((1000,)) == 2                  # two batches
    assert not any(len(m) >= 3 for m in moved)
