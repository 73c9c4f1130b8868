#!/usr/bin/env python3
"""Capture the trajectory of the REFERENCE's Stable-Diffusion evolutionary search -- integer candidates (DDIM / PLMS) and
DPM-Solver candidates (K + 1 continuous times) -- under a synthetic fitness, by importing the reference's own driver
("Stable Diffusion"/scripts/search_ea.py).

Runs only in the build container (needs /root/reference); the GPU box never sees the reference.  Output:
sd_ea_trajectory.npz next to this script (candidate values, fitness values, the DPM time grids: data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_sd_ea.py

As in capture_ea_dynamic.py, stand-in modules are registered *in this capture process only* for imports the EA logic never
uses and that are absent here (``torchvision(.transforms)``, ``pytorch_lightning.seed_everything``, ``omegaconf.OmegaConf``,
``pytorch_fid.inception.InceptionV3``) or that fail to import beside a stub torchvision (``transformers.AutoFeatureExtractor``).
``EvolutionSearcher.__init__`` loads the reference statistics from disk, so the instance is made with ``object.__new__`` and
given the attributes the recorded methods read.  The DPM time grids come from the reference's own ``DPM_Solver.get_time_steps``
as main() calls it (:888-902).
"""
import os
import random
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/examples/Stable Diffusion"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "scripts"))


def _stub(name, **attrs):
    m = sys.modules.get(name)
    if m is None:
        m = sys.modules[name] = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


_stub("torchvision", transforms=_stub("torchvision.transforms"))
_stub("pytorch_lightning", seed_everything=lambda seed: None)
_stub("omegaconf", OmegaConf=type("OmegaConf", (), {}))
_stub("pytorch_fid", inception=_stub("pytorch_fid.inception", InceptionV3=type("InceptionV3", (), {})))
_stub("transformers", AutoFeatureExtractor=type("AutoFeatureExtractor", (), {}))

import search_ea as drv  # noqa: E402
from ldm.models.diffusion.dpm_solver.dpm_solver import DPM_Solver, NoiseScheduleVP  # noqa: E402

TIME_STEP = 4


def fitness_of(cand):
    """Synthetic, deterministic, a function of the candidate's sorted numeric values only (str(cand) would carry numpy 2's
    ``np.int64(...)`` spelling): a crc32 of their float reprs, scaled to [0, 100)."""
    key = ",".join(repr(float(v)) for v in sorted(cand))
    return zlib.crc32(key.encode()) / 2.0 ** 32 * 100.0


def dpm_params(time_step):
    """search_ea.py:888-902 with the v1 schedule's alphas_cumprod (only its length enters the time grid)."""
    import torch
    betas = torch.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, 1000, dtype=torch.float64) ** 2
    ns = NoiseScheduleVP('discrete', alphas_cumprod=torch.cumprod(1.0 - betas, dim=0).float())
    solver = DPM_Solver(None, ns, predict_x0=True, thresholding=False)
    t_0, t_T = 1. / solver.noise_schedule.total_N, solver.noise_schedule.T
    full = list(solver.get_time_steps(skip_type="time_uniform", t_T=t_T, t_0=t_0, N=1000, device='cpu'))
    init = list(solver.get_time_steps(skip_type="time_uniform", t_T=t_T, t_0=t_0, N=time_step, device='cpu'))
    return {'full_timesteps': [full[i].item() for i in range(len(full))],
            'init_timesteps': [init[i].item() for i in range(len(init))]}


def run(dpm, use_ddim_init_x, params):
    class Opt:
        pass
    opt = Opt()
    opt.dpm_solver = dpm
    opt.max_epochs, opt.select_num, opt.population_num = 3, 4, 10
    opt.m_prob, opt.crossover_num, opt.mutation_num = 0.25, 3, 4

    class _Sampler:
        ddpm_num_timesteps = 1000

    s = object.__new__(drv.EvolutionSearcher)
    s.opt, s.sampler, s.time_step = opt, _Sampler(), TIME_STEP
    s.max_epochs, s.select_num, s.population_num = opt.max_epochs, opt.select_num, opt.population_num
    s.m_prob, s.crossover_num, s.mutation_num = opt.m_prob, opt.crossover_num, opt.mutation_num
    s.ddim_discretize = "uniform"
    s.keep_top_k = {s.select_num: [], 50: []}
    s.epoch, s.candidates, s.vis_dict = 0, [], {}
    s.use_ddim_init_x = use_ddim_init_x
    s.dpm_params = params if dpm else None
    evaluated, tops, top_fids = [], [], []

    def fitness(cand=None, opt=None, device='cuda'):
        evaluated.append([float(v) for v in cand])
        return fitness_of(cand)
    s.get_cand_fid = fitness

    # the per-epoch top list, read where the reference logs it: update_top_k(k=50) is the last step before the log lines
    inner = s.update_top_k

    def update_top_k(candidates, *, k, key, reverse=False):
        inner(candidates, k=k, key=key, reverse=reverse)
        if k == 50:
            top = list(s.keep_top_k[50])
            tops.append([[float(v) for v in eval(c, {"np": np})] for c in top])
            top_fids.append([s.vis_dict[c]['fid'] for c in top])
    s.update_top_k = update_top_k
    drv.logging.disable(drv.logging.CRITICAL)
    random.seed(0)
    np.random.seed(0)
    s.search()
    out = dict(evaluated=np.array(evaluated, dtype=np.float64), epochs=np.array(len(tops)))
    for e, (t, f) in enumerate(zip(tops, top_fids)):
        out[f"top50_e{e}"] = np.array(t, dtype=np.float64)
        out[f"top50_fid_e{e}"] = np.array(f, dtype=np.float64)
    return out


if __name__ == "__main__":
    params = dpm_params(TIME_STEP)
    out = {"full_timesteps": np.array(params['full_timesteps'], dtype=np.float64),
           "init_timesteps": np.array(params['init_timesteps'], dtype=np.float64), "time_step": np.array(TIME_STEP)}
    for tag, (dpm, init) in {"int_random": (False, False), "int_init": (False, True),
                             "dpm_random": (True, False), "dpm_init": (True, True)}.items():
        r = run(dpm, init, params)
        print(tag, "evaluations:", len(r["evaluated"]), "epochs:", int(r["epochs"]), "first:", r["evaluated"][0],
              "distinct members everywhere:", all(len(set(c)) == len(c) for c in r["evaluated"].tolist()))
        for k, v in r.items():
            out[f"{tag}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "sd_ea_trajectory.npz"), **out)
