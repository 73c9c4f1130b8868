"""Host: autodiffusion_amd/sd_script_util.py, what the Stable-Diffusion command lines share, and the four scripts on top of it.

The namespaces below were written down from the scripts' own parsers before the shared flag table existed: every flag, default and
the ORDER of definition (``log.txt``'s first line is ``str(opt)``, and an ``argparse.Namespace`` prints in insertion order)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from autodiffusion_amd import logger, sd_script_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
CONFIG, CKPT = "configs/stable-diffusion/v1-inference.yaml", "models/ldm/stable-diffusion-v1/model.ckpt"
PROMPT = "a painting of a virus monster playing guitar"

MINIMAL = {   # script -> (the required arguments alone, vars() of what they parse to)
    "sd_search_ea": ([], dict(
        outdir="outputs/txt2img-samples", plms=False, dpm_solver=False, fixed_code=False, ddim_eta=0.0, H=512, W=512, C=4, f=8,
        n_samples=3, scale=7.5, config=CONFIG, ckpt=CKPT, seed=42, num_sample=4, max_epochs=10, select_num=10, population_num=50,
        m_prob=0.1, crossover_num=25, mutation_num=25, max_fid=3.0, thres=0.2, ref_mu="", ref_sigma="", fitness="fid", ref_feats="",
        time_step=50, use_ddim_init_x=False, prompt=None, skip_grid=None, skip_save=None, ddim_steps=None, laion400m=None, n_iter=None,
        n_rows=None, precision=None, data_dir=None, cal_fid=None, captions="", tokenizer_dir="", prompt_ids="", inception_path="",
        allow_random_inception=False, torso="bf16", population_parallel=False, clip_ckpt="", evaluate="", synthetic="")),
    "sd_img2img": (["--init-img", "init.npy"], dict(
        prompt=PROMPT, init_img="init.npy", outdir="outputs/img2img-samples", ddim_steps=50, plms=False, ddim_eta=0.0, n_iter=1,
        n_samples=2, scale=5.0, strength=0.75, config=CONFIG, ckpt=CKPT, seed=42, tokenizer_dir="", prompt_ids="", torso="bf16",
        synthetic="", use_timestep="", side_multiple=64)),
    "sd_inpaint": (["--init-img", "init.npy", "--mask", "mask.npy"], dict(
        prompt=PROMPT, init_img="init.npy", mask="mask.npy", outdir="outputs/inpaint-samples", ddim_steps=50, plms=False, prompt_mask="",
        no_composite=False, ddim_eta=0.0, n_iter=1, n_samples=2, scale=5.0, config=CONFIG, ckpt=CKPT, seed=42, tokenizer_dir="",
        prompt_ids="", torso="bf16", synthetic="", use_timestep="", side_multiple=64)),
    "sd_clip_score": (["samples.npz"], dict(
        samples="samples.npz", clip_ckpt="", prompt_ids="", captions="", tokenizer_dir="", batch_size=64, torso="bf16", synthetic="")),
}
# tests/test_hip_sd_search.py's BASE and the str() of what scripts/sd_search_ea.py parses it to: log.txt's argument line
SEARCH_BASE = ["--synthetic", "tiny", "--allow_random_inception", "--H", "128", "--W", "128", "--n_samples", "2", "--num_sample", "3",
               "--scale", "7.5", "--population_num", "4", "--select_num", "2", "--mutation_num", "1", "--crossover_num", "1",
               "--max_epochs", "2", "--seed", "7"]
SEARCH_BASE_STR = (
    "Namespace(outdir='outputs/txt2img-samples', plms=False, dpm_solver=False, fixed_code=False, ddim_eta=0.0, H=128, W=128, C=4, f=8, "
    "n_samples=2, scale=7.5, config='configs/stable-diffusion/v1-inference.yaml', ckpt='models/ldm/stable-diffusion-v1/model.ckpt', "
    "seed=7, num_sample=3, max_epochs=2, select_num=2, population_num=4, m_prob=0.1, crossover_num=1, mutation_num=1, max_fid=3.0, "
    "thres=0.2, ref_mu='', ref_sigma='', fitness='fid', ref_feats='', time_step=50, use_ddim_init_x=False, prompt=None, "
    "skip_grid=None, skip_save=None, ddim_steps=None, laion400m=None, n_iter=None, n_rows=None, precision=None, data_dir=None, "
    "cal_fid=None, captions='', tokenizer_dir='', prompt_ids='', inception_path='', allow_random_inception=True, torso='bf16', "
    "population_parallel=False, clip_ckpt='', evaluate='', synthetic='tiny')")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(SCRIPTS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ the parsers
@pytest.mark.parametrize("name", sorted(MINIMAL))
def test_parser_reproduces_the_recorded_namespace(name):
    argv, want = MINIMAL[name]
    opt = _script(name).create_argparser().parse_args(argv)
    assert list(vars(opt).items()) == list(want.items())


def test_search_argument_line_is_the_recorded_one():
    assert str(_script("sd_search_ea").create_argparser().parse_args(SEARCH_BASE)) == SEARCH_BASE_STR


# ------------------------------------------------------------------ no script imports another
def test_inpaint_loads_no_other_script_and_names_itself(tmp_path, monkeypatch):
    before = set(sys.modules)
    mod = _script("sd_inpaint")
    new = [m for k, m in sys.modules.items() if k not in before]
    assert not [m for m in new if (getattr(m, "__file__", None) or "").startswith(SCRIPTS + os.sep)]
    assert SCRIPTS not in sys.path
    assert mod.load_prompts is sd_script_util.load_prompts and mod.build_model is sd_script_util.build_model
    # main() up to the shared prompt loader, on the host: a 1-D --prompt_ids file is refused under the running script's name
    np.save(tmp_path / "init.npy", np.zeros((1, 32, 32, 3), np.uint8))
    np.save(tmp_path / "mask.npy", np.zeros((1, 32, 32), np.uint8))
    np.save(tmp_path / "ids.npy", np.arange(5))
    monkeypatch.setattr(logger, "configure", lambda *a, **k: None)
    monkeypatch.setattr(mod, "require_gpu", lambda prog: torch.device("cpu"))
    with pytest.raises(SystemExit) as e:
        mod.main(["--init-img", str(tmp_path / "init.npy"), "--mask", str(tmp_path / "mask.npy"), "--prompt_ids", str(tmp_path / "ids.npy")])
    assert str(e.value).startswith("sd_inpaint.py: --prompt_ids must hold an integer [1 | n_samples, T] array")


# ------------------------------------------------------------------ --prompt_ids
def test_prompt_id_reader(tmp_path):
    path = str(tmp_path / "ids.npy")
    for bad in (np.arange(5), np.zeros((2, 5), np.float32)):          # 1-D; not integer
        np.save(path, bad)
        for prog in ("sd_search_ea.py", "sd_clip_score.py"):
            with pytest.raises(SystemExit) as e:
                sd_script_util.read_prompt_ids(path, prog)
            assert str(e.value).startswith(prog + ": --prompt_ids must hold an integer [num, T] array, got ")
    ids = np.array([[3, 1, 4, 1, 5]], np.int32)
    np.save(path, ids)
    got = sd_script_util.read_prompt_ids(path, "sd_search_ea.py")
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == ids.tolist()


def test_load_prompts_repeats_one_row_or_takes_n_samples_rows(tmp_path):
    path = str(tmp_path / "ids.npy")
    opt = argparse.Namespace(prompt_ids=path, n_samples=3, tokenizer_dir="", prompt="a cat")
    rows = np.arange(3 * 7, dtype=np.int64).reshape(3, 7)
    np.save(path, rows[:1])
    ids, empty, t = sd_script_util.load_prompts(opt, "cpu", "sd_img2img.py")
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.tolist() == [rows[0].tolist()] * 3 and empty == ["", "", ""] and t == 7
    np.save(path, rows)
    assert sd_script_util.load_prompts(opt, "cpu", "sd_img2img.py")[0].tolist() == rows.tolist()
    np.save(path, rows[:2])
    with pytest.raises(SystemExit) as e:
        sd_script_util.load_prompts(opt, "cpu", "sd_img2img.py")
    assert str(e.value).startswith("sd_img2img.py: --prompt_ids must hold an integer [1 | n_samples, T] array, got int64 (2, 7)")
    opt.prompt_ids = ""
    with pytest.raises(SystemExit) as e:                                # strings need a tokenizer
        sd_script_util.load_prompts(opt, "cpu", "sd_inpaint.py")
    assert str(e.value).startswith("sd_inpaint.py: --prompt needs --tokenizer_dir")
    opt.tokenizer_dir = str(tmp_path)
    assert sd_script_util.load_prompts(opt, "cpu", "sd_inpaint.py") == (["a cat"] * 3, [""] * 3, None)


# ------------------------------------------------------------------ build_model
class _NoUNet:
    """Stands in for the latent UNet, which takes no part in what the case below checks and two of the three seconds a tiny
    LatentDiffusion takes to build on the host."""

    def __init__(self, **cfg):
        self.seed = None

    def set_torso(self, torso):
        return self

    def randomize_(self, seed):
        self.seed = seed

    def to(self, device):
        return self


@pytest.mark.parametrize("with_encoder", [False, True])
def test_build_model_takes_the_encoder_from_its_keyword_alone(with_encoder, monkeypatch):
    """--synthetic tiny builds on the host (nothing is launched before the first forward).  The first stage has its image encoder
    exactly when with_encoder= says so; an ``opt.with_encoder`` attribute, how the scripts once asked for it, changes nothing."""
    monkeypatch.setattr(sd_script_util, "UNetModel", _NoUNet)
    monkeypatch.setattr(logger, "log", lambda *a: None)
    opt = argparse.Namespace(synthetic="tiny", config="", ckpt="", tokenizer_dir="", torso="bf16", with_encoder=not with_encoder)
    model = sd_script_util.build_model(opt, torch.device("cpu"), prompt_len=8, with_encoder=with_encoder)
    assert (model.first_stage_model.encoder is not None) == with_encoder
    assert model.model.seed == 1234 and isinstance(model.cond_stage_model._tokenizer, sd_script_util.EmptyPromptTokenizer)
