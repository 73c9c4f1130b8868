"""The two command lines of the CLIP score on the GPU, end to end on the tiny networks: scripts/sd_clip_score.py as a child
process on a sample file, and scripts/sd_search_ea.py --clip_ckpt scoring one candidate with both CLIP towers read from one file."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_under_test", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tiny_clip_checkpoint(path, openai=False):
    """Both tiny towers in one plain state dict, CLIPModel layout (or the OpenAI one)."""
    from autodiffusion_amd.sd_clip import CLIP_TINY_TEXT_PROJ, CLIP_TINY_VISION, CLIPTextTransformer, CLIPVisionTransformer
    vis = CLIPVisionTransformer(**CLIP_TINY_VISION).randomize_(11).state_dict()
    txt = CLIPTextTransformer(**CLIP_TINY_TEXT_PROJ).randomize_(12).state_dict()
    if openai:
        from test_clip_image_host import to_openai
        sd = dict(to_openai(vis), **to_openai(txt, tower=""))
    else:
        sd = dict(vis, **txt)
    torch.save({k: v.clone() for k, v in sd.items()}, path)
    return path


def test_clip_score_cli(tmp_path):
    rs = np.random.RandomState(4)
    np.savez(tmp_path / "samples_5x48x40x3.npz", rs.randint(0, 256, size=(5, 48, 40, 3)).astype(np.uint8))
    ids = rs.randint(0, 500, size=(6, 77)).astype(np.int64)
    np.save(tmp_path / "ids.npy", ids)
    base = [sys.executable, os.path.join(ROOT, "scripts", "sd_clip_score.py"), str(tmp_path / "samples_5x48x40x3.npz"),
            "--prompt_ids", str(tmp_path / "ids.npy"), "--batch_size", "2"]
    res = subprocess.run(base + ["--synthetic", "tiny"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "images: 5," in res.stdout and "RANDOM weights" in res.stdout
    score = float(re.search(r"^CLIP score: (\S+)$", res.stdout, re.M).group(1))
    assert np.isfinite(score) and 0.0 <= score <= 100.0
    # in this process: another batching gives the same score; neither --clip_ckpt nor --synthetic is refused
    cli = _script("sd_clip_score")
    assert cli.main(base[2:] + ["--synthetic", "tiny", "--batch_size", "5"]) == score
    with pytest.raises(SystemExit, match="--clip_ckpt"):
        cli.main(base[2:])


def test_search_cli_logs_the_clip_score_of_a_candidate(tmp_path, capsys):
    cli = _script("sd_search_ea")
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "ref.npz", mu=rs.randn(2048) * 0.05, sigma=0.25 * np.eye(2048))
    np.save(tmp_path / "ids.npy", torch.randint(0, 512, (6, 77), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int64))
    argv = ["--synthetic", "tiny", "--allow_random_inception", "--H", "128", "--W", "128", "--n_samples", "2", "--num_sample", "3",
            "--scale", "7.5", "--seed", "7", "--time_step", "2", "--evaluate", "[300, 800]", "--ref_mu", str(tmp_path / "ref.npz"),
            "--prompt_ids", str(tmp_path / "ids.npy"), "--outdir", str(tmp_path / "out")]
    fid = cli.main(argv + ["--clip_ckpt", _tiny_clip_checkpoint(str(tmp_path / "clip.pt"))])
    out = capsys.readouterr().out
    scores = re.findall(r"CLIP score: ([-+.e\d]+)", out)
    assert np.isfinite(fid) and len(scores) == 1 and np.isfinite(float(scores[0]))
    # the same towers from the OpenAI layout: the same score to the bit
    assert cli.main(argv + ["--clip_ckpt", _tiny_clip_checkpoint(str(tmp_path / "clip_openai.pt"), openai=True)]) == fid
    assert re.findall(r"CLIP score: ([-+.e\d]+)", capsys.readouterr().out) == scores
