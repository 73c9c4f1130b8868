"""GPU: the Stable Diffusion 2.x family on the HIP path -- linear-shaped proj_in / proj_out weights in the latent
UNet with 64-wide heads and a 77-row context, the OpenCLIP-style text tower (exact GELU, last and penultimate exits) against the
float64 capture of transformers' CLIPTextModel (tests/golden/capture_openclip_text.py), and the command lines under
``--synthetic tiny2``.

Bounds.  UNet: the project's SD UNet bound (tests/test_hip_sd.py): relative Frobenius <= 2e-2, max |err| <= 6e-2 max |ref|.  Text
tower: the caps tests/test_hip_clip.py holds the v1 tower to: relative Frobenius <= 2e-2 in bf16, 5e-3 in fp16.  A tower run with
quick_gelu in place of the exact GELU lies about 1e-2 from the stored outputs (8.9e-3 penultimate, 1.1e-2 last, measured on the CPU
in float64 when the fixture was captured): outside the fp16 cap, which is asserted; INSIDE the bf16 cap, whose 2e-2 cannot tell
the two activations apart on any tower of this depth -- in bf16 the test asserts instead that the quick_gelu run is farther from
the reference than the gelu run.  Per element, both torsos tell them apart (tests/test_hip_sd_param.py, tests/test_sd_param_host.py).
"""
import ast

import numpy as np
import pytest
import torch

from helpers import golden
from oracle.fill import fill_state_dict
from test_hip_sd import _model, check
from test_hip_sd_search import _cli, _cli_flags, _leading_fid  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRO = {"bf16": 2e-2, "fp16": 5e-3}   # tests/test_hip_clip.py


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ use_linear_in_transformer
def test_linear_projection_weights_are_the_same_network_as_the_1x1_convs():
    from autodiffusion_amd.sd_arch import SDTransformerSpec, sd_unet_plan
    from autodiffusion_amd.sd_script_util import TINY2_UNET
    from oracle import sd_nets
    lin = sd_unet_plan(**TINY2_UNET)
    conv = sd_unet_plan(**dict(TINY2_UNET, use_linear_in_transformer=False))
    assert {(b.heads, b.d_head) for b in lin.all_blocks() if isinstance(b, SDTransformerSpec)} == {(1, 64), (2, 64)}
    P = {k: torch.from_numpy(v) for k, v in fill_state_dict(lin.param_shapes()).items()}
    shapes = conv.param_shapes()
    Pc = {k: v.reshape(shapes[k]) for k, v in P.items()}
    moved = [k for k in P if P[k].shape != Pc[k].shape]
    n_tr = sum(isinstance(b, SDTransformerSpec) for b in lin.all_blocks())
    assert n_tr == 7 and len(moved) == 2 * n_tr and all(P[k].dim() == 2 and Pc[k].dim() == 4 for k in moved)
    g = torch.Generator().manual_seed(21)
    x, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 77, 128, generator=g)
    t = torch.tensor([981, 37])
    out = _model(lin, P)(x.to(DEV), t.to(DEV), ctx.to(DEV))
    out_conv = _model(conv, Pc)(x.to(DEV), t.to(DEV), ctx.to(DEV))
    assert out.shape == (2, 4, 16, 16) and torch.equal(out, out_conv)
    ref = sd_nets.sd_unet_forward(Pc, conv, x, t, ctx)
    check(out, ref.numpy(), "tiny2 UNet, linear proj_in / proj_out, 64-wide heads, 77-row context")


# ------------------------------------------------------------------ the OpenCLIP-style text tower
def _openclip_case():
    g = golden("openclip_text_tiny")
    sd = {}
    for k in g.files:
        if k.startswith("q::"):
            sd[k[3:]] = torch.from_numpy(g[k].astype(np.float32) * g["s::" + k[3:]])
        elif k.startswith("v::"):
            sd[k[3:]] = torch.from_numpy(g[k])
    return g, ast.literal_eval(str(g["cfg"])), sd


def _tower(cfg, sd, layer, torso):
    from autodiffusion_amd.sd_clip import FrozenOpenCLIPEmbedder
    emb = FrozenOpenCLIPEmbedder(device="cpu", max_length=77, layer=layer, config=cfg)
    emb.load_state_dict({**sd, "model.text_projection": torch.zeros(128, 64), "model.logit_scale": torch.zeros(())}, strict=True)
    return emb.set_torso(torso).to(DEV)


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
def test_text_tower_matches_the_float64_capture_at_both_exits(torso):
    g, cfg, sd = _openclip_case()
    assert cfg["hidden_act"] == "gelu" and len(sd) == 2 + 12 * cfg["num_hidden_layers"] + 2
    ids = torch.from_numpy(g["ids"])
    assert int(ids[2, 76]) == cfg["vocab_size"] - 1 and bool((ids[0, 7:] == 0).all())
    fro = {}
    for act in ("gelu", "quick_gelu"):
        for layer in ("penultimate", "last"):
            ref = torch.from_numpy(g[layer])
            got = _tower(dict(cfg, hidden_act=act), sd, layer, torso)(ids.to(DEV)).cpu()
            assert got.shape == ref.shape == (3, 77, 128) and got.dtype == torch.float32 and torch.isfinite(got).all()
            fro[act, layer] = float((got - ref).norm() / ref.norm())
            print(f"openclip_text_tiny {torso} {act} {layer}: rel fro {fro[act, layer]:.4g}")
    # the two exits are different tensors: the other exit's reference is far away
    pen = _tower(cfg, sd, "penultimate", torso)(ids.to(DEV)).cpu()
    assert float((pen - torch.from_numpy(g["last"])).norm() / torch.from_numpy(g["last"]).norm()) > 0.3
    for layer in ("penultimate", "last"):
        assert fro["gelu", layer] <= FRO[torso], (layer, fro)
        assert fro["quick_gelu", layer] > fro["gelu", layer], (layer, fro)
        if torso == "fp16":       # module docstring: the bf16 cap is wider than the distance between the two activations
            assert fro["quick_gelu", layer] > FRO[torso], (layer, fro)


# ------------------------------------------------------------------ the command lines
def test_search_and_evaluate_under_synthetic_tiny2(_leading_fid, tmp_path, monkeypatch):  # noqa: F811
    from autodiffusion_amd import sd_sampler
    from autodiffusion_amd.sd_clip import FrozenOpenCLIPEmbedder
    from autodiffusion_amd.sd_search import parse_sd_candidate
    seen = []
    real = sd_sampler.sd_step

    def sd_step(*a, **kw):
        seen.append(kw.get("param", "eps"))
        return real(*a, **kw)
    monkeypatch.setattr(sd_sampler, "sd_step", sd_step)
    flags = _cli_flags(tmp_path) + ["--synthetic", "tiny2", "--time_step", "2", "--max_epochs", "1"]
    s = _cli().main(flags)
    model = s.sampler.model
    assert model.parameterization == "v" and type(model.cond_stage_model) is FrozenOpenCLIPEmbedder
    assert model.cond_stage_model.transformer.plan.run_layers == 1
    assert seen and set(seen) == {"v"}
    lines = (tmp_path / "out" / "log.txt").read_text().splitlines()
    assert "synthetic='tiny2'" in lines[0] and "epoch = 0" in lines and "epoch = 1" not in lines
    fits = {c: info["fid"] for c, info in s.vis_dict.items()}
    assert len(fits) >= 4 and all(len(parse_sd_candidate(c)) == 2 for c in fits) and all(np.isfinite(f) for f in fits.values())
    best = s.keep_top_k[50][0]
    assert fits[best] == min(fits.values())
    fid = _cli().main(flags + ["--evaluate", best])
    assert fid == fits[best]


def test_img2img_cli_under_synthetic_tiny2(tmp_path):
    """scripts/sd_img2img.py as a child process, as tests/test_hip_sd_vae_encode.py runs it for ``tiny``."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rs = np.random.RandomState(3)
    np.save(tmp_path / "init.npy", rs.randint(0, 256, size=(1, 64, 64, 3)).astype(np.uint8))
    np.save(tmp_path / "ids.npy", rs.randint(1, 500, size=(1, 8)).astype(np.int64))
    cmd = [sys.executable, os.path.join(root, "scripts", "sd_img2img.py"), "--synthetic", "tiny2", "--init-img", str(tmp_path / "init.npy"),
           "--prompt_ids", str(tmp_path / "ids.npy"), "--n_samples", "2", "--n_iter", "1", "--ddim_steps", "2", "--strength", "0.5",
           "--use_timestep", "[424, 926]", "--scale", "3.0", "--outdir", str(tmp_path / "out"), "--seed", "7"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "--synthetic tiny2" in res.stdout + res.stderr
    arr = np.load(tmp_path / "out" / "samples_2x64x64x3.npz")["arr_0"]
    assert arr.shape == (2, 64, 64, 3) and arr.dtype == np.uint8 and arr.std() > 0
