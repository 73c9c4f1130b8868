#!/usr/bin/env python3
"""Do two commits of the host code launch the same kernels and compute the same bits?  For a refactor of the model files
(unet.py, classifier.py, sd_unet.py, sd_vae.py) that claims to change neither.  Run it once per tree, in one GPU job, against the
SAME two built libraries (ADM_HIP_LIB / ADM_HIP_LIB_F16 point a tree without libraries at the other's), each step under its own
time limit, and compare:
    timeout -k 10 600 python tools/model_fingerprint.py PARENT_TREE > profiles/<change>/fingerprint_parent.txt
    timeout -k 10 600 python tools/model_fingerprint.py             > profiles/<change>/fingerprint_head.txt
    cmp profiles/<change>/fingerprint_parent.txt profiles/<change>/fingerprint_head.txt
It imports the package and the test helpers of the given tree (default: the tree this file is in) and uses only public
constructors, tests/helpers.py, the fixtures under tests/golden/ and tests/launch_replay.Recorder.  The small models of the GPU
tests run at batch 2 on inputs seeded on the CPU, in both torsos, eagerly and -- where the model has enable_graph -- replayed
twice; the maps span 8x8, 16x16 and 32x32, the smallest at which the skip fold, the fused statistics, the phase convs and the
virtual upsample switch on.  One line per output tensor (SHA-256 of its bytes) and one per case for the launches (SHA-256 of the
sorted (record, count) list the recorder saw).  One shot: nothing is retried.
"""
import ast
import collections
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pytest  # noqa: E402
import torch  # noqa: E402

import launch_replay as lr  # noqa: E402
from helpers import filled, golden, plan_c64, plan_m32, plan_m64  # noqa: E402
from oracle.fill import fill_array  # noqa: E402
from test_sd_oracle import sd_case  # noqa: E402
from test_variants import CASES, CLF_CASES, clf_plan_of, plan_of  # noqa: E402

DEV = torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def case(name, fn):
    """Run fn() -> tensor or tuple of tensors under the launch recorder and print the fingerprint lines."""
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        seen, add = collections.Counter(), rec._add
        rec._add = lambda r: (seen.update([r]), add(r))
        out = fn()
        torch.cuda.synchronize()
    for i, t in enumerate(out if isinstance(out, tuple) else (out,)):
        data = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
        print(f"{name} out{i} {tuple(t.shape)} {hashlib.sha256(data).hexdigest()}")
    launches = sorted((repr(r), c) for r, c in seen.items())
    print(f"{name} launches {len(launches)} records {sum(seen.values())} calls {hashlib.sha256(repr(launches).encode()).hexdigest()}")


def each_torso(name, model, runs, graph=True):
    """runs: {tag: callable}; every one eagerly, then (graph) captured and replayed -- two replays of one capture."""
    for torso in ("bf16", "fp16"):
        model.set_torso(torso)
        for tag, fn in runs.items():
            case(f"{name} {torso} {tag} eager", fn)
            if graph:
                model.enable_graph(True)
                case(f"{name} {torso} {tag} graph capture+replay", fn)
                case(f"{name} {torso} {tag} graph replay", fn)
                model.enable_graph(False)
    torch.cuda.empty_cache()


def adm_unet(name, plan, size, skips):
    from autodiffusion_amd.unet import UNetModel
    model = UNetModel(plan)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled(plan).items()})
    model.to(DEV).eval()
    x, t, y = rnd((2, 3, size, size), 1), torch.tensor([10, 500], device=DEV), torch.tensor([1, 7], device=DEV)
    each_torso(name, model, {f"skip {s}": (lambda s=s: model(x, t, y, skip_layer=s) if s else model(x, t, y)) for s in skips})


def adm_classifier(name, plan):
    from autodiffusion_amd.classifier import EncoderUNetModel
    model = EncoderUNetModel(plan)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled(plan).items()})
    model.to(DEV).eval()
    x, t, y = rnd((2, 3, 64, 64), 2), torch.tensor([10, 500], device=DEV), torch.tensor([1, 7], device=DEV)
    each_torso(name, model, {"logits": lambda: model(x, t)}, graph=False)
    each_torso(name, model, {"log_prob_grad": lambda: model.log_prob_grad(x, t, y, 1.0, return_logits=True)})


def sd_unet(name):
    from autodiffusion_amd.sd_unet import UNetModel
    g, plan, P = sd_case(name)
    model = UNetModel(image_size=32, use_spatial_transformer=True, **ast.literal_eval(str(g["cfg"])))
    model.load_state_dict(P)
    model.to(DEV).eval()
    t = torch.tensor([10, 500], device=DEV)
    ctx = rnd((2, g["context"].shape[1], plan.context_dim), 4)
    for hw in (16, 32):
        x = rnd((2, 4, hw, hw), 3)
        each_torso(f"{name} {hw}x{hw}", model, {"plain": lambda: model(x, t, ctx),
                                               "context_key twice": lambda: (model(x, t, ctx, context_key="a"), model(x, t, ctx, context_key="a"))})
        model.enable_splitk(True)
        each_torso(f"{name} {hw}x{hw} splitk", model, {"plain": lambda: model(x, t, ctx)})
        model.enable_splitk(False).enable_upconv_phases(False)
        each_torso(f"{name} {hw}x{hw} one-launch upsample", model, {"plain": lambda: model(x, t, ctx)})
        model.enable_upconv_phases(True)


def sd_vae(name):
    from autodiffusion_amd.sd_vae import AutoencoderKL
    g = golden(name)
    vae = AutoencoderKL(ast.literal_eval(str(g["cfg"])), int(g["embed_dim"]))
    vae.load_state_dict({k: torch.from_numpy(fill_array("first_stage_model." + k, tuple(v.shape))) for k, v in vae.state_dict().items()})
    vae.to(DEV)
    for hw in (8, 16):
        z = rnd((2, vae.embed_dim, hw, hw), 5, 0.18215 * 4)
        each_torso(f"{name} {hw}x{hw}", vae, {"decode": lambda: vae.decode(z, 1.0 / 0.18215)}, graph=False)


if __name__ == "__main__":
    adm_unet("plan_m32", plan_m32(dynamic=True), 32, ([], [1], [0, 5]))
    adm_unet("plan_m32 legacy", plan_m32(dynamic=True, legacy=True), 32, ([],))
    adm_unet("plan_m64", plan_m64(), 64, ([],))
    for tag in CASES:
        skip = golden("unet_m32_variants")[f"skip_{tag}"].tolist() if CASES[tag][2] else None
        adm_unet(f"unet_m32_variants {tag}", plan_of(tag), 32, ([],) + ((skip,) if skip else ()))
    for tag in CLF_CASES:
        adm_classifier(f"clf_variants {tag}", clf_plan_of(tag))
    adm_classifier("plan_c64", plan_c64())
    for name in ("sd_unet_tiny", "sd_unet_w320"):
        sd_unet(name)
    for name in ("sd_vae_tiny", "sd_vae_mid512"):
        sd_vae(name)
