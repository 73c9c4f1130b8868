"""GPU parity of the Stable-Diffusion first stage's encode half and of image-to-image on the HIP path: adm_resample mode 5 and the
Downsample it makes of a stride-1 conv, adm_vec_act modes 3 / 4 and the eps-free adm_sd_step against their float64 restatements
(tests/f32_vae_kernels.py), the encoder against golden vectors captured from the reference's own ``Encoder``
(tests/golden/capture_sd_vae_encoder.py), batch / chunk independence, ``DDIMSampler.stochastic_encode`` / ``.decode`` against the
reference's (tests/golden/capture_sd_img2img.py), and image -> latent -> noised -> denoised -> image end to end.

Bounds: the kernel bound of test_hip_kernels.py (assert_close_bf16: max <= 1e-2 max|ref|, Frobenius <= 4e-3) for the Downsample
composite; the network caps of test_hip_fullsize.py on the moments (relative Frobenius <= 2e-2 in bf16, 5e-3 in fp16: what the
decoder test uses; the encoder is a chain of the same kernels); rtol = atol = 2e-5, test_hip_sd.py's bound on the DDIM step, for
axpby_noise against fp32 torch and for the img2img latents.  Measured on MI355X, moments bf16 / fp16:
sd_vae_enc_tiny 1.12e-2 / 1.35e-3, sd_vae_enc_mid512 8.7e-3 / 1.08e-3, full_sd_vae_enc 1.28e-2 / 1.61e-3; worst error / bound of the
posterior's sample 0.43, of gauss_std 0.13, of axpby_noise 0.99 (two roundings of three at 2 M elements); Downsample composite
Frobenius 1.7e-3 / 2.1e-4.
"""
import ast
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_vae_kernels as V
from oracle.fill import fill_array

from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FRO = {"bf16": 2e-2, "fp16": 5e-3}   # tests/test_hip_fullsize.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def assert_close_bf16(got, ref, what=""):   # tests/test_hip_kernels.py
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    fro = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
    print(f"{what}: max err {err:.4g} (scale {scale:.4g}), fro {fro:.4g}")
    assert err <= 1e-2 * scale and fro <= 4e-3, f"{what}: max err {err:.4g} (scale {scale:.4g}), fro {fro:.4g}"


def _hold(what, got, ref, bound):
    """Every element within its bound of the float64 restatement; prints the worst ratio before asserting."""
    got = got.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    worst = float(((got - ref).abs() / bound).max())
    print(f"{what}: worst err/bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst err/bound {worst:.3f}"


# ------------------------------------------------------------------ adm_resample mode 5
@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("n,h,w,c", [(1, 2, 2, 32), (2, 6, 10, 32), (1, 16, 16, 64)])
def test_stride2_odd(n, h, w, c, torso):
    from autodiffusion_amd import ops
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, h, w, c, generator=g).to(DTYPES[torso]).to(DEV)
    got = ops.resample(x, "stride2_odd")
    assert got.shape == (n, h // 2, w // 2, c) and got.dtype == x.dtype
    assert torch.equal(got, x[:, 1::2, 1::2].contiguous())
    assert not torch.equal(got, ops.resample(x, "stride2"))
    # the entry point itself on a caller-owned buffer with a sentinel-filled guard region behind the output
    from autodiffusion_amd import _lib
    items = got.numel()
    buf = torch.full((items + 4096,), -7.0, dtype=x.dtype, device=DEV)
    _lib.check(_lib.load("f16" if torso == "fp16" else "bf16").adm_resample(x.data_ptr(), None, None, buf.data_ptr(), n, h, w, c, 5,
                                                                          torch.cuda.current_stream().cuda_stream), "adm_resample")
    torch.cuda.synchronize()
    assert torch.equal(buf[:items].view_as(got), got) and bool((buf[items:] == -7.0).all()), "written beyond the output"
    # with the affine: SiLU(a x + b) of the picked pixel, as mode 3 computes it on the map shifted by one pixel
    a = (torch.rand(n, c, generator=g) + 0.5).to(DEV)
    b = (torch.randn(n, c, generator=g) * 0.3).to(DEV)
    shifted = torch.zeros_like(x)
    shifted[:, :h - 1, :w - 1] = x[:, 1:, 1:]
    assert torch.equal(ops.resample(x, "stride2_odd", (a, b)), ops.resample(shifted, "stride2", (a, b)))


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", [16, 8])
def test_downsample_composite_matches_the_padded_stride2_conv(hw, torso):
    """model.py:60-79 on the same 16-bit operands: conv2d(pad(x, (0, 1, 0, 1)), w, b, stride=2) in fp32."""
    from autodiffusion_amd import ops
    dt = DTYPES[torso]
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(2, 32, hw, hw, generator=g).to(dt)
    w = (torch.randn(32, 32, 3, 3, generator=g) * (32 * 9) ** -0.5).to(dt)
    b = torch.randn(32, generator=g) * 0.1
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b, stride=2).permute(0, 2, 3, 1)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = ops.resample(ops.conv(xd, ops.pack_conv_weight(w.float().to(DEV), dt), b.to(DEV), 32, 9), "stride2_odd")
    assert got.shape == (2, hw // 2, hw // 2, 32)
    assert_close_bf16(got.float().cpu(), ref, f"Downsample {hw} -> {hw // 2} {torso}")


# ------------------------------------------------------------------ adm_vec_act modes 3 / 4, adm_sd_step as a x + b noise
def _gauss_inputs(items):
    g = torch.Generator().manual_seed(items)
    x = torch.randn(items, generator=g) * 12
    x[:len(V.GAUSS_SPECIALS)] = torch.tensor(V.GAUSS_SPECIALS)
    return x, torch.randn(items, generator=g)


@pytest.mark.parametrize("items", [11, 1000, 4096 * 256 + 259])   # below a block; no multiple of 256; past the 4096-block grid cap
def test_gauss_std_and_logvar(items):
    from autodiffusion_amd import ops
    x, dy = _gauss_inputs(items)
    xd, dyd = x.to(DEV), dy.to(DEV)
    assert bool((x < -30).any()) and bool((x > 20).any())
    _hold(f"gauss_std {items}", ops.vec_act(xd, "gauss_std"), *V.gauss_std_restate(x))
    _hold(f"gauss_std x dy {items}", ops.vec_act(xd, "gauss_std", dy=dyd), *V.gauss_std_restate(x, dy))
    lv = ops.vec_act(xd, "gauss_logvar").cpu()
    want = V.gauss_logvar_restate(x)
    assert torch.equal(lv, want) and torch.equal(torch.signbit(lv), torch.signbit(want))
    assert float(lv.min()) == -30.0 and float(lv.max()) == 20.0
    nan = ops.vec_act(torch.tensor([float("nan"), 1.0], device=DEV), "gauss_logvar").cpu()
    assert bool(torch.isnan(nan[0])) and float(nan[1]) == 1.0   # torch.clamp keeps a NaN, too


@pytest.mark.parametrize("a,b", [(0.9991, 0.0424), (0.0683, 0.9977), (0.18215, 0.18215), (0.18215, 0.0)])
@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (3, 4, 9, 7), (8192 * 256 + 259,)])
def test_axpby_noise(shape, a, b):
    from autodiffusion_amd.sd_sampler import axpby_noise
    g = torch.Generator().manual_seed(len(shape))
    x, n = torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g)
    got = axpby_noise(x.to(DEV), a, n.to(DEV), b)
    assert got.shape == x.shape and got.dtype == torch.float32
    _hold(f"axpby_noise {shape} a={a} b={b}", got, *V.axpby_noise_restate(x, a, n, b))
    want = torch.tensor(np.float32(a)) * x + torch.tensor(np.float32(b)) * n
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
    if b == 0.0:   # scale_factor * z with the tensor itself as the (finite) eps operand: one rounding
        assert torch.equal(got.cpu(), torch.tensor(np.float32(a)) * x)


# ------------------------------------------------------------------ the network
_VAES = {}


def _vae(name, torso):
    """AutoencoderKL(with_encoder=True) of a fixture's config; the encode half filled from oracle/fill.py under the checkpoint's
    names (the decode half keeps what the constructor drew: these tests do not decode with it)."""
    from autodiffusion_amd.sd_vae import AutoencoderKL
    key = (name, torso)
    if key not in _VAES:
        g = golden(name)
        vae = AutoencoderKL(ast.literal_eval(str(g["cfg"])), int(g["embed_dim"]), with_encoder=True)
        sd = vae.state_dict()
        sd.update({k: torch.from_numpy(fill_array("first_stage_model." + k, tuple(v.shape))) for k, v in sd.items()
                   if k.startswith(("encoder.", "quant_conv."))})
        vae.load_state_dict(sd)
        _VAES[key] = (vae.set_torso(torso).to(DEV), g)
    return _VAES[key]


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["sd_vae_enc_tiny", "sd_vae_enc_mid512", "full_sd_vae_enc"])
def test_encode_matches_the_reference_encoder(name, torso):
    """Moments after quant_conv against the reference's, inside the network caps; the posterior's halves are copies of them, and
    its sample with the fixture's noise follows from the KERNEL's moments through the float64 restatement (a logvar error enters
    the reference's sample through exp, so that one is printed, not bounded)."""
    vae, g = _vae(name, torso)
    ref = torch.from_numpy(g["moments"])
    x = torch.from_numpy(g["x"]).to(DEV)
    post = vae.encode(x)
    got = post.parameters.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    fro = float((got - ref).norm() / ref.norm())
    print(f"{name} {torso}: moments rel fro {fro:.4g}, max |err| {float((got - ref).abs().max()):.4g} (max |ref| {float(ref.abs().max()):.4g})")
    assert fro <= FRO[torso], f"{name} {torso}: rel fro {fro:.4g}"
    e = int(g["embed_dim"])
    assert torch.equal(post.mean.cpu(), got[:, :e]) and torch.equal(post.mode(), post.mean) and post.mean.is_contiguous()
    assert torch.equal(post.logvar.cpu(), got[:, e:])   # inside (-30, 20): the clamp is a copy here
    _hold(f"{name} {torso} std", post.std, *V.gauss_std_restate(got[:, e:].contiguous()))
    noise = torch.from_numpy(g["noise"])
    z = post.sample(noise=noise.to(DEV))
    _hold(f"{name} {torso} sample", z, *V.posterior_sample_restate(got[:, :e], got[:, e:], noise))
    zr = torch.from_numpy(g["sample"])
    print(f"{name} {torso}: sample vs the reference's rel fro {float((z.cpu() - zr).norm() / zr.norm()):.4g}")
    if name == "full_sd_vae_enc":
        _VAES.pop((name, torso))   # 83.7 M parameters twice over: not kept for the session


def test_encode_is_independent_of_batch_and_chunk():
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    vae, _ = _vae("sd_vae_enc_tiny", "bf16")
    x = torch.tanh(torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(9))).to(DEV)
    both = vae.encode_moments(x)
    assert both.shape == (3, 8, 8, 8)
    for i in range(3):
        assert torch.equal(vae.encode_moments(x[i:i + 1].contiguous())[0], both[i]), i
    ld = LatentDiffusion(types.SimpleNamespace(device=torch.device(DEV)), first_stage=vae)
    posts = [ld.encode_first_stage(x, chunk=ch) for ch in (1, 2, 3, None)]
    for p in posts:
        assert torch.equal(p.parameters, both) and torch.equal(p.mean, posts[0].mean) and torch.equal(p.std, posts[0].std)
    # scale_factor * z: the mode of the posterior is its zero-noise sample
    zero = torch.zeros_like(posts[0].mean)
    z0 = ld.get_first_stage_encoding(posts[0], noise=zero)
    assert torch.equal(z0, posts[0].mode() * ld.scale_factor) and ld.scale_factor == 0.18215
    assert torch.equal(ld.get_first_stage_encoding(posts[0].mean), z0)   # a tensor is scaled as it is (ddpm.py:545-546)
    noise = torch.randn(zero.shape, generator=torch.Generator().manual_seed(10)).to(DEV)
    z = ld.get_first_stage_encoding(posts[0], noise=noise)
    _hold("get_first_stage_encoding", z, *V.posterior_sample_restate(both[:, :4].cpu(), both[:, 4:].cpu(), noise.cpu(), ld.scale_factor))
    gen = torch.Generator(device=DEV)
    a, b = posts[0].sample(generator=gen.manual_seed(5)), posts[0].sample(generator=gen.manual_seed(5))
    assert torch.equal(a, b) and not torch.equal(a, posts[0].sample(generator=gen.manual_seed(6)))


# ------------------------------------------------------------------ img2img against the reference's DDIMSampler
class _ToyLatentModel:
    """The attributes of LatentDiffusion the samplers read; apply_model = the capture script's toy model, on the GPU."""

    def __init__(self):
        from autodiffusion_amd.sd_sampler import LatentDiffusion
        base = LatentDiffusion(None, device=DEV)
        self.num_timesteps, self.device = base.num_timesteps, base.device
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = base.betas, base.alphas_cumprod, base.alphas_cumprod_prev
        self.q_sample = base.q_sample

    def apply_model(self, x, t, c):
        from oracle.sd_sampler import toy_model
        return toy_model(x, t, c)


def test_stochastic_encode_and_decode_match_reference_goldens():
    from autodiffusion_amd.sd_sampler import DDIMSampler
    g = golden("sd_img2img")
    x0, noise, c, uc = (torch.from_numpy(g[k]).to(DEV) for k in ("x0", "noise", "c", "uc"))
    steps = int(g["steps"])
    m = _ToyLatentModel()
    for tag, cand in (("uniform4", None), ("k4", [153, 424, 926, 690])):
        s = DDIMSampler(m)
        s.make_schedule(ddim_num_steps=steps, ddim_eta=0.0, verbose=False, sampled_timestep=None if cand is None else np.array(sorted(cand)))
        np.testing.assert_array_equal(np.asarray(s.ddim_timesteps), g[f"timesteps_{tag}"])
        for t_enc in (1, 2, steps):
            t_idx = min(t_enc, steps - 1)   # entry `steps` does not exist (capture_sd_img2img.py)
            z = s.stochastic_encode(x0, torch.tensor([t_idx] * x0.shape[0]), noise=noise)
            np.testing.assert_allclose(z.cpu().numpy(), g[f"enc_{tag}_{t_idx}"], rtol=2e-5, atol=2e-5, err_msg=f"encode {tag} {t_idx}")
            assert torch.equal(z, s.stochastic_encode(x0, t_idx, noise=noise))
            # entry t of the table is timestep ddim_timesteps[t]: q_sample at that timestep is the same noising
            qs = m.q_sample(x0, int(np.asarray(s.ddim_timesteps)[t_idx]), noise=noise)
            np.testing.assert_allclose(qs.cpu().numpy(), z.cpu().numpy(), rtol=2e-6, atol=2e-6)
            for gtag, (scale, u) in {"cfg": (7.5, uc), "plain": (1.0, None)}.items():
                z_ref = torch.from_numpy(g[f"enc_{tag}_{t_idx}"]).to(DEV)
                got = s.decode(z_ref, c, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=u)
                np.testing.assert_allclose(got.cpu().numpy(), g[f"dec_{tag}_{t_enc}_{gtag}"], rtol=2e-5, atol=2e-5,
                                           err_msg=f"decode {tag} {t_enc} {gtag}")
    with pytest.raises(IndexError):
        s.stochastic_encode(x0, steps, noise=noise)
    with pytest.raises(NotImplementedError):   # masked sampling stays out of scope
        s.sample(S=4, batch_size=3, shape=[4, 8, 8], conditioning=c, x_T=x0, mask=torch.ones(1))


def _tiny_pipeline():
    from autodiffusion_amd.sd_sampler import DDIMSampler, LatentDiffusion
    from autodiffusion_amd.sd_unet import UNetModel
    from test_sd_oracle import sd_case
    g, plan, P = sd_case("sd_unet_tiny")
    unet = UNetModel(image_size=32, use_spatial_transformer=True, **ast.literal_eval(str(g["cfg"])))
    unet.load_state_dict(P)
    unet.to(DEV)
    vae, _ = _vae("sd_vae_enc_tiny", "bf16")
    ld = LatentDiffusion(unet, device=DEV, first_stage=vae)
    ctx = torch.from_numpy(g["context"]).to(DEV)
    return ld, DDIMSampler(ld), ctx, (ctx.flip(1).contiguous() * 0.5)


def test_decode_under_split_guidance_is_bit_identical():
    ld, s, c, uc = _tiny_pipeline()
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(12)).to(DEV)
    s.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False, sampled_timestep=np.array([153, 424, 690, 926]))
    outs = []
    for split in (True, False):
        s.split_guidance = split
        outs.append(s.decode(z, c, 3, unconditional_guidance_scale=3.0, unconditional_conditioning=uc).clone())
        torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and not torch.equal(outs[0], z)


def test_img2img_end_to_end_tiny():
    """image -> encode_first_stage -> get_first_stage_encoding -> stochastic_encode -> decode -> decode_first_stage on the tiny UNet
    and the tiny first stage: finite, of the right shape, repeatable, and equal to the same pieces composed by hand."""
    from autodiffusion_amd import ops
    from autodiffusion_amd.sd_sampler import axpby_noise, sd_step
    ld, s, c, uc = _tiny_pipeline()
    x = torch.tanh(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(14))).to(DEV)
    cand, t_enc = np.array([153, 424, 690, 926]), 2

    def run():
        gen = torch.Generator(device=DEV).manual_seed(15)
        post = ld.encode_first_stage(x)
        z0 = ld.get_first_stage_encoding(post, noise=torch.randn(post.mean.shape, generator=gen, device=DEV))
        s.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False, sampled_timestep=cand)
        z_enc = s.stochastic_encode(z0, torch.tensor([t_enc] * 2), noise=torch.randn(z0.shape, generator=gen, device=DEV))
        z = s.decode(z_enc, c, t_enc, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        return z0, z_enc, z, ld.decode_first_stage(z)
    z0, z_enc, z, img = run()
    assert z0.shape == (2, 4, 16, 16) and img.shape == (2, 3, 64, 64) and img.dtype == torch.float32
    assert all(bool(torch.isfinite(t).all()) for t in (z0, z_enc, z, img))
    for a, b in zip(run(), (z0, z_enc, z, img)):
        assert torch.equal(a, b)
    # by hand: the moments, the posterior's sample, the noising and the two DDIM updates of entries 1 and 0
    gen = torch.Generator(device=DEV).manual_seed(15)
    vae = ld.first_stage_model
    mom = vae.encode_moments(x)
    n1 = torch.randn(2, 4, 16, 16, generator=gen, device=DEV)
    n2 = torch.randn(2, 4, 16, 16, generator=gen, device=DEV)
    sf = ld.scale_factor
    h0 = axpby_noise(mom[:, :4].contiguous(), sf, ops.vec_act(mom[:, 4:].contiguous(), "gauss_std", dy=n1), sf)
    assert torch.equal(h0, z0)
    ac = ld.alphas_cumprod.cpu().numpy()
    a_t = ac[cand]
    a_prev = np.concatenate([ac[:1], ac[cand[:-1]]])
    henc = axpby_noise(z0, np.sqrt(a_t[t_enc]), n2, np.sqrt(np.float32(1) - a_t[t_enc]))
    assert torch.equal(henc, z_enc)
    h = henc
    for index in (1, 0):
        ts = torch.full((2,), int(cand[index]), device=DEV, dtype=torch.long)
        eps = torch.cat([ld.apply_model(h, ts, uc), ld.apply_model(h, ts, c)])
        h, _, _ = sd_step(h, eps, 2, 3.0, (1.0,), (), a_t[index], a_prev[index], 0.0, None, want_e=False)
    assert torch.equal(h, z) and torch.equal(ld.decode_first_stage(h), img)


def test_img2img_cli_synthetic_tiny(tmp_path):
    """scripts/sd_img2img.py as a child process: a uint8 .npy image in, the project's samples_{N}x{H}x{W}x3.npz out."""
    rs = np.random.RandomState(3)
    np.save(tmp_path / "init.npy", rs.randint(0, 256, size=(1, 64, 64, 3)).astype(np.uint8))
    np.save(tmp_path / "ids.npy", rs.randint(0, 500, size=(1, 8)).astype(np.int64))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "sd_img2img.py"), "--synthetic", "tiny", "--init-img", str(tmp_path / "init.npy"),
           "--prompt_ids", str(tmp_path / "ids.npy"), "--n_samples", "2", "--n_iter", "2", "--ddim_steps", "4", "--strength", "0.5",
           "--use_timestep", "[153, 424, 926, 690]", "--scale", "3.0", "--outdir", str(tmp_path / "out"), "--seed", "7"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "target t_enc is 2 steps" in res.stdout
    arr = np.load(tmp_path / "out" / "samples_4x64x64x3.npz")["arr_0"]
    assert arr.shape == (4, 64, 64, 3) and arr.dtype == np.uint8 and arr.std() > 0
    assert not np.array_equal(arr[:2], arr[2:])   # the second iteration draws new noise
