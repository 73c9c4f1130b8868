"""GPU parity of the Stable-Diffusion first stage on the HIP path: the 512-wide single-head attention kernel and the latent
entry / image exit kernels against PyTorch fp32, the decoder against golden vectors captured from the reference's own
``Decoder`` (tests/golden/capture_sd_vae.py), batch / chunk independence, and the SD candidate evaluator end to end.

Bounds: the kernel bound of test_hip_kernels.py (assert_close_bf16: max <= 1e-2 max|ref|, Frobenius <= 4e-3) for the attention;
the full-size SD UNet's bounds of test_hip_fullsize.py for the network (relative Frobenius <= 2e-2 in bf16, 5e-3 in fp16: the
decoder is a shorter chain of the same kernels, so these are caps).  Measured on MI355X: sd_vae_tiny
1.32e-2 / 1.66e-3, sd_vae_mid512 9.8e-3 / 1.12e-3, full_sd_vae 1.35e-2 / 1.71e-3 (bf16 / fp16); attention at T = 4096: Frobenius
2.3e-3 / 2.8e-4.
"""
import ast
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.fill import fill_array

from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FRO = {"bf16": 2e-2, "fp16": 5e-3}   # tests/test_hip_fullsize.py


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


# ------------------------------------------------------------------ attention, one head of 512 channels
def _attn_ref(qkv):
    """softmax(q k^T 512^-1/2) v in fp32 on the same 16-bit operands (model.py:186-198), one image at a time."""
    out = []
    for x in qkv.float():
        q, k, v = x.chunk(3, dim=-1)
        out.append(torch.softmax((q @ k.T) * (512 ** -0.5), dim=-1) @ v)
    return torch.stack(out)


def _attn_raw(qkv, guard=4096):
    """The entry point itself on a caller-owned buffer with a sentinel-filled guard region behind `out`."""
    from autodiffusion_amd import _lib
    n, t, _ = qkv.shape
    lib = _lib.load("f16" if qkv.dtype == torch.float16 else "bf16")
    buf = torch.full((n * t * 512 + guard,), -7.0, dtype=qkv.dtype, device=qkv.device)
    _lib.check(lib.adm_attention_1h512(qkv.data_ptr(), buf.data_ptr(), n, t, torch.cuda.current_stream().cuda_stream), "adm_attention_1h512")
    torch.cuda.synchronize()
    assert bool((buf[n * t * 512:] == -7.0).all()), "rows beyond T were written"
    return buf[:n * t * 512].view(n, t, 512)


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("n,t", [(1, 64), (2, 80), (3, 200), (1, 1), (1, 1024), (1, 4096)])
def test_attention_1h512(n, t, torso):
    from autodiffusion_amd import ops
    g = torch.Generator().manual_seed(n * 10000 + t)
    qkv = torch.randn(n, t, 1536, generator=g).to(DTYPES[torso]).to(DEV)
    ref = _attn_ref(qkv)
    got = ops.attention(qkv, 1, True)
    assert got.shape == (n, t, 512) and got.dtype == qkv.dtype
    assert torch.isfinite(got.float()).all()
    assert_close_bf16(got.float(), ref, f"attention_1h512 n={n} T={t} {torso}")
    raw = _attn_raw(qkv)
    assert torch.equal(raw, got)
    assert torch.equal(ops.attention(qkv, 1, False), got)   # one head: both channel orders are q | k | v


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
def test_attention_1h512_is_stable_for_large_logits(torso):
    from autodiffusion_amd import ops
    g = torch.Generator().manual_seed(8)
    qkv = (torch.randn(1, 128, 1536, generator=g) * 6.0).to(DTYPES[torso]).to(DEV)   # logits ~ +-100: needs the running-max rescale
    logits = (qkv.float()[0, :, :512] @ qkv.float()[0, :, 512:1024].T) * 512 ** -0.5
    assert logits.abs().max().item() > 80
    got = ops.attention(qkv, 1, True).float()
    assert torch.isfinite(got).all()
    assert_close_bf16(got, _attn_ref(qkv), f"attention_1h512 large logits {torso}")


def test_attention_1h512_does_not_depend_on_the_batch_and_has_no_lse():
    from autodiffusion_amd import ops
    from autodiffusion_amd._lib import AdmError
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(3, 200, 1536, generator=g).to(torch.bfloat16).to(DEV)
    got = ops.attention(qkv, 1, True)
    for i in range(3):
        assert torch.equal(ops.attention(qkv[i:i + 1].contiguous(), 1, True)[0], got[i]), i
    with pytest.raises(AdmError):
        ops.attention(qkv, 1, True, want_lse=True)


# ------------------------------------------------------------------ entry / exit kernels
@pytest.mark.parametrize("torso", ["bf16", "fp16"])
def test_latent_in(torso):
    """post_quant_conv(inv_scale * z) in fp32, rounded once to the 16-bit torso type: the stored value must be the rounding of
    a number within 1e-6 (relative to max|ref|) of fp32 torch's result; the pad channels are exactly zero."""
    from autodiffusion_amd import ops
    dt = DTYPES[torso]
    g = torch.Generator().manual_seed(4)
    n, e, zc, h, w = 3, 4, 4, 9, 9
    z = torch.randn(n, e, h, w, generator=g) * 4
    wt, b = torch.randn(zc, e, 1, 1, generator=g) * 0.5, torch.randn(zc, generator=g) * 0.1
    inv = float(np.float32(1.0 / 0.18215))
    ref = F.conv2d(z * inv, wt, b).permute(0, 2, 3, 1)
    got = ops.vae_latent_in(z.to(DEV), wt.to(DEV), b.to(DEV), inv, dt).cpu()
    assert got.shape == (n, h, w, 32) and got.dtype == dt
    assert bool((got[..., zc:] == 0).all())
    d = 1e-6 * ref.abs().max()
    lo, hi = (ref - d).to(dt).float(), (ref + d).to(dt).float()
    val = got[..., :zc].float()
    print(f"latent_in {torso}: max |got - ref| {float((val - ref).abs().max()):.3g}, {int((val != ref.to(dt).float()).sum())} of {val.numel()} off the direct rounding")
    assert bool(((val >= lo) & (val <= hi)).all())


@pytest.mark.parametrize("outputs", ["unit", "u8", "both"])
def test_image_out_is_bit_exact(outputs):
    from autodiffusion_amd import ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 3, 9, 11, generator=g) * 1.2
    flat = x.view(-1)
    flat[:12] = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -1e-45, 0.9999999, -0.9999999, 1.0000001, 0.003921569])
    unit_ref = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)
    u8_ref = (255.0 * unit_ref).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    unit, u8 = ops.vae_image_out(x.to(DEV), want_unit=outputs != "u8", want_u8=outputs != "unit")
    assert (unit is None) == (outputs == "u8") and (u8 is None) == (outputs == "unit")
    if unit is not None:
        assert unit.shape == x.shape and torch.equal(unit.cpu(), unit_ref)
    if u8 is not None:
        assert u8.shape == (3, 9, 11, 3) and u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), u8_ref)


# ------------------------------------------------------------------ the network
_VAES = {}


def _vae(name, torso):
    from autodiffusion_amd.sd_vae import AutoencoderKL
    key = (name, torso)
    if key not in _VAES:
        g = golden(name)
        cfg = ast.literal_eval(str(g["cfg"]))
        vae = AutoencoderKL(cfg, int(g["embed_dim"]))
        vae.load_state_dict({k: torch.from_numpy(fill_array("first_stage_model." + k, tuple(v.shape))) for k, v in vae.state_dict().items()})
        _VAES[key] = (vae.set_torso(torso).to(DEV), g)
    return _VAES[key]


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["sd_vae_tiny", "sd_vae_mid512", "full_sd_vae"])
def test_decode_matches_the_reference_decoder(name, torso):
    vae, g = _vae(name, torso)
    ref = torch.from_numpy(g["out"])
    got = vae.decode(torch.from_numpy(g["z"]).to(DEV)).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    fro = float((got - ref).norm() / ref.norm())
    print(f"{name} {torso}: rel fro {fro:.4g}, max |err| {float((got - ref).abs().max()):.4g} (max |ref| {float(ref.abs().max()):.4g})")
    assert fro <= FRO[torso], f"{name} {torso}: rel fro {fro:.4g}"
    if name == "full_sd_vae":
        _VAES.pop((name, torso))   # 49.5 M parameters twice over: not kept for the session


def test_decode_is_independent_of_batch_and_chunk():
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    vae, _ = _vae("sd_vae_tiny", "bf16")
    z = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(9)).to(DEV) * 0.18215
    both = vae.decode(z)
    for i in range(3):
        assert torch.equal(vae.decode(z[i:i + 1].contiguous())[0], both[i]), i
    ld = LatentDiffusion(types.SimpleNamespace(device=torch.device(DEV)), first_stage=vae)
    one, three = ld.decode_first_stage(z, chunk=1), ld.decode_first_stage(z, chunk=3)
    assert one.dtype == torch.float32 and one.shape == (3, 3, 32, 32) and torch.equal(one, three)
    assert torch.equal(ld.decode_first_stage(z), three) and torch.equal(ld.decode_first_stage(z, chunk=2), three)
    assert torch.equal(three, vae.decode(z, float(np.float32(1.0 / 0.18215))))


# ------------------------------------------------------------------ end to end: candidate -> FID on decoded images
def test_candidate_fid_end_to_end():
    from autodiffusion_amd.fid import calculate_frechet_distance
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator, batch_seed, candidate_seed
    from autodiffusion_amd.sd_sampler import DDIMSampler, LatentDiffusion
    from autodiffusion_amd.sd_unet import UNetModel
    from test_sd_oracle import sd_case
    g, plan, P = sd_case("sd_unet_tiny")
    cfg = ast.literal_eval(str(g["cfg"]))
    unet = UNetModel(image_size=32, use_spatial_transformer=True, **cfg)
    unet.load_state_dict(P)
    unet.to(DEV)
    vae, _ = _vae("sd_vae_tiny", "bf16")
    ld = LatentDiffusion(unet, device=DEV, first_stage=vae)
    sampler = DDIMSampler(ld)
    gen = torch.Generator().manual_seed(21)
    cond = [(torch.randn(2, 7, 96, generator=gen).to(DEV), torch.randn(2, 7, 96, generator=gen).to(DEV)) for _ in range(4)]
    W = torch.randn(3 * 4 * 4, 24, generator=gen).to(DEV)

    def stub(images):   # a linear extractor of 24 features
        return F.adaptive_avg_pool2d(images, 4).reshape(images.shape[0], -1) @ W
    rs = np.random.RandomState(2)
    a = rs.randn(64, 24)
    ref_mu, ref_sigma = a.mean(0), np.cov(a, rowvar=False)
    opt = types.SimpleNamespace(n_samples=2, C=4, H=128, W=128, f=8, scale=7.5, ddim_eta=0.0, time_step=2, fixed_code=False)
    ev = SDCandidateEvaluator(ld, sampler, cond, ref_mu, ref_sigma, 3, features=stub, dims=24, seed=5, device=DEV)
    cand = [300, 800]
    fid = ev.get_cand_fid(cand, opt)
    assert ev.last_times["images"] == 4 and ev.last_times["batches"] == 2   # 2, then 4 > 3

    # the same value from the public pieces, composed by hand
    imgs = []
    seed0 = candidate_seed(5, cand)
    for itr in range(2):
        c, uc = cond[itr]
        x_T = torch.randn([2, 4, 16, 16], generator=torch.Generator().manual_seed(batch_seed(seed0, itr))).to(DEV)
        z, _ = sampler.sample(S=2, conditioning=c, batch_size=2, shape=[4, 16, 16], verbose=False, unconditional_guidance_scale=7.5,
                              unconditional_conditioning=uc, eta=0.0, x_T=x_T, sampled_timestep=np.array(cand))
        x = ld.decode_first_stage(z)
        assert x.shape == (2, 3, 64, 64)
        imgs.append(torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0))
    acts = stub(torch.cat(imgs)).double().cpu().numpy()
    want = calculate_frechet_distance(np.mean(acts, axis=0), np.cov(acts, rowvar=False), ref_mu, ref_sigma)
    print(f"candidate FID {fid!r} vs hand-composed {want!r}: rel {abs(fid - want) / abs(want):.3g}")
    assert np.isfinite(fid) and abs(fid - want) <= 1e-9 * abs(want)
    assert ev.get_cand_fid(cand, opt) == fid
    assert ev.get_cand_fid([300, 801], opt) != fid
