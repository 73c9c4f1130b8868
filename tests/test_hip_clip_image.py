"""GPU parity of the CLIP image tower and the CLIP score on the HIP path.

The bicubic mode of adm_resize_bilinear (half_pixel == 2), per element, against the float64 restatement of
tests/clip_image_replay.py within its derived bound (one 16-bit rounding plus the fp32 evaluation of 16 taps), on all three input
kinds, into a caller-owned buffer followed by a sentinel guard.  ``image_embeds`` against golden vectors captured from
transformers' own ``CLIPVisionModelWithProjection`` behind the reference embedder's preprocessing
(tests/golden/capture_clip_image.py; weights regenerated here from oracle/fill.py) under the full-network caps of
test_hip_clip.py (relative Frobenius <= 2e-2 in bf16, 5e-3 in fp16).  torch's own 16-bit run of the same filled models on a CPU
gives 7.96e-3 / 1.05e-3 (tiny), 5.86e-3 / 8.56e-4 (p16), 7.41e-3 / 9.59e-4 (l14w), bf16 / fp16; what this path measures on MI355X
is printed by every run and recorded in DESIGN.md section 8.5.  The caps are not tightened to either.

Then the properties: an image's embedding does not depend on its batch, nor on what the dead rows hold; both key layouts give the
same bits; the pair's cosines within the first-order bound 2 (eps_img + eps_txt) of renormalised vectors; the score is its
definition; and the candidate evaluator with a scorer returns the FID it returns without one.
"""
import ast
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_image_replay as cr
from oracle.fill import fill_array

from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FRO = {"bf16": 2e-2, "fp16": 5e-3}   # tests/test_hip_clip.py
SENTINEL = -7.0
TEXT_PREFIX = "cond_stage_model.transformer."


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ the bicubic mode
def _raw_resize(images, kind, mode, scale, shift, oh, ow, dtype, guard=4096):
    """The entry point itself on a caller-owned, sentinel-filled output cut off right after the last pixel and followed by a guard."""
    from autodiffusion_amd import _lib
    n = images.shape[0]
    h, w = (images.shape[2], images.shape[3]) if kind == 1 else (images.shape[1], images.shape[2])
    held = n * oh * ow * 8
    buf = torch.full((held + guard,), SENTINEL, dtype=dtype, device=images.device)
    lib = _lib.load("f16" if dtype == torch.float16 else "bf16")
    rc = lib.adm_resize_bilinear(images.data_ptr(), buf.data_ptr(), n, h, w, oh, ow, 8, kind, mode, scale, shift,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf[:held].view(n, oh, ow, 8), buf[held:]


def _images(kind, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 0:
        return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(DEV)
    return (torch.rand((n, 3, h, w) if kind == 1 else (n, h, w, 3), generator=g) * 2 - 1).to(DEV)


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["u8_nhwc", "f32_nchw", "f32_nhwc"])
@pytest.mark.parametrize("h,w,oh,ow", [(1, 1, 8, 8), (2, 3, 56, 56), (40, 72, 56, 56), (64, 64, 64, 64), (512, 512, 224, 224)])
def test_bicubic_mode_matches_float64(h, w, oh, ow, kind, torso):
    from autodiffusion_amd import ops
    dt = DTYPES[torso]
    images = _images(kind, 2, h, w, 7 + h * 1000 + w + kind)
    scale, shift = (1 / 255.0, 0.0) if kind == 0 else (0.5, 0.5)
    rc, got, guard = _raw_resize(images, kind, 2, scale, shift, oh, ow, dt)
    assert rc == 0
    assert bool((guard == SENTINEL).all()), "something beyond the last output pixel was written"
    assert bool((got[..., 3:] == 0).all()) and torch.isfinite(got).all()
    ref, bound = cr.bicubic_restate(images, kind, scale, shift, oh, ow, dt)
    worst = float(((got[..., :3].double() - ref).abs() / bound).max())
    print(f"bicubic {h}x{w}->{oh}x{ow} kind {kind} {torso}: worst err / bound {worst:.3f}, max |err| {float((got[..., :3].double() - ref).abs().max()):.3g}")
    assert worst <= 1.0
    via_ops = ops.resize_bilinear(images, oh, ow, 8, {0: "u8_nhwc", 1: "f32_nchw", 2: "f32_nhwc"}[kind], 2, scale, shift, dt)
    assert torch.equal(via_ops, got)
    if (h, w) == (oh, ow):   # the identity returns the pixels' rounding
        _, same, _ = _raw_resize(images, kind, 2, 1.0, 0.0, oh, ow, dt)
        px = images.permute(0, 2, 3, 1) if kind == 1 else images
        assert torch.equal(same[..., :3], px.to(dt))


def test_resize_refuses_other_modes_and_keeps_the_bilinear_ones():
    from autodiffusion_amd import ops
    from autodiffusion_amd._lib import AdmError
    images = _images(1, 1, 8, 8, 1)
    for mode in (3, -1):
        rc, got, _ = _raw_resize(images, 1, mode, 1.0, 0.0, 8, 8, torch.bfloat16)
        assert rc != 0 and bool((got == SENTINEL).all())
        with pytest.raises(AdmError):
            ops.resize_bilinear(images, 8, 8, 8, "f32_nchw", mode, 1.0, 0.0, torch.bfloat16)
    # bilinear, align_corners=False, still is what True selects; upsampling 8 -> 16 it differs from the bicubic mode
    a = ops.resize_bilinear(images, 16, 16, 8, "f32_nchw", True, 1.0, 0.0, torch.float16)
    want = F.interpolate(images, (16, 16), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert float((a[..., :3].float() - want).abs().max()) <= 2e-3
    assert not torch.equal(a, ops.resize_bilinear(images, 16, 16, 8, "f32_nchw", 2, 1.0, 0.0, torch.float16))


# ------------------------------------------------------------------ the network
_NETS, _FILLS = {}, {}


def _filled(cfg):
    """The image tower's state dict filled under its own key names (once per config, shared by the torsos, never modified)."""
    from autodiffusion_amd.sd_clip import CLIPVisionPlan
    if repr(cfg) not in _FILLS:
        _FILLS[repr(cfg)] = {k: torch.from_numpy(fill_array(k, shape)) for k, shape in CLIPVisionPlan(**cfg).param_shapes().items()}
    return _FILLS[repr(cfg)]


def _net(name, torso, openai=False):
    from autodiffusion_amd.sd_clip import FrozenClipImageEmbedder
    g = golden(name)
    cfg = ast.literal_eval(str(g["cfg"]))
    key = (repr(cfg), torso, openai)
    if key not in _NETS:
        emb = FrozenClipImageEmbedder(cfg, device="cpu")
        if openai:
            from test_clip_image_host import to_openai
            emb.load_state_dict(to_openai(_filled(cfg)))
        else:
            emb.load_state_dict(_filled(cfg))
        _NETS[key] = emb.set_torso(torso).to(DEV)
    return _NETS[key], g


def _inputs(g):
    """The [-1, 1] fp32 NCHW images the capture script fed the reference preprocessing (the same expression on the same uint8)."""
    return (torch.from_numpy(g["images"]).permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0).to(DEV)


def _text(torso):
    from autodiffusion_amd.sd_clip import CLIPTextPlan, FrozenCLIPTextEmbedder
    g = golden("clip_pair_tiny")
    cfg = ast.literal_eval(str(g["cfg"]))
    key = ("text", torso)
    if key not in _NETS:
        emb = FrozenCLIPTextEmbedder(device="cpu", config=cfg, normalize=False)
        emb.load_state_dict({"transformer." + k: torch.from_numpy(fill_array((TEXT_PREFIX if k.startswith("text_model.") else "") + k, s))
                             for k, s in CLIPTextPlan(**cfg).param_shapes().items()})
        _NETS[key] = emb.set_torso(torso).to(DEV)
    return _NETS[key], g


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["clip_image_tiny", "clip_image_p16", "clip_image_l14w"])
def test_image_embeds_match_clip_vision_model(name, torso):
    emb, g = _net(name, torso)
    ref = torch.from_numpy(g["out"])
    got = emb(_inputs(g)).cpu()
    assert got.shape == ref.shape == (g["images"].shape[0], emb.model.plan.projection_dim)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    fro = float((got - ref).norm() / ref.norm())
    print(f"{name} {torso}: rel fro {fro:.4g}, max |err| {float((got - ref).abs().max()):.4g} (max |ref| {float(ref.abs().max()):.4g})")
    assert fro <= FRO[torso], f"{name} {torso}: rel fro {fro:.4g}"


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["clip_image_tiny", "clip_image_l14w"])
def test_embedding_is_independent_of_the_batch_and_of_the_dead_rows(name, torso):
    emb, g = _net(name, torso)
    x = _inputs(g)
    out = emb(x)
    for i in range(x.shape[0]):
        assert torch.equal(emb(x[i:i + 1])[0], out[i]), i
    assert torch.equal(emb(torch.cat([x[1:], x[:1]]))[-1], out[0])
    # NaN planted in every dead row of the token rows: never a key, never the class row
    model = emb.model
    rows = model.tokens(model.preprocess(x))
    t, pitch = model.plan.tokens, model.plan.pitch
    assert rows.shape == (x.shape[0], pitch, model.plan.hidden_size) and pitch > t and torch.isfinite(rows).all()
    assert torch.equal(model.encode_tokens(rows), out)
    dirty = rows.clone()
    dirty[:, t:] = float("nan")
    assert torch.equal(model.encode_tokens(dirty), out)
    # uint8 images enter through the same kernel: x / 255 instead of (x + 1) / 2 on the same pixels
    u8 = emb(torch.from_numpy(g["images"]).to(DEV), unit=True)
    assert float((u8 - out).norm() / out.norm()) <= FRO[torso]


def test_both_key_layouts_give_the_same_bits():
    a, g = _net("clip_image_tiny", "bf16")
    b, _ = _net("clip_image_tiny", "bf16", openai=True)
    x = _inputs(g)
    assert a is not b and torch.equal(a(x), b(x))


@pytest.mark.parametrize("torso", ["bf16", "fp16"])
def test_pair_cosines_and_score(torso):
    from autodiffusion_amd.sd_clip import CLIPScorer
    image, gi = _net("clip_image_tiny", torso)
    text, gp = _text(torso)
    ids = torch.from_numpy(gp["ids"]).to(DEV)
    ref_img, ref_txt, ref_cos = torch.from_numpy(gi["out"]).double(), torch.from_numpy(gp["text_embeds"]).double(), torch.from_numpy(gp["cosines"])
    txt = text(ids).cpu().double()
    assert txt.shape == ref_txt.shape
    fro = float((txt - ref_txt).norm() / ref_txt.norm())
    print(f"clip_pair_tiny {torso}: text_embeds rel fro {fro:.4g}")
    assert fro <= FRO[torso]
    unit = (_inputs(gi) + 1.0) / 2.0   # the scorer takes the [0, 1] images the evaluator stages
    img = image(unit, unit=True).cpu().double()
    e_img = (img - ref_img).norm(dim=-1) / ref_img.norm(dim=-1)
    e_txt = (txt - ref_txt).norm(dim=-1) / ref_txt.norm(dim=-1)
    scorer = CLIPScorer(image, text)
    cos = scorer.cosine(unit, ids)
    assert cos.shape == (3,) and cos.dtype == torch.float32
    err = (cos.double() - ref_cos).abs()
    print(f"clip_pair_tiny {torso}: cosines {cos.tolist()} ref {ref_cos.tolist()}; |err| {err.tolist()} "
          f"bound {(2 * (e_img + e_txt)).tolist()} (eps_img {e_img.tolist()}, eps_txt {e_txt.tolist()})")
    assert bool((err <= 2 * (e_img + e_txt)).all())
    assert scorer.score(unit, ids) == float(100.0 * cos.double().clamp_min(0).mean())
    # the normalised embedder and encode's repeat
    text.normalize, text.n_repeat = True, 2
    try:
        z = text.encode(ids)
        assert z.shape == (3, 2, 64) and torch.equal(z[:, 0], z[:, 1])
        assert float((z[:, 0].double().norm(dim=-1) - 1).abs().max()) <= 1e-6
        assert float((z[:, 0].cpu().double() - txt / txt.norm(dim=-1, keepdim=True)).abs().max()) <= 1e-6
    finally:
        text.normalize, text.n_repeat = False, 1


# ------------------------------------------------------------------ end to end: prompts -> candidate FID and CLIP score
def test_candidate_fid_is_unchanged_by_the_scorer():
    from autodiffusion_amd.sd_arch import sd_unet_plan
    from autodiffusion_amd.sd_clip import CLIPScorer, FrozenCLIPEmbedder
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    from autodiffusion_amd.sd_sampler import DDIMSampler, LatentDiffusion
    from autodiffusion_amd.sd_unet import UNetModel
    from oracle.fill import fill_state_dict
    from test_hip_clip import _IdTokenizer, _net as _text_net
    from test_hip_sd_vae import _vae
    cfg = dict(ast.literal_eval(str(golden("sd_unet_tiny")["cfg"])), context_dim=128)
    unet = UNetModel(image_size=32, use_spatial_transformer=True, **cfg)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state_dict(sd_unet_plan(**cfg).param_shapes()).items()})
    unet.to(DEV)
    vae, _ = _vae("sd_vae_tiny", "bf16")
    tiny, g = _text_net("clip_text_tiny", "bf16")
    clip = FrozenCLIPEmbedder(device="cpu", max_length=77, tokenizer=_IdTokenizer(), config=ast.literal_eval(str(g["cfg"])))
    clip.load_state_dict(tiny.state_dict())
    clip.to(DEV)
    ld = LatentDiffusion(unet, device=DEV, first_stage=vae, cond_stage=clip)
    sampler = DDIMSampler(ld)
    gen = torch.Generator().manual_seed(21)
    prompts = [torch.randint(0, 512, (2, 77), generator=gen).to(DEV) for _ in range(4)]
    W = torch.randn(3 * 4 * 4, 24, generator=gen).to(DEV)

    def stub(images):   # a linear extractor of 24 features
        return F.adaptive_avg_pool2d(images, 4).reshape(images.shape[0], -1) @ W
    a = np.random.RandomState(2).randn(64, 24)
    opt = types.SimpleNamespace(n_samples=2, C=4, H=128, W=128, f=8, scale=7.5, ddim_eta=0.0, time_step=2, fixed_code=False)
    kw = dict(ref_mu=a.mean(0), ref_sigma=np.cov(a, rowvar=False), num_samples=3, features=stub, dims=24, seed=5, device=DEV)
    scorer = CLIPScorer(_net("clip_image_tiny", "bf16")[0], _text("bf16")[0])
    cand = [300, 800]
    fid = SDCandidateEvaluator(ld, sampler, prompts=prompts, **kw).get_cand_fid(cand, opt)
    ev = SDCandidateEvaluator(ld, sampler, prompts=prompts, clip_scorer=scorer, **kw)
    assert ev.get_cand_fid(cand, opt) == fid and np.isfinite(fid)
    first = ev.last_clip
    assert first["cosines"].shape == (4,) and ev.last_times["images"] == 4 and torch.isfinite(first["cosines"]).all()
    assert first["score"] == CLIPScorer.score_of(first["cosines"])
    assert ev.get_cand_fid(cand, opt) == fid
    assert torch.equal(ev.last_clip["cosines"], first["cosines"]) and ev.last_clip["score"] == first["score"]
    # other prompts for the same noise: other images, other cosines, another score
    other = SDCandidateEvaluator(ld, sampler, prompts=prompts[::-1], clip_scorer=scorer, **kw)
    other.get_cand_fid(cand, opt)
    print(f"CLIP score {first['score']!r} cosines {first['cosines'].tolist()}; prompts permuted: {other.last_clip['score']!r} "
          f"{other.last_clip['cosines'].tolist()}")
    assert not torch.equal(other.last_clip["cosines"], first["cosines"]) and other.last_clip["score"] != first["score"]
    with pytest.raises(ValueError, match="prompts="):
        SDCandidateEvaluator(ld, sampler, [(None, None)], clip_scorer=scorer, **kw)
