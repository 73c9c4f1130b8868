"""Host checks (no GPU) of the CLIP image tower's plumbing: the parameter names against transformers' own ViT-L/14 key list, the
OpenAI-layout remap, the mean / std fold and the im2col rows against F.conv2d(normalize(x)) in float64, the float64 restatement of
the bicubic resize mode (tests/clip_image_replay.py) against torch's CPU F.interpolate with the named defects outside its bound,
every refusal, the scorer's definition and the evaluator's scorer plumbing on a stub."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_image_replay as cr
from autodiffusion_amd import sd_clip
from autodiffusion_amd._lib import AdmError
from autodiffusion_amd.sd_clip import (CLIP_MEAN, CLIP_STD, CLIP_VIT_L14_VISION, CLIPScorer, CLIPTextTransformer, CLIPVisionPlan,
                                       CLIPVisionTransformer, FrozenClipImageEmbedder, FrozenCLIPTextEmbedder)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
            projection_dim=64)
TEXT_TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77)


# ------------------------------------------------------------------ names and layouts
def test_param_shapes_are_the_vit_l14_state_dict():
    with open(os.path.join(GOLDEN, "clip_image_keys.json")) as f:
        keys = json.load(f)
    shapes = CLIPVisionPlan(**CLIP_VIT_L14_VISION).param_shapes()
    assert list(shapes) == list(keys)
    assert {k: list(v) for k, v in shapes.items()} == keys
    plan = CLIPVisionPlan(**CLIP_VIT_L14_VISION)
    assert (plan.tokens, plan.pitch, plan.patch_k) == (257, 320, 608)
    assert (CLIPVisionPlan(**TINY).tokens, CLIPVisionPlan(**TINY).pitch) == (17, 64)


def to_openai(sd, tower="visual."):
    """The inverse of the loader's mapping, written out independently: CLIPModel names -> the OpenAI ``clip`` package's."""
    out = {}
    hf = "vision_model." if tower == "visual." else "text_model."
    layers = sorted({int(k.split(".")[3]) for k in sd if k.startswith(hf + "encoder.layers.")})
    for l in layers:
        p, q = f"{hf}encoder.layers.{l}.", f"{tower}transformer.resblocks.{l}."
        for leaf in ("weight", "bias"):
            out[f"{q}attn.in_proj_{leaf}"] = torch.cat([sd[f"{p}self_attn.{n}_proj.{leaf}"] for n in "qkv"], 0)
            for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"),
                         ("mlp.fc1", "mlp.c_fc"), ("mlp.fc2", "mlp.c_proj")):
                out[f"{q}{b}.{leaf}"] = sd[f"{p}{a}.{leaf}"]
    if tower == "visual.":
        out["visual.conv1.weight"] = sd["vision_model.embeddings.patch_embedding.weight"]
        out["visual.class_embedding"] = sd["vision_model.embeddings.class_embedding"]
        out["visual.positional_embedding"] = sd["vision_model.embeddings.position_embedding.weight"]
        for a, b in (("pre_layrnorm", "ln_pre"), ("post_layernorm", "ln_post")):
            for leaf in ("weight", "bias"):
                out[f"visual.{b}.{leaf}"] = sd[f"vision_model.{a}.{leaf}"]
        out["visual.proj"] = sd["visual_projection.weight"].t().contiguous()
    else:
        out["token_embedding.weight"] = sd["text_model.embeddings.token_embedding.weight"]
        out["positional_embedding"] = sd["text_model.embeddings.position_embedding.weight"]
        out["ln_final.weight"], out["ln_final.bias"] = sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"]
        out["text_projection"] = sd["text_projection.weight"].t().contiguous()
    return out


def test_openai_and_hf_layouts_load_to_equal_state():
    a = CLIPVisionTransformer(**TINY).randomize_(3)
    sd = a.state_dict()
    oa = to_openai(sd)
    assert not any(k.startswith("vision_model.") for k in oa) and len(oa) == 1 + 2 + 4 + 1 + 2 * 12
    b = CLIPVisionTransformer(**TINY)
    b.load_state_dict(dict(oa, logit_scale=torch.zeros(()), **{"token_embedding.weight": torch.zeros(2, 2)}))   # a joint file
    c = CLIPVisionTransformer(**TINY)
    c.load_state_dict(sd)
    assert list(b.state_dict()) == list(c.state_dict()) == list(sd)
    assert all(torch.equal(b.state_dict()[k], v) and torch.equal(c.state_dict()[k], v) for k, v in sd.items())
    # the text tower with its projection, the same way
    t = CLIPTextTransformer(**TEXT_TINY, projection_dim=64).randomize_(4)
    u = CLIPTextTransformer(**TEXT_TINY, projection_dim=64)
    u.load_state_dict(to_openai(t.state_dict(), tower=""))
    assert all(torch.equal(u.state_dict()[k], v) for k, v in t.state_dict().items())
    # one checkpoint, both towers, either layout
    joint = dict(sd, **t.state_dict())
    for ckpt in (joint, dict(oa, **to_openai(t.state_dict(), tower=""))):
        vis, txt = sd_clip.split_clip_state_dict(ckpt)
        assert set(vis) == set(sd) and set(txt) == set(t.state_dict())
        assert all(torch.equal(vis[k], v) for k, v in sd.items()) and all(torch.equal(txt[k], v) for k, v in t.state_dict().items())


def test_load_refuses_missing_misshaped_and_unknown_tensors():
    m = CLIPVisionTransformer(**TINY)
    sd = m.state_dict()
    with pytest.raises(RuntimeError, match="missing keys"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "visual_projection.weight"})
    with pytest.raises(RuntimeError, match="unexpected keys"):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))
    m.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=False)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(dict(sd, **{"visual_projection.weight": torch.zeros(64, 64)}))
    # an SD checkpoint's text tower (no text_projection) loads into the plain tower as before, and not into the projected one
    plain = CLIPTextTransformer(**TEXT_TINY)
    assert "text_projection.weight" not in plain.state_dict()
    plain.load_state_dict(plain.state_dict())
    with pytest.raises(RuntimeError, match="missing keys"):
        CLIPTextTransformer(**TEXT_TINY, projection_dim=64).load_state_dict(plain.state_dict())


# ------------------------------------------------------------------ the fold and the rows
@pytest.mark.parametrize("size,patch", [(56, 14), (64, 16)])
def test_fold_and_im2col_reproduce_the_normalised_patch_conv(size, patch):
    g = torch.Generator().manual_seed(size)
    c, grid = 32, size // patch
    t = 1 + grid * grid
    pitch, kpad = (t + 63) // 64 * 64, (3 * patch * patch + 31) // 32 * 32
    w = torch.randn(c, 3, patch, patch, generator=g, dtype=torch.float64) * 0.05
    cls, pos = torch.randn(c, generator=g, dtype=torch.float64), torch.randn(t, c, generator=g, dtype=torch.float64)
    x = torch.rand(2, 3, size, size, generator=g, dtype=torch.float64)
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    emb = F.conv2d((x - mean) / std, w, stride=patch).flatten(2).transpose(1, 2)
    ref = torch.cat([cls.expand(2, 1, c), emb], 1) + pos
    w2, pos2 = sd_clip.fold_patch_embedding(w, cls, pos, pitch, kpad)
    px = torch.zeros(2, size, size, 8, dtype=torch.float64)
    px[..., :3] = x.permute(0, 2, 3, 1)
    px[..., 3:] = 99.0   # the padding channels are not read
    rows = sd_clip.im2col_rows(px, patch, pitch, kpad)
    assert rows.shape == (2, pitch, kpad) and w2.shape == (c, kpad) and pos2.shape == (pitch, c)
    got = rows @ w2.t() + pos2
    assert float((got[:, :t] - ref).abs().max()) <= 1e-12
    assert bool((got[:, t:] == 0).all()) and bool((rows[:, 0] == 0).all()) and bool((rows[:, :, 3 * patch * patch:] == 0).all())


# ------------------------------------------------------------------ the bicubic restatement
SHAPES = [(1, 1, 8, 8), (2, 3, 56, 56), (40, 72, 56, 56), (64, 64, 64, 64), (128, 128, 224, 224)]


def _images(kind, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 0:
        return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    return torch.rand((n, 3, h, w) if kind == 1 else (n, h, w, 3), generator=g) * 2 - 1


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("h,w,oh,ow", SHAPES)
def test_bicubic_restatement_is_torchs_interpolate(h, w, oh, ow, kind):
    images = _images(kind, 2, h, w, h * 1000 + w)
    scale, shift = (1 / 255.0, 0.0) if kind == 0 else (0.5, 0.5)
    ref, bound = cr.bicubic_restate(images, kind, scale, shift, oh, ow, torch.bfloat16)
    nchw = images.permute(0, 3, 1, 2).float() if kind != 1 else images
    want = F.interpolate(nchw, (oh, ow), mode="bicubic", align_corners=True).permute(0, 2, 3, 1).double() * np.float32(scale) + np.float32(shift)
    err = float((ref - want).abs().max())
    print(f"bicubic restatement {h}x{w}->{oh}x{ow} kind {kind}: max |restatement - F.interpolate| {err:.3g}")
    assert ref.shape == (2, oh, ow, 3) and err <= 1e-5
    assert bool((bound > 0).all())
    if (h, w) == (oh, ow):   # the identity: exactly the pixels
        assert torch.equal(ref, (nchw.permute(0, 2, 3, 1).double() * np.float32(scale) + np.float32(shift)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("defect", [dict(a=-0.5), dict(align_corners=False), dict(clamp=False)])
def test_named_defects_lie_outside_the_bound(defect, dtype):
    images = _images(1, 1, 40, 72, 5)
    ref, bound = cr.bicubic_restate(images, 1, 0.5, 0.5, 56, 56, dtype)
    bad, _ = cr.bicubic_restate(images, 1, 0.5, 0.5, 56, 56, dtype, **defect)
    worst = float(((bad - ref).abs() / bound).max())
    print(f"defect {defect} {dtype}: worst |defect - ref| / bound {worst:.3g}")
    assert worst > 4.0
    # and rounding the restatement itself stays inside it
    assert float(((ref.to(dtype).double() - ref).abs() / bound).max()) <= 1.0


# ------------------------------------------------------------------ refusals
def test_constructors_refuse_what_is_not_built():
    with pytest.raises(NotImplementedError, match="64-wide"):
        CLIPVisionTransformer(**dict(TINY, num_attention_heads=4))
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        CLIPVisionTransformer(**dict(TINY, intermediate_size=500))
    with pytest.raises(NotImplementedError, match="64-wide"):
        CLIPVisionTransformer(**dict(TINY, hidden_size=96, num_attention_heads=1))   # a multiple of 32, but one head of 96
    with pytest.raises(NotImplementedError, match="multiple of patch_size"):
        CLIPVisionTransformer(**dict(TINY, image_size=60))
    with pytest.raises(NotImplementedError, match="antialias"):
        FrozenClipImageEmbedder(TINY, device="cpu", antialias=True)
    with pytest.raises(NotImplementedError, match="ViT-L/14"):
        FrozenClipImageEmbedder("ViT-B/32", device="cpu")
    with pytest.raises(ValueError, match="projection_dim"):
        FrozenCLIPTextEmbedder(device="cpu", config=TEXT_TINY)
    emb = FrozenCLIPTextEmbedder(device="cpu", config=dict(TEXT_TINY, projection_dim=64), n_repeat=3)
    assert emb.n_repeat == 3 and emb.normalize and emb.transformer.plan.projection_dim == 64
    with pytest.raises(AdmError, match="projection_dim"):
        CLIPTextTransformer(**TEXT_TINY).pooled(torch.zeros(1, 77, dtype=torch.int64))
    with pytest.raises(AdmError):   # parameters on the CPU: no fallback
        FrozenClipImageEmbedder(TINY, device="cpu").model.tokens(torch.zeros(1, 56, 56, 8, dtype=torch.bfloat16))
    full = FrozenClipImageEmbedder("ViT-L/14", device="cpu")
    assert full.model.plan == CLIPVisionPlan(**CLIP_VIT_L14_VISION)


def test_score_is_its_definition():
    cos = torch.tensor([0.25, -0.5, 0.125, 0.0])
    assert CLIPScorer.score_of(cos) == 100.0 * (0.25 + 0.125) / 4


# ------------------------------------------------------------------ SDCandidateEvaluator(clip_scorer=)
class _StubScorer:
    """cosine = mean pixel of the image plus the prompt's first id / 1000: depends on both, and on nothing else."""

    def __init__(self):
        self.calls = []

    def cosine(self, images, prompts):
        assert images.dtype == torch.float32 and images.dim() == 4 and float(images.min()) >= 0.0 and float(images.max()) <= 1.0
        self.calls.append((images.clone(), prompts))
        return images.mean(dim=(1, 2, 3)) - 0.5 + prompts[:, 0].float() / 1000.0

    score_of = staticmethod(CLIPScorer.score_of)


def test_evaluator_scores_every_batch_against_its_prompts_and_leaves_the_fid_alone(capsys):
    from test_sd_vae_host import _HostStats, _StubSampler, _opt
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    model = types.SimpleNamespace(device=torch.device("cpu"), get_learned_conditioning=lambda c: torch.zeros(len(c), 2, 4),
                                  decode_first_stage=lambda z: torch.tanh(z[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3)))
    prompts = [torch.full((2, 5), i, dtype=torch.int64) + torch.arange(2).view(2, 1) * 10 for i in range(4)]
    a = np.random.RandomState(1).randn(40, 12)
    W = torch.from_numpy(np.random.RandomState(0).randn(3 * 8 * 8, 12)).float()
    seen = []

    def feats(im):
        seen.append(im.clone())
        return im.reshape(im.shape[0], -1) @ W
    kw = dict(ref_mu=a.mean(0), ref_sigma=np.cov(a, rowvar=False), num_samples=4, features=feats, device="cpu", accumulator=_HostStats,
              image_out=lambda x, out: out.copy_(torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)))
    plain = SDCandidateEvaluator(model, _StubSampler(), prompts=prompts, **kw)
    fid = plain.get_cand_fid([100, 500, 900], _opt(2))
    assert plain.last_clip is None
    seen.clear()
    scorer = _StubScorer()
    ev = SDCandidateEvaluator(model, _StubSampler(), prompts=prompts, clip_scorer=scorer, **kw)
    assert ev.get_cand_fid([100, 500, 900], _opt(2)) == fid
    out = capsys.readouterr().out
    assert "CLIP score: " in out
    # three batches of two (2, 4, then 6 > 4), each with its own prompts; the images are the extractor's
    assert [p[:, 0].tolist() for _, p in scorer.calls] == [[0, 10], [1, 11], [2, 12]]
    assert torch.equal(torch.cat([im for im, _ in scorer.calls]), torch.cat(seen))
    clip = ev.last_clip
    assert set(clip) == {"score", "cosines", "clip_time"} and clip["cosines"].shape == (6,) and clip["clip_time"] >= 0.0
    assert torch.equal(clip["cosines"], torch.cat([scorer.cosine(im, p) for im, p in list(scorer.calls)]))
    assert clip["score"] == CLIPScorer.score_of(clip["cosines"])
    with pytest.raises(ValueError, match="prompts="):
        SDCandidateEvaluator(model, _StubSampler(), [(None, None)], clip_scorer=scorer, **kw)
