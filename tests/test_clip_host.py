"""Host-side checks of the Stable-Diffusion cond stage (no GPU): the CLIP text transformer's parameter table against the
state-dict names and shapes of transformers' ViT-L/14 ``CLIPTextModel`` (tests/golden/clip_text_keys.json, written by
capture_clip_text.py), state-dict loading, ``FrozenCLIPEmbedder``'s tokenizer plumbing on a stub, the routing of
``cond_stage_model.*`` by ``LatentDiffusion.load_state_dict``, the ``prompts=`` argument of ``SDCandidateEvaluator`` and the C ABI
declarations of the new entry points.
"""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from autodiffusion_amd import _lib
from autodiffusion_amd._lib import AdmError
from autodiffusion_amd.sd_clip import CLIP_VIT_L14_TEXT, CLIPTextTransformer, FrozenCLIPEmbedder, map_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77)
NEW_ENTRY_POINTS = ("adm_clip_embed", "adm_attention_causal", "adm_quick_gelu", "adm_layernorm_f32out")


def _keys():
    with open(os.path.join(HERE, "golden", "clip_text_keys.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


# ------------------------------------------------------------------ parameter table / state dict
def test_vitl14_parameter_table_matches_the_checkpoint_layout():
    keys = _keys()
    net = CLIPTextTransformer(**CLIP_VIT_L14_TEXT)
    mine = {"transformer." + k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert mine == keys
    assert list(mine) == list(keys)   # CLIPTextModel's own order
    assert sum(int(np.prod(s)) for s in mine.values()) == 123_060_480
    assert net.plan.flops(77) == pytest.approx(13.19e9, rel=1e-2)   # "about 13 GFLOP per prompt"


def test_constructor_refuses_what_the_kernels_do_not_take():
    with pytest.raises(NotImplementedError):
        CLIPTextTransformer(**dict(TINY, num_attention_heads=4))       # 32-wide heads
    with pytest.raises(NotImplementedError):
        CLIPTextTransformer(**dict(TINY, max_position_embeddings=300))
    with pytest.raises(ValueError):
        FrozenCLIPEmbedder(device="cpu", config=TINY, max_length=78)   # beyond the position table
    assert [map_rows(t) for t in (1, 20, 64, 65, 77, 128, 129, 256)] == [64, 64, 64, 128, 128, 128, 256, 256]
    with pytest.raises(NotImplementedError):
        map_rows(257)


def _tiny_sd(prefix="text_model."):
    net = CLIPTextTransformer(**TINY)
    g = torch.Generator().manual_seed(1)
    return {prefix + k[len("text_model."):]: torch.randn(v.shape, generator=g) for k, v in net.state_dict().items()}


@pytest.mark.parametrize("prefix", ["text_model.", ""])
def test_load_state_dict_takes_both_layouts_and_skips_position_ids(prefix):
    sd = _tiny_sd(prefix)
    sd[prefix + "embeddings.position_ids"] = torch.arange(77).unsqueeze(0)
    net = CLIPTextTransformer(**TINY)
    net.load_state_dict(sd)
    got = net.state_dict()
    assert "text_model.embeddings.position_ids" not in got
    for k, v in sd.items():
        if not k.endswith("position_ids"):
            assert torch.equal(got["text_model." + k[len(prefix):]], v), k


def test_load_state_dict_refuses_missing_misshaped_and_unknown_tensors():
    sd = _tiny_sd()
    short = dict(sd)
    del short["text_model.encoder.layers.1.mlp.fc2.bias"]
    with pytest.raises(RuntimeError, match="missing keys"):
        CLIPTextTransformer(**TINY).load_state_dict(short)
    with pytest.raises(RuntimeError, match="missing keys"):
        CLIPTextTransformer(**TINY).load_state_dict(short, strict=False)   # a missing tensor raises either way
    bad = dict(sd)
    bad["text_model.encoder.layers.0.mlp.fc1.weight"] = torch.zeros(128, 512)   # transposed
    with pytest.raises(RuntimeError, match="size mismatch"):
        CLIPTextTransformer(**TINY).load_state_dict(bad)
    extra = dict(sd)
    extra["text_model.text_projection.weight"] = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        CLIPTextTransformer(**TINY).load_state_dict(extra)
    CLIPTextTransformer(**TINY).load_state_dict(extra, strict=False)


def test_embedder_state_dict_round_trip_under_the_checkpoint_prefix():
    emb = FrozenCLIPEmbedder(device="cpu", config=TINY)
    sd = emb.state_dict()
    assert all(k.startswith("transformer.text_model.") for k in sd) and len(sd) == 2 + 16 * 2 + 2
    other = FrozenCLIPEmbedder(device="cpu", config=TINY).randomize_(7)
    other.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    with pytest.raises(RuntimeError, match="unexpected keys"):
        other.load_state_dict(dict(sd, **{"logit_scale": torch.zeros(())}))


def test_forward_refuses_cpu_parameters_and_bad_ids():
    emb = FrozenCLIPEmbedder(device="cpu", config=TINY)
    with pytest.raises(AdmError):
        emb(torch.zeros(1, 77, dtype=torch.int64))          # parameters on the CPU: no fallback
    with pytest.raises(AdmError):
        emb.transformer(torch.zeros(1, 78, dtype=torch.int64))   # beyond the position table
    with pytest.raises(AdmError):
        emb.transformer(torch.zeros(1, 77))                 # not integers
    from autodiffusion_amd import ops
    with pytest.raises(AdmError):
        ops.attention_causal(torch.zeros(1, 77, 384, dtype=torch.bfloat16), 2)
    with pytest.raises(AdmError):
        ops.quick_gelu(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(AdmError):
        ops.layernorm_f32out(torch.zeros(1, 77, 128, dtype=torch.bfloat16), 77, torch.ones(128), torch.zeros(128))
    with pytest.raises(AdmError):
        ops.clip_embed(torch.zeros(1, 77, dtype=torch.int64), torch.zeros(512, 128), torch.zeros(77, 128), 128)


# ------------------------------------------------------------------ tokenizer plumbing
class _StubTokenizer:
    def __init__(self):
        self.calls = []

    def __call__(self, text, **kw):
        self.calls.append((text, kw))
        ids = torch.zeros((len(text), kw["max_length"]), dtype=torch.int64)
        for i, s in enumerate(text):
            ids[i, :len(s)] = torch.tensor([ord(ch) % 500 for ch in s[:kw["max_length"]]], dtype=torch.int64)
        return {"input_ids": ids, "length": torch.full((len(text),), kw["max_length"])}


def test_embedder_calls_the_tokenizer_with_the_reference_arguments():
    tok = _StubTokenizer()
    emb = FrozenCLIPEmbedder(version="/nonexistent/ignored-when-a-tokenizer-is-given", device="cpu", max_length=20, tokenizer=tok,
                             config=TINY)
    assert emb.tokenizer is tok and emb.max_length == 20 and isinstance(emb.transformer, CLIPTextTransformer)
    assert emb.freeze() is emb
    seen = []
    emb.transformer.forward = lambda ids: seen.append(ids) or torch.zeros(ids.shape + (128,))
    for text in (["a cat", "a dog"], ("a cat", "a dog")):   # the reference turns a tuple into a list (search_ea.py:524-525)
        out = emb.encode(text)
        assert out.shape == (2, 20, 128)
    assert len(tok.calls) == 2
    for text, kw in tok.calls:
        assert text == ["a cat", "a dog"] and isinstance(text, list)
        assert kw == dict(truncation=True, max_length=20, return_length=True, return_overflowing_tokens=False, padding="max_length",
                          return_tensors="pt")
    assert torch.equal(seen[0], seen[1]) and seen[0].shape == (2, 20) and seen[0][0, 0] == ord("a")
    # token ids enter directly: no tokenizer call
    emb(torch.ones(3, 20, dtype=torch.int32))
    assert len(tok.calls) == 2 and seen[-1].shape == (3, 20)


def test_a_version_that_is_no_local_directory_is_refused_before_any_library_call(monkeypatch, tmp_path):
    loads = []
    fake = types.ModuleType("transformers")

    class CLIPTokenizer:
        @classmethod
        def from_pretrained(cls, *a, **kw):
            loads.append((a, kw))
            return _StubTokenizer()
    fake.CLIPTokenizer = CLIPTokenizer
    monkeypatch.setitem(sys.modules, "transformers", fake)
    emb = FrozenCLIPEmbedder(device="cpu", config=TINY)   # the reference's default: a hub name
    assert emb.version == "openai/clip-vit-large-patch14"
    for bad in ("openai/clip-vit-large-patch14", "https://example.invalid/clip", str(tmp_path / "missing"), None):
        emb.version = bad
        with pytest.raises(AdmError, match="not an existing local directory"):
            emb.encode(["a cat"])
    assert loads == []
    # a local directory goes to CLIPTokenizer.from_pretrained, once, and only when the first string arrives
    emb.version = str(tmp_path)
    emb.transformer.forward = lambda ids: torch.zeros(ids.shape + (128,))
    emb(torch.zeros(1, 77, dtype=torch.int64))
    assert loads == []
    emb.encode(["a cat"])
    emb.encode(["a dog"])
    assert len(loads) == 1 and loads[0][0] == (str(tmp_path),)


def test_a_missing_transformers_package_is_named(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "transformers", None)   # import transformers -> ImportError
    emb = FrozenCLIPEmbedder(version=str(tmp_path), device="cpu", config=TINY)
    with pytest.raises(AdmError, match="transformers"):
        emb.encode(["a cat"])


# ------------------------------------------------------------------ LatentDiffusion
class _Sink:
    device = torch.device("cpu")

    def load_state_dict(self, sd, strict=True):
        self.got = dict(sd)


_CKPT = {"model.diffusion_model.out.2.bias": torch.zeros(4), "first_stage_model.decoder.conv_in.bias": torch.ones(3),
         "cond_stage_model.transformer.text_model.final_layer_norm.bias": torch.zeros(1),
         "cond_stage_model.transformer.text_model.embeddings.position_ids": torch.zeros(1, 77),
         "model_ema.decay": torch.zeros(()), "betas": torch.zeros(5)}


def test_latent_diffusion_without_a_cond_stage_is_what_it_was(capsys):
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    unet, vae = _Sink(), _Sink()
    ld = LatentDiffusion(unet, first_stage=vae)
    assert ld.cond_stage_model is None
    res = ld.load_state_dict(_CKPT)
    assert res == {"model": 1, "first_stage_model": 1, "ignored": {"cond_stage_model": 2, "model_ema": 1, "betas": 1}}
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "load_state_dict" in ln]
    assert len(lines) == 1
    assert lines[0].endswith("LatentDiffusion.load_state_dict: 1 UNet tensors, 1 first-stage tensors; not used on this path: "
                             "betas (1), cond_stage_model (2), model_ema (1)")
    with pytest.raises(AdmError, match="cond_stage"):
        ld.get_learned_conditioning(["a cat"])


def test_latent_diffusion_routes_the_cond_stage(capsys):
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    unet, vae, clip = _Sink(), _Sink(), _Sink()
    clip.encode = lambda c: ("encoded", c)
    ld = LatentDiffusion(unet, first_stage=vae, cond_stage=clip)
    res = ld.load_state_dict(_CKPT)
    assert sorted(clip.got) == ["transformer.text_model.embeddings.position_ids", "transformer.text_model.final_layer_norm.bias"]
    assert res == {"model": 1, "first_stage_model": 1, "cond_stage_model": 2, "ignored": {"model_ema": 1, "betas": 1}}
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "load_state_dict" in ln]
    assert len(lines) == 1 and "2 cond-stage tensors" in lines[0] and "cond_stage_model (" not in lines[0]
    assert ld.get_learned_conditioning(["a cat"]) == ("encoded", ["a cat"])
    # the real cond stage behind the route: the checkpoint's names load, a missing tensor raises
    emb = FrozenCLIPEmbedder(device="cpu", config=TINY)
    ld = LatentDiffusion(unet, cond_stage=emb)
    want = {"cond_stage_model." + k: v + 1 for k, v in emb.state_dict().items()}
    ld.load_state_dict(dict(_CKPT, **want))
    assert all(torch.equal(emb.state_dict()[k[len("cond_stage_model."):]], v) for k, v in want.items())
    with pytest.raises(RuntimeError, match="missing keys"):
        ld.load_state_dict(_CKPT)


# ------------------------------------------------------------------ SDCandidateEvaluator(prompts=)
def test_evaluator_takes_exactly_one_of_prompts_and_conditioning():
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    model = types.SimpleNamespace(device=torch.device("cpu"))
    feats = lambda x: x   # noqa: E731
    kw = dict(ref_mu=np.zeros(4), ref_sigma=np.eye(4), num_samples=10, features=feats)
    with pytest.raises(ValueError, match="exactly one"):
        SDCandidateEvaluator(model, None, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        SDCandidateEvaluator(model, None, conditioning=[], prompts=[["a cat"]], **kw)
    with pytest.raises(ValueError, match="exactly one"):
        SDCandidateEvaluator(model, None, [], np.zeros(4), np.eye(4), 10, prompts=[["a cat"]], features=feats)
    assert SDCandidateEvaluator(model, None, prompts=[["a cat"]], **kw).conditioning is None
    assert SDCandidateEvaluator(model, None, [], np.zeros(4), np.eye(4), 10, features=feats).prompts is None
    with pytest.raises(ValueError, match="required"):
        SDCandidateEvaluator(model, None, prompts=[["a cat"]], features=feats)


def test_evaluator_encodes_prompts_per_batch_and_the_empty_prompt_once():
    from test_sd_vae_host import _HostStats, _StubSampler, _opt
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    calls = []

    def encode(c):
        calls.append(c)
        return torch.full((len(c), 2, 4), float(len(calls)))
    model = types.SimpleNamespace(device=torch.device("cpu"), get_learned_conditioning=encode,
                                  decode_first_stage=lambda z: torch.tanh(z[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3)))
    prompts = [["a", "b"], ("c", "d"), ["e", "f"], ["g", "h"]]
    sampler = _StubSampler()
    a = np.random.RandomState(1).randn(40, 12)
    W = torch.from_numpy(np.random.RandomState(0).randn(3 * 8 * 8, 12)).float()
    ev = SDCandidateEvaluator(model, sampler, ref_mu=a.mean(0), ref_sigma=np.cov(a, rowvar=False), num_samples=4, prompts=prompts,
                              features=lambda im: im.reshape(im.shape[0], -1) @ W, device="cpu", accumulator=_HostStats,
                              image_out=lambda x, out: out.copy_(torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)))
    ev.get_cand_fid([100, 500, 900], _opt(2))
    # the empty prompt first (search_ea.py:521-523), once; then one call per batch, tuples as lists (:524-525)
    assert calls == [["", ""], ["a", "b"], ["c", "d"], ["e", "f"]] and all(isinstance(c, list) for c in calls)
    assert all(kw["unconditional_conditioning"] is sampler.calls[0]["unconditional_conditioning"] for kw in sampler.calls)
    ev.get_cand_fid([100, 500, 900], _opt(2))
    assert len(calls) == 7 and calls[4] == ["a", "b"]          # not encoded again by the second candidate
    calls.clear()
    ev.get_cand_fid([100, 500, 900], _opt(2, scale=1.0))       # no guidance: the empty prompt is not needed
    assert calls == [["a", "b"], ["c", "d"], ["e", "f"]]
    assert all(kw["unconditional_conditioning"] is None for kw in sampler.calls[-3:])


# ------------------------------------------------------------------ C ABI
def test_the_new_entry_points_are_declared_on_both_sides():
    with open(os.path.join(ROOT, "include", "adm_hip.h")) as f:
        header = f.read()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/adm_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 10 and re.search(r"#define\s+ADM_ABI_VERSION\s+10\b", header)
