#!/usr/bin/env python3
"""Capture golden vectors of the CLIP image tower and of the projected text tower: ``transformers``' own
``CLIPVisionModelWithProjection`` / ``CLIPTextModelWithProjection``, built offline from configs, behind the preprocessing of the
reference's ``FrozenClipImageEmbedder`` ("Stable Diffusion"/ldm/modules/encoders/modules.py:197-228: bicubic
``align_corners=True`` resize, (x + 1) / 2, CLIP mean / std; restated here with torch's own F.interpolate).  The text pooling is
the row at argmax(ids) (modules.py:165-194 via ``encode_text``; ``eos_token_id=2`` selects that rule in transformers).

Runs only in the build container (needs ``transformers``); the GPU box never imports it.  No reference program text is
imported.  Only inputs (uint8 images, token ids), expected fp32 outputs, configs and the ViT-L/14 key list are stored -- weights
are regenerated on both sides from ``oracle/fill.py`` under their state-dict names (the text tower under the checkpoint names of
capture_clip_text.py, so the tiny text tower is the same model; ``text_projection.weight`` under its bare name).

Also printed, for context: torch's own CPU error when the same models run with 16-bit weights and activations.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_clip_image.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle.fill import fill_array  # noqa: E402
from transformers import (CLIPTextConfig, CLIPTextModelWithProjection, CLIPVisionConfig,  # noqa: E402
                          CLIPVisionModelWithProjection)

torch.set_num_threads(8)

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
TINY = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
            projection_dim=64)
P16 = dict(TINY, image_size=64, patch_size=16)
L14W = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16, image_size=224, patch_size=14,
            projection_dim=768)
VITL14 = dict(L14W, num_hidden_layers=24)
TEXT_TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77, projection_dim=64)
IMAGES = {
    "clip_image_tiny": dict(cfg=TINY, n=3, h=40, w=72),    # T = 17: one row past a 16-row tile; one axis up, one down
    "clip_image_p16": dict(cfg=P16, n=2, h=64, w=64),      # K = 768; the resize is the identity
    "clip_image_l14w": dict(cfg=L14W, n=2, h=128, w=128),  # ViT-L/14's shapes at depth 2: T = 257, K = 588
}
TEXT_PREFIX = "cond_stage_model.transformer."


def own_name(k):
    return k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k


def fill_(model, prefix=""):
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                name = own_name(k) if prefix else k
                v.copy_(torch.from_numpy(fill_array((prefix if name.startswith("text_model.") else "") + name, tuple(v.shape))))
    return model.eval()


def preprocess(x, size):
    """modules.py:211-219 on images in [-1, 1]."""
    x = F.interpolate(x, (size, size), mode="bicubic", align_corners=True)
    x = (x + 1.0) / 2.0
    return (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


if __name__ == "__main__":
    embeds = {}
    for name, c in IMAGES.items():
        cfg = c["cfg"]
        model = fill_(CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg)))
        gen = torch.Generator().manual_seed(11)
        # smooth structure plus noise, so that the resize has something to get wrong and the patches differ
        yy, xx = torch.meshgrid(torch.linspace(0, 1, c["h"]), torch.linspace(0, 1, c["w"]), indexing="ij")
        base = torch.stack([torch.sin(6.0 * xx + i) * torch.cos(4.0 * yy - i) for i in range(3)], -1)
        u8 = ((base.unsqueeze(0) * 0.35 + 0.5 + 0.3 * (torch.rand(c["n"], c["h"], c["w"], 3, generator=gen) - 0.5)).clamp(0, 1) * 255).to(torch.uint8)
        x = u8.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0   # the [-1, 1] images the embedder takes
        with torch.no_grad():
            pv = preprocess(x, cfg["image_size"])
            out = model(pixel_values=pv).image_embeds.to(torch.float32)
            ctx = [rel(copy.deepcopy(model).to(dt)(pixel_values=pv.to(dt)).image_embeds.float(), out) for dt in (torch.bfloat16, torch.float16)]
        embeds[name] = out
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, images=u8.numpy(), out=out.numpy(), cfg=np.array(repr(cfg)))
        print(name, "params", sum(p.numel() for p in model.parameters()), "out", tuple(out.shape), "rms", float(out.pow(2).mean().sqrt()),
              f"torch CPU 16-bit rel fro bf16 {ctx[0]:.3g} fp16 {ctx[1]:.3g}", f"{os.path.getsize(path) / 1024:.1f} KiB")

    # the pair: projected text features of the tiny text tower and their cosines with clip_image_tiny's embeddings
    text_model = fill_(CLIPTextModelWithProjection(CLIPTextConfig(**TEXT_TINY, eos_token_id=2, bos_token_id=0, pad_token_id=1)), TEXT_PREFIX)
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(0, TEXT_TINY["vocab_size"] - 1, (3, 77), generator=gen, dtype=torch.int64)
    for i, at in enumerate((76, 20, 5)):   # the end-of-text token (the largest id) at the end, inside, and near the start
        ids[i, at] = TEXT_TINY["vocab_size"] - 1
    with torch.no_grad():
        res = text_model(input_ids=ids)
        text = res.text_embeds.to(torch.float32)
    g = np.load(os.path.join(HERE, "clip_text_tiny.npz"))   # the same tower as CLIPTextModel's fixture
    with torch.no_grad():
        same = rel(text_model(input_ids=torch.from_numpy(g["ids"])).last_hidden_state, torch.from_numpy(g["out"]))
    print(f"tiny text tower vs clip_text_tiny.npz: rel fro {same:.3g}")
    assert same <= 1e-5
    img = embeds["clip_image_tiny"].double()
    cos = (img * text.double()).sum(-1) / (img.norm(dim=-1) * text.double().norm(dim=-1))
    np.savez_compressed(os.path.join(HERE, "clip_pair_tiny.npz"), ids=ids.numpy(), text_embeds=text.numpy(), cosines=cos.numpy(),
                        cfg=np.array(repr(TEXT_TINY)))
    print("clip_pair_tiny text_embeds", tuple(text.shape), "cosines", cos.tolist())

    full = CLIPVisionModelWithProjection(CLIPVisionConfig(**VITL14))
    keys = {k: list(v.shape) for k, v in full.state_dict().items() if v.is_floating_point()}
    with open(os.path.join(HERE, "clip_image_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("clip_image_keys.json:", len(keys), "entries")
