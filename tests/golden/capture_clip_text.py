#!/usr/bin/env python3
"""Capture golden vectors of the Stable-Diffusion cond stage: ``transformers.CLIPTextModel``, the class the reference's
``FrozenCLIPEmbedder`` calls ("Stable Diffusion"/ldm/modules/encoders/modules.py:137-162), built offline from a config.

Runs only in the build container (needs ``transformers``); the GPU box never imports it.  No reference program text is
imported.  Only the token ids, the expected fp32 ``last_hidden_state``, the config and ``max_length`` are stored -- weights are
regenerated on both sides from ``oracle/fill.py`` under their checkpoint names (``cond_stage_model.transformer.text_model.*``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_clip_text.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle.fill import fill_array  # noqa: E402
from transformers import CLIPTextConfig, CLIPTextModel  # noqa: E402

torch.set_num_threads(8)

TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77)
VITL14 = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
              max_position_embeddings=77)
CONFIGS = {
    "clip_text_tiny": dict(cfg=TINY, n=3, t=77),
    "clip_text_t20": dict(cfg=TINY, n=3, t=20),       # a max_length below the position table
    "clip_text_vitl14": dict(cfg=VITL14, n=2, t=77),  # the SD v1 cond stage at full width
}
PREFIX = "cond_stage_model.transformer.text_model."


def own_name(k):
    """The model's own state-dict key without a leading ``text_model.`` (transformers 4 has it, 5 does not)."""
    return k[len("text_model."):] if k.startswith("text_model.") else k


def build(cfg):
    model = CLIPTextModel(CLIPTextConfig(**cfg)).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                v.copy_(torch.from_numpy(fill_array(PREFIX + own_name(k), tuple(v.shape))))
    return model


if __name__ == "__main__":
    models = {}
    for name, c in CONFIGS.items():
        key = repr(c["cfg"])
        if key not in models:
            models[key] = build(c["cfg"])
        model = models[key]
        g = torch.Generator().manual_seed(5)
        ids = torch.randint(0, c["cfg"]["vocab_size"], (c["n"], c["t"]), generator=g, dtype=torch.int64)
        with torch.no_grad():
            out = model(input_ids=ids).last_hidden_state.to(torch.float32)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, ids=ids.numpy(), out=out.numpy(), cfg=np.array(repr(c["cfg"])), max_length=np.array(c["t"]))
        print(name, "params", sum(p.numel() for p in model.parameters()), "out", tuple(out.shape), "rms",
              float(out.pow(2).mean().sqrt()), f"{os.path.getsize(path) / 1024:.1f} KiB")
    full = models[repr(VITL14)]
    keys = {"transformer.text_model." + own_name(k): list(v.shape) for k, v in full.state_dict().items() if v.is_floating_point()}
    with open(os.path.join(HERE, "clip_text_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("clip_text_keys.json:", len(keys), "entries")
