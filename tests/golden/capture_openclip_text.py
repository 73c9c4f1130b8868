#!/usr/bin/env python3
"""Capture golden vectors of the Stable-Diffusion 2.x cond stage: an OpenCLIP-style text tower (exact GELU, the last and the
last-but-one layer through ``ln_final``), computed by ``transformers.CLIPTextModel`` with ``hidden_act="gelu"`` on the CPU in
float64.  The reference tree has no SD 2 code; transformers' class is the same pre-LN causal transformer OpenCLIP's
``text_transformer_forward`` runs, and ``final_layer_norm(hidden_states[-2])`` is Stability's ``layer="penultimate"``.

Runs only in the build container (needs ``transformers``); the GPU box never imports it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_openclip_text.py

Stored in tests/golden/openclip_text_tiny.npz, under OpenCLIP's state-dict names (``model.*``, as an SD 2 checkpoint holds them
behind ``cond_stage_model.``): every matrix as seeded int8 ``q::<name>`` with an fp32 ``s::<name>`` (weight = q * s, exact in
fp32: the file stays a few hundred KiB), every vector as fp32 ``v::<name>``; the ids [3, 77] (zero-padded behind end-of-text, as
OpenCLIP's tokenizer pads; row 2 has end-of-text at position 76); ``penultimate`` and ``last`` [3, 77, 128] fp32.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

from transformers import CLIPTextConfig, CLIPTextModel  # noqa: E402

torch.set_num_threads(8)

CFG = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=77, hidden_act="gelu")
BOS, EOS = CFG["vocab_size"] - 2, CFG["vocab_size"] - 1


def openclip_tensors(rng):
    """name -> fp32 array under OpenCLIP's names, and the stored form of each."""
    c, i = CFG["hidden_size"], CFG["intermediate_size"]
    shapes = {"model.token_embedding.weight": (CFG["vocab_size"], c), "model.positional_embedding": (CFG["max_position_embeddings"], c)}
    for l in range(CFG["num_hidden_layers"]):
        p = f"model.transformer.resblocks.{l}."
        shapes.update({p + "ln_1.weight": (c,), p + "ln_1.bias": (c,), p + "attn.in_proj_weight": (3 * c, c), p + "attn.in_proj_bias": (3 * c,),
                       p + "attn.out_proj.weight": (c, c), p + "attn.out_proj.bias": (c,), p + "ln_2.weight": (c,), p + "ln_2.bias": (c,),
                       p + "mlp.c_fc.weight": (i, c), p + "mlp.c_fc.bias": (i,), p + "mlp.c_proj.weight": (c, i), p + "mlp.c_proj.bias": (c,)})
    shapes.update({"model.ln_final.weight": (c,), "model.ln_final.bias": (c,)})
    w, stored = {}, {}
    for name, shape in shapes.items():
        if len(shape) == 2:
            q = rng.integers(-127, 128, size=shape, dtype=np.int8)
            emb = name in ("model.token_embedding.weight", "model.positional_embedding")
            # mlp.c_proj three times the fan-in scale of the other matrices: the MLP branch then carries enough of the residual
            # stream for a tower run with quick_gelu to land about 1e-2 (relative Frobenius) away from these outputs
            gain = 0.5 if emb else (5.1 if "mlp.c_proj" in name else 1.7) / np.sqrt(shape[1])
            s = np.float32(gain / 127.0)
            w[name] = q.astype(np.float32) * s
            stored["q::" + name], stored["s::" + name] = q, s
        else:
            v = (rng.standard_normal(shape) * 0.1 + (1.0 if name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")) else 0.0))
            w[name] = v.astype(np.float32)
            stored["v::" + name] = w[name]
    return w, stored


def to_hf(w):
    """OpenCLIP's names -> CLIPTextModel's own (without a leading ``text_model.``)."""
    out = {"embeddings.token_embedding.weight": w["model.token_embedding.weight"],
           "embeddings.position_embedding.weight": w["model.positional_embedding"],
           "final_layer_norm.weight": w["model.ln_final.weight"], "final_layer_norm.bias": w["model.ln_final.bias"]}
    c = CFG["hidden_size"]
    for l in range(CFG["num_hidden_layers"]):
        p, q = f"model.transformer.resblocks.{l}.", f"encoder.layers.{l}."
        for j, n in enumerate("qkv"):
            out[q + f"self_attn.{n}_proj.weight"] = w[p + "attn.in_proj_weight"][j * c:(j + 1) * c]
            out[q + f"self_attn.{n}_proj.bias"] = w[p + "attn.in_proj_bias"][j * c:(j + 1) * c]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
                     ("mlp.c_proj", "mlp.fc2")):
            out[q + b + ".weight"], out[q + b + ".bias"] = w[p + a + ".weight"], w[p + a + ".bias"]
    return out


if __name__ == "__main__":
    rng = np.random.default_rng(2024)
    w, stored = openclip_tensors(rng)
    model = CLIPTextModel(CLIPTextConfig(**CFG)).eval().double()
    hf = to_hf(w)
    seen = set()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if not v.is_floating_point():
                continue
            own = k[len("text_model."):] if k.startswith("text_model.") else k
            v.copy_(torch.from_numpy(hf[own]).double())
            seen.add(own)
    assert seen == set(hf), seen ^ set(hf)
    ids = np.zeros((3, 77), dtype=np.int64)
    for r, n_tok in enumerate((5, 30, 75)):            # 75 tokens: end-of-text lands on position 76, nothing is padded
        ids[r, 0] = BOS
        ids[r, 1:1 + n_tok] = rng.integers(1, BOS, size=n_tok)
        ids[r, 1 + n_tok] = EOS
    assert ids[2, 76] == EOS and (ids[0, 7:] == 0).all()
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(ids), output_hidden_states=True)
        lnf = model.text_model.final_layer_norm if hasattr(model, "text_model") else model.final_layer_norm
        pen = lnf(out.hidden_states[-2])
        last = out.last_hidden_state
        assert len(out.hidden_states) == CFG["num_hidden_layers"] + 1
        assert torch.allclose(lnf(out.hidden_states[-1]), last, rtol=0, atol=1e-12)
    path = os.path.join(HERE, "openclip_text_tiny.npz")
    np.savez_compressed(path, ids=ids, penultimate=pen.to(torch.float32).numpy(), last=last.to(torch.float32).numpy(),
                        cfg=np.array(repr(CFG)), **stored)
    print("params", sum(v.size for v in w.values()), "rms", float(last.pow(2).mean().sqrt()), float(pen.pow(2).mean().sqrt()),
          "penultimate vs last rel", float((pen - last).norm() / last.norm()), f"{os.path.getsize(path) / 1024:.1f} KiB")
