"""Stable-Diffusion cond stage on the HIP path: the CLIP text transformer behind ``FrozenCLIPEmbedder``.

Host-side mirror of ``ldm.modules.encoders.modules.FrozenCLIPEmbedder`` (reference "Stable Diffusion"/ldm/modules/encoders/
modules.py:137-162), which tokenises with ``transformers.CLIPTokenizer`` and returns ``CLIPTextModel(...).last_hidden_state``:
the same constructor arguments and surface (``forward`` / ``encode`` / ``freeze``, ``.tokenizer``, ``.transformer``,
``.max_length``), the same state-dict keys (the ``cond_stage_model.transformer.text_model.*`` tensors of an SD-v1 checkpoint load
unchanged; the flat layout newer ``transformers`` releases write, without ``text_model.``, loads too).

Engine: 16-bit activations, every op a libadm_hip.so launch (ops.py).  A prompt's T tokens ride as the first T pixels of a
64-, 128- or 256-pixel map (8 x 8, 8 x 16, 16 x 16) so that the six projections of a layer are 1x1 convs; at T = 77 that is a
128-row map with 51 dead rows (39.8 %).  Dead rows start as zeros, stay finite (LayerNorm of a zero row is its beta; the
attention output's dead rows are zeros) and never meet a live row: every launch but the attention is row-wise, and the attention
reads and writes rows < T only.
  entry      adm_clip_embed: token_embedding[ids] + position_embedding[:T], one rounding
  layer      layernorm -> fused q | k | v 1x1 -> adm_attention_causal -> out_proj 1x1 (+x)
             layernorm -> fc1 1x1 -> adm_quick_gelu -> fc2 1x1 (+x)
  exit       adm_layernorm_f32out: final_layer_norm of the T live rows as fp32 [N, T, C] (no second rounding)
Tokenisation is host plumbing: ``transformers.CLIPTokenizer`` from a LOCAL directory, imported lazily, or any callable with its
interface passed as ``tokenizer=``; integer tensors [N, T] of token ids enter ``forward`` directly.  Nothing is ever fetched.
Pooled / projected outputs and attention masks are not built (the reference passes no mask: pad tokens are attended).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import ops
from ._lib import AdmError
from .unet import HipModule, _Prep

_LAYER_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")


@dataclass
class CLIPTextPlan:
    vocab_size: int
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5

    def param_shapes(self) -> "OrderedDict[str, tuple]":
        """name -> shape under ``text_model.``, in CLIPTextModel's state-dict order."""
        c, i = self.hidden_size, self.intermediate_size
        out: "OrderedDict[str, tuple]" = OrderedDict()
        out["text_model.embeddings.token_embedding.weight"] = (self.vocab_size, c)
        out["text_model.embeddings.position_embedding.weight"] = (self.max_position_embeddings, c)
        for l in range(self.num_hidden_layers):
            p = f"text_model.encoder.layers.{l}"
            for k in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj"):
                out[f"{p}.{k}.weight"], out[f"{p}.{k}.bias"] = (c, c), (c,)
            out[f"{p}.layer_norm1.weight"], out[f"{p}.layer_norm1.bias"] = (c,), (c,)
            out[f"{p}.mlp.fc1.weight"], out[f"{p}.mlp.fc1.bias"] = (i, c), (i,)
            out[f"{p}.mlp.fc2.weight"], out[f"{p}.mlp.fc2.bias"] = (c, i), (c,)
            out[f"{p}.layer_norm2.weight"], out[f"{p}.layer_norm2.bias"] = (c,), (c,)
        out["text_model.final_layer_norm.weight"], out["text_model.final_layer_norm.bias"] = (c,), (c,)
        return out

    def flops(self, t: int) -> float:
        """Algorithmic FLOPs of one prompt of t tokens: the six projections + 4 t^2 C / 2 for the causal attention."""
        c, i = self.hidden_size, self.intermediate_size
        return self.num_hidden_layers * (2.0 * t * (4 * c * c + 2 * c * i) + 2.0 * t * t * c)


def map_rows(t: int) -> int:
    """Rows of the pixel map a prompt of t tokens rides in (the conv kernels tile 8 x 8, 8 x 16 and 16 x 16 maps)."""
    if not 1 <= t <= 256:
        raise NotImplementedError(f"CLIP text transformer: {t} tokens (1 .. 256 are built)")
    return 64 if t <= 64 else (128 if t <= 128 else 256)


class CLIPTextTransformer(HipModule):
    """``transformers.CLIPTextModel`` up to ``last_hidden_state``: ids int64 [N, T] -> fp32 [N, T, hidden_size]."""

    ZERO_INIT = ()

    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                 max_position_embeddings=77, layer_norm_eps=1e-5):
        plan = CLIPTextPlan(int(vocab_size), int(hidden_size), int(intermediate_size), int(num_hidden_layers),
                            int(num_attention_heads), int(max_position_embeddings), float(layer_norm_eps))
        if plan.hidden_size != 64 * plan.num_attention_heads:
            raise NotImplementedError(f"CLIP text transformer: heads of {plan.hidden_size} / {plan.num_attention_heads} channels; "
                                      "the causal attention kernel takes 64-wide heads (every CLIP text tower has them)")
        if plan.hidden_size % 32 or plan.intermediate_size % 32 or plan.hidden_size > 2048:
            raise NotImplementedError("CLIP text transformer: hidden / intermediate sizes must be multiples of 32, hidden <= 2048")
        if not 1 <= plan.max_position_embeddings <= 256:
            raise NotImplementedError("CLIP text transformer: 1 .. 256 positions are built")
        super().__init__(plan, False)

    # ------------------------------------------------------------------ state dict
    def load_state_dict(self, sd, strict=True):
        """Takes CLIPTextModel's keys with or without the leading ``text_model.``; ``...embeddings.position_ids`` (a buffer) is
        skipped.  A missing or mis-shaped tensor raises; so does an unknown key under ``strict``."""
        mine = {}
        for k, v in sd.items():
            if k.endswith("embeddings.position_ids"):
                continue
            mine[k if k.startswith("text_model.") else "text_model." + k] = v
        missing = [k for k in self._params if k not in mine]
        unexpected = [k for k in mine if k not in self._params]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for CLIPTextTransformer: missing keys {missing[:5]}... "
                               f"unexpected keys {unexpected[:5]}...")
        return super().load_state_dict({k: v for k, v in mine.items() if k in self._params}, strict=True)

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self):
        P, dev, plan = self._params, self.device, self.plan
        if dev.type != "cuda":
            raise AdmError("CLIP text transformer: parameters are on the CPU; call .to(device) first (no CPU fallback)")
        f32 = lambda k: P["text_model." + k].to(torch.float32).contiguous()  # noqa: E731
        pack = lambda w: ops.pack_conv_weight(w, self.compute_dtype)  # noqa: E731
        pr = _Prep()
        pr.tok, pr.pos = f32("embeddings.token_embedding.weight"), f32("embeddings.position_embedding.weight")
        pr.layers = []
        for l in range(plan.num_hidden_layers):
            p = f"encoder.layers.{l}"
            pr.layers.append(dict(
                ln1=(f32(f"{p}.layer_norm1.weight"), f32(f"{p}.layer_norm1.bias")),
                wqkv=pack(torch.cat([f32(f"{p}.self_attn.{k}_proj.weight") for k in "qkv"], 0)),
                bqkv=torch.cat([f32(f"{p}.self_attn.{k}_proj.bias") for k in "qkv"]).contiguous(),
                wo=pack(f32(f"{p}.self_attn.out_proj.weight")), bo=f32(f"{p}.self_attn.out_proj.bias"),
                ln2=(f32(f"{p}.layer_norm2.weight"), f32(f"{p}.layer_norm2.bias")),
                w1=pack(f32(f"{p}.mlp.fc1.weight")), b1=f32(f"{p}.mlp.fc1.bias"),
                w2=pack(f32(f"{p}.mlp.fc2.weight")), b2=f32(f"{p}.mlp.fc2.bias")))
        pr.lnf = (f32("final_layer_norm.weight"), f32("final_layer_norm.bias"))
        self._packed = pr
        return pr

    # ------------------------------------------------------------------ forward
    def forward(self, ids):
        plan: CLIPTextPlan = self.plan
        if not torch.is_tensor(ids) or ids.dim() != 2 or ids.is_floating_point() or ids.dtype == torch.bool:
            raise AdmError("CLIP text transformer: expected an integer tensor [N, T] of token ids")
        n, t = ids.shape
        if n < 1 or not 1 <= t <= plan.max_position_embeddings:
            raise AdmError(f"CLIP text transformer: {n} x {t} ids; the position table holds {plan.max_position_embeddings}")
        pr = self._packed or self._prepare()
        ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        c, inner, heads, eps = plan.hidden_size, plan.intermediate_size, plan.num_attention_heads, plan.layer_norm_eps
        rows = map_rows(t)
        hh = rows // 16 if rows > 64 else 8
        ww = rows // hh
        with torch.no_grad():
            x = ops.clip_embed(ids, pr.tok, pr.pos, rows, self.compute_dtype).view(n, hh, ww, c)
            # one attention output for all layers: its dead rows are zeroed once and never written
            a = torch.zeros((n, rows, c), dtype=self.compute_dtype, device=x.device)
            for L in pr.layers:
                y = ops.layernorm(x, *L["ln1"], eps=eps)
                qkv = ops.conv(y, L["wqkv"], L["bqkv"], 3 * c, 1).view(n, rows, 3 * c)
                ops.attention_causal(qkv, heads, t, out=a)
                x = ops.conv(a.view(n, hh, ww, c), L["wo"], L["bo"], c, 1, res=x)
                y = ops.layernorm(x, *L["ln2"], eps=eps)
                u = ops.quick_gelu(ops.conv(y, L["w1"], L["b1"], inner, 1))
                x = ops.conv(u, L["w2"], L["b2"], c, 1, res=x)
            return ops.layernorm_f32out(x.view(n, rows, c), t, *pr.lnf, eps=eps)


# CLIPTextConfig of openai/clip-vit-large-patch14, the v1 cond stage (configs/stable-diffusion/v1-inference.yaml)
CLIP_VIT_L14_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                         max_position_embeddings=77)


class FrozenCLIPEmbedder:
    """modules.py:137-162.  ``version``: a LOCAL directory holding the tokenizer files (``CLIPTokenizer.from_pretrained``
    reads it when the first string arrives, unless ``tokenizer=`` was given); ``config``: the CLIPTextTransformer arguments
    (default: ViT-L/14's text tower)."""

    def __init__(self, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, tokenizer=None, config=None):
        self.version = version
        self.transformer = CLIPTextTransformer(**dict(CLIP_VIT_L14_TEXT if config is None else config))
        self.max_length = int(max_length)
        if not 1 <= self.max_length <= self.transformer.plan.max_position_embeddings:
            raise ValueError(f"FrozenCLIPEmbedder: max_length {max_length} outside the position table "
                             f"(1 .. {self.transformer.plan.max_position_embeddings})")
        self._tokenizer = tokenizer
        self.device = torch.device(device)
        self.transformer.to(self.device)
        self.freeze()

    # ------------------------------------------------------------------ tokenizer (host)
    @property
    def tokenizer(self):
        if self._tokenizer is None:
            v = self.version
            if not isinstance(v, (str, os.PathLike)) or not os.path.isdir(v):
                raise AdmError(f"FrozenCLIPEmbedder: version={v!r} is not an existing local directory; nothing is fetched here: "
                               "point it at a directory holding the CLIP tokenizer files (vocab.json, merges.txt), pass "
                               "tokenizer=, or call forward with an integer tensor of token ids")
            try:
                from transformers import CLIPTokenizer
            except ImportError as e:
                raise AdmError("FrozenCLIPEmbedder: tokenising strings needs the `transformers` package (CLIPTokenizer), which "
                               "is not installed; pass tokenizer= or token ids") from e
            self._tokenizer = CLIPTokenizer.from_pretrained(os.fspath(v), local_files_only=True)
        return self._tokenizer

    # ------------------------------------------------------------------ nn.Module-like surface
    def freeze(self):
        self.transformer.eval()   # inference-only engine: there is nothing to train
        return self

    def eval(self):
        return self

    def to(self, device):
        self.device = torch.device(device)
        self.transformer.to(self.device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def set_torso(self, torso: str):
        self.transformer.set_torso(torso)
        return self

    def randomize_(self, seed: int = 2468):
        self.transformer.randomize_(seed)
        return self

    @property
    def compute_dtype(self):
        return self.transformer.compute_dtype

    def state_dict(self):
        return OrderedDict(("transformer." + k, v) for k, v in self.transformer.state_dict().items())

    def load_state_dict(self, sd, strict=True):
        """The ``cond_stage_model.*`` tensors of a checkpoint, prefix stripped: ``transformer.text_model.*`` or ``transformer.*``."""
        inner, unexpected = {}, []
        for k, v in sd.items():
            if k.startswith("transformer."):
                inner[k[len("transformer."):]] = v
            else:
                unexpected.append(k)
        if strict and unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict for FrozenCLIPEmbedder: unexpected keys {unexpected[:5]}...")
        self.transformer.load_state_dict(inner, strict=strict)
        return [], unexpected

    # ------------------------------------------------------------------ modules.py:152-162
    def forward(self, text):
        if torch.is_tensor(text):
            tokens = text
        else:
            if isinstance(text, tuple):
                text = list(text)
            batch_encoding = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                            return_overflowing_tokens=False, padding="max_length", return_tensors="pt")
            tokens = batch_encoding["input_ids"]
        return self.transformer(tokens.to(self.device))

    def encode(self, text):
        return self(text)

    def __call__(self, text):
        return self.forward(text)
