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
             layernorm -> fc1 1x1 -> adm_quick_gelu (hidden_act "gelu": adm_gelu, the exact GELU) -> fc2 1x1 (+x)
  exit       adm_layernorm_f32out: final_layer_norm of the T live rows as fp32 [N, T, C] (no second rounding)
``FrozenOpenCLIPEmbedder`` (Stable Diffusion 2.x: OpenCLIP ViT-H/14's text tower, exact GELU, the "penultimate" exit that runs all
layers but the last before ``ln_final``, pad id 0) is the same engine under OpenCLIP's state-dict keys.
Tokenisation is host plumbing: ``transformers.CLIPTokenizer`` from a LOCAL directory, imported lazily, or any callable with its
interface passed as ``tokenizer=``; integer tensors [N, T] of token ids enter ``forward`` directly.  Nothing is ever fetched.
Attention masks are not built (the reference passes no mask: pad tokens are attended).

The CLIP IMAGE tower (``CLIPVisionTransformer``, ``transformers.CLIPVisionModelWithProjection``) shares the layer code; its
attention is the non-causal ``adm_attention_cross`` over the first T rows.  An image's T = 1 + (S / P)^2 tokens ride in a pitch
of ceil(T / 64) * 64 rows, presented to the row-wise 1x1 convs as 8 x 8 maps (T = 257: 320 rows, 63 dead, 19.7 %).
  entry      adm_resize_bilinear mode 2 (bicubic, align_corners=True) -> raw [0, 1] pixels [N, S, S, 8]
  patches    im2col (view / permute / copy) -> rows [N, pitch, K]; ONE 1x1 conv over all rows with CLIP's mean / std folded
             into the weight (1 / std_c) and into the residual operand POS (position_embedding - sum mean_c / std_c w; row 0 =
             class_embedding + pos[0], whose im2col row is zero); dead rows of both are zero
  pre-LN     adm_layernorm; then the layers above
  exit       adm_layernorm_f32out of row 0 (post_layernorm of the class token) -> adm_linear_f32 with visual_projection
Pooled text features (``CLIPTextTransformer.pooled``: the final-LN row at argmax(ids) through ``text_projection``), the two
reference embedder classes ``FrozenClipImageEmbedder`` / ``FrozenCLIPTextEmbedder`` (modules.py:165-228) and ``CLIPScorer``
(this project's definition of the CLIP score: the reference has none) sit on top.
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


def _layer_shapes(out, prefix, plan):
    """The encoder layers' tensors under ``prefix.N.``, in CLIPEncoderLayer's state-dict order (both towers)."""
    c, i = plan.hidden_size, plan.intermediate_size
    for l in range(plan.num_hidden_layers):
        p = f"{prefix}.{l}"
        for k in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj"):
            out[f"{p}.{k}.weight"], out[f"{p}.{k}.bias"] = (c, c), (c,)
        out[f"{p}.layer_norm1.weight"], out[f"{p}.layer_norm1.bias"] = (c,), (c,)
        out[f"{p}.mlp.fc1.weight"], out[f"{p}.mlp.fc1.bias"] = (i, c), (i,)
        out[f"{p}.mlp.fc2.weight"], out[f"{p}.mlp.fc2.bias"] = (c, i), (c,)
        out[f"{p}.layer_norm2.weight"], out[f"{p}.layer_norm2.bias"] = (c,), (c,)


def _prepare_layers(f32, pack, prefix, count):
    """Kernel-ready tensors of ``count`` encoder layers: f32(name) fetches a parameter, pack packs a 1x1 conv weight."""
    layers = []
    for l in range(count):
        p = f"{prefix}.{l}"
        layers.append(dict(
            ln1=(f32(f"{p}.layer_norm1.weight"), f32(f"{p}.layer_norm1.bias")),
            wqkv=pack(torch.cat([f32(f"{p}.self_attn.{k}_proj.weight") for k in "qkv"], 0)),
            bqkv=torch.cat([f32(f"{p}.self_attn.{k}_proj.bias") for k in "qkv"]).contiguous(),
            wo=pack(f32(f"{p}.self_attn.out_proj.weight")), bo=f32(f"{p}.self_attn.out_proj.bias"),
            ln2=(f32(f"{p}.layer_norm2.weight"), f32(f"{p}.layer_norm2.bias")),
            w1=pack(f32(f"{p}.mlp.fc1.weight")), b1=f32(f"{p}.mlp.fc1.bias"),
            w2=pack(f32(f"{p}.mlp.fc2.weight")), b2=f32(f"{p}.mlp.fc2.bias")))
    return layers


def _run_layers(x, layers, plan, n, rows, attend):
    """The pre-LN encoder layers of both towers on x 16-bit [maps, h, w, C] holding [n, rows, C]; attend(qkv [n, rows, 3 C]) is
    the tower's attention -> [n, rows, C]."""
    c, inner, eps = plan.hidden_size, plan.intermediate_size, plan.layer_norm_eps
    act = ops.gelu if getattr(plan, "hidden_act", "quick_gelu") == "gelu" else ops.quick_gelu
    for L in layers:
        y = ops.layernorm(x, *L["ln1"], eps=eps)
        qkv = ops.conv(y, L["wqkv"], L["bqkv"], 3 * c, 1).view(n, rows, 3 * c)
        a = attend(qkv)
        x = ops.conv(a.view(x.shape), L["wo"], L["bo"], c, 1, res=x)
        y = ops.layernorm(x, *L["ln2"], eps=eps)
        u = act(ops.conv(y, L["w1"], L["b1"], inner, 1))
        x = ops.conv(u, L["w2"], L["b2"], c, 1, res=x)
    return x


@dataclass
class CLIPTextPlan:
    vocab_size: int
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    projection_dim: int = 0   # > 0: ``text_projection.weight`` [E, C] of CLIPTextModelWithProjection / CLIPModel (absent in SD checkpoints)
    hidden_act: str = "quick_gelu"   # "gelu": the exact GELU (OpenCLIP's towers)
    run_layers: int = 0       # > 0: only the first run_layers encoder layers run before final_layer_norm (all are still loaded)

    def param_shapes(self) -> "OrderedDict[str, tuple]":
        """name -> shape under ``text_model.``, in CLIPTextModel's state-dict order (``text_projection.weight`` last)."""
        c = self.hidden_size
        out: "OrderedDict[str, tuple]" = OrderedDict()
        out["text_model.embeddings.token_embedding.weight"] = (self.vocab_size, c)
        out["text_model.embeddings.position_embedding.weight"] = (self.max_position_embeddings, c)
        _layer_shapes(out, "text_model.encoder.layers", self)
        out["text_model.final_layer_norm.weight"], out["text_model.final_layer_norm.bias"] = (c,), (c,)
        if self.projection_dim:
            out["text_projection.weight"] = (self.projection_dim, c)
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
                 max_position_embeddings=77, layer_norm_eps=1e-5, projection_dim=0, hidden_act="quick_gelu", run_layers=None):
        if hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"CLIP text transformer: hidden_act {hidden_act!r} (\"quick_gelu\" or \"gelu\")")
        if run_layers is not None and not 1 <= int(run_layers) <= int(num_hidden_layers):
            raise ValueError(f"CLIP text transformer: run_layers {run_layers} outside 1 .. {num_hidden_layers}")
        plan = CLIPTextPlan(int(vocab_size), int(hidden_size), int(intermediate_size), int(num_hidden_layers),
                            int(num_attention_heads), int(max_position_embeddings), float(layer_norm_eps), int(projection_dim or 0),
                            hidden_act, int(run_layers or 0))
        if plan.projection_dim < 0:
            raise ValueError("CLIP text transformer: projection_dim must be positive (or 0 / None for no text_projection)")
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
        skipped; ``text_projection.weight`` (models built with projection_dim) keeps its name.  The OpenAI ``clip``-package layout
        (``token_embedding.weight``, ``transformer.resblocks.N...``) is remapped.  A missing or mis-shaped tensor raises; so does an
        unknown key under ``strict``."""
        if any(k.startswith("transformer.resblocks.") for k in sd):
            sd = openai_to_hf(sd)[1]
        mine = {}
        for k, v in sd.items():
            if k.endswith("embeddings.position_ids"):
                continue
            mine[k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k] = v
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
        pr.layers = _prepare_layers(f32, pack, "encoder.layers", plan.num_hidden_layers)
        pr.lnf = (f32("final_layer_norm.weight"), f32("final_layer_norm.bias"))
        pr.proj = P["text_projection.weight"].to(torch.float32).contiguous() if plan.projection_dim else None
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
        c, heads, eps = plan.hidden_size, plan.num_attention_heads, plan.layer_norm_eps
        rows = map_rows(t)
        hh = rows // 16 if rows > 64 else 8
        ww = rows // hh
        with torch.no_grad():
            x = ops.clip_embed(ids, pr.tok, pr.pos, rows, self.compute_dtype).view(n, hh, ww, c)
            # one attention output for all layers: its dead rows are zeroed once and never written
            a = torch.zeros((n, rows, c), dtype=self.compute_dtype, device=x.device)
            layers = pr.layers[:plan.run_layers] if plan.run_layers else pr.layers
            x = _run_layers(x, layers, plan, n, rows, lambda qkv: ops.attention_causal(qkv, heads, t, out=a))
            return ops.layernorm_f32out(x.view(n, rows, c), t, *pr.lnf, eps=eps)

    def pooled(self, ids):
        """CLIPTextModelWithProjection's ``text_embeds`` (``encode_text`` of the OpenAI package): the final-LN row at argmax(ids) --
        the end-of-text token, the largest id of the vocabulary -- through ``text_projection``: fp32 [N, E], not normalised."""
        if not self.plan.projection_dim:
            raise AdmError("CLIP text transformer: built without projection_dim: there is no text_projection to pool through")
        last = self.forward(ids)
        n, t, c = last.shape
        at = ids.to(device=last.device, dtype=torch.int64).argmax(dim=-1) + torch.arange(n, device=last.device) * t
        return ops.linear_f32(last.view(n * t, c).index_select(0, at), self._packed.proj)


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


# ====================================================================== the SD 2.x cond stage
# OpenCLIP ViT-H/14 (laion2b_s32b_b79k), the text tower: CLIP's BPE vocabulary, 16 heads of 64, the exact GELU
OPENCLIP_VIT_H14_TEXT = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                             max_position_embeddings=77, hidden_act="gelu")
_OPENCLIP_IGNORED = ("text_projection", "logit_scale", "attn_mask")   # and visual.*: not on the path to the UNet's context


def openclip_pad(ids, eos: int):
    """OpenCLIP's tokenizer pads with id 0 where CLIP's pads with end-of-text: every id after the first ``eos`` of a row becomes 0
    (a row without ``eos`` is left as it is).  The causal attention lets the pad rows see their prefix and the UNet attends to
    all 77 rows, so the pad id changes the context."""
    ids = torch.as_tensor(ids).clone()
    is_eos = ids == int(eos)
    after = (is_eos.to(torch.int64).cumsum(dim=-1) - is_eos.to(torch.int64)) > 0
    ids[after] = 0
    return ids


class FrozenOpenCLIPEmbedder(FrozenCLIPEmbedder):
    """Stable Diffusion 2.x's cond stage (Stability's ldm/modules/encoders/modules.py FrozenOpenCLIPEmbedder): OpenCLIP's text
    tower up to ``ln_final`` of the last (``layer="last"``) or the last-but-one (``"penultimate"``: ``text_transformer_forward``
    with ``layer_idx = 1``) resblock.  ``version`` names the pretrained tag there; here, as in FrozenCLIPEmbedder, it is only read
    as a LOCAL tokenizer directory when strings arrive (OpenCLIP's BPE is CLIP's; the padding is rewritten by ``openclip_pad``).
    ``load_state_dict`` takes the ``cond_stage_model.*`` tensors of an SD 2 checkpoint, prefix stripped: ``model.*``."""

    LAYERS = ("last", "penultimate")

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True, layer="last",
                 tokenizer=None, config=None):
        if layer not in self.LAYERS:
            raise ValueError(f"FrozenOpenCLIPEmbedder: layer {layer!r} (one of {self.LAYERS})")
        if config is None:
            if arch != "ViT-H-14":
                raise NotImplementedError(f"FrozenOpenCLIPEmbedder: arch {arch!r}; pass \"ViT-H-14\" or config= (the tower's arguments)")
            config = OPENCLIP_VIT_H14_TEXT
        config = dict(config)
        config.setdefault("hidden_act", "gelu")
        if layer == "penultimate":
            if int(config["num_hidden_layers"]) < 2:
                raise ValueError("FrozenOpenCLIPEmbedder: layer=\"penultimate\" needs at least two layers")
            config["run_layers"] = int(config["num_hidden_layers"]) - 1
        self.arch, self.layer = arch, layer
        super().__init__(version, device, max_length, tokenizer, config)

    def state_dict(self):
        raise NotImplementedError("FrozenOpenCLIPEmbedder: state_dict() in OpenCLIP's layout is not built; the tower's own is "
                                  ".transformer.state_dict()")

    def load_state_dict(self, sd, strict=True):
        """``model.token_embedding.weight``, ``model.positional_embedding``, ``model.transformer.resblocks.N.*``, ``model.ln_final.*``
        (remapped by ``openai_to_hf``); ``model.text_projection``, ``model.logit_scale``, ``model.attn_mask`` and ``model.visual.*``
        are not on this path and are ignored, also under ``strict``."""
        inner, unexpected = {}, []
        for k, v in sd.items():
            if not k.startswith("model."):
                unexpected.append(k)
                continue
            name = k[len("model."):]
            if name in _OPENCLIP_IGNORED or name.startswith("visual."):
                continue
            if name.startswith("transformer.resblocks.") or name in ("token_embedding.weight", "positional_embedding", "ln_final.weight",
                                                                     "ln_final.bias"):
                inner[name] = v
            else:
                unexpected.append(k)
        if strict and unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict for FrozenOpenCLIPEmbedder: unexpected keys {unexpected[:5]}...")
        self.transformer.load_state_dict(openai_to_hf(inner)[1], strict=strict)
        return [], unexpected

    def forward(self, text):
        if torch.is_tensor(text):
            tokens = text          # ids enter unchanged: the caller pads them
        else:
            if isinstance(text, tuple):
                text = list(text)
            tokens = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                    return_overflowing_tokens=False, padding="max_length", return_tensors="pt")["input_ids"]
            tokens = openclip_pad(tokens, self.transformer.plan.vocab_size - 1)   # <|endoftext|> is the vocabulary's last id
        return self.transformer(tokens.to(self.device))


# ====================================================================== the image tower
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # the OpenAI package's preprocessing constants (modules.py:209-210)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass
class CLIPVisionPlan:
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    image_size: int
    patch_size: int
    projection_dim: int
    layer_norm_eps: float = 1e-5

    @property
    def tokens(self) -> int:
        return 1 + (self.image_size // self.patch_size) ** 2

    @property
    def pitch(self) -> int:
        """Rows an image's tokens ride in: the next multiple of 64, presented to the row-wise 1x1 convs as 8 x 8 maps."""
        return (self.tokens + 63) // 64 * 64

    @property
    def patch_k(self) -> int:
        """Columns of an im2col row: 3 P^2, zero-padded to the 1x1 conv's channel multiple."""
        return (3 * self.patch_size ** 2 + 31) // 32 * 32

    def param_shapes(self) -> "OrderedDict[str, tuple]":
        """name -> shape, in CLIPVisionModelWithProjection's state-dict order."""
        c, p = self.hidden_size, self.patch_size
        out: "OrderedDict[str, tuple]" = OrderedDict()
        out["vision_model.embeddings.class_embedding"] = (c,)
        out["vision_model.embeddings.patch_embedding.weight"] = (c, 3, p, p)
        out["vision_model.embeddings.position_embedding.weight"] = (self.tokens, c)
        out["vision_model.pre_layrnorm.weight"], out["vision_model.pre_layrnorm.bias"] = (c,), (c,)
        _layer_shapes(out, "vision_model.encoder.layers", self)
        out["vision_model.post_layernorm.weight"], out["vision_model.post_layernorm.bias"] = (c,), (c,)
        out["visual_projection.weight"] = (self.projection_dim, c)
        return out

    def flops(self) -> float:
        """Algorithmic FLOPs of one image: patch embedding, the six projections, 4 T^2 C for the full attention, the head."""
        c, i, t = self.hidden_size, self.intermediate_size, self.tokens
        return (2.0 * (t - 1) * 3 * self.patch_size ** 2 * c + self.num_hidden_layers * (2.0 * t * (4 * c * c + 2 * c * i) + 4.0 * t * t * c)
                + 2.0 * c * self.projection_dim)


_OPENAI_BLOCK = {"ln_1.": "layer_norm1.", "ln_2.": "layer_norm2.", "attn.out_proj.": "self_attn.out_proj.", "mlp.c_fc.": "mlp.fc1.",
                 "mlp.c_proj.": "mlp.fc2."}


def _openai_blocks(sd, src, dst, out):
    """``src.N.{attn.in_proj_*, attn.out_proj, ln_1, ln_2, mlp.c_fc, mlp.c_proj}`` -> CLIPEncoderLayer's names under ``dst.N.``."""
    for k, v in sd.items():
        if not k.startswith(src + "."):
            continue
        l, rest = k[len(src) + 1:].split(".", 1)
        if rest in ("attn.in_proj_weight", "attn.in_proj_bias"):
            leaf = rest.rsplit("_", 1)[1]
            for name, part in zip("qkv", torch.as_tensor(v).chunk(3, dim=0)):
                out[f"{dst}.{l}.self_attn.{name}_proj.{leaf}"] = part
            continue
        for a, b in _OPENAI_BLOCK.items():
            if rest.startswith(a):
                out[f"{dst}.{l}.{b}{rest[len(a):]}"] = v
                break
        else:
            out[f"{dst}.{l}.{rest}"] = v   # unknown: reported by the loader under its new name


def openai_to_hf(sd):
    """A state dict in the OpenAI ``clip``-package layout -> (vision tensors, text tensors) under transformers' CLIPModel names.
    ``visual.proj`` and ``text_projection`` are stored [C, E] there and are transposed; ``logit_scale`` and the buffers are dropped."""
    vis, txt = OrderedDict(), OrderedDict()
    simple_v = {"visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
                "visual.class_embedding": "vision_model.embeddings.class_embedding",
                "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
                "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
                "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias"}
    simple_t = {"token_embedding.weight": "text_model.embeddings.token_embedding.weight",
                "positional_embedding": "text_model.embeddings.position_embedding.weight",
                "ln_final.weight": "text_model.final_layer_norm.weight", "ln_final.bias": "text_model.final_layer_norm.bias"}
    for k, v in sd.items():
        if k in simple_v:
            vis[simple_v[k]] = v
        elif k in simple_t:
            txt[simple_t[k]] = v
        elif k == "visual.proj":
            vis["visual_projection.weight"] = torch.as_tensor(v).t()
        elif k == "text_projection":
            txt["text_projection.weight"] = torch.as_tensor(v).t()
    _openai_blocks(sd, "visual.transformer.resblocks", "vision_model.encoder.layers", vis)
    _openai_blocks(sd, "transformer.resblocks", "text_model.encoder.layers", txt)
    return vis, txt


def split_clip_state_dict(sd):
    """One CLIP checkpoint (a plain state dict in transformers' CLIPModel layout or the OpenAI layout) -> (the image tower's tensors,
    the text tower's), both under CLIPModel's names."""
    if any(k.startswith("visual.") for k in sd):
        return openai_to_hf(sd)
    vis = OrderedDict((k, v) for k, v in sd.items() if k.startswith(("vision_model.", "visual_projection.")) and not k.endswith("position_ids"))
    txt = OrderedDict((k, v) for k, v in sd.items() if k.startswith(("text_model.", "text_projection.")) and not k.endswith("position_ids"))
    return vis, txt


def fold_patch_embedding(weight, class_embedding, position_embedding, pitch: int, kpad: int):
    """CLIP's ``(x - mean_c) / std_c`` folded into the patch embedding, in the arithmetic of the operands (fp32 at prepare time):
    conv(normalize(x)) + pos = conv'(x) + POS with w' = w / std_c and POS[r >= 1] = pos[r] - sum_{c,y,x} w mean_c / std_c;
    POS[0] = class_embedding + pos[0] (the class token's im2col row is zero).  -> (w' [C, kpad] with the (c, y, x) columns of
    ``im2col_rows`` and zero padding, POS [pitch, C] with zero dead rows)."""
    c = weight.shape[0]
    k = weight[0].numel()
    mean = torch.tensor(CLIP_MEAN, dtype=weight.dtype, device=weight.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=weight.dtype, device=weight.device).view(1, 3, 1, 1)
    w = torch.zeros((c, kpad), dtype=weight.dtype, device=weight.device)
    w[:, :k] = (weight / std).reshape(c, k)
    t = position_embedding.shape[0]
    pos = torch.zeros((pitch, c), dtype=weight.dtype, device=weight.device)
    pos[1:t] = position_embedding[1:] - (weight * (mean / std)).sum(dim=(1, 2, 3))
    pos[0] = class_embedding + position_embedding[0]
    return w, pos


def im2col_rows(px, patch: int, pitch: int, kpad: int):
    """px [N, S, S, >= 3] NHWC -> rows [N, pitch, kpad]: row 1 + gy (S / P) + gx of an image holds its patch (gy, gx) as
    (channel, y, x) -- the column order of conv weight [C, 3, P, P] flattened -- row 0, the dead rows and the padding columns are zero.
    Data movement only (view, permute, copy)."""
    n, s = px.shape[0], px.shape[1]
    g = s // patch
    rows = torch.zeros((n, pitch, kpad), dtype=px.dtype, device=px.device)
    patches = px[..., :3].reshape(n, g, patch, g, patch, 3).permute(0, 1, 3, 5, 2, 4)   # n, gy, gx, c, y, x
    rows[:, 1:1 + g * g, :3 * patch * patch] = patches.reshape(n, g * g, 3 * patch * patch)
    return rows


MAP_PIXELS = 64   # rows per map handed to the row-wise 1x1 convs (8 x 8): divides every pitch, so a batch of any size tiles


def _row_maps(rows_total: int):
    """(maps, h, w) of the pixel maps that n * pitch token rows are presented as."""
    return rows_total // MAP_PIXELS, 8, MAP_PIXELS // 8


class CLIPVisionTransformer(HipModule):
    """``transformers.CLIPVisionModelWithProjection``: images -> fp32 ``image_embeds`` [N, projection_dim], not normalised (the
    OpenAI package's ``encode_image``).  ``forward`` takes fp32 NCHW images in [-1, 1] or uint8 NHWC images of any size."""

    ZERO_INIT = ()

    def __init__(self, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, image_size, patch_size, projection_dim,
                 layer_norm_eps=1e-5):
        plan = CLIPVisionPlan(int(hidden_size), int(intermediate_size), int(num_hidden_layers), int(num_attention_heads),
                              int(image_size), int(patch_size), int(projection_dim), float(layer_norm_eps))
        if plan.hidden_size != 64 * plan.num_attention_heads:
            raise NotImplementedError(f"CLIP image tower: heads of {plan.hidden_size} / {plan.num_attention_heads} channels; 64-wide "
                                      "heads are built (every CLIP ViT has them)")
        if plan.hidden_size % 32 or plan.intermediate_size % 32 or plan.projection_dim < 1:
            raise NotImplementedError("CLIP image tower: hidden / intermediate sizes must be multiples of 32, projection_dim >= 1")
        if plan.patch_size < 1 or plan.image_size < plan.patch_size or plan.image_size % plan.patch_size:
            raise NotImplementedError(f"CLIP image tower: image_size {plan.image_size} is not a multiple of patch_size {plan.patch_size}")
        super().__init__(plan, False)

    # ------------------------------------------------------------------ state dict
    def load_state_dict(self, sd, strict=True):
        """CLIPVisionModelWithProjection's keys, or the OpenAI layout's ``visual.*`` (remapped; a joint checkpoint's other tensors are
        then ignored).  A missing or mis-shaped tensor raises; so does an unknown key under ``strict``."""
        if any(k.startswith("visual.") for k in sd):
            sd = openai_to_hf(sd)[0]
        mine = {k: v for k, v in sd.items() if not k.endswith("embeddings.position_ids")}
        missing = [k for k in self._params if k not in mine]
        unexpected = [k for k in mine if k not in self._params]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for CLIPVisionTransformer: missing keys {missing[:5]}... "
                               f"unexpected keys {unexpected[:5]}...")
        return super().load_state_dict({k: v for k, v in mine.items() if k in self._params}, strict=True)

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self):
        P, dev, plan = self._params, self.device, self.plan
        if dev.type != "cuda":
            raise AdmError("CLIP image tower: parameters are on the CPU; call .to(device) first (no CPU fallback)")
        f32 = lambda k: P["vision_model." + k].to(torch.float32).contiguous()  # noqa: E731
        pack = lambda w: ops.pack_conv_weight(w, self.compute_dtype)  # noqa: E731
        pr = _Prep()
        w, pos = fold_patch_embedding(f32("embeddings.patch_embedding.weight"), f32("embeddings.class_embedding"),
                                      f32("embeddings.position_embedding.weight"), plan.pitch, plan.patch_k)
        pr.wpatch, pr.pos = pack(w), pos.to(self.compute_dtype)
        pr.zero_bias = torch.zeros(plan.hidden_size, dtype=torch.float32, device=dev)
        pr.ln_pre = (f32("pre_layrnorm.weight"), f32("pre_layrnorm.bias"))
        pr.layers = _prepare_layers(f32, pack, "encoder.layers", plan.num_hidden_layers)
        pr.ln_post = (f32("post_layernorm.weight"), f32("post_layernorm.bias"))
        pr.proj = P["visual_projection.weight"].to(torch.float32).contiguous()
        self._packed = pr
        return pr

    # ------------------------------------------------------------------ forward, in three steps
    def preprocess(self, images, unit: bool = False):
        """-> raw [0, 1] pixels, 16-bit NHWC [N, S, S, 8] (channels 3.. zero), by the bicubic ``align_corners=True`` resize of
        modules.py:213-216.  fp32 NCHW images in [-1, 1] ((x + 1) / 2 in the kernel; ``unit``: already in [0, 1]) or uint8 NHWC
        (x / 255).  CLIP's mean / std live in the patch embedding."""
        if not torch.is_tensor(images) or images.dim() != 4:
            raise AdmError("CLIP image tower: expected fp32 [N, 3, H, W] or uint8 [N, H, W, 3] images")
        s = self.plan.image_size
        images = images.to(self.device).contiguous()
        if images.dtype == torch.uint8:
            return ops.resize_bilinear(images, s, s, 8, "u8_nhwc", 2, 1.0 / 255.0, 0.0, self.compute_dtype)
        if images.dtype != torch.float32:
            raise AdmError(f"CLIP image tower: images of {images.dtype}; fp32 NCHW or uint8 NHWC are taken")
        scale, shift = (1.0, 0.0) if unit else (0.5, 0.5)
        return ops.resize_bilinear(images, s, s, 8, "f32_nchw", 2, scale, shift, self.compute_dtype)

    def tokens(self, px):
        """Raw pixels [N, S, S, 8] -> the pre-LN'd token rows, 16-bit [N, pitch, C] (rows >= T: LayerNorm of zero rows)."""
        plan: CLIPVisionPlan = self.plan
        pr = self._packed or self._prepare()
        n, c, pitch = px.shape[0], plan.hidden_size, plan.pitch
        if tuple(px.shape) != (n, plan.image_size, plan.image_size, 8) or px.dtype != self.compute_dtype:
            raise AdmError(f"CLIP image tower: pixels {tuple(px.shape)} {px.dtype}; preprocess() makes them")
        maps, mh, mw = _row_maps(n * pitch)
        with torch.no_grad():
            rows = im2col_rows(px, plan.patch_size, pitch, plan.patch_k)
            pos = pr.pos.unsqueeze(0).expand(n, pitch, c).contiguous()
            x = ops.conv(rows.view(maps, mh, mw, plan.patch_k), pr.wpatch, pr.zero_bias, c, 1, res=pos.view(maps, mh, mw, c))
            return ops.layernorm(x, *pr.ln_pre, eps=plan.layer_norm_eps).view(n, pitch, c)

    def encode_tokens(self, x):
        """Token rows [N, pitch, C] -> fp32 [N, E].  Rows >= T are never keys (the attention reads tk = T rows), and only row 0
        leaves: whatever they hold changes nothing."""
        plan: CLIPVisionPlan = self.plan
        pr = self._packed or self._prepare()
        n, c, pitch, t, heads = x.shape[0], plan.hidden_size, plan.pitch, plan.tokens, plan.num_attention_heads
        if tuple(x.shape) != (n, pitch, c) or x.dtype != self.compute_dtype:
            raise AdmError(f"CLIP image tower: token rows {tuple(x.shape)} {x.dtype}; expected [N, {pitch}, {c}] {self.compute_dtype}")
        with torch.no_grad():
            maps, mh, mw = _row_maps(n * pitch)
            x = _run_layers(x.view(maps, mh, mw, c), pr.layers, plan, n, pitch,
                            lambda qkv: ops.attention_cross(qkv, qkv[:, :, c:], heads, 64, tk=t, scale=0.125))
            cls = ops.layernorm_f32out(x.view(n, pitch, c), 1, *pr.ln_post, eps=plan.layer_norm_eps)
            return ops.linear_f32(cls.view(n, c), pr.proj)

    def forward(self, images, unit: bool = False):
        return self.encode_tokens(self.tokens(self.preprocess(images, unit)))


# openai/clip-vit-large-patch14: the image tower and the projected text tower
CLIP_VIT_L14_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                           patch_size=14, projection_dim=768)
CLIP_VIT_L14_TEXT_PROJ = dict(CLIP_VIT_L14_TEXT, projection_dim=768)


class FrozenClipImageEmbedder:
    """modules.py:197-228.  ``model``: "ViT-L/14" or the CLIPVisionTransformer arguments as a dict; nothing is fetched: weights
    come through ``load_state_dict`` (CLIPVisionModelWithProjection's keys or the OpenAI layout).  ``forward`` takes fp32 NCHW
    images in [-1, 1] and returns ``encode_image``'s fp32 [N, E], not normalised."""

    def __init__(self, model="ViT-L/14", jit=False, device="cuda", antialias=False):
        if antialias:
            raise NotImplementedError("FrozenClipImageEmbedder: the antialiased resize is not built (the reference's default is off)")
        if isinstance(model, str):
            if model != "ViT-L/14":
                raise NotImplementedError(f"FrozenClipImageEmbedder: model {model!r}; pass \"ViT-L/14\" or a config dict")
            model = CLIP_VIT_L14_VISION
        self.antialias = False
        self.device = torch.device(device)
        self.model = CLIPVisionTransformer(**dict(model)).to(self.device)
        self.model.eval()

    def to(self, device):
        self.device = torch.device(device)
        self.model.to(self.device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def set_torso(self, torso: str):
        self.model.set_torso(torso)
        return self

    def randomize_(self, seed: int = 1357):
        self.model.randomize_(seed)
        return self

    @property
    def compute_dtype(self):
        return self.model.compute_dtype

    def state_dict(self):
        return self.model.state_dict()

    def load_state_dict(self, sd, strict=True):
        return self.model.load_state_dict(sd, strict=strict)

    def preprocess(self, x, unit: bool = False):
        return self.model.preprocess(x, unit)

    def forward(self, x, unit: bool = False):
        return self.model.forward(x, unit)

    def __call__(self, x, unit: bool = False):
        return self.forward(x, unit)


def _squared_norms(z):
    """fp32 [N, E] on the device -> float64 [N] on the host; the sums over E are adm_linear_f32's (the diagonal of z z^T)."""
    out = []
    for i in range(0, z.shape[0], 256):
        zi = z[i:i + 256].contiguous()
        out.append(ops.linear_f32(zi, zi).diagonal().double().cpu())
    return torch.cat(out)


class FrozenCLIPTextEmbedder(FrozenCLIPEmbedder):
    """modules.py:165-194: ``encode_text`` -- the final-LN row at argmax(ids) through ``text_projection`` -- L2-normalised when
    ``normalize``.  ``forward`` -> fp32 [N, E]; ``encode`` -> [N, n_repeat, E].  ``version``, ``tokenizer`` and token ids as in
    FrozenCLIPEmbedder; ``config``: the CLIPTextTransformer arguments with ``projection_dim`` (default: ViT-L/14's)."""

    def __init__(self, version="ViT-L/14", device="cuda", max_length=77, n_repeat=1, normalize=True, tokenizer=None, config=None):
        config = dict(CLIP_VIT_L14_TEXT_PROJ if config is None else config)
        if not config.get("projection_dim"):
            raise ValueError("FrozenCLIPTextEmbedder: config needs projection_dim (the text_projection this class pools through)")
        super().__init__(version, device, max_length, tokenizer, config)
        self.n_repeat, self.normalize = int(n_repeat), bool(normalize)

    def tokens(self, text):
        """Token ids [N, T] on the device: an integer tensor as it is, strings through the tokenizer."""
        if not torch.is_tensor(text):
            text = list(text) if isinstance(text, tuple) else text
            text = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                  return_overflowing_tokens=False, padding="max_length", return_tensors="pt")["input_ids"]
        return text.to(self.device)

    def forward(self, text):
        z = self.transformer.pooled(self.tokens(text))
        if self.normalize:   # the N norms finish in float64 on the host, as CLIPScorer's cosines do
            z = (z.double().cpu() / _squared_norms(z).sqrt().unsqueeze(1)).to(torch.float32).to(z.device)
        return z

    def encode(self, text):
        z = self(text)
        return z[:, None, :].expand(-1, self.n_repeat, -1).contiguous()


class CLIPScorer:
    """Prompt-image alignment.  The reference has no CLIP-score script; this project's definition is the usual one:
    cos_i = <image_embeds_i, text_embeds_i> / (|image_embeds_i| |text_embeds_i|) and score = 100 * mean(max(cos, 0)).
    The sums over E run on the device (adm_linear_f32 on the two embeddings); the N-scalar finish is float64 on the host, as the
    Frechet distance's is."""

    def __init__(self, image_embedder, text_embedder):
        self.image_embedder, self.text_embedder = image_embedder, text_embedder

    def cosine(self, images, ids):
        """images: uint8 NHWC or fp32 NCHW in [0, 1]; ids: integer [N, T] (or strings, where the text embedder has a tokenizer)
        -> fp32 [N] on the host."""
        return self.cosine_and_embeds(images, ids)[0]

    def embeds(self, images):
        """fp32 device [N, E]: ``encode_image`` of the images (projected, NOT normalised) -- the rows CMMD works on (cmmd.py)."""
        return self.image_embedder(images, unit=True).to(torch.float32)

    def cosine_and_embeds(self, images, ids):
        """(cosine(images, ids), embeds(images)) from ONE pass of the image tower."""
        img = self.image_embedder(images, unit=True)
        txt = self.text_embedder.transformer.pooled(self.text_embedder.tokens(ids))   # not normalised: the norms are taken below
        if txt.shape != img.shape:
            raise AdmError(f"CLIPScorer: image embeddings {tuple(img.shape)} vs text embeddings {tuple(txt.shape)}")
        dots = []
        for i in range(0, img.shape[0], 256):
            dots.append(ops.linear_f32(img[i:i + 256].contiguous(), txt[i:i + 256].contiguous()).diagonal().double().cpu())
        cos = torch.cat(dots) / (_squared_norms(img) * _squared_norms(txt)).sqrt()
        return cos.to(torch.float32), img.to(torch.float32)

    @staticmethod
    def score_of(cosines) -> float:
        return float(100.0 * torch.as_tensor(cosines).double().clamp_min(0.0).mean())

    def score(self, images, ids) -> float:
        return self.score_of(self.cosine(images, ids))


# the smallest towers the test suite runs (--synthetic tiny of the command lines)
CLIP_TINY_VISION = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                        projection_dim=64)
CLIP_TINY_TEXT_PROJ = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                           max_position_embeddings=77, projection_dim=64)


def build_clip_scorer(state_dict=None, vision_config=None, text_config=None, device="cuda", torso=None, tokenizer_dir=None,
                      max_length=77):
    """A CLIPScorer whose two towers load from ONE CLIP checkpoint: a plain state dict in transformers' CLIPModel layout or in
    the OpenAI layout (default configs: ViT-L/14).  ``state_dict=None``: random weights (``randomize_()``), for tests and
    throughput runs.  ``tokenizer_dir``: the LOCAL tokenizer directory, needed only where prompts arrive as strings."""
    image = FrozenClipImageEmbedder(CLIP_VIT_L14_VISION if vision_config is None else vision_config, device="cpu")
    text = FrozenCLIPTextEmbedder(tokenizer_dir or "ViT-L/14", device="cpu", max_length=max_length, config=text_config)
    if state_dict is None:
        image.randomize_(1357)
        text.randomize_(2468)
    else:
        vis, txt = split_clip_state_dict(state_dict)
        image.load_state_dict(vis)
        text.load_state_dict(OrderedDict(("transformer." + k, v) for k, v in txt.items()))
    if torso is not None:
        image.set_torso(torso)
        text.set_torso(torso)
    return CLIPScorer(image.to(device), text.to(device))
