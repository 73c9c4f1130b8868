"""Stable-Diffusion first stage on the HIP path: the KL-f8 autoencoder's decoder (latents -> images) and, opt-in, its encoder
(images -> the posterior's moments).

Host-side mirror of ``ldm.modules.diffusionmodules.model.Decoder`` / ``Encoder`` (reference "Stable Diffusion"/ldm/modules/
diffusionmodules/model.py:462-568, 368-459) and of ``ldm.models.autoencoder.AutoencoderKL.decode`` / ``.encode``
(autoencoder.py:285-333): the same constructor arguments, the same state-dict keys (the ``first_stage_model.decoder.*`` /
``post_quant_conv.*`` -- and with ``with_encoder=True`` the ``encoder.*`` / ``quant_conv.*`` -- tensors of an SD-v1 checkpoint
load unchanged), the reference's forward order.

Engine: 16-bit NHWC activations, every op a libadm_hip.so launch (ops.py).  Per block:
  entry                          adm_vae_latent_in: z * (1 / scale_factor) -> post_quant_conv -> 16-bit NHWC padded to 32 channels
  conv_in                        conv3x3 over the padded latent (weights zero-padded to 32 input channels)
  ResnetBlock (model.py:121-141) gn(eps 1e-6) -> conv3x3[affine+SiLU] -> gn -> conv3x3[affine+SiLU, + x | nin_shortcut 1x1(x)]
  AttnBlock (:178-202)           gn -> fused q|k|v 1x1 [affine] -> attention (one head: width <= 256 on adm_attention, 512 on
                                 adm_attention_1h512) -> 1x1 proj_out (+x)
  Upsample (:53-57)              conv3x3 reading its input through the virtual nearest 2x upsample (four 2x2-tap phase convs
                                 from 16x16 sources up), or ops.resample(x, "up") without the conv
  head                           gn -> conv3x3[affine+SiLU] with the fp32 NCHW epilogue
The encoder (``AutoencoderKL(..., with_encoder=True)``) runs the same blocks downwards:
  conv_in                        adm_stem_conv3x3: the direct fp32 stem, 3 -> ch, from the fp32 NCHW image
  Downsample (model.py:60-79)    pad (0,1,0,1) + stride-2 pad-0 conv3x3 == the pad-1 stride-1 conv3x3 sampled at the odd pixels:
                                 conv3x3, then ops.resample(h, "stride2_odd") (4x the layer's algorithmic MACs: VaeEncoderPlan.flops);
                                 AvgPool2d(2) = ops.resample(h, "down") without the conv
  head                           gn -> conv3x3[affine+SiLU], fp32 NCHW epilogue (mid maps that are no multiple of 16, e.g. 8 x 8: activated,
                                 zero-padded to one and convolved there, Encoder._head).  In ``AutoencoderKL.encode`` the 1x1 ``quant_conv``
                                 is folded into ``conv_out`` when the weights are prepared (fp32, on the device, per tap:
                                 W' = Wq Wout, b' = Wq b_out + b_q), so this one launch writes the moments [N, 2 embed_dim, h, w]:
                                 no 8 -> 8 launch, no extra tensor.  The state dict keeps the two layers apart under their names.
  posterior                      DiagonalGaussian: mean | logvar halves copied apart, std = adm_vec_act mode 3, the sample
                                 mean + std * noise on adm_sd_step (sd_sampler.axpby_noise)
Non-square maps are not built (the CLIP text encoder is sd_clip.py).  The conv kernels tile maps of 8 x 8 or of a multiple of 16 pixels
a side, so the encoder takes images whose mid map is one of those (v1: sides of 64, or a multiple of 128) and refuses the rest
before its first launch (Encoder.check_images).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

from . import blocks, ops
from ._lib import AdmError
from .unet import HipModule, _Prep, load_checked

_ATTN_WIDTHS = (32, 48, 64, 80, 96, 128, 160, 192, 256, 512)   # adm_attention's head widths + adm_attention_1h512


@dataclass
class VaeResSpec:
    prefix: str
    cin: int
    cout: int


@dataclass
class VaeAttnSpec:
    prefix: str
    channels: int


@dataclass
class VaeUpSpec:
    prefix: str
    channels: int
    with_conv: bool


@dataclass
class VaeDownSpec:
    prefix: str
    channels: int
    with_conv: bool


def _emit_params(out, b):
    """The tensors of one ResnetBlock / AttnBlock / resampling conv, in the reference's registration order."""
    def conv(p, co, ci, k):
        out[f"{p}.weight"], out[f"{p}.bias"] = (co, ci, k, k), (co,)

    def norm(p, c):
        out[f"{p}.weight"], out[f"{p}.bias"] = (c,), (c,)

    if isinstance(b, VaeResSpec):
        norm(f"{b.prefix}.norm1", b.cin)
        conv(f"{b.prefix}.conv1", b.cout, b.cin, 3)
        norm(f"{b.prefix}.norm2", b.cout)
        conv(f"{b.prefix}.conv2", b.cout, b.cout, 3)
        if b.cin != b.cout:
            conv(f"{b.prefix}.nin_shortcut", b.cout, b.cin, 1)
    elif isinstance(b, VaeAttnSpec):
        norm(f"{b.prefix}.norm", b.channels)
        for k in ("q", "k", "v", "proj_out"):
            conv(f"{b.prefix}.{k}", b.channels, b.channels, 1)
    elif b.with_conv:
        conv(f"{b.prefix}.conv", b.channels, b.channels, 3)


@dataclass
class VaeDecoderPlan:
    """The layer list of ``Decoder.__init__`` (model.py:478-533) in forward order."""
    ch: int
    out_ch: int
    ch_mult: Tuple[int, ...]
    num_res_blocks: int
    attn_resolutions: Tuple[int, ...]
    resamp_with_conv: bool
    resolution: int
    z_channels: int
    block_in: int = 0                      # width of conv_in's output / the mid block
    block_out: int = 0                     # width in front of norm_out
    seq: List[object] = field(default_factory=list)

    def param_shapes(self) -> "OrderedDict[str, tuple]":
        """name -> shape, in the reference's state-dict order (up.0 first: model.py:525 prepends the levels)."""
        out: "OrderedDict[str, tuple]" = OrderedDict()

        out["conv_in.weight"], out["conv_in.bias"] = (self.block_in, self.z_channels, 3, 3), (self.block_in,)
        for b in self.seq:
            if b.prefix.startswith("mid."):
                _emit_params(out, b)
        for lvl in range(len(self.ch_mult)):   # registration order inside a level: block, attn, upsample
            mine = [b for b in self.seq if b.prefix.startswith(f"up.{lvl}.")]
            for kind in (VaeResSpec, VaeAttnSpec, VaeUpSpec):
                for b in mine:
                    if isinstance(b, kind):
                        _emit_params(out, b)
        out["norm_out.weight"], out["norm_out.bias"] = (self.block_out,), (self.block_out,)
        out["conv_out.weight"], out["conv_out.bias"] = (self.out_ch, self.block_out, 3, 3), (self.out_ch,)
        return out

    def flops(self, h: int, w: int) -> float:
        """Algorithmic FLOPs of one latent of h x w: sum 2 H W Cout Cin taps over the convs (post_quant_conv included, the
        Upsample convs as 9-tap convs on the upsampled map, as the reference states them) + 4 T^2 D per attention."""
        f = 2.0 * h * w * self.z_channels * self.z_channels + 2.0 * h * w * self.block_in * self.z_channels * 9
        for b in self.seq:
            if isinstance(b, VaeResSpec):
                f += 2.0 * h * w * b.cout * (b.cin * 9 + b.cout * 9 + (b.cin if b.cin != b.cout else 0))
            elif isinstance(b, VaeAttnSpec):
                f += 2.0 * h * w * b.channels * b.channels * 4 + 4.0 * (h * w) ** 2 * b.channels
            elif isinstance(b, VaeUpSpec):
                h, w = 2 * h, 2 * w
                if b.with_conv:
                    f += 2.0 * h * w * b.channels * b.channels * 9
        return f + 2.0 * h * w * self.out_ch * self.block_out * 9


def vae_decoder_plan(ch, out_ch, ch_mult, num_res_blocks, attn_resolutions, resamp_with_conv, resolution,
                     z_channels) -> VaeDecoderPlan:
    plan = VaeDecoderPlan(int(ch), int(out_ch), tuple(int(m) for m in ch_mult), int(num_res_blocks),
                          tuple(int(r) for r in attn_resolutions), bool(resamp_with_conv), int(resolution), int(z_channels))
    levels = len(plan.ch_mult)
    block_in = plan.ch * plan.ch_mult[levels - 1]
    curr_res = plan.resolution // 2 ** (levels - 1)
    plan.block_in = block_in
    plan.seq += [VaeResSpec("mid.block_1", block_in, block_in), VaeAttnSpec("mid.attn_1", block_in),
                 VaeResSpec("mid.block_2", block_in, block_in)]
    for lvl in reversed(range(levels)):
        block_out = plan.ch * plan.ch_mult[lvl]
        for i in range(plan.num_res_blocks + 1):
            plan.seq.append(VaeResSpec(f"up.{lvl}.block.{i}", block_in, block_out))
            block_in = block_out
            if curr_res in plan.attn_resolutions:
                plan.seq.append(VaeAttnSpec(f"up.{lvl}.attn.{i}", block_in))
        if lvl != 0:
            plan.seq.append(VaeUpSpec(f"up.{lvl}.upsample", block_in, plan.resamp_with_conv))
            curr_res *= 2
    plan.block_out = block_in
    return plan


class Decoder(HipModule):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, give_pre_end=False, tanh_out=False,
                 use_linear_attn=False, attn_type="vanilla", use_conv_shortcut=False, **ignorekwargs):
        if use_linear_attn:
            attn_type = "linear"
        unsupported = dict(attn_type=attn_type != "vanilla", tanh_out=tanh_out, give_pre_end=give_pre_end,
                           use_conv_shortcut=use_conv_shortcut)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"VAE Decoder on the HIP path: unsupported constructor arguments {bad} "
                                      "(built: vanilla attention, nin_shortcut, the plain conv_out head)")
        plan = vae_decoder_plan(ch, out_ch, ch_mult, num_res_blocks, attn_resolutions, resamp_with_conv, resolution, z_channels)
        if plan.z_channels > 32:
            raise NotImplementedError("VAE Decoder: more than 32 latent channels")
        for b in plan.seq:
            c = [b.cin, b.cout] if isinstance(b, VaeResSpec) else [b.channels]
            if any(v % 32 for v in c):
                raise NotImplementedError(f"VAE Decoder: {b.prefix} has {c} channels; the conv kernels take multiples of 32")
            if isinstance(b, VaeAttnSpec) and b.channels not in _ATTN_WIDTHS:
                raise NotImplementedError(f"VAE Decoder: {b.prefix} is a single head of {b.channels} channels; the attention "
                                          f"kernels take widths {_ATTN_WIDTHS}")
        super().__init__(plan, False)
        self.ch, self.resolution, self.in_channels = ch, resolution, in_channels
        self.num_resolutions, self.num_res_blocks = len(plan.ch_mult), num_res_blocks
        curr_res = resolution // 2 ** (len(plan.ch_mult) - 1)
        self.z_shape = (1, z_channels, curr_res, curr_res)

    ZERO_INIT = ()   # the reference zero-initialises nothing in this network; HipModule's rule would zero every proj_out

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self):
        P, dev, plan = self._params, self.device, self.plan
        if dev.type != "cuda":
            raise AdmError("VAE Decoder: parameters are on the CPU; call .to(device) first (no CPU fallback)")
        pr = _Prep()
        f32, pack = blocks.packers(P, self.compute_dtype)
        pr.conv_in = blocks.stem_weights(P, f32, pack, "conv_in", plan.z_channels, plan.block_in)
        pr.blocks: Dict[str, dict] = {}
        for b in plan.seq:
            p = b.prefix
            if isinstance(b, VaeResSpec):
                # fold=False: nin_shortcut has always been its own 1x1 launch here; folding it is a change of the launch sequence
                pr.blocks[p] = blocks.resblock_weights(P, f32, pack, p, blocks.VAE_RES_KEYS, b.cin != b.cout, fold=False)
            elif isinstance(b, VaeAttnSpec):
                pr.blocks[p] = _attn_weights(P, f32, pack, p)
            elif isinstance(b, VaeUpSpec):
                pr.blocks[p] = blocks.upsample_weights(P, f32, pack, f"{p}.conv", self.compute_dtype) if b.with_conv else {}
        pr.head = blocks.head_weights(P, f32, pack, "norm_out", "conv_out")
        self._packed = pr
        return pr

    # ------------------------------------------------------------------ blocks
    GN_EPS = 1e-6   # Normalize (model.py:38-39)

    def _resblock(self, d, s: VaeResSpec, x):
        aff1 = ops.gn_affine(x, d["g1"], d["b1"], eps=self.GN_EPS)
        h = ops.conv(x, d["w1"], d["c1b"], s.cout, 9, aff=aff1, silu=True, want_stats=True)
        aff2 = ops.gn_affine(h, d["g2"], d["b2"], eps=self.GN_EPS)
        return blocks.resblock_tail(d, s.cout, h, aff2, x)

    def forward_nhwc(self, x):
        """x: 16-bit NHWC [N, H, W, 32] latent map (channels beyond z_channels zero) -> fp32 NCHW [N, out_ch, f H, f W]."""
        pr = self._packed or self._prepare()
        plan: VaeDecoderPlan = self.plan
        n, hh, ww, c = x.shape
        if c != 32 or x.dtype != self.compute_dtype:
            raise AdmError(f"VAE Decoder: expected a {self.compute_dtype} NHWC map padded to 32 channels, got {tuple(x.shape)} {x.dtype}")
        if hh != ww or hh < 8 or hh % 8:
            raise AdmError(f"VAE Decoder: latent map {hh} x {ww} unsupported (square, a multiple of 8, at least 8 x 8)")
        with torch.no_grad():
            h = ops.conv(x, pr.conv_in["w"], pr.conv_in["b"], plan.block_in, 9, want_stats=True)
            for b in plan.seq:
                d = pr.blocks[b.prefix]
                if isinstance(b, VaeResSpec):
                    h = self._resblock(d, b, h)
                elif isinstance(b, VaeAttnSpec):   # one head: softmax(q k^T c^-1/2) v (model.py:186-198)
                    h = blocks.attention(d, h, 1, True, eps=self.GN_EPS)
                elif b.with_conv:
                    h = blocks.upsample_conv(d, h, b.channels, True)
                else:
                    h = ops.resample(h, "up")
            return blocks.head(pr.head, h, plan.out_ch, eps=self.GN_EPS)

    def forward(self, z):
        """z fp32 NCHW [N, z_channels, H, W] (the tensor the reference's Decoder takes) -> fp32 NCHW images."""
        if not z.is_cuda:
            raise AdmError("VAE Decoder.forward: z must be a device tensor (no CPU fallback)")
        return self.forward_nhwc(ops.nchw_to_nhwc_pad(z.to(torch.float32).contiguous(), 32, self.compute_dtype))


@dataclass
class VaeEncoderPlan:
    """The layer list of ``Encoder.__init__`` (model.py:382-432) in forward order."""
    ch: int
    ch_mult: Tuple[int, ...]
    num_res_blocks: int
    attn_resolutions: Tuple[int, ...]
    resamp_with_conv: bool
    in_channels: int
    resolution: int
    z_channels: int
    out_ch: int = 0                        # conv_out's width: 2 z_channels (double_z)
    block_in: int = 0                      # width of the mid block / in front of norm_out
    seq: List[object] = field(default_factory=list)

    def param_shapes(self) -> "OrderedDict[str, tuple]":
        """name -> shape, in the reference's state-dict order (inside a level: block, attn, downsample)."""
        out: "OrderedDict[str, tuple]" = OrderedDict()
        out["conv_in.weight"], out["conv_in.bias"] = (self.ch, self.in_channels, 3, 3), (self.ch,)
        for lvl in range(len(self.ch_mult)):
            mine = [b for b in self.seq if b.prefix.startswith(f"down.{lvl}.")]
            for kind in (VaeResSpec, VaeAttnSpec, VaeDownSpec):
                for b in mine:
                    if isinstance(b, kind):
                        _emit_params(out, b)
        for b in self.seq:
            if b.prefix.startswith("mid."):
                _emit_params(out, b)
        out["norm_out.weight"], out["norm_out.bias"] = (self.block_in,), (self.block_in,)
        out["conv_out.weight"], out["conv_out.bias"] = (self.out_ch, self.block_in, 3, 3), (self.out_ch,)
        return out

    def flops(self, h: int, w: int, executed: bool = False, embed_dim: int = None) -> float:
        """FLOPs of one image of h x w: sum 2 H W Cout Cin taps over the convs + 4 T^2 D per attention.  Algorithmic (default):
        every Downsample conv on its OUTPUT map, as the reference's stride-2 conv computes it, and with ``embed_dim`` the 1x1
        quant_conv behind conv_out.  executed=True: what the launches do -- the Downsample convs at stride 1 on their INPUT map
        (4x their algorithmic MACs; the odd-pixel pick keeps a quarter), quant_conv folded into a conv_out of 2 embed_dim outputs."""
        f = 2.0 * h * w * self.ch * self.in_channels * 9
        for b in self.seq:
            if isinstance(b, VaeResSpec):
                f += 2.0 * h * w * b.cout * (b.cin * 9 + b.cout * 9 + (b.cin if b.cin != b.cout else 0))
            elif isinstance(b, VaeAttnSpec):
                f += 2.0 * h * w * b.channels * b.channels * 4 + 4.0 * (h * w) ** 2 * b.channels
            elif isinstance(b, VaeDownSpec):
                if b.with_conv:
                    f += 2.0 * (h * w if executed else (h // 2) * (w // 2)) * b.channels * b.channels * 9
                h, w = h // 2, w // 2
        if embed_dim is None:
            return f + 2.0 * h * w * self.out_ch * self.block_in * 9
        if executed:
            return f + 2.0 * h * w * 2 * embed_dim * self.block_in * 9
        return f + 2.0 * h * w * self.out_ch * self.block_in * 9 + 2.0 * h * w * 2 * embed_dim * self.out_ch


def vae_encoder_plan(ch, ch_mult, num_res_blocks, attn_resolutions, resamp_with_conv, in_channels, resolution,
                     z_channels) -> VaeEncoderPlan:
    plan = VaeEncoderPlan(int(ch), tuple(int(m) for m in ch_mult), int(num_res_blocks), tuple(int(r) for r in attn_resolutions),
                          bool(resamp_with_conv), int(in_channels), int(resolution), int(z_channels))
    levels = len(plan.ch_mult)
    in_ch_mult = (1,) + plan.ch_mult
    curr_res = plan.resolution
    block_in = plan.ch
    for lvl in range(levels):
        block_in, block_out = plan.ch * in_ch_mult[lvl], plan.ch * plan.ch_mult[lvl]
        for i in range(plan.num_res_blocks):
            plan.seq.append(VaeResSpec(f"down.{lvl}.block.{i}", block_in, block_out))
            block_in = block_out
            if curr_res in plan.attn_resolutions:
                plan.seq.append(VaeAttnSpec(f"down.{lvl}.attn.{i}", block_in))
        if lvl != levels - 1:
            plan.seq.append(VaeDownSpec(f"down.{lvl}.downsample", block_in, plan.resamp_with_conv))
            curr_res //= 2
    plan.seq += [VaeResSpec("mid.block_1", block_in, block_in), VaeAttnSpec("mid.attn_1", block_in),
                 VaeResSpec("mid.block_2", block_in, block_in)]
    plan.block_in, plan.out_ch = block_in, 2 * plan.z_channels
    return plan


def _attn_weights(P, f32, pack, p):
    return dict(g=f32(f"{p}.norm.weight"), b=f32(f"{p}.norm.bias"),
                wqkv=pack(torch.cat([P[f"{p}.{k}.weight"].to(torch.float32) for k in "qkv"], 0)),
                bqkv=torch.cat([f32(f"{p}.{k}.bias") for k in "qkv"]).contiguous(),
                wproj=pack(P[f"{p}.proj_out.weight"]), bproj=f32(f"{p}.proj_out.bias"))


class Encoder(HipModule):
    def __init__(self, *, ch, out_ch=None, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, double_z=True, use_linear_attn=False,
                 attn_type="vanilla", **ignore_kwargs):
        if use_linear_attn:
            attn_type = "linear"
        bad = [k for k, v in dict(attn_type=attn_type != "vanilla", double_z=not double_z).items() if v]
        if bad:
            raise NotImplementedError(f"VAE Encoder on the HIP path: unsupported constructor arguments {bad} "
                                      "(built: vanilla attention, double_z=True)")
        plan = vae_encoder_plan(ch, ch_mult, num_res_blocks, attn_resolutions, resamp_with_conv, in_channels, resolution, z_channels)
        if not 1 <= plan.in_channels <= 8 or plan.ch > 512:
            raise NotImplementedError(f"VAE Encoder: conv_in {plan.in_channels} -> {plan.ch}; the direct stem takes up to 8 input "
                                      "and 512 output channels")
        if plan.out_ch > 32:
            raise NotImplementedError("VAE Encoder: more than 16 latent channels")
        for b in plan.seq:
            c = [b.cin, b.cout] if isinstance(b, VaeResSpec) else [b.channels]
            if any(v % 32 for v in c):
                raise NotImplementedError(f"VAE Encoder: {b.prefix} has {c} channels; the conv kernels take multiples of 32")
            if isinstance(b, VaeAttnSpec) and b.channels not in _ATTN_WIDTHS:
                raise NotImplementedError(f"VAE Encoder: {b.prefix} is a single head of {b.channels} channels; the attention "
                                          f"kernels take widths {_ATTN_WIDTHS}")
        super().__init__(plan, False)
        self.ch, self.resolution, self.in_channels = ch, resolution, in_channels
        self.num_resolutions, self.num_res_blocks = len(plan.ch_mult), num_res_blocks
        self.side_multiple = 8 * 2 ** (len(plan.ch_mult) - 1)   # the mid map is a multiple of 8, as the decoder's latent

    ZERO_INIT = ()   # as the Decoder: nothing is zero-initialised
    GN_EPS = 1e-6    # Normalize (model.py:38-39)

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self):
        P, dev, plan = self._params, self.device, self.plan
        if dev.type != "cuda":
            raise AdmError("VAE Encoder: parameters are on the CPU; call .to(device) first (no CPU fallback)")
        pr = _Prep()
        f32, pack = blocks.packers(P, self.compute_dtype)
        pr.conv_in = dict(w=f32("conv_in.weight"), b=f32("conv_in.bias"))   # the direct stem reads fp32 [cout, cin, 3, 3]
        pr.blocks: Dict[str, dict] = {}
        for b in plan.seq:
            p = b.prefix
            if isinstance(b, VaeResSpec):
                pr.blocks[p] = blocks.resblock_weights(P, f32, pack, p, blocks.VAE_RES_KEYS, b.cin != b.cout, fold=False)
            elif isinstance(b, VaeAttnSpec):
                pr.blocks[p] = _attn_weights(P, f32, pack, p)
            elif isinstance(b, VaeDownSpec):
                pr.blocks[p] = dict(w=pack(P[f"{p}.conv.weight"]), b=f32(f"{p}.conv.bias")) if b.with_conv else {}
        pr.head = blocks.head_weights(P, f32, pack, "norm_out", "conv_out")
        self._packed = pr
        return pr

    def folded_head(self, wq, bq):
        """The head with a 1x1 conv (wq fp32 [o, 2 z, 1, 1], bq [o]) folded into conv_out, in fp32 on the device, per tap:
        W'[o, c, tap] = sum_m wq[o, m] Wout[m, c, tap], b' = wq b_out + bq -- blocks.head on it writes wq (conv_out(.)) + bq."""
        P = self._params
        f32, pack = blocks.packers(P, self.compute_dtype)
        wq2 = wq.to(torch.float32).reshape(wq.shape[0], -1)
        w = torch.einsum("om,mcyx->ocyx", wq2, P["conv_out.weight"].to(torch.float32)).contiguous()
        cb = (wq2 @ P["conv_out.bias"].to(torch.float32) + bq.to(torch.float32)).contiguous()
        return dict(g=f32("norm_out.weight"), b=f32("norm_out.bias"), w=pack(w), cb=cb)

    # ------------------------------------------------------------------ blocks
    _resblock = Decoder._resblock

    def check_images(self, x, who="VAE Encoder"):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.plan.in_channels:
            raise AdmError(f"{who}: expected fp32 NCHW images [N, {self.plan.in_channels}, H, W], got "
                           f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        n, _, hh, ww = x.shape
        m = self.side_multiple
        if n < 1 or hh != ww or hh < m or hh % m:
            raise AdmError(f"{who}: images of {hh} x {ww} unsupported (square, sides a multiple of {m} = 8 * 2^(levels - 1))")
        mid = hh // (m // 8)
        if mid != 8 and mid % 16:   # adm_conv tiles maps of 8 x 8 or of a multiple of 16 pixels a side: refuse before the first launch
            raise AdmError(f"{who}: images of {hh} x {ww} unsupported: their {mid} x {mid} mid map does not tile into the conv kernels' "
                           f"16-pixel-wide patches (sides of {m}, or a multiple of {2 * m})")
        if not x.is_cuda:
            raise AdmError(f"{who}: the images must be a device tensor (the HIP path has no CPU fallback)")

    def forward_nhwc(self, x):
        """x fp32 NCHW images -> the 16-bit NHWC map in front of norm_out, [N, H / f, W / f, block_in]."""
        self.check_images(x)
        pr = self._packed or self._prepare()
        plan: VaeEncoderPlan = self.plan
        with torch.no_grad():
            h = ops.stem_conv3x3(x.to(torch.float32).contiguous(), pr.conv_in["w"], pr.conv_in["b"], self.compute_dtype)
            for b in plan.seq:
                d = pr.blocks[b.prefix]
                if isinstance(b, VaeResSpec):
                    h = self._resblock(d, b, h)
                elif isinstance(b, VaeAttnSpec):
                    h = blocks.attention(d, h, 1, True, eps=self.GN_EPS)
                elif b.with_conv:   # the stride-1 conv, then its odd pixels (module docstring)
                    h = ops.resample(ops.conv(h, d["w"], d["b"], b.channels, 9), "stride2_odd")
                else:
                    h = ops.resample(h, "down")
            return h

    def forward(self, x, head=None):
        """x fp32 NCHW [N, in_channels, H, W] -> fp32 NCHW [N, 2 z_channels, H / f, W / f] (the reference's Encoder.forward);
        head: another packed head (folded_head) in place of norm_out -> conv_out."""
        h = self.forward_nhwc(x)
        hd = self._packed.head if head is None else head
        with torch.no_grad():
            return self._head(hd, h)

    def _head(self, hd, h):
        """norm_out -> SiLU -> conv_out with the fp32 NCHW epilogue.  That epilogue's kernel takes 16 x 16-pixel tiles of one image, and
        the mid map may be 8 x 8 (a 64-pixel v1 image; the torso's convs take no other map that is no multiple of 16, check_images,
        though this function takes any multiple of 8): such a map is activated on its own pixels
        (resample(up) then resample(stride2, aff): SiLU(a h + b), rounded once to 16 bits as the conv's prologue rounds it), copied
        into the corner of a zeroed map of the next multiple of 16 -- the zeros to the right and below are the conv's own padding --
        convolved without a prologue, and the corner copied out.  Per image, like every launch: independent of the batch."""
        n, hh, ww, c = h.shape
        cout = hd["cb"].shape[0]
        if hh % 16 == 0 and ww % 16 == 0:
            return blocks.head(hd, h, cout, eps=self.GN_EPS)
        aff = ops.gn_affine(h, hd["g"], hd["b"], eps=self.GN_EPS)
        act = ops.resample(ops.resample(h, "up"), "stride2", aff)
        big = torch.zeros((n, -(-hh // 16) * 16, -(-ww // 16) * 16, c), dtype=h.dtype, device=h.device)
        big[:, :hh, :ww].copy_(act)
        out = ops.conv(big, hd["w"], hd["cb"], cout, 9, out_f32_nchw=True)
        return out[:, :, :hh, :ww].contiguous()


class DiagonalGaussianPosterior:
    """``DiagonalGaussianDistribution`` (ldm/modules/distributions/distributions.py:24-37) of fp32 NCHW moments [N, 2 e, h, w] on
    the device: ``mean`` and ``logvar`` (clamped to [-30, 20]) are contiguous copies of the two halves, ``std`` =
    exp(0.5 logvar).  No torch arithmetic: the clamp and the exponential are adm_vec_act modes 4 / 3, the sample is adm_sd_step."""

    def __init__(self, moments):
        if not torch.is_tensor(moments) or not moments.is_cuda or moments.dim() != 4 or moments.shape[1] % 2:
            raise AdmError("DiagonalGaussianPosterior: expected fp32 NCHW device moments [N, 2 e, h, w]")
        e = moments.shape[1] // 2
        self.parameters = moments
        self.mean = moments[:, :e].contiguous()
        self._raw = moments[:, e:].contiguous()
        self.logvar = ops.vec_act(self._raw, "gauss_logvar")
        self.std = ops.vec_act(self._raw, "gauss_std")

    def sample(self, generator=None, noise=None, scale: float = 1.0):
        """scale * (mean + std * noise) as scale * mean + scale * (std * noise); noise: fp32 device tensor of mean's shape (default:
        drawn from ``generator``, on the generator's device, or from the device's global generator)."""
        from .sd_sampler import axpby_noise
        if noise is None:
            gdev = self.mean.device if generator is None else generator.device
            noise = torch.randn(self.mean.shape, generator=generator, device=gdev, dtype=torch.float32)
        noise = noise.to(device=self.mean.device, dtype=torch.float32).contiguous()
        if noise.shape != self.mean.shape:
            raise AdmError(f"DiagonalGaussianPosterior.sample: noise {tuple(noise.shape)} vs mean {tuple(self.mean.shape)}")
        return axpby_noise(self.mean, scale, ops.vec_act(self._raw, "gauss_std", dy=noise), scale)

    def mode(self):
        return self.mean


class AutoencoderKL:
    """ldm.models.autoencoder.AutoencoderKL (autoencoder.py:285-333): post_quant_conv + Decoder, and with ``with_encoder=True``
    Encoder + quant_conv (the default object is the decode half alone and ignores the other half of a checkpoint)."""

    _IGNORED = ("encoder.", "quant_conv.", "loss.")

    def __init__(self, ddconfig, embed_dim, with_encoder=False, **ignorekwargs):
        self.decoder = Decoder(**dict(ddconfig))   # double_z and the like fall into **ignorekwargs, as in the reference
        self.embed_dim = int(embed_dim)
        zc = self.decoder.plan.z_channels
        if self.embed_dim > 16:
            raise NotImplementedError("AutoencoderKL: embed_dim above 16")
        g = torch.Generator().manual_seed(1)
        self._params = OrderedDict()
        self._params["post_quant_conv.weight"] = (torch.rand((zc, self.embed_dim, 1, 1), generator=g) * 2 - 1) * self.embed_dim ** -0.5
        self._params["post_quant_conv.bias"] = torch.zeros((zc,))
        self.encoder = None
        if with_encoder:
            if 2 * self.embed_dim > 16:
                raise NotImplementedError("AutoencoderKL(with_encoder=True): more than 16 moment channels (2 embed_dim)")
            self.encoder = Encoder(**dict(ddconfig))
            self._ignored = ("loss.",)
            self._enc_params = OrderedDict()   # quant_conv = Conv2d(2 z_channels, 2 embed_dim, 1) (autoencoder.py:302)
            self._enc_params["quant_conv.weight"] = (torch.rand((2 * self.embed_dim, 2 * zc, 1, 1), generator=g) * 2 - 1) * (2 * zc) ** -0.5
            self._enc_params["quant_conv.bias"] = torch.zeros((2 * self.embed_dim,))
            self._enc_head = None              # norm_out -> [quant_conv . conv_out], packed (Encoder.folded_head)
        else:
            self._ignored, self._enc_params = self._IGNORED, OrderedDict()

    # ------------------------------------------------------------------ nn.Module-like surface
    def state_dict(self):
        """The reference's registration order: encoder, decoder, quant_conv, post_quant_conv (autoencoder.py:298-303)."""
        sd = OrderedDict()
        if self.encoder is not None:
            sd.update((f"encoder.{k}", v) for k, v in self.encoder.state_dict().items())
        sd.update((f"decoder.{k}", v) for k, v in self.decoder.state_dict().items())
        sd.update(self._enc_params)
        sd.update(self._params)
        return sd

    def load_state_dict(self, sd, strict=True):
        """Takes ``decoder.*`` and ``post_quant_conv.*`` -- with the encoder also ``encoder.*`` and ``quant_conv.*``; without it
        those and ``loss.*`` (the training half of a first-stage checkpoint) are ignored, whatever their shape.  A missing or
        mis-shaped tensor of a part this object has raises."""
        parts = {"decoder.": (self.decoder, {})}
        if self.encoder is not None:
            parts["encoder."] = (self.encoder, {})
        own = OrderedDict(list(self._enc_params.items()) + list(self._params.items()))
        mine, unexpected = {}, []
        for k, v in sd.items():
            for prefix, (_, got) in parts.items():
                if k.startswith(prefix):
                    got[k[len(prefix):]] = v
                    break
            else:
                if k in own:
                    mine[k] = v
                elif not k.startswith(self._ignored):
                    unexpected.append(k)
        missing = [prefix + k for prefix, (net, got) in parts.items() for k in net._params if k not in got] + [k for k in own if k not in mine]
        bad = [prefix + k for prefix, (net, got) in parts.items() for k in got if k not in net._params]
        if missing or bad or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for AutoencoderKL: missing keys {missing[:5]}... "
                               f"unexpected keys {(bad + unexpected)[:5]}...")
        for net, got in parts.values():
            net.load_state_dict(got, strict=True)
        load_checked(self._params, mine)
        load_checked(self._enc_params, mine)
        self._enc_head = None
        return [], unexpected

    def to(self, device):
        self.decoder.to(device)
        if self.encoder is not None:
            self.encoder.to(device)
        for P in (self._params, self._enc_params):
            for k in P:
                P[k] = P[k].to(torch.device(device))
        self._enc_head = None
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def set_torso(self, torso: str):
        self.decoder.set_torso(torso)
        if self.encoder is not None:
            self.encoder.set_torso(torso)
        self._enc_head = None
        return self

    def randomize_(self, seed: int = 4321):
        self.decoder.randomize_(seed)
        if self.encoder is not None:
            self.encoder.randomize_(seed + 1000)
        self._enc_head = None
        return self

    @property
    def device(self):
        return self.decoder.device

    @property
    def compute_dtype(self):
        return self.decoder.compute_dtype

    # ------------------------------------------------------------------ decode
    def decode(self, z, inv_scale: float = 1.0):
        """z fp32 NCHW [N, embed_dim, H, W] -> fp32 NCHW images; ``inv_scale`` is LatentDiffusion's 1 / scale_factor
        (ddpm.py:713), applied in fp32 in front of post_quant_conv by the same launch."""
        if not torch.is_tensor(z) or not z.is_cuda:
            raise AdmError("AutoencoderKL.decode: z must be a device tensor (the HIP path has no CPU fallback)")
        if z.dim() != 4 or z.shape[1] != self.embed_dim:
            raise AdmError(f"AutoencoderKL.decode: expected [N, {self.embed_dim}, H, W] latents, got {tuple(z.shape)}")
        if self._params["post_quant_conv.weight"].device != z.device:
            raise AdmError("AutoencoderKL.decode: parameters and latents live on different devices; call .to(device) first")
        x = ops.vae_latent_in(z.to(torch.float32).contiguous(), self._params["post_quant_conv.weight"],
                              self._params["post_quant_conv.bias"], inv_scale, self.compute_dtype)
        return self.decoder.forward_nhwc(x)

    # ------------------------------------------------------------------ encode
    def encode_moments(self, x):
        """x fp32 NCHW images in [-1, 1] on the device -> fp32 NCHW moments [N, 2 embed_dim, H / f, W / f] = quant_conv(encoder(x))
        (autoencoder.py:322-324), written by the encoder's head launch (quant_conv folded into conv_out: module docstring)."""
        if self.encoder is None:
            raise NotImplementedError("AutoencoderKL.encode: constructed without the encoder; pass with_encoder=True")
        self.encoder.check_images(x, "AutoencoderKL.encode")
        if self._enc_params["quant_conv.weight"].device != x.device:
            raise AdmError("AutoencoderKL.encode: parameters and images live on different devices; call .to(device) first")
        if self._enc_head is None:
            self._enc_head = self.encoder.folded_head(self._enc_params["quant_conv.weight"], self._enc_params["quant_conv.bias"])
        return self.encoder.forward(x, head=self._enc_head)

    def encode(self, x):
        """-> DiagonalGaussianPosterior of quant_conv(encoder(x)) (autoencoder.py:321-326)."""
        return DiagonalGaussianPosterior(self.encode_moments(x))

    def __call__(self, z):
        return self.decode(z)


# ddconfig / embed_dim of the v1 first stage (configs/stable-diffusion/v1-inference.yaml: first_stage_config)
SD_V1_VAE = dict(ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 4, 4),
                               num_res_blocks=2, attn_resolutions=(), dropout=0.0), embed_dim=4)
