"""Stable-Diffusion first stage on the HIP path: the KL-f8 autoencoder's decoder (latents -> images).

Host-side mirror of ``ldm.modules.diffusionmodules.model.Decoder`` (reference "Stable Diffusion"/ldm/modules/diffusionmodules/
model.py:462-568) and of the decode half of ``ldm.models.autoencoder.AutoencoderKL`` (autoencoder.py:285-333): the same
constructor arguments, the same state-dict keys (the ``first_stage_model.decoder.*`` / ``first_stage_model.post_quant_conv.*``
tensors of an SD-v1 checkpoint load unchanged), the reference's forward order.

Engine: 16-bit NHWC activations, every op a libadm_hip.so launch (ops.py).  Per block:
  entry                          adm_vae_latent_in: z * (1 / scale_factor) -> post_quant_conv -> 16-bit NHWC padded to 32 channels
  conv_in                        conv3x3 over the padded latent (weights zero-padded to 32 input channels)
  ResnetBlock (model.py:121-141) gn(eps 1e-6) -> conv3x3[affine+SiLU] -> gn -> conv3x3[affine+SiLU, + x | nin_shortcut 1x1(x)]
  AttnBlock (:178-202)           gn -> fused q|k|v 1x1 [affine] -> attention (one head: width <= 256 on adm_attention, 512 on
                                 adm_attention_1h512) -> 1x1 proj_out (+x)
  Upsample (:53-57)              conv3x3 reading its input through the virtual nearest 2x upsample (four 2x2-tap phase convs
                                 from 16x16 sources up), or ops.resample(x, "up") without the conv
  head                           gn -> conv3x3[affine+SiLU] with the fp32 NCHW epilogue
The encoder and non-square latents are not built (the CLIP text encoder is sd_clip.py).
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

        def conv(p, co, ci, k):
            out[f"{p}.weight"], out[f"{p}.bias"] = (co, ci, k, k), (co,)

        def norm(p, c):
            out[f"{p}.weight"], out[f"{p}.bias"] = (c,), (c,)

        def emit(b):
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
            elif isinstance(b, VaeUpSpec) and b.with_conv:
                conv(f"{b.prefix}.conv", b.channels, b.channels, 3)

        conv("conv_in", self.block_in, self.z_channels, 3)
        for b in self.seq:
            if b.prefix.startswith("mid."):
                emit(b)
        for lvl in range(len(self.ch_mult)):   # registration order inside a level: block, attn, upsample
            mine = [b for b in self.seq if b.prefix.startswith(f"up.{lvl}.")]
            for kind in (VaeResSpec, VaeAttnSpec, VaeUpSpec):
                for b in mine:
                    if isinstance(b, kind):
                        emit(b)
        norm("norm_out", self.block_out)
        conv("conv_out", self.out_ch, self.block_out, 3)
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
                pr.blocks[p] = dict(g=f32(f"{p}.norm.weight"), b=f32(f"{p}.norm.bias"),
                                    wqkv=pack(torch.cat([P[f"{p}.{k}.weight"].to(torch.float32) for k in "qkv"], 0)),
                                    bqkv=torch.cat([f32(f"{p}.{k}.bias") for k in "qkv"]).contiguous(),
                                    wproj=pack(P[f"{p}.proj_out.weight"]), bproj=f32(f"{p}.proj_out.bias"))
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


class AutoencoderKL:
    """The decode half of ldm.models.autoencoder.AutoencoderKL (autoencoder.py:285-333): post_quant_conv + Decoder."""

    _IGNORED = ("encoder.", "quant_conv.", "loss.")

    def __init__(self, ddconfig, embed_dim, **ignorekwargs):
        self.decoder = Decoder(**dict(ddconfig))   # double_z and the like fall into **ignorekwargs, as in the reference
        self.embed_dim = int(embed_dim)
        zc = self.decoder.plan.z_channels
        if self.embed_dim > 16:
            raise NotImplementedError("AutoencoderKL: embed_dim above 16")
        g = torch.Generator().manual_seed(1)
        self._params = OrderedDict()
        self._params["post_quant_conv.weight"] = (torch.rand((zc, self.embed_dim, 1, 1), generator=g) * 2 - 1) * self.embed_dim ** -0.5
        self._params["post_quant_conv.bias"] = torch.zeros((zc,))

    # ------------------------------------------------------------------ nn.Module-like surface
    def state_dict(self):
        sd = OrderedDict((f"decoder.{k}", v) for k, v in self.decoder.state_dict().items())
        sd.update(self._params)
        return sd

    def load_state_dict(self, sd, strict=True):
        """Takes ``decoder.*`` and ``post_quant_conv.*``; ``encoder.*``, ``quant_conv.*`` and ``loss.*`` (the training half of a
        first-stage checkpoint) are ignored.  A missing or mis-shaped decoder / post_quant_conv tensor raises."""
        dec, mine, unexpected = {}, {}, []
        for k, v in sd.items():
            if k.startswith("decoder."):
                dec[k[len("decoder."):]] = v
            elif k in self._params:
                mine[k] = v
            elif not k.startswith(self._IGNORED):
                unexpected.append(k)
        missing = [f"decoder.{k}" for k in self.decoder._params if k not in dec] + [k for k in self._params if k not in mine]
        bad = [k for k in dec if k not in self.decoder._params]
        if missing or bad or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for AutoencoderKL: missing keys {missing[:5]}... "
                               f"unexpected keys {([f'decoder.{k}' for k in bad] + unexpected)[:5]}...")
        self.decoder.load_state_dict(dec, strict=True)
        load_checked(self._params, mine)
        return [], unexpected

    def to(self, device):
        self.decoder.to(device)
        for k in self._params:
            self._params[k] = self._params[k].to(torch.device(device))
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def set_torso(self, torso: str):
        self.decoder.set_torso(torso)
        return self

    def randomize_(self, seed: int = 4321):
        self.decoder.randomize_(seed)
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

    def encode(self, x):
        raise NotImplementedError("AutoencoderKL.encode: the VAE encoder is not built on the HIP path (the search only decodes)")

    def __call__(self, z):
        return self.decode(z)


# ddconfig / embed_dim of the v1 first stage (configs/stable-diffusion/v1-inference.yaml: first_stage_config)
SD_V1_VAE = dict(ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 4, 4),
                               num_res_blocks=2, attn_resolutions=(), dropout=0.0), embed_dim=4)
