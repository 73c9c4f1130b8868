"""Stable-Diffusion latent UNet forward on hand-written HIP kernels.

Host-side mirror of ``ldm.modules.diffusionmodules.openaimodel.UNetModel`` (reference "Stable Diffusion"/ldm/modules/
diffusionmodules/openaimodel.py:413-742) in the form the reference's configs instantiate (v1-inference*.yaml:
``use_spatial_transformer``, conv resampling, no scale-shift norm): same constructor arguments, the same state-dict
keys (an SD-v1 ``model.diffusion_model.*`` checkpoint loads unchanged), ``__call__(x, timesteps, context)`` taking and
returning fp32 NCHW latents.

Engine: activations are bf16 NHWC, so a token of the SpatialTransformer IS a pixel and every Linear is an ``adm_conv``
1x1 launch.  Per block:
  ResBlock (openaimodel.py:236-262)   gn -> conv3x3[affine+SiLU] -> gn of (h + emb) folded into the affine
                                      (adm_gn_finalize_add: h + emb is never written) -> conv3x3[affine+SiLU, +skip]
  Downsample (:118-145)               stride-2 conv3x3 at its 9 taps per output pixel (adm_conv2d); ADM_SD_STRIDE2=0: stride-1 conv + pick
  Upsample (:78-104)                  conv3x3 reading its input through the virtual nearest 2x upsample (in_up)
  SpatialTransformer (attention.py:218-260)
      gn(eps 1e-6) -> 1x1 proj_in [affine prologue]
      LayerNorm -> fused q|k|v 1x1 -> attention -> 1x1 to_out (+x)
      LayerNorm -> 1x1 to_q; context -> 1x1 k|v (77 tokens padded to a 8x16 map) -> attention -> 1x1 to_out (+x)
      LayerNorm -> 1x1 (C -> 8C) -> GEGLU -> 1x1 (4C -> C) (+x);  1x1 proj_out (+x_in)
  The reference's 40-channel heads are zero-padded to 48 by the packed projection weights (the MFMA attention kernels
  take head widths 32, 48, 64, 80, 96, 128, 160, 192, 256: 80 and 160 run as they are); the logit scale stays
  dim_head^-0.5.

Layer skipping (``forward(..., skip_layer=[ids])``): the ids of ``sd_arch`` (ResBlocks and transformers in
construction order) under the rule of guided_diffusion/dynamic_unet.py -- a skipped ResBlock is ``skip_connection(x)`` alone
(:245-250: x itself, or the unfused 1x1 over the block input), a skipped transformer is ``x`` (:316-318).  No launch is added.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, Sequence

import torch

from . import blocks, ops
from ._lib import AdmError
from .sd_arch import (SDDownSpec, SDResBlockSpec, SDStemSpec, SDTransformerSpec, SDUNetPlan, SDUpSpec,
                      sd_unet_plan)
from .unet import HipModule, _Prep

_HEAD_WIDTHS = (32, 48, 64, 80, 96, 128, 160, 192, 256)
# Downsample (openaimodel.py:149-152): the stride-2 3x3 conv at its own 9 taps per OUTPUT pixel (adm_conv2d), or as a stride-1
# conv on the faster tile kernel + an every-second-pixel pick (4 x the MACs); A/B switch ADM_SD_STRIDE2
STRIDE2_TAPS = os.environ.get("ADM_SD_STRIDE2", "1") != "0"
# with enable_splitk(): also the wide 1x1 projections of the 16x16 / 8x8 levels.  OFF by default -- measured (same box, SD v1 bench, two runs
# each): off 63.4 / 63.8, every 1280-wide projection split 61.8 / 61.7, only the 5120 -> 1280 ones 63.3 / 63.1 latents/s: the two guidance
# half batches on two streams already fill the CUs a 30-60-tile launch leaves idle, and the split adds fp32 partials + a reduce launch
SPLITK_1X1 = os.environ.get("ADM_SD_SPLITK_1X1", "0") != "0"


def _padded_head(d: int) -> int:
    for w in _HEAD_WIDTHS:
        if d <= w:
            return w
    raise NotImplementedError(f"attention heads of {d} channels exceed the widest kernel (256)")


def _pad_heads_out(w: torch.Tensor, heads: int, d: int, dp: int) -> torch.Tensor:
    """Linear weight [heads*d, cin] -> [heads*dp, cin]: every head's output rows zero-padded to dp."""
    cin = w.shape[1]
    out = torch.zeros((heads, dp, cin), dtype=torch.float32, device=w.device)
    out[:, :d] = w.to(torch.float32).reshape(heads, d, cin)
    return out.reshape(heads * dp, cin)


def _pad_heads_in(w: torch.Tensor, heads: int, d: int, dp: int) -> torch.Tensor:
    """Linear weight [cout, heads*d] -> [cout, heads*dp]: zero columns where the padded head channels arrive."""
    cout = w.shape[0]
    out = torch.zeros((cout, heads, dp), dtype=torch.float32, device=w.device)
    out[:, :, :d] = w.to(torch.float32).reshape(cout, heads, d)
    return out.reshape(cout, heads * dp)


class UNetModel(HipModule):
    def __init__(self, image_size=None, in_channels=4, model_channels=320, out_channels=4, num_res_blocks=2,
                 attention_resolutions=(4, 2, 1), dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2,
                 num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1, num_head_channels=-1,
                 num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None,
                 n_embed=None, legacy=True, use_linear_in_transformer=False):
        unsupported = dict(conv_resample=not conv_resample, dims=dims != 2, num_classes=num_classes is not None,
                           use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
                           use_spatial_transformer=not use_spatial_transformer, n_embed=n_embed is not None,
                           num_heads_upsample=num_heads_upsample not in (-1, num_heads))
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"latent UNet on the HIP path: unsupported constructor arguments {bad} "
                                      "(built: the v1-inference configuration family)")
        plan = sd_unet_plan(in_channels, model_channels, out_channels, num_res_blocks, tuple(attention_resolutions),
                            tuple(channel_mult), num_heads, num_head_channels, transformer_depth,
                            int(context_dim) if not isinstance(context_dim, (list, tuple)) else int(context_dim[0]),
                            legacy, bool(use_linear_in_transformer))
        super().__init__(plan, use_fp16)
        self.image_size = image_size
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.num_classes = None

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self):
        P, dev, plan = self._params, self.device, self.plan
        if dev.type != "cuda":
            raise AdmError("latent UNetModel: parameters are on the CPU; call .to(device) first (no CPU fallback)")
        pr = _Prep()
        f32, pack = blocks.packers(P, self.compute_dtype)
        pr.te0_w, pr.te0_b = f32("time_embed.0.weight"), f32("time_embed.0.bias")
        pr.te2_w, pr.te2_b = f32("time_embed.2.weight"), f32("time_embed.2.bias")
        ws, bs, off = [], [], 0
        pr.emb_off: Dict[str, int] = {}
        pr.blocks: Dict[str, dict] = {}
        zmax = 0
        for b in plan.all_blocks():
            p = b.prefix
            if isinstance(b, SDStemSpec):
                pr.blocks[p] = blocks.stem_weights(P, f32, pack, p, b.cin, b.cout)
            elif isinstance(b, SDResBlockSpec):
                ws.append(f32(f"{p}.emb_layers.1.weight"))
                bs.append(f32(f"{p}.emb_layers.1.bias"))
                pr.emb_off[p] = off
                off += b.cout
                pr.blocks[p] = blocks.resblock_weights(P, f32, pack, p, blocks.ADM_RES_KEYS, b.has_skip_conv, self.fold_skip)
            elif isinstance(b, SDDownSpec):
                pr.blocks[p] = dict(w=pack(P[f"{p}.op.weight"]), b=f32(f"{p}.op.bias"),
                                    w2d=ops.pack_conv2d_weight(P[f"{p}.op.weight"], None, self.compute_dtype))   # real stride-2 taps (adm_conv2d)
            elif isinstance(b, SDUpSpec):
                pr.blocks[p] = blocks.upsample_weights(P, f32, pack, f"{p}.conv", self.compute_dtype)
            elif isinstance(b, SDTransformerSpec):
                h, dh, dp = b.heads, b.d_head, _padded_head(b.d_head)
                # proj_in / proj_out: [out, in, 1, 1] or, with use_linear_in_transformer, nn.Linear's [out, in] -- one packed 1x1 conv
                d = dict(g=f32(f"{p}.norm.weight"), b=f32(f"{p}.norm.bias"), dp=dp,
                         w_in=pack(P[f"{p}.proj_in.weight"]), b_in=f32(f"{p}.proj_in.bias"),
                         w_out=pack(P[f"{p}.proj_out.weight"]), b_out=f32(f"{p}.proj_out.bias"), layers=[])
                zmax = max(zmax, 3 * h * dp)
                for li in range(b.depth):
                    q = f"{p}.transformer_blocks.{li}"
                    L = {}
                    for k in ("norm1", "norm2", "norm3"):
                        L[k] = (f32(f"{q}.{k}.weight"), f32(f"{q}.{k}.bias"))
                    L["qkv1"] = pack(torch.cat([_pad_heads_out(P[f"{q}.attn1.to_{c}.weight"], h, dh, dp) for c in "qkv"]))
                    L["o1"] = pack(_pad_heads_in(P[f"{q}.attn1.to_out.0.weight"], h, dh, dp))
                    L["o1b"] = f32(f"{q}.attn1.to_out.0.bias")
                    L["q2"] = pack(_pad_heads_out(P[f"{q}.attn2.to_q.weight"], h, dh, dp))
                    L["kv2"] = pack(torch.cat([_pad_heads_out(P[f"{q}.attn2.to_{c}.weight"], h, dh, dp) for c in "kv"]))
                    L["o2"] = pack(_pad_heads_in(P[f"{q}.attn2.to_out.0.weight"], h, dh, dp))
                    L["o2b"] = f32(f"{q}.attn2.to_out.0.bias")
                    L["ff1"] = pack(P[f"{q}.ff.net.0.proj.weight"])
                    L["ff1b"] = f32(f"{q}.ff.net.0.proj.bias")
                    if b.inner <= 640:   # GEGLU in the projection's epilogue: (value, gate) rows interleaved (the resident-tile 1x1
                        wi, bi = ops.geglu_interleave(P[f"{q}.ff.net.0.proj.weight"], P[f"{q}.ff.net.0.proj.bias"])   # kernel holds
                        L["ff1g"], L["ff1gb"] = pack(wi), bi.to(torch.float32).contiguous()   # <= 640 input channels per 64-pixel tile)
                    L["ff2"] = pack(P[f"{q}.ff.net.2.weight"])
                    L["ff2b"] = f32(f"{q}.ff.net.2.bias")
                    d["layers"].append(L)
                pr.blocks[p] = d
            else:
                raise TypeError(b)
        pr.emb_w = torch.cat(ws, dim=0).contiguous()
        pr.emb_b = torch.cat(bs, dim=0).contiguous()
        pr.emb_total = off
        pr.zero_bias = torch.zeros(max(zmax, 32), dtype=torch.float32, device=dev)  # the bias-free Linear layers
        pr.head = blocks.head_weights(P, f32, pack, "out.0", "out.2")
        pr.graphs = {}  # captured evaluations; they die with the packed weights they point into
        pr.skip_graphs = OrderedDict()  # ... those of a non-empty layer-skip set: a bounded LRU (plan_graphs)
        pr.kv_cache = None  # (context key, k|v projections of the cross-attention layers)
        self._packed = pr
        return pr

    # ------------------------------------------------------------------ blocks
    def _resblock(self, pr, s: SDResBlockSpec, x0, x1, emb, skipped=False):
        d = pr.blocks[s.prefix]
        if skipped:   # dynamic_unet.py:245-250: the body bypassed, skip_connection(x) kept
            if not s.has_skip_conv:
                assert x1 is None
                return x0   # with the statistics its producer accumulated (x0._adm_stats), if it did
            # the unfused 1x1 over (x0 | x1), never the folded 3x3 weights on zeros; its epilogue accumulates the GroupNorm
            # statistics the next block's gn_affine reads (where the kernel does not offer them, gn_affine runs its own pass)
            return ops.conv(x0, d["ws"], d["wsb"], s.cout, 1, x1=x1, want_stats=True)
        aff1 = ops.gn_affine(x0, d["g1"], d["b1"], x1)
        h = ops.conv(x0, d["w1"], d["c1b"], s.cout, 9, x1=x1, aff=aff1, silu=True, want_stats=True,
                     ksplit=self._ks(x0, x0.shape[3] + (0 if x1 is None else x1.shape[3])))
        off = pr.emb_off[s.prefix]
        aff2 = ops.gn_affine(h, d["g2"], d["b2"], add=emb[:, off:off + s.cout])
        ks2 = self._ks(h, h.shape[3])
        assert s.has_skip_conv or x1 is None
        return blocks.resblock_tail(d, s.cout, h, aff2, x0, x1, fold=ks2 == 1, ksplit=ks2)   # the folded conv has no split-K schedule

    def _transformer(self, pr, s: SDTransformerSpec, x, kvs, n_ctx):
        d = pr.blocks[s.prefix]
        n, hh, ww, c = x.shape
        t, heads, dp, inner = hh * ww, s.heads, d["dp"], s.inner
        hd = heads * dp
        scale = float(s.d_head) ** -0.5
        zb = pr.zero_bias
        aff = ops.gn_affine(x, d["g"], d["b"], eps=1e-6)
        h = ops.conv(x, d["w_in"], d["b_in"], inner, 1, aff=aff, silu=False, ksplit=self._ks1(x, c, inner))
        for li, L in enumerate(d["layers"]):
            # self-attention
            y = ops.layernorm(h, *L["norm1"])
            qkv = ops.conv(y, L["qkv1"], zb, 3 * hd, 1).view(n, t, 3 * hd)
            a = ops.attention_cross(qkv, qkv[:, :, hd:], heads, dp, t, scale)
            h = ops.conv(a.view(n, hh, ww, hd), L["o1"], L["o1b"], inner, 1, res=h, ksplit=self._ks1(x, hd, inner))
            # cross-attention over the conditioning tokens
            y = ops.layernorm(h, *L["norm2"])
            q = ops.conv(y, L["q2"], zb, hd, 1, ksplit=self._ks1(x, inner, hd)).view(n, t, hd)
            kv = kvs[(s.prefix, li)]
            a = ops.attention_cross(q, kv.view(n, -1, 2 * hd), heads, dp, n_ctx, scale)
            h = ops.conv(a.view(n, hh, ww, hd), L["o2"], L["o2b"], inner, 1, res=h, ksplit=self._ks1(x, hd, inner))
            # gated feed-forward
            y = ops.layernorm(h, *L["norm3"])
            if self.fuse_geglu and "ff1g" in L and t % 64 == 0 and ops.geglu_fusable(y, 8 * inner):
                gl = ops.conv(y, L["ff1g"], L["ff1gb"], 8 * inner, 1, geglu=True)    # [n, hh, ww, 4 * inner]: u never exists
            else:
                gl = ops.geglu(ops.conv(y, L["ff1"], L["ff1b"], 8 * inner, 1))
            h = ops.conv(gl, L["ff2"], L["ff2b"], inner, 1, res=h, ksplit=self._ks1(x, 4 * inner, inner))
        return ops.conv(h, d["w_out"], d["b_out"], c, 1, res=x, want_stats=True, ksplit=self._ks1(x, inner, c))

    def _run_seq(self, pr, seq, h, skip, emb, kvs, n_ctx, x_nchw=None, skip_ids=()):
        first = True
        for blk in seq:
            d = pr.blocks[blk.prefix]
            if isinstance(blk, SDStemSpec):
                h = blocks.stem(d, x_nchw, blk.cout, self.compute_dtype)
            elif isinstance(blk, SDResBlockSpec):
                h = self._resblock(pr, blk, h, skip if first else None, emb, blk.layer_id in skip_ids)
            elif isinstance(blk, SDTransformerSpec):
                if blk.layer_id not in skip_ids:   # dynamic_unet.py:316-318: a skipped attention-type layer returns x
                    h = self._transformer(pr, blk, h, kvs, n_ctx)
            elif isinstance(blk, SDDownSpec):
                if STRIDE2_TAPS:   # the 9 taps at the output pixels only (general conv2d kernel, csrc/adm_convg.hip)
                    h = ops.conv2d(h, d["w2d"], d["b"], 3, 3, stride=2, pad=(1, 1), relu=False)
                else:              # stride-1 conv + every-second-pixel pick: 4 x the MACs on the faster tile kernel
                    h = ops.resample(ops.conv(h, d["w"], d["b"], blk.channels, 9), "stride2")
            elif isinstance(blk, SDUpSpec):
                h = blocks.upsample_conv(d, h, blk.channels, self.upconv_phases)
            else:
                raise TypeError(blk)
            first = False
        return h

    # ------------------------------------------------------------------ forward
    use_graph = False  # replay one captured hipGraph per input shape (set by .enable_graph())

    fold_skip = os.environ.get("ADM_FOLD_SKIP", "1") != "0"   # ResBlock skip_connection inside the out_layers conv's K loop (read when the weights are packed)
    fuse_geglu = os.environ.get("ADM_SD_FUSE_GEGLU", "1") != "0"   # GEGLU in the C -> 8C projection's epilogue (per model, never by batch)
    small_batch_splitk = False  # split the K loop of the 8x8 / 16x16-level 3x3 convs (set by .enable_splitk())
    upconv_phases = ops.UPCONV_PHASES   # Upsample convs as four 2x2-tap phase convs (a per-model choice, never by batch)

    def enable_upconv_phases(self, on: bool = True):
        self.upconv_phases = bool(on)
        if self._packed is not None:
            self._packed.graphs = {}
            self._packed.skip_graphs = OrderedDict()
        return self

    def enable_splitk(self, flag: bool = True):
        """For the search's batch (n_samples 6, i.e. 6-latent half batches under guidance): the 3x3 convs of the 8x8 and
        16x16 levels launch 30-60 tiles with 40-80-chunk K loops on 256 CUs; their K loops are cut into 4 / 2 runs that go
        out as separate tiles (`ops.splitk_for`: by shape only, so results do not depend on the batch size) and a reduce
        pass adds them.  Changes the fp32 summation order of those layers (deterministic; the parity tests hold either way)."""
        self.small_batch_splitk = bool(flag)
        return self

    def _ks(self, t, cin):
        return ops.splitk_for(t.shape[1], t.shape[2], cin) if self.small_batch_splitk else 1

    def _ks1(self, t, cin, cout):   # the transformer's wide 1x1 projections at 16x16 / 8x8 (ops.splitk_1x1_for)
        return ops.splitk_1x1_for(t.shape[1], t.shape[2], cin, cout) if self.small_batch_splitk and SPLITK_1X1 else 1

    def enable_graph(self, flag: bool = True):
        """Capture the ~700 launches of one evaluation in a hipGraph per (latent shape, context shape) and replay it:
        at the reference's batch (n_samples 6 x 2 for classifier-free guidance) the eager path is bound by the host's
        launch rate, not by the GPU.  Outputs are bit-identical to the eager path."""
        self.use_graph = bool(flag)
        return self

    # ------------------------------------------------------------------ layer-skip sets and their graphs
    # A layer-skip set is another launch sequence, hence another captured graph per (shape, stream).  Graphs of the empty set
    # stay in pr.graphs as before; those of non-empty sets live in pr.skip_graphs, an LRU bounded as unet.py's plan_graphs /
    # _graphed bound the ADM cache: SKIP_GRAPH_CACHE graphs, raised to the announced candidate's needs up to
    # SKIP_GRAPH_CACHE_MAX, and never more than GRAPH_POOL_FRACTION of the device's memory in private pools.
    SKIP_GRAPH_CACHE = 12
    SKIP_GRAPH_CACHE_MAX = 32
    GRAPH_POOL_FRACTION = float(os.environ.get("ADM_GRAPH_POOL_FRACTION", "0.45"))
    _graph_eager = False    # the announced candidate's skip sets do not fit: its skipped evaluations launch eagerly
    _planned_graphs = 1
    _pool_bytes_seen = 0    # largest private pool a capture of a skipped evaluation has needed so far

    @property
    def layer_num(self) -> int:
        return self.plan.layer_num

    def _skip_key(self, skip_layer) -> tuple:
        """The sorted tuple of distinct ids; an id outside range(layer_num) raises before anything is launched."""
        ids = [] if skip_layer is None else list(skip_layer)
        for v in ids:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < self.plan.layer_num:
                raise ValueError(f"skip_layer: {v!r} is not a layer id of this UNet (range({self.plan.layer_num}))")
        return tuple(sorted({int(v) for v in ids}))

    def _graph_budget(self) -> int:
        dev = self.device
        return int(self.GRAPH_POOL_FRACTION * torch.cuda.get_device_properties(dev).total_memory) if dev.type == "cuda" else 0

    def plan_graphs(self, distinct_sets: int, streams: int = 1):
        """Called per candidate (SDCandidateEvaluator) with the number of DISTINCT non-empty layer-skip sets of its steps and the
        number of streams each is evaluated from (2 under split guidance: a graph belongs to one launching stream).  The LRU
        grows to hold them all, up to SKIP_GRAPH_CACHE_MAX graphs and GRAPH_POOL_FRACTION of the device's memory in pools (the
        pool of a capture is known after the first one; forward() re-checks at every capture); beyond either bound the
        candidate's skipped evaluations launch eagerly, with one log line -- an LRU smaller than the candidate's needs would
        recapture at every step of every batch."""
        from . import logger
        sets = max(0, int(distinct_sets))
        need = max(1, sets * max(1, int(streams)))
        self._planned_graphs = need
        too_many = need > self.SKIP_GRAPH_CACHE_MAX
        too_big = self._pool_bytes_seen > 0 and need * self._pool_bytes_seen > self._graph_budget()
        if not (too_many or too_big):
            self.SKIP_GRAPH_CACHE = max(type(self).SKIP_GRAPH_CACHE, need)
            self._graph_eager = False
        else:
            if not self._graph_eager and self.use_graph:
                why = (f"{sets} distinct layer-skip sets x {max(1, int(streams))} stream(s) > {self.SKIP_GRAPH_CACHE_MAX} cached graphs"
                       if too_many else f"{need} graphs x {self._pool_bytes_seen / 1e9:.2f} GB of private pool > "
                                        f"{self._graph_budget() / 1e9:.0f} GB budget")
                logger.log(f"hipGraph replay off for this candidate's skipped evaluations: {why} (eager launches instead of "
                           "recapturing every step)")
            self._graph_eager = True
        return self

    def _context_kv(self, pr, context, n):
        """The k|v projections of every cross-attention layer: they depend on the conditioning only.  The tokens ride as a
        bf16 pixel map (8x16 or 16x16, zero rows beyond S) so that the projections are 1x1 convs.  Transformers that a step's
        skip list leaves out are projected too: this runs once per sample() call, whose steps may skip different layers, and the
        graphs take the projections as a fixed list of static inputs."""
        plan: SDUNetPlan = self.plan
        if context is None or context.dim() != 3 or context.shape[2] != plan.context_dim or context.shape[0] != n:
            raise AdmError(f"context must be [N = {n}, S, {plan.context_dim}]")
        s_ctx = context.shape[1]
        if s_ctx > 256:
            raise NotImplementedError("more than 256 conditioning tokens")
        if not context.is_cuda:
            raise AdmError("latent UNetModel.forward: context must be a device tensor (no CPU fallback)")
        with torch.no_grad():
            rows = 128 if s_ctx <= 128 else 256
            ctx_map = torch.zeros((n, rows, plan.context_dim), dtype=self.compute_dtype, device=context.device)
            ctx_map[:, :s_ctx] = context.to(self.compute_dtype)
            ctx_map = ctx_map.view(n, rows // 16, 16, plan.context_dim)
            kvs = {}
            for b in plan.all_blocks():
                if isinstance(b, SDTransformerSpec):
                    d = pr.blocks[b.prefix]
                    hd = b.heads * d["dp"]
                    for li, L in enumerate(d["layers"]):
                        kvs[(b.prefix, li)] = ops.conv(ctx_map, L["kv2"], pr.zero_bias, 2 * hd, 1)
        return kvs

    def _kv_for(self, pr, context, n, context_key):
        """context_key: a token under which the CALLER guarantees the conditioning does not change (the samplers pass one
        per sample() call: a candidate's K steps share their conditioning); None = recompute."""
        if context_key is None:
            return self._context_kv(pr, context, n), True
        ck = (context_key, tuple(context.shape))
        sid = torch.cuda.current_stream(context.device).cuda_stream  # per launching stream: see forward()
        if pr.kv_cache is None:
            pr.kv_cache = {}
        hit = pr.kv_cache.get(sid)
        if hit is None or hit[0] != ck:
            hit = pr.kv_cache[sid] = (ck, self._context_kv(pr, context, n))
            return hit[1], True
        return hit[1], False

    accepts_context_key = True

    def forward(self, x, timesteps=None, context=None, y=None, context_key=None, skip_layer: Sequence[int] = (), **kwargs):
        """x fp32 [N, C, H, W] latents, timesteps [N], context [N, S, context_dim] -> fp32 [N, out, H, W].
        skip_layer: layer ids (sd_arch: range(layer_num)) whose body this evaluation bypasses."""
        skip = self._skip_key(skip_layer)
        pr = self._packed or self._prepare()
        if not x.is_cuda:
            raise AdmError("latent UNetModel.forward: x must be a device tensor (no CPU fallback)")
        n = x.shape[0]
        kvs, fresh = self._kv_for(pr, context, n, context_key)
        if not self.use_graph or (skip and self._graph_eager):
            return self._forward(x, timesteps, kvs, context.shape[1], y, skip)
        if not timesteps.is_cuda:
            raise AdmError("latent UNetModel (graph mode): timesteps must be a device tensor")
        # one captured graph (hipGraphExec + static input / output buffers + private allocator pool) per input shape AND
        # per launching stream: the same entry replayed from two streams would put one exec in flight twice and race its
        # static buffers (the memory fault recorded in round 1 when two half-batches were replayed concurrently).  With
        # the stream in the key, evaluations on different streams own disjoint graphs and may overlap; replays on one
        # stream serialise by stream order.
        # the launch-sequence switches are part of the key: toggling one after the first replay must not keep the old capture
        key = (tuple(x.shape), x.dtype, tuple(timesteps.shape), timesteps.dtype, tuple(context.shape),
               torch.cuda.current_stream(x.device).cuda_stream, self.small_batch_splitk, self.upconv_phases, self.fuse_geglu)
        if skip:   # ... and so is a non-empty layer-skip set; the empty set keeps the key and the cache it has always had
            key += (skip,)
        cache = pr.skip_graphs if skip else pr.graphs
        entry = cache.get(key)
        if entry is None:   # static inputs: x, timesteps, then the k|v projections in the order of kvs
            names = list(kvs)
            graph, static_in, so, pool = blocks.capture_graph(
                lambda x_, t_, *kv: self._forward(x_, t_, dict(zip(names, kv)), context.shape[1], y, skip), (x, timesteps, *kvs.values()))
            entry = cache[key] = [graph, static_in, so, None]   # None: the k|v dict the static buffers were last filled from
            fresh = True
            if skip:
                entry.append(pool)
                self._pool_bytes_seen = max(self._pool_bytes_seen, pool)
                budget = self._graph_budget()
                while len(cache) > 1 and (len(cache) > self.SKIP_GRAPH_CACHE or sum(e[4] for e in cache.values()) > budget):
                    torch.cuda.synchronize(x.device)   # a graph of any stream may still be replaying out of the pool that is freed here
                    cache.popitem(last=False)
                if self._planned_graphs * pool > budget:
                    # this candidate's launch sequences do not fit together: replay this one, then go eager (plan_graphs logs why)
                    res = blocks.replay_graph(*entry[:3], (x, timesteps, *kvs.values()))
                    torch.cuda.synchronize(x.device)   # the replay reads the pool that goes with the graph
                    cache.pop(key, None)
                    self.plan_graphs(self._planned_graphs)
                    return res
        elif skip:
            cache.move_to_end(key)
        ins = (x, timesteps)
        if fresh or entry[3] is not kvs:  # the graph reads its own k|v buffers: refill them only when the conditioning changed
            ins += tuple(kvs.values())
            entry[3] = kvs if context_key is not None else None
        return blocks.replay_graph(*entry[:3], ins)

    def _forward(self, x, timesteps, kvs, s_ctx, y=None, skip_ids=()):
        assert y is None, "must specify y if and only if the model is class-conditional"
        pr = self._packed or self._prepare()
        plan: SDUNetPlan = self.plan
        x = x.to(torch.float32).contiguous()
        with torch.no_grad():
            e = ops.timestep_embedding(timesteps, plan.model_channels)
            e = ops.linear_f32(e, pr.te0_w, pr.te0_b)
            e = ops.linear_f32(e, pr.te2_w, pr.te2_b, silu_in=True)
            emb = ops.linear_f32(e, pr.emb_w, pr.emb_b, silu_in=True)  # every ResBlock's emb_layers at once
            h = blocks.u_walk(plan, lambda seq, h, skip: self._run_seq(pr, seq, h, skip, emb, kvs, s_ctx, x_nchw=x, skip_ids=skip_ids))
            return blocks.head(pr.head, h, plan.out_channels)
