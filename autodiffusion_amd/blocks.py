"""The straight-line launch sequences the ADM UNet / classifier (unet.py, classifier.py), the latent UNet (sd_unet.py) and the
KL-f8 decoder (sd_vae.py) have in common, once: stateless functions over packed-weight dicts.  What differs between the
networks arrives as data (state-dict key names, eps, ksplit, whether the fold is allowed, res_up); nothing here asks which
network is calling.  Every launch goes through ``ops.<name>(...)`` so that the launch recorders and ``ops.CONV_PROFILE``,
which patch attributes of the ops module, see it.
"""
from __future__ import annotations

import torch

from . import ops

ADM_RES_KEYS = ("in_layers.0", "in_layers.2", "out_layers.0", "out_layers.3", "skip_connection")   # guided_diffusion / ldm openaimodel
VAE_RES_KEYS = ("norm1", "conv1", "norm2", "conv2", "nin_shortcut")                                # ldm model.py ResnetBlock


# ------------------------------------------------------------------ weight preparation
def packers(P, cd):
    """-> (f32, pack): state-dict key -> contiguous fp32 tensor; conv weight -> the kernels' packed image in the torso type."""
    return (lambda k: P[k].to(torch.float32).contiguous()), (lambda w: ops.pack_conv_weight(w, cd))


def stem_weights(P, f32, pack, p, cin, cout):
    # stem on the MFMA conv kernel: input channels zero-padded to one 32-channel chunk
    wpad = torch.zeros((cout, 32, 3, 3), dtype=torch.float32, device=P[f"{p}.weight"].device)
    wpad[:, :cin] = P[f"{p}.weight"].to(torch.float32)
    return dict(w=pack(wpad), b=f32(f"{p}.bias"))


def resblock_weights(P, f32, pack, p, keys, has_skip, fold):
    """keys: the names of (GroupNorm 1, conv 1, GroupNorm 2, conv 2, the 1x1 skip) under prefix p; fold: also pack the skip as
    extra K-steps of conv 2 (resblock_tail launches it where the map allows)."""
    n1, c1, n2, c2, sk = keys
    d = dict(g1=f32(f"{p}.{n1}.weight"), b1=f32(f"{p}.{n1}.bias"), w1=pack(P[f"{p}.{c1}.weight"]), c1b=f32(f"{p}.{c1}.bias"),
             g2=f32(f"{p}.{n2}.weight"), b2=f32(f"{p}.{n2}.bias"), w2=pack(P[f"{p}.{c2}.weight"]), c2b=f32(f"{p}.{c2}.bias"))
    if has_skip:
        d["ws"], d["wsb"] = pack(P[f"{p}.{sk}.weight"]), f32(f"{p}.{sk}.bias")
        if fold:   # skip_connection as extra K-steps of the out_layers conv (ops.conv(fold=))
            d["w2f"] = ops.fold_weights(d["w2"], d["ws"])
            d["c2fb"] = (d["c2b"] + d["wsb"]).contiguous()
    return d


def upsample_weights(P, f32, pack, p, cd):
    # conv3x3(nearest 2x): the virtual-upsample conv, and its four 2x2-tap phase convs (ops.pack_conv_weight_up)
    return dict(w=pack(P[f"{p}.weight"]), b=f32(f"{p}.bias"), w_up=ops.pack_conv_weight_up(P[f"{p}.weight"], cd))


def head_weights(P, f32, pack, norm, conv):
    return dict(g=f32(f"{norm}.weight"), b=f32(f"{norm}.bias"), w=pack(P[f"{conv}.weight"]), cb=f32(f"{conv}.bias"))


# ------------------------------------------------------------------ launches
def stem(d, x_nchw, cout, cd):
    return ops.conv(ops.nchw_to_nhwc_pad(x_nchw, 32, cd), d["w"], d["b"], cout, 9, want_stats=True)


def resblock_tail(d, cout, h, aff2, xs, xs1=None, fold=True, ksplit=1, res_up=False):
    """`skip_connection(x) + out_layers(h)`: h is the first conv's output, aff2 the second GroupNorm's affine, (xs | xs1) the block
    input; fold=False keeps the 1x1 launch where the caller's schedule (resampled input, split-K) rules the folded conv out."""
    if "ws" in d:
        if fold and "w2f" in d and ops.fold_ok(h.shape[1], h.shape[2]):
            # `self.skip_connection(x) + h` (reference unet.py:256, openaimodel.py:262) inside the out_layers conv as extra one-tap
            # K-steps (adm_conv_args.fold0): no 1x1 launch, no residual operand
            return ops.conv(h, d["w2f"], d["c2fb"], cout, 9, aff=aff2, silu=True, fold=(xs, xs1), want_stats=True)
        res = ops.conv(xs, d["ws"], d["wsb"], cout, 1, x1=xs1)
    else:
        res = xs
    return ops.conv(h, d["w2"], d["c2b"], cout, 9, aff=aff2, silu=True, res=res, res_up=res_up, want_stats=True, ksplit=ksplit)


def attention(d, x, heads, new_order, eps=None):
    """Single-projection attention block: gn -> fused qkv 1x1 [affine prologue] -> attention -> proj 1x1 (+x)."""
    n, hh, ww, c = x.shape
    aff = ops.gn_affine(x, d["g"], d["b"], eps=eps)
    qkv = ops.conv(x, d["wqkv"], d["bqkv"], 3 * c, 1, aff=aff, silu=False)
    a = ops.attention(qkv.view(n, hh * ww, 3 * c), heads, new_order)
    return ops.conv(a.view(n, hh, ww, c), d["wproj"], d["bproj"], c, 1, res=x, want_stats=True)


def upsample_conv(d, x, channels, phases):
    """Upsample with a conv: conv3x3 reading x through the virtual nearest 2x upsample.  phases: as the four 2x2-tap phase convs
    in one launch (adm_conv_args.up_phase = 5; from 16x16 sources up): 4/9 of the MACs, x 1.5 on ADM at batch 256, x 1.2-1.3 on
    the latent UNet's layers at the search's 6-latent half batches (tools/upconv_bench.py)."""
    if x.shape[1] >= 8 and x.shape[2] >= 8:
        return ops.conv(x, d["w"], d["b"], channels, 9, in_up=True, want_stats=True, w_up=d["w_up"] if phases else None)
    return ops.conv(ops.resample(x, "up"), d["w"], d["b"], channels, 9, want_stats=True)   # maps below 8x8: materialised


def head(hd, h, cout, eps=None):
    aff = ops.gn_affine(h, hd["g"], hd["b"], eps=eps)
    return ops.conv(h, hd["w"], hd["cb"], cout, 9, aff=aff, silu=True, out_f32_nchw=True)


def u_walk(plan, run_seq):
    """run_seq(seq, h, skip) -> h over input_blocks (outputs pushed), middle_block, output_blocks (each with the popped skip)."""
    hs, h = [], None
    for seq in plan.input_blocks:
        h = run_seq(seq, h, None)
        hs.append(h)
    h = run_seq(plan.middle_block, h, None)
    for seq in plan.output_blocks:
        h = run_seq(seq, h, hs.pop())
    return h


# ------------------------------------------------------------------ hipGraph capture and replay
def _graph_pool_bytes(graph, dev, reserved0, free0) -> int:
    """Bytes of the private allocator pool a just-captured graph owns: the segments tagged with the graph's pool id in the caching
    allocator's snapshot; if the snapshot does not tell (older / newer torch), the growth of reserved memory or the drop of free
    device memory across the capture, whichever is larger."""
    try:
        pid = tuple(graph.pool())
        got = sum(seg["total_size"] for seg in torch.cuda.memory_snapshot() if tuple(seg.get("segment_pool_id", (0, 0))) == pid
                  and seg.get("device", dev.index) == dev.index)
        if got > 0:
            return int(got)
    except Exception:
        pass
    return int(max(0, torch.cuda.memory_reserved(dev) - reserved0, free0 - torch.cuda.mem_get_info(dev)[0]))


def capture_graph(fn, inputs):
    """Capture fn(*inputs) -> tensor or tuple of tensors on clones of the device tensors `inputs`
    -> (graph, static inputs, static output, bytes of the graph's private pool)."""
    dev = inputs[0].device
    static_in = [t.clone() for t in inputs]
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):  # first calls size per-kernel attributes; they must not land in the capture
        for _ in range(2):
            fn(*static_in)
    cur.wait_stream(side)
    reserved0, free0 = torch.cuda.memory_reserved(dev), torch.cuda.mem_get_info(dev)[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(*static_in)
    return graph, static_in, out, _graph_pool_bytes(graph, dev, reserved0, free0)


def replay_graph(graph, static_in, out, inputs):
    """Copy `inputs` over the static ones, replay, clone the output.  `inputs` may be a prefix of the static inputs: the rest
    keep what an earlier replay put there."""
    for s_, t in zip(static_in, inputs):
        s_.copy_(t)
    graph.replay()
    return tuple(o.clone() for o in out) if isinstance(out, tuple) else out.clone()
