"""Launch recorder, float64 restatements and per-element error bounds of the Inception-v3 extractor's kernels
(csrc/adm_convg.hip) for tests/test_hip_inception_replay.py; the host checks are tests/test_inception_replay_host.py.

Recording: ops.conv2d / pool2d / resize_bilinear / global_avgpool_f32 are patched (pytest's monkeypatch); a record is hashable
and pointer-free -- shapes, channel strides, the channel offset of `out` inside its parent tensor, flags.  With keep=True the
recorder also keeps each call's actual tensors (the assembled network, layer by layer).

Restatement: the op in float64 (torch float64 ops on the tensors' own device) on the operands exactly as the kernel sees them:
T-rounded activations, the packed weights read back (and checked on their own: `packing` below), fp32 bias; the resize takes the source coordinate in fp32 by the kernel's own expression
(resize_coords; both references compute it in fp32: with float64 coordinates the result moves by up to 5e-5 at 512 pixels, a fifth of half an
fp16 ulp, which would need a bound loose enough to hide a rounding defect) and interpolates in float64.

Per-element bounds, u = 2^-8 (bf16) or 2^-11 (fp16), ulp_T(v) = 2u * 2^floor(log2 |v|) (launch_replay.ulp_t):
  conv2d     on the pre-ReLU value z = sum_k w_k x_k + bias (ReLU is 1-Lipschitz):
             |got - relu(ref)| <= ulp_T(|z|) + (K + 2) 2^-24 sum_k |w_k x_k|,   K = taps x cin_pad
             -- launch_replay's conv bound without its prologue and residual terms: one rounding to T, fp32 accumulation of K
             products and the bias add.  On deep layers (K ~ 18000) the second term reaches several fp16 ulps: the Frobenius
             bound is the tight check there.
  pool2d     max: equal as values to the max of the T values, no tolerance (+0 == -0).
             avg (count_include_pad=False): ulp_T(|ref|) / 2 + 16 x 2^-24 mean|x| over the counted taps: at most 9 fp32 adds and
             one multiply by the fp32 reciprocal of the count (each within 2^-24 of the running magnitude, <= 9 mean|x|), then
             one round-to-nearest to T.  ulp_t's floor (fp16 subnormal spacing, zero) carries over; where the fp32 value rounds
             across a binade edge the result is the edge itself, within the lower binade's half ulp of ref.
  gap        global_avgpool_f32 (fp32 output): (hw + 1) 2^-24 mean|x|: hw fp32 adds and one multiply.
  resize     ulp_T(|ref|) / 2 + 8 x 2^-24 (|scale| max|pixel| + |shift|): six fp32 multiply-adds of the two lerps, the scale and
             the shift on values <= max|pixel|, then one round-to-nearest; with fp32 coordinates the fp32 interpolation stays
             within 2^-22 of float64 on outputs in [-1, 1] at every size.  Channels 3.. exactly zero.
  packing    adm_pack_conv2d_weight on fp32 w and scale: the exact product w s has 48 bits, and a packed weight must be a correct
             rounding of it -- equal to round_T(fl32(w s)) (two roundings: the bf16 build's multiply, then convert) or at least
             as close to w s as that value is (one rounding: the fp16 build's fused multiply-convert, which differs from the
             former on ~2^-13 of the weights).  No ulp of slack: a truncating or bf16-rounded packing fails on about half the
             weights.  Channels beyond cin exactly zero.
  fold       w_packed against round_T(w gamma / sqrt(var + 1e-3)) from float64: at most one ulp_T(|w|) apart (fp32 fold, one
             rounding); bias against beta - mean gamma / sqrt(var + 1e-3) within 4 x 2^-24 (|beta| + |mean gamma / sqrt(..)|).
  Frobenius  ||got - ref|| / ||ref|| <= launch_replay.fro_bound(1, u) = 0.6 u on the conv outputs: one rounding to T has an RMS
             relative error of at most u / sqrt(3) ~ 0.58 u.  This is what catches a truncating output conversion (0.85 u),
             which stays inside the per-element bound.
Every byte of a sliced output's parent tensor outside the slice must keep its sentinel, bit for bit.

Compared conv elements: the whole tensor where M x cout <= 2^22; else all channels of (a) the first and last pixel of every
64-pixel run of the flattened (image, oy, ox) index -- the wave tile of all three kernels, hence every 128- and 256-pixel block
edge -- (b) the border ring of the first, the last and one seeded image, (c) seeded random pixels.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from launch_replay import FRO_U, KIND_DTYPE, U, fro_bound, round_t, ulp_t  # noqa: F401  (shared with the sampling-side replay)

SENTINEL = -1234.0
FULL_BELOW = 1 << 22
LAYOUTS = {0: "u8_nhwc", 1: "f32_nchw", 2: "f32_nhwc"}
DTYPE_KIND = {v: k for k, v in KIND_DTYPE.items()}


# ------------------------------------------------------------------ the kernel adm_conv2d picks
def conv_kernel_pick(cout: int, no_lds: bool = False) -> str:
    """The pick of adm_conv2d, from cout alone (csrc/adm_convg.hip): block width by least padding."""
    pad128, pad64, pad32 = (cout + 127) // 128 * 128, (cout + 63) // 64 * 64, (cout + 31) // 32 * 32
    if cout > 32 and not no_lds:
        return "convg_lds_kernel<2,2>" if pad128 == pad64 else "convg_lds_kernel<4,1>"
    return "convg_kernel<2>" if pad32 < pad64 else "convg_kernel<4>"


def block_width(pick: str) -> int:
    return {"convg_lds_kernel<2,2>": 128, "convg_lds_kernel<4,1>": 64, "convg_kernel<2>": 32, "convg_kernel<4>": 64}[pick]


# ------------------------------------------------------------------ recording
def _rec(op, kind, d):
    return (op, kind) + tuple(sorted(d.items()))


def record_dict(rec: tuple) -> dict:
    return dict(rec[2:])


def _slice_of(out, c):
    """(channel stride, channel offset inside the parent) of an NHWC tensor or channel slice of a dense parent."""
    if out is None:
        return c, 0
    cs = out.stride(2)
    off = out.storage_offset()
    if off >= cs or off + c > cs:
        raise NotImplementedError(f"out is not a channel slice of a dense NHWC tensor at storage offset 0 (offset {off}, stride {cs})")
    return cs, off


def conv2d_record(cin_cache: dict, x, w_packed, bias, kh, kw, stride, pad, relu, out) -> tuple:
    """The record of one ops.conv2d call (also taken by launch_replay.Recorder for the UNets' stride-2 convs); cin_cache keeps
    each weight's cin: the last input channel with a non-zero weight."""
    n, h, w, _ = x.shape
    cout, taps, cin_pad = w_packed.shape
    key = (w_packed.data_ptr(), tuple(w_packed.shape))
    if key not in cin_cache:
        cin_cache[key] = int((w_packed != 0).any(0).any(0).nonzero().max()) + 1
    os_, off = _slice_of(out, cout)
    return _rec("conv2d", DTYPE_KIND[x.dtype], dict(
        n=n, h=h, w=w, in_stride=x.stride(2), cin=cin_cache[key], cin_pad=cin_pad, cout=cout, kh=kh, kw=kw, stride=stride,
        ph=pad[0], pw=pad[1], relu=bool(relu), has_bias=bias is not None, out_stride=os_, out_off=off))


class Recorder:
    """Patches the four Inception entry points of ops.  records: the distinct launches; calls (keep=True): every call's
    (op, record, tensors) in order."""

    def __init__(self, monkeypatch, keep: bool = False):
        from autodiffusion_amd import ops
        self.records, self.counts, self.calls, self.keep = set(), {}, [], keep
        self._cin = {}
        o_conv, o_pool, o_resize, o_gap = ops.conv2d, ops.pool2d, ops.resize_bilinear, ops.global_avgpool_f32

        def conv2d(x, w_packed, bias, kh, kw, stride=1, pad=(0, 0), relu=True, out=None):
            rec = conv2d_record(self._cin, x, w_packed, bias, kh, kw, stride, pad, relu, out)
            res = o_conv(x, w_packed, bias, kh, kw, stride, pad, relu, out)
            self._add(rec, x=x, w_packed=w_packed, bias=bias, out=res)
            return res

        def pool2d(x, k, stride, pad, mode, out=None):
            n, h, w, c = x.shape
            os_, off = _slice_of(out, c)
            rec = _rec("pool2d", DTYPE_KIND[x.dtype], dict(n=n, h=h, w=w, c=c, in_stride=x.stride(2), k=k, stride=stride, pad=pad,
                                                           mode=mode, out_stride=os_, out_off=off))
            res = o_pool(x, k, stride, pad, mode, out)
            self._add(rec, x=x, out=res)
            return res

        def resize_bilinear(images, oh, ow, cpad, layout, half_pixel, scale, shift, dtype=torch.float16):
            kind = {v: k for k, v in LAYOUTS.items()}[layout]
            h, w = (images.shape[2], images.shape[3]) if kind == 1 else (images.shape[1], images.shape[2])
            rec = _rec("resize", DTYPE_KIND[dtype], dict(n=images.shape[0], h=h, w=w, oh=oh, ow=ow, cpad=cpad, kind=kind,
                                                         half_pixel=bool(half_pixel), scale=float(scale), shift=float(shift)))
            res = o_resize(images, oh, ow, cpad, layout, half_pixel, scale, shift, dtype)
            self._add(rec, x=images, out=res)
            return res

        def global_avgpool_f32(x):
            n, h, w, c = x.shape
            rec = _rec("gap", DTYPE_KIND[x.dtype], dict(n=n, h=h, w=w, c=c))
            res = o_gap(x)
            self._add(rec, x=x, out=res)
            return res

        for name, fn in (("conv2d", conv2d), ("pool2d", pool2d), ("resize_bilinear", resize_bilinear),
                         ("global_avgpool_f32", global_avgpool_f32)):
            monkeypatch.setattr(ops, name, fn)

    def _add(self, rec, **tensors):
        self.records.add(rec)
        self.counts[rec[0]] = self.counts.get(rec[0], 0) + 1
        if self.keep:
            self.calls.append((rec, tensors))


# ------------------------------------------------------------------ families (coverage guard)
def families(rec: tuple) -> set:
    op, kind, d = rec[0], rec[1], record_dict(rec)
    out = set()
    if op == "conv2d":
        pick = conv_kernel_pick(d["cout"])
        out.add(pick)
        ks = f"{d['kh']}x{d['kw']}"
        out.add(f"{ks} s{d['stride']}" if ks == "3x3" else ks)
        if d["cout"] % 128:                     # not whole 128-wide blocks: the pick matters, and where cout % block_width(pick)
            out.add(f"cout {d['cout']}")        # (48, 80, 96) the last block is partly beyond cout
        if d["out_stride"] != d["cout"]:
            out.add("sliced output")
        if conv_out_hw(d)[0] * conv_out_hw(d)[1] * d["n"] % 256:
            out.add("M % 256 != 0")
    elif op == "pool2d":
        out.add(f"pool {d['mode']} {d['k']}/{d['stride']}/{d['pad']}" + (" sliced" if d["out_stride"] != d["c"] else ""))
    elif op == "resize":
        out.add("resize half_pixel" if d["half_pixel"] else "resize tf1")
    else:
        out.add(op)
    return {(kind, f) for f in out}


REQUIRED_FAMILIES = (["convg_lds_kernel<2,2>", "convg_lds_kernel<4,1>", "convg_kernel<2>",
                      "1x1", "3x3 s1", "3x3 s2", "5x5", "1x7", "7x1", "1x3", "3x1",
                      "cout 80", "cout 48", "cout 96", "cout 320", "sliced output", "M % 256 != 0",
                      "pool max 3/2/0", "pool max 3/2/0 sliced", "pool avg 3/1/1", "pool max 3/1/1",
                      "resize half_pixel", "resize tf1", "gap"])
REPLAYED = {"conv2d", "pool2d", "resize", "gap"}


# ------------------------------------------------------------------ pixel sampler
def conv_out_hw(d: dict):
    return (d["h"] + 2 * d["ph"] - d["kh"]) // d["stride"] + 1, (d["w"] + 2 * d["pw"] - d["kw"]) // d["stride"] + 1


def ring_images(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return sorted({0, n - 1, int(torch.randint(0, n, (1,), generator=g))})


def sample_pixels(n: int, oh: int, ow: int, cout: int, seed: int, extra: int = 2048) -> torch.Tensor:
    """Sorted flattened (image, oy, ox) indices to restate (see the module docstring)."""
    m_tot = n * oh * ow
    if m_tot * cout <= FULL_BELOW:
        return torch.arange(m_tot)
    first = torch.arange(0, m_tot, 64)
    parts = [first, (first + 63).clamp(max=m_tot - 1)]
    yy, xx = torch.meshgrid(torch.arange(oh), torch.arange(ow), indexing="ij")
    edge = (yy == 0) | (yy == oh - 1) | (xx == 0) | (xx == ow - 1)
    ring = (yy * ow + xx)[edge]
    for img in ring_images(n, seed):
        parts.append(img * oh * ow + ring)
    g = torch.Generator().manual_seed(seed + 1)
    parts.append(torch.randint(0, m_tot, (extra,), generator=g))
    return torch.unique(torch.cat(parts))


# ------------------------------------------------------------------ conv2d
def conv_restate(x, wq, bias, d: dict, m: torch.Tensor):
    """float64 z = sum_k w_k x_k (+ bias) and S = sum_k |w_k x_k| at the flattened output pixels m -> ([P, cout], [P, cout]).
    x: [n, h, w, >= cin_pad] holding T values; wq: [cout, taps, cin_pad] holding T values (the packed layout)."""
    dev = x.device
    oh, ow = conv_out_hw(d)
    m = m.to(dev)
    img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
    h, w, cp = d["h"], d["w"], d["cin_pad"]
    cols = []
    for ky in range(d["kh"]):
        for kx in range(d["kw"]):
            iy, ix = oy * d["stride"] - d["ph"] + ky, ox * d["stride"] - d["pw"] + kx
            ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
            v = x[img, iy.clamp(0, h - 1), ix.clamp(0, w - 1), :cp].double()
            cols.append(v * ok[:, None].to(v.dtype))
    pa = torch.stack(cols, 1).reshape(m.numel(), -1)            # [P, taps * cin_pad], tap-major like the packed weights
    wm = wq.double().reshape(wq.shape[0], -1)
    z, s = pa @ wm.T, pa.abs() @ wm.abs().T
    if bias is not None:
        z = z + bias.double()
    return z, s


def conv_bound(z, s, d: dict, dtype):
    return ulp_t(z, dtype) + (d["kh"] * d["kw"] * d["cin_pad"] + 2) * 2.0 ** -24 * s


def reference_weights(w32, scale, cin_pad: int, dtype):
    """round_T(fp32 w x fp32 scale) in the packed [cout][kh*kw][cin_pad] layout, channels beyond cin zero (float32 tensor)."""
    cout, cin, kh, kw = w32.shape
    ws = w32.float() if scale is None else w32.float() * scale.float().view(-1, 1, 1, 1)
    wq = round_t(ws, dtype).permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    return F.pad(wq, (0, cin_pad - cin))


def packing_errors(packed, w32, scale, dtype) -> int:
    """Number of packed weights [cout, taps, cin_pad] that are not a correct rounding of the exact product w32 x scale (see the
    module docstring), plus the number of non-zero pad channels."""
    cout, cin, kh, kw = w32.shape
    e = w32.double() if scale is None else w32.double() * scale.double().view(-1, 1, 1, 1)    # exact: 24 x 24 bits
    e = e.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    twice = e.float().to(dtype).double()
    got = packed[..., :cin].double()
    ok = (got == twice) | ((got - e).abs() <= (twice - e).abs())
    return int((~ok).sum()) + int((packed[..., cin:] != 0).sum())


def sentinel_intact(parent, off: int, c: int) -> bool:
    """Every element of parent [n, h, w, stride] outside channels [off, off + c) still holds the sentinel's bit pattern."""
    bits = torch.full((1,), SENTINEL, dtype=parent.dtype, device=parent.device).view(torch.int16)
    pv = parent.view(torch.int16)
    return bool((pv[..., :off] == bits).all()) and bool((pv[..., off + c:] == bits).all())


def compare_conv(x, wq, bias, d: dict, dtype, out, m, budget: int = 1 << 25):
    """(worst err / bound, relative Frobenius error, report of the worst element) of out [n, oh, ow, cout] at pixels m."""
    oh, ow = conv_out_hw(d)
    kk = d["kh"] * d["kw"] * d["cin_pad"]
    per = max(1, budget // kk)
    worst, num, den, report = 0.0, 0.0, 0.0, ""
    flat = out.reshape(-1, out.shape[3]) if out.is_contiguous() else None
    for i0 in range(0, m.numel(), per):
        mm = m[i0:i0 + per].to(x.device)
        z, s = conv_restate(x, wq, bias, d, mm)
        ref = z.clamp_min(0) if d["relu"] else z
        bound = conv_bound(z, s, d, dtype)
        got = (flat[mm] if flat is not None else out[mm // (oh * ow), (mm // ow) % oh, mm % ow]).double()
        if not torch.isfinite(got).all():
            return float("inf"), float("inf"), "non-finite output"
        err = (got - ref).abs()
        r = err / bound
        rmax = r.max().item()
        if rmax > worst:
            worst = rmax
            j = int(r.argmax())
            p, c = j // r.shape[1], j % r.shape[1]
            mp = int(mm[p])
            report = (f"img {mp // (oh * ow)} y {(mp // ow) % oh} x {mp % ow} ch {c}: got {got[p, c].item():.8g} ref {ref[p, c].item():.8g} "
                      f"bound {bound[p, c].item():.4g}")
        num += (err ** 2).sum().item()
        den += (ref ** 2).sum().item()
    return worst, (num / max(den, 1e-300)) ** 0.5, report


def conv_operands(ops, d: dict, dtype, seed: int, dev):
    """Fresh seeded operands of a recorded conv2d launch -> (x, packed, bias, parent, out, number of wrongly packed weights)."""
    if d["out_off"] + d["cout"] > d["out_stride"] or d["cin"] > d["cin_pad"] or d["cin_pad"] > d["in_stride"]:
        raise NotImplementedError(f"the restatement does not express {d}")
    g = torch.Generator(device=dev).manual_seed(seed)
    n, h, w, cin, cp, cs, cout = d["n"], d["h"], d["w"], d["cin"], d["cin_pad"], d["in_stride"], d["cout"]
    x = torch.zeros((n, h, w, cs), dtype=dtype, device=dev)   # channels cin .. cin_pad: the zeros the network guarantees
    x[..., :cin] = torch.randn((n, h, w, cin), generator=g, device=dev).to(dtype)
    if cs > cp:                                               # beyond cin_pad: never read
        x[..., cp:] = torch.randn((n, h, w, cs - cp), generator=g, device=dev).to(dtype)
    w32 = torch.randn((cout, cin, d["kh"], d["kw"]), generator=g, device=dev) * (cin * d["kh"] * d["kw"]) ** -0.5
    scale = 1 + 0.2 * torch.randn((cout,), generator=g, device=dev)
    bias = 0.3 * torch.randn((cout,), generator=g, device=dev) if d["has_bias"] else None
    packed = ops.pack_conv2d_weight(w32, scale, dtype)
    oh, ow = conv_out_hw(d)
    parent = torch.full((n, oh, ow, d["out_stride"]), SENTINEL, dtype=dtype, device=dev)
    return x, packed, bias, parent, parent[..., d["out_off"]:d["out_off"] + cout], packing_errors(packed, w32, scale, dtype)


def replay_conv(ops, rec: tuple, seed: int, dev):
    """Launch a recorded conv2d again on fresh operands -> (worst err/bound, fro, report); a touched sentinel is worst = inf."""
    d, dtype = record_dict(rec), KIND_DTYPE[rec[1]]
    x, packed, bias, parent, out, misrounded = conv_operands(ops, d, dtype, seed, dev)
    if tuple(packed.shape) != (d["cout"], d["kh"] * d["kw"], d["cin_pad"]) or misrounded:
        return float("inf"), float("inf"), f"{misrounded} packed weights are not a correct rounding of w x scale"
    ops.conv2d(x, packed, bias, d["kh"], d["kw"], d["stride"], (d["ph"], d["pw"]), d["relu"], out=out)
    if dev != "cpu":
        torch.cuda.synchronize()
    if not sentinel_intact(parent, d["out_off"], d["cout"]):
        return float("inf"), float("inf"), "wrote outside its channel slice"
    oh, ow = conv_out_hw(d)
    return compare_conv(x, packed, bias, d, dtype, out, sample_pixels(d["n"], oh, ow, d["cout"], seed))


def conv_label(rec):
    d = record_dict(rec)
    return (f"{rec[1]} n{d['n']} {d['h']}x{d['w']} {d['cin']}({d['cin_pad']}/{d['in_stride']})->{d['cout']} {d['kh']}x{d['kw']} s{d['stride']} "
            f"p{d['ph']},{d['pw']} out {d['out_off']}/{d['out_stride']} {conv_kernel_pick(d['cout'])}")


# ------------------------------------------------------------------ pooling
def pool_restate(x, k: int, stride: int, pad: int, mode: str, dtype):
    """float64 pooling of x [n, h, w, c] (T values) -> (ref, bound) [n, oh, ow, c]; bound is None for max (exact)."""
    n, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xd = x.double()
    fill = float("-inf") if mode == "max" else 0.0
    xp = F.pad(xd, (0, 0, pad, pad, pad, pad), value=fill)
    ones = F.pad(torch.ones((1, h, w, 1), dtype=torch.float64, device=x.device), (0, 0, pad, pad, pad, pad))
    ref = sab = cnt = None
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + (oh - 1) * stride + 1, stride), slice(kx, kx + (ow - 1) * stride + 1, stride))
            v = xp[sl]
            if mode == "max":
                ref = v if ref is None else torch.maximum(ref, v)
            else:
                ref = v if ref is None else ref + v
                sab = v.abs() if sab is None else sab + v.abs()
                cnt = ones[sl] if cnt is None else cnt + ones[sl]
    if mode == "max":
        return ref, None
    ref = ref / cnt
    return ref, 0.5 * ulp_t(ref, dtype) + 16 * 2.0 ** -24 * (sab / cnt)


def compare_pool(x, d: dict, dtype, out, budget: int = 1 << 26):
    """Worst err/bound (max pooling: 0 where equal as values, inf where not) of out against the restatement, whole tensor."""
    per = max(1, budget // (d["h"] * d["w"] * d["c"]))
    worst = 0.0
    for i0 in range(0, d["n"], per):
        ref, bound = pool_restate(x[i0:i0 + per], d["k"], d["stride"], d["pad"], d["mode"], dtype)
        got = out[i0:i0 + per].double()
        if tuple(got.shape) != tuple(ref.shape) or not torch.isfinite(got).all():
            return float("inf")
        if bound is None:
            worst = max(worst, 0.0 if bool((got == ref).all()) else float("inf"))
        else:
            worst = max(worst, ((got - ref).abs() / bound).max().item())
    return worst


def replay_pool(ops, rec: tuple, seed: int, dev):
    d, dtype = record_dict(rec), KIND_DTYPE[rec[1]]
    if d["out_off"] + d["c"] > d["out_stride"] or d["in_stride"] < d["c"]:
        raise NotImplementedError(f"the restatement does not express {d}")
    g = torch.Generator(device=dev).manual_seed(seed)
    xs = torch.randn((d["n"], d["h"], d["w"], d["in_stride"]), generator=g, device=dev).to(dtype)
    x = xs[..., :d["c"]]
    oh, ow = (d["h"] + 2 * d["pad"] - d["k"]) // d["stride"] + 1, (d["w"] + 2 * d["pad"] - d["k"]) // d["stride"] + 1
    parent = torch.full((d["n"], oh, ow, d["out_stride"]), SENTINEL, dtype=dtype, device=dev)
    out = parent[..., d["out_off"]:d["out_off"] + d["c"]]
    ops.pool2d(x, d["k"], d["stride"], d["pad"], d["mode"], out=out)
    torch.cuda.synchronize()
    if not sentinel_intact(parent, d["out_off"], d["c"]):
        return float("inf")
    return compare_pool(x, d, dtype, out)


def gap_restate(x):
    """float64 mean over the pixels of x [n, h, w, c] -> (ref, bound) [n, c]."""
    xd = x.double()
    hw = x.shape[1] * x.shape[2]
    return xd.mean((1, 2)), (hw + 1) * 2.0 ** -24 * xd.abs().mean((1, 2))


def compare_gap(x, got):
    """Worst err/bound of got [n, c] fp32; a channel that is zero at every pixel (bound 0) must come out as exactly 0."""
    ref, bound = gap_restate(x)
    if got.dtype != torch.float32 or tuple(got.shape) != tuple(ref.shape) or not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


def replay_gap(ops, rec: tuple, seed: int, dev):
    d, dtype = record_dict(rec), KIND_DTYPE[rec[1]]
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((d["n"], d["h"], d["w"], d["c"]), generator=g, device=dev).to(dtype)
    got = ops.global_avgpool_f32(x)
    torch.cuda.synchronize()
    return compare_gap(x, got)


# ------------------------------------------------------------------ bilinear resize
def resize_coords(size_in: int, size_out: int, half_pixel: bool, dev):
    """(i0, i1, frac) of every output index in fp32 as the kernel computes them: r = fl(in / out); half-pixel centres take
    s = fma(o + 0.5, r, -0.5) -- ONE rounding, which is also what torch's CPU F.interpolate does (the restatement then agrees with
    it to 1e-7 at every size; with the product rounded separately it is 1.7e-6 .. 3.6e-6 off at 128 .. 512 pixels); the
    TensorFlow-1 convention is the single product o r.  The float64 expression below is exact before its one rounding to fp32
    (24-bit r times an 11-bit o + 0.5)."""
    f32 = torch.float32
    r = torch.tensor(float(size_in), dtype=f32, device=dev) / torch.tensor(float(size_out), dtype=f32, device=dev)
    o = torch.arange(size_out, dtype=f32, device=dev)
    s = ((o.double() + 0.5) * r.double() - 0.5).to(f32) if half_pixel else o * r
    s = s.clamp_min(0.0)
    i0 = s.to(torch.int64).clamp(max=size_in - 1)
    i1 = (i0 + 1).clamp(max=size_in - 1)
    return i0, i1, (s - i0.to(f32)).double()


def resize_restate(images, kind: int, half_pixel: bool, scale: float, shift: float, oh: int, ow: int, dtype):
    """float64 bilinear resize of 3-channel images (uint8 NHWC / fp32 NCHW / fp32 NHWC) -> (ref, bound) [n, oh, ow, 3]."""
    px = (images.permute(0, 2, 3, 1) if kind == 1 else images).double()
    dev = px.device
    y0, y1, fy = resize_coords(px.shape[1], oh, half_pixel, dev)
    x0, x1, fx = resize_coords(px.shape[2], ow, half_pixel, dev)
    fy, fx = fy.view(1, -1, 1, 1), fx.view(1, 1, -1, 1)
    r0, r1 = px[:, y0], px[:, y1]
    top = r0[:, :, x0] * (1 - fx) + r0[:, :, x1] * fx
    bot = r1[:, :, x0] * (1 - fx) + r1[:, :, x1] * fx
    sc = torch.tensor(scale, dtype=torch.float32).double().item()     # the kernel takes fp32 scale and shift
    sh = torch.tensor(shift, dtype=torch.float32).double().item()
    ref = (top * (1 - fy) + bot * fy) * sc + sh
    bound = 0.5 * ulp_t(ref, dtype) + 8 * 2.0 ** -24 * (abs(sc) * px.abs().max().item() + abs(sh))
    return ref, bound


def resize_images(d: dict, constant: bool, seed: int, dev):
    """Full-range noise (uint8: 0..255, adjacent pixels up to 255 apart; fp32: [0, 1]) or a constant image."""
    g = torch.Generator(device=dev).manual_seed(seed)
    n, h, w, kind = d["n"], d["h"], d["w"], d["kind"]
    shape = (n, 3, h, w) if kind == 1 else (n, h, w, 3)
    if kind == 0:
        return (torch.full(shape, 200, dtype=torch.uint8, device=dev) if constant
                else torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8))
    top = 1.0 if abs(d["scale"]) >= 0.5 else 255.0     # [0, 1] floats (scale 2 or 1) or [0, 255] values (scale 1/128, 2/255)
    return (torch.full(shape, 0.7 * top, device=dev) if constant else torch.rand(shape, generator=g, device=dev) * top)


def compare_resize(images, d: dict, dtype, got, sel):
    """Worst err/bound of got [n, oh, ow, cpad] on the images sel; inf where channels 3.. are not exactly zero."""
    if not bool((got[..., 3:] == 0).all()) or not torch.isfinite(got).all():
        return float("inf")
    worst = 0.0
    for j in sel:
        ref, bound = resize_restate(images[j:j + 1], d["kind"], d["half_pixel"], d["scale"], d["shift"], d["oh"], d["ow"], dtype)
        worst = max(worst, ((got[j:j + 1, :, :, :3].double() - ref).abs() / bound).max().item())
    return worst


def replay_resize(ops, rec: tuple, seed: int, dev):
    """-> (worst err/bound on noise, worst on a constant image -- there against c * scale + shift)."""
    d, dtype = record_dict(rec), KIND_DTYPE[rec[1]]
    sel = list(range(d["n"])) if d["n"] <= 4 else ring_images(d["n"], seed)
    res = []
    for constant in (False, True):
        images = resize_images(d, constant, seed, dev)
        got = ops.resize_bilinear(images, d["oh"], d["ow"], d["cpad"], LAYOUTS[d["kind"]], d["half_pixel"], d["scale"], d["shift"], dtype)
        torch.cuda.synchronize()
        worst = compare_resize(images, d, dtype, got, sel)
        if constant and worst != float("inf"):
            c = float(images.reshape(-1)[0].item())
            sc, sh = torch.tensor([d["scale"], d["shift"]], dtype=torch.float32).double().tolist()
            ref = torch.full((1,), c * sc + sh, dtype=torch.float64, device=dev)
            bound = 0.5 * ulp_t(ref, dtype) + 8 * 2.0 ** -24 * (abs(sc) * abs(c) + abs(sh))
            worst = max(worst, ((got[sel][..., :3].double() - ref).abs() / bound).max().item())
        res.append(worst)
    return tuple(res)


# ------------------------------------------------------------------ the BatchNorm fold
def fold_reference(p: dict, name: str, dtype):
    """float64 fold of one BasicConv2d from the state dict -> (w gamma / sqrt(var + eps) [cout, taps, cin], bias, its two terms)."""
    w = p[name + ".conv.weight"].double()
    s = p[name + ".bn.weight"].double() / torch.sqrt(p[name + ".bn.running_var"].double() + 1e-3)
    ws = (w * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1])
    beta, ms = p[name + ".bn.bias"].double(), p[name + ".bn.running_mean"].double() * s
    return ws, beta - ms, beta.abs() + ms.abs()


def fold_errors(w_packed, bias, p: dict, name: str, dtype):
    """(worst |w_packed - round_T(fold)| / ulp_T(|w|), pad channels exactly zero, worst bias err / bound)."""
    ws, b, babs = (t.cpu() for t in fold_reference(p, name, dtype))
    w_packed, bias = w_packed.cpu(), bias.cpu()      # on the host: ulp_t's ldexp is exact there, and one ulp apart must read 1.0
    cin = ws.shape[2]
    wq = round_t(ws, dtype)
    werr = ((w_packed[..., :cin].double() - wq).abs() / ulp_t(ws, dtype)).max().item()
    pad_zero = bool((w_packed[..., cin:] == 0).all())
    berr = ((bias.double() - b).abs() / (4 * 2.0 ** -24 * babs + 1e-300)).max().item()
    return werr, pad_zero, berr
