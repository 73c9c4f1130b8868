"""Launch recorder, float64 restatements and per-element error bounds for tests/test_hip_launch_replay.py.

Recording: every adm_conv call (on both loaded libraries) is captured as a copy of its adm_conv_args without the pointers, plus
which optional pointers were set (those are flags); attention and GroupNorm calls are captured at the ops level by shape and flags.

Restatement: the op in float64 on the operands exactly as the kernel sees them -- 16-bit inputs, weights and residuals; the
GroupNorm affine (+ SiLU) prologue in fp32, rounded once to the 16-bit type T.

Per-element bounds, u = 2^-8 (bf16) or 2^-11 (fp16), ulp_T(v) = 2u * 2^floor(log2 |v|):
  conv       |got - ref| <= ulp_T(|ref|) + [residual / GroupNorm-backward epilogue] ulp_T(|A|) / 2
                            + Σ_k ulp_T(h_k) |w_k| [h_k within PRO_ULPS fp32 ulps of a T rounding midpoint]
                            + (K + ksplit + 2) 2^-24 Σ_k |w_k h_k|
             A = acc + bias is rounded to T before the residual is added (the reference's T-typed add); the third term is the
             c u max_k |w_k h_k| term made exact: only a prologue value whose fp32 computation (fma, approximate exp / rcp on the
             GPU, PRO_ULPS = 8 fp32 ulps of slack) straddles a rounding midpoint can round the other way, by one ulp_T; the last
             term is fp32 accumulation over K products.  fp32 NCHW output: no ulp_T term, a 2^-24 |ref| one instead.
             The last term is the worst case of fp32 summation: on deep convs (K ~ 9216) it reaches a few % of |ref|, ~30 fp16
             ulps, so there the per-element check is loose and a small worst ratio does not mean near-ulp agreement; the Frobenius
             bound below is the tight check on those launches.
  attention  |got - ref| <= ulp_T(|ref|) + C_ATTN u max_j |v_j| + fp32 terms (logits, PV accumulation; fp16: underflow of P)
             C_ATTN = 2: P is rounded to T before the PV product (numerator) and the row sum (denominator) -- u each.
  attn bwd   dq / dk: ulp_T(|ref|) + 4 u scale Σ_j P_j (|dP_j| + |δ|) |k_j| (resp. |q_i|); dv: ulp_T(|ref|) + 2 u Σ_i P_i |do_i|
             -- P and dS = P (dP - δ) are rounded to T before their products (u each, and dS inherits P's), fp32 terms far below.
  lse        log2-domain log-sum-exp of the scaled logits: |got - ref| <= u / ln 2 + 2^-18 (1 + |ref| + max_j |s_j c|): the row sum
             adds P after its rounding to T (relative u, log2(1 + u) <= u / ln 2), the rest is fp32 exp2 / log2.
  gn_bwd     dx = a dz + k1 (x + e) + k0 (+ add): ulp_T(|ref|) + 2^-20 (|a dz| + |k1 (x + e)| + |k0| + |add|) + |x + e| E1 + E0,
             E1 / E0 the fp32 slab sums' worst case (hw 2^-24 Σ|terms|) carried through k1 / k0.
  gn_affine  y = a x + b against float64 GroupNorm (+ FiLM / + add) of the stored tensor: u / 8 (1 + |y|), well below the
             rounding to T that the consuming conv's prologue applies next.
  Frobenius  ||got - ref|| / ||ref|| <= FRO_U u sqrt(r), FRO_U = 0.6: one rounding to T has an RMS relative error of at most
             u / sqrt(3) ~ 0.58 u; r roundings in sequence (A, then A + residual; dz, then dz SiLU'; P, then the output) add in
             quadrature.
"""
from __future__ import annotations

import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
KIND_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
PRO_ULPS = 8
C_ATTN = 2.0
FRO_U = 0.6
SILU_REL = 2.0 ** -20   # fp32 SiLU' / GELU on the accumulators: approximate exp / rcp / erf, a few fp32 ulps


def fro_bound(roundings: int, u: float) -> float:
    return FRO_U * u * math.sqrt(roundings)


def conv_roundings(d: dict) -> int:
    """Roundings to T in sequence on a conv's output: one, two where A is rounded before the residual / SiLU' epilogue."""
    if d["out_mode"] == 1:
        return 1
    return 2 if (d["has_res"] or d["prologue"] == 3) else 1


CONV_PTR_FLAGS = ("in1", "res", "aff_a", "fold0", "fold1", "out_stats", "w_packed32", "ws")
_CONV_SKIP = {"in0", "in1", "w_packed", "bias", "aff_a", "aff_b", "res", "out", "out_stats", "w_packed32", "ws", "fold0", "fold1"}


# ------------------------------------------------------------------ recording
def conv_record(kind: str, a) -> tuple:
    """Hashable record of one adm_conv_args: every non-pointer field, and which optional pointers were non-null."""
    d = {name: getattr(a, name) for name, _ in a._fields_ if name not in _CONV_SKIP}
    d["out_scale"] = float(a.out_scale)
    for f in CONV_PTR_FLAGS:
        d["has_" + f] = bool(getattr(a, f))
    return ("conv", kind) + tuple(sorted(d.items()))


def record_dict(rec: tuple) -> dict:
    return dict(rec[2:])


class Recorder:
    """Patches (through pytest's monkeypatch) adm_conv on both libraries and the attention / GroupNorm wrappers of ops."""

    def __init__(self, monkeypatch):
        from autodiffusion_amd import _lib, ops
        self.records = set()
        self.counts = {}
        self.orig = {}
        for kind in ("bf16", "f16"):
            lib = _lib.load(kind)
            fn = lib.adm_conv
            self.orig[kind] = fn

            def wrapped(args, stream, _fn=fn, _kind=kind):
                a = args._obj if hasattr(args, "_obj") else args.contents
                self._add(conv_record(_kind, _lib.ConvArgs.from_buffer_copy(a)))
                return _fn(args, stream)
            monkeypatch.setattr(lib, "adm_conv", wrapped)

        def kind_of(t):
            return "f16" if t.dtype == torch.float16 else "bf16"

        o_att, o_cross, o_bwd, o_gn, o_gnb = ops.attention, ops.attention_cross, ops.attention_bwd, ops.gn_affine, ops.gn_bwd

        def attention(qkv, heads, new_order, want_lse=False):
            n, t, c3 = qkv.shape
            self._add(("attention", kind_of(qkv), n, t, c3, heads, bool(new_order), bool(want_lse)))
            return o_att(qkv, heads, new_order, want_lse)

        def attention_cross(q, kv, heads, d, tk, scale, q_cols=None):
            self._add(("attention_cross", kind_of(q), q.shape[0], q.shape[1], q.stride(1), kv.shape[1], kv.stride(1), tk, heads, d,
                       float(scale)))
            return o_cross(q, kv, heads, d, tk, scale, q_cols)

        def attention_bwd(qkv, out, dout, lse, heads, new_order):
            n, t, c3 = qkv.shape
            self._add(("attention_bwd", kind_of(qkv), n, t, c3, heads, bool(new_order)))
            return o_bwd(qkv, out, dout, lse, heads, new_order)

        def gn_affine(x0, gamma, beta, x1=None, film=None, film_stride=0, partial=None, want_stats=False, eps=None, add=None):
            n, h, w, c0 = x0.shape
            self._add(("gn_affine", kind_of(x0), n, h, w, c0, 0 if x1 is None else x1.shape[3], film is not None, add is not None,
                       getattr(x0, "_adm_stats", None) is not None, bool(want_stats), float(ops.GN_EPS if eps is None else eps)))
            return o_gn(x0, gamma, beta, x1, film, film_stride, partial, want_stats, eps, add)

        def gn_bwd(x, dy, aff, stats, silu, dy_half=False, add=None, add_half=False, partial=None, norm_add=None):
            n, h, w, c = x.shape
            self._add(("gn_bwd", kind_of(x), n, h, w, c, bool(silu), bool(dy_half), add is not None, bool(add_half),
                       partial is not None, norm_add is not None))
            return o_gnb(x, dy, aff, stats, silu, dy_half, add, add_half, partial, norm_add)

        for name, fn in (("attention", attention), ("attention_cross", attention_cross), ("attention_bwd", attention_bwd),
                         ("gn_affine", gn_affine), ("gn_bwd", gn_bwd)):
            monkeypatch.setattr(ops, name, fn)

    def _add(self, rec):
        self.records.add(rec)
        self.counts[rec[0]] = self.counts.get(rec[0], 0) + 1


# ------------------------------------------------------------------ families (coverage guard)
def families(rec: tuple) -> set:
    """The (library, family) labels a record belongs to."""
    kind, op = rec[1], rec[0]
    out = set()
    if op == "conv":
        d = record_dict(rec)
        out.add(f"variant {d['variant']}")
        if d["ksplit"] > 1:
            out.add("ksplit > 1")
        if d["up_phase"] == 5:
            out.add("up_phase 5")
        if d["has_fold0"]:
            out.add("fold")
        if d["prologue"] == 3:
            out.add("prologue 3")
        if d["geglu"]:
            out.add("geglu")
        if d["out_mode"] == 1:
            out.add("out_mode 1 + out_scale" if d["out_scale"] != 0.0 else "out_mode 1")
        out.add("8x8 map" if d["h"] * d["w"] <= 64 else ">= 16x16 map")
    elif op == "attention":
        _, _, n, t, c3, heads, new_order, lse = rec
        out.add(f"attention d {c3 // 3 // heads}")
    elif op == "attention_cross":
        _, _, n, tq, qs, rows, kvs, tk, heads, d, scale = rec
        out.add(f"attention_cross d {d} ({'self' if tk == tq and qs == kvs else 'cross'})")
    else:
        out.add(op)
    return {(kind, f) for f in out}


# variant 7 (the 32x32x16 kernel) needs w_packed32, which no shipped model passes: tests/test_hip_kernels.py covers it
REQUIRED_FAMILIES = (["variant 3", "variant 5", "variant 6", "variant 10", "ksplit > 1", "up_phase 5", "fold",
                      "prologue 3", "geglu", "out_mode 1", "out_mode 1 + out_scale", "8x8 map", ">= 16x16 map"]
                     + [f"attention d {d}" for d in (64, 128, 192, 256)]
                     + [f"attention_cross d {d} ({k})" for d in (48, 80, 160) for k in ("self", "cross")]
                     + ["attention_bwd", "gn_bwd"])


# ------------------------------------------------------------------ arithmetic helpers
def round_t(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).to(x.dtype)


def ulp_t(v: torch.Tensor, dtype) -> torch.Tensor:
    """One unit in the last place of T at |v| (float64); fp16's subnormal spacing 2^-24 below 2^-14."""
    v = v.abs().double()
    _, e = torch.frexp(v)
    ul = torch.ldexp(torch.full_like(v, 2.0 * U[dtype]), (e - 1).to(torch.int32))
    floor = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    return torch.where(v == 0, torch.full_like(v, floor), ul.clamp_min(floor))


def prologue(x32: torch.Tensor, a32, b32, mode: int, dtype):
    """fp32 GroupNorm affine (+ SiLU) as the kernel's prologue computes it, rounded once to T; also the rounding-risk tensor: the
    step to the other T neighbour where the fp32 value lies within PRO_ULPS fp32 ulps of a T rounding midpoint, else 0."""
    if mode == 0:
        return x32, torch.zeros_like(x32)
    z = torch.addcmul(b32, a32, x32)
    if mode == 2:
        z = z * torch.sigmoid(z)
    r = round_t(z, dtype)
    # perturb by the slack and see whether the rounding moves (at a binade boundary the step below is half the step above)
    dz = PRO_ULPS * 2.0 ** -23 * z.abs()
    risk = torch.maximum((round_t(z - dz, dtype) - r).abs(), (round_t(z + dz, dtype) - r).abs())
    return r, risk


def sample_pixels(n: int, h: int, w: int, seed: int, extra: int = 16):
    """Output pixels (img, y, x) to restate: all of them on maps of <= 256 pixels; else the four corners of every 16x16
    (8x8 below 16) output tile of every image plus `extra` seeded random pixels per image."""
    if h * w <= 256:
        img, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij")
        return img.reshape(-1), y.reshape(-1), x.reshape(-1)
    tile = 16 if h >= 16 and w >= 16 else 8

    def corners(size):
        s = set()
        for t0 in range(0, size, tile):
            s.update((t0, min(size, t0 + tile) - 1))
        return torch.tensor(sorted(s))
    cy, cx = corners(h), corners(w)
    gy, gx = torch.meshgrid(cy, cx, indexing="ij")
    gy, gx = gy.reshape(-1), gx.reshape(-1)
    g = torch.Generator().manual_seed(seed)
    ry, rx = torch.randint(0, h, (n, extra), generator=g), torch.randint(0, w, (n, extra), generator=g)
    img = torch.cat([torch.arange(n).repeat_interleave(gy.numel()), torch.arange(n).repeat_interleave(extra)])
    y = torch.cat([gy.repeat(n), ry.reshape(-1)])
    x = torch.cat([gx.repeat(n), rx.reshape(-1)])
    return img, y, x


# ------------------------------------------------------------------ conv restatement
def conv_restate(d: dict, dtype, t: dict, img, oy, ox):
    """float64 restatement of one adm_conv launch at output pixels (img, oy, ox) -> (ref [P, cout_out], bound [P, cout_out]).

    d: the record's fields; t: the operands as float32 tensors holding T values (x0, x1, a, b, w, w1, f0, f1, bias, res,
    gnb_a, gnb_b): w is [cout, cin, k, k] -- for up_phase 5 the [4, cout, cin, 3, 3] T-rounded phase weights -- and w1 the
    folded skip connection's [cout, fc]."""
    dev = t["x0"].device
    taps, pro = d["taps"], d["prologue"]
    src = t["x0"] if t.get("x1") is None else torch.cat([t["x0"], t["x1"]], 3)
    imgs = torch.unique(img)
    loc = torch.empty(int(img.max()) + 1, dtype=torch.long)
    loc[imgs] = torch.arange(imgs.numel())
    sub = src[imgs.to(dev)].float()
    if pro in (1, 2):
        act, risk = prologue(sub, t["a"][imgs.to(dev)][:, None, None, :].float(), t["b"][imgs.to(dev)][:, None, None, :].float(),
                             pro, dtype)
    else:
        act, risk = sub, torch.zeros_like(sub)
    n_, hs, ws_, cin = act.shape
    li = loc[img].to(dev)
    oy, ox = oy.to(dev), ox.to(dev)
    if d["up_phase"]:
        sy, sx, up = oy // 2, ox // 2, False
    elif d["in_up"]:
        sy, sx, up = oy, ox, True
    else:
        sy, sx, up = oy, ox, False
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if taps == 9 else [(0, 0)]
    lim_y, lim_x = (2 * hs, 2 * ws_) if up else (hs, ws_)
    pa, pr = [], []
    for dy, dx in offs:
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < lim_y) & (xx >= 0) & (xx < lim_x)
        yi, xi = yy.clamp(0, lim_y - 1), xx.clamp(0, lim_x - 1)
        if up:
            yi, xi = yi // 2, xi // 2
        m = ok[:, None].to(act.dtype)
        pa.append(act[li, yi, xi] * m)
        pr.append(risk[li, yi, xi] * m)
    pa = torch.stack(pa, 1).reshape(li.numel(), -1).double()   # [P, taps * cin], tap-major
    pr = torch.stack(pr, 1).reshape(li.numel(), -1).double()
    w = t["w"].double()
    if d["up_phase"]:
        ph = (oy % 2) * 2 + (ox % 2)
        wm = w.permute(0, 1, 3, 4, 2).reshape(4, w.shape[1], -1)   # [4, cout, 9 * cin]
        acc = torch.empty((li.numel(), wm.shape[1]), dtype=torch.float64, device=dev)
        sab, srk = torch.empty_like(acc), torch.empty_like(acc)
        for p_ in range(4):
            s_ = ph == p_
            acc[s_] = pa[s_] @ wm[p_].T
            sab[s_] = pa[s_].abs() @ wm[p_].abs().T
            srk[s_] = pr[s_] @ wm[p_].abs().T
    else:
        wm = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)          # [cout, taps * cin]
        acc, sab, srk = pa @ wm.T, pa.abs() @ wm.abs().T, pr @ wm.abs().T
    kk = pa.shape[1]
    if d["has_fold0"]:
        fs = t["f0"] if t.get("f1") is None else torch.cat([t["f0"], t["f1"]], 3)
        pf = fs[img.to(dev), oy, ox].double()
        w1 = t["w1"].double()
        acc, sab = acc + pf @ w1.T, sab + pf.abs() @ w1.abs().T
        kk += pf.shape[1]
    bias = t["bias"].double()
    A = acc + bias
    E = srk + (kk + max(1, d["ksplit"]) + 2) * 2.0 ** -24 * (sab + bias.abs())
    if d["geglu"]:
        v, g = A[:, 0::2], A[:, 1::2]
        gel = 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))
        ref = v * gel
        bound = ulp_t(ref, dtype) + gel.abs() * E[:, 0::2] + 1.13 * v.abs() * E[:, 1::2] + SILU_REL * (ref.abs() + v.abs())
        return ref, bound
    if d["out_mode"] == 1:
        s = d["out_scale"] if d["out_scale"] != 0.0 else 1.0
        return A * s, s * (E + 2.0 ** -24 * A.abs())
    if pro == 3:
        xg = t["res"][img.to(dev), oy, ox].double()
        z = t["gnb_a"][img.to(dev)].double() * xg + t["gnb_b"][img.to(dev)].double()
        sg = torch.sigmoid(z)
        dsl = sg * (1 + z * (1 - sg))
        ref = A * dsl
        return ref, ulp_t(ref, dtype) + dsl.abs() * (0.5 * ulp_t(A, dtype) + E) + SILU_REL * (ref.abs() + A.abs())
    if d["has_res"]:
        r = t["res"][img.to(dev), oy // 2, ox // 2] if d["res_up"] else t["res"][img.to(dev), oy, ox]
        ref = A + r.double()
        return ref, ulp_t(ref, dtype) + 0.5 * ulp_t(A, dtype) + E
    return A, ulp_t(A, dtype) + E


# ------------------------------------------------------------------ attention restatement
def attention_restate(q, k, v, scale: float, dtype):
    """float64 softmax(q k^T scale) v for q [B, tq, d], k / v [B, tk, d] holding T values -> (ref, bound) [B, tq, d]."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.transpose(1, 2)) * scale
    p = torch.softmax(s, -1)
    ref = p @ v
    tk, d = k.shape[1], q.shape[2]
    vmax = v.abs().amax(1, keepdim=True)                             # [B, 1, d]
    ds = (d + 2) * 2.0 ** -24 * (q.abs() @ k.abs().transpose(1, 2)) * scale + 2.0 ** -22 * s.abs()
    bound = ulp_t(ref, dtype) + (C_ATTN * U[dtype] + 2.0 * ds.amax(-1, keepdim=True) + (tk + 2) * 2.0 ** -24) * vmax
    if dtype == torch.float16:
        bound = bound + tk * 2.0 ** -25 * vmax                        # P below fp16's normal range: absolute spacing 2^-24
    return ref, bound


def split_qkv(qkv, heads: int, new_order: bool):
    """[N, T, 3 H D] (ops.attention's layout) -> q, k, v [N * H, T, D] (the reference's qkv order: new or legacy)."""
    n, t, c3 = qkv.shape
    d = c3 // 3 // heads
    if new_order:
        x = qkv.reshape(n, t, 3, heads, d).permute(2, 0, 3, 1, 4)
    else:
        x = qkv.reshape(n, t, heads, 3, d).permute(3, 0, 2, 1, 4)
    q, k, v = (x[i].reshape(n * heads, t, d) for i in range(3))
    return q, k, v


def merge_heads(o, n: int, heads: int):
    """[N * H, T, D] -> [N, T, H D]."""
    _, t, d = o.shape
    return o.reshape(n, heads, t, d).permute(0, 2, 1, 3).reshape(n, t, heads * d)


def lse_restate(q, k, scale: float, dtype):
    """log2-domain log-sum-exp of the scaled logits (what adm_attention_lse stores) -> (ref, bound) [B, tq]."""
    s = (q.double() @ k.double().transpose(1, 2)) * scale
    ref = torch.logsumexp(s, -1) / math.log(2.0)
    return ref, U[dtype] / math.log(2.0) + 2.0 ** -18 * (1 + ref.abs() + (s.abs().amax(-1) / math.log(2.0)))


def attention_bwd_restate(q, k, v, o, do, scale: float, dtype):
    """float64 backward of softmax(q k^T scale) v with the forward output o as the kernel is given it (δ = rowsum(do o)):
    -> ((dq, dk, dv), (bound_q, bound_k, bound_v)), each [B, t, d]."""
    q, k, v, o, do = (x.double() for x in (q, k, v, o, do))
    p = torch.softmax((q @ k.transpose(1, 2)) * scale, -1)
    dp = do @ v.transpose(1, 2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq, dk, dv = (ds @ k) * scale, (ds.transpose(1, 2) @ q) * scale, p.transpose(1, 2) @ do
    u = U[dtype]
    a = p * (dp.abs() + delta.abs())
    bq = ulp_t(dq, dtype) + 4 * u * scale * (a @ k.abs())
    bk = ulp_t(dk, dtype) + 4 * u * scale * (a.transpose(1, 2) @ q.abs())
    bv = ulp_t(dv, dtype) + 2 * u * (p.transpose(1, 2) @ do.abs())
    return (dq, dk, dv), (bq, bk, bv)


def _half_up(t, h, w):
    """[n, h/2, w/2, c] read through the nearest 2x upsample with the AvgPool2d backward's 1/4."""
    return 0.25 * t.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w]


def gn_bwd_restate(x, dy, a, b, stats, silu: bool, dy_half: bool, add, add_half: bool, e, dtype):
    """float64 dx of y = act(a x + b) through the GroupNorm whose (mean, rstd) = stats [n, 32, 2] (of x + e when e is given),
    as adm_gn_bwd_* state it: dz = dy act'(a x + b); dx = a dz + k1 (x + e) + k0 (+ add) -> (ref, bound) [n, h, w, c]."""
    n, h, w, c = x.shape
    x, a, b = x.double(), a.double()[:, None, None, :], b.double()[:, None, None, :]
    dz = _half_up(dy.double(), h, w) if dy_half else dy.double()
    if silu:
        z = a * x + b
        sg = torch.sigmoid(z)
        dz = dz * sg * (1 + z * (1 - sg))
    xe = x if e is None else x + e.double()[:, None, None, :]
    cpg = c // 32
    mean = stats[..., 0].double().repeat_interleave(cpg, 1)[:, None, None, :]
    r = stats[..., 1].double().repeat_interleave(cpg, 1)[:, None, None, :]
    m = cpg * h * w

    def gsum(t):   # per (image, group) sum, broadcast back to channels
        return t.sum((1, 2)).reshape(n, 32, cpg).sum(-1).repeat_interleave(cpg, 1)[:, None, None, :]
    s1 = gsum(a * dz) / r
    s2 = gsum(a * dz * (xe - mean))
    k1 = -r * r * s2 / m
    k0 = -r * s1 / m - mean * k1
    ad = 0.0 if add is None else (_half_up(add.double(), h, w) if add_half else add.double())
    ref = a * dz + k1 * xe + k0 + ad
    acc = h * w * 2.0 ** -24
    e1 = r * r / m * gsum((a * dz).abs() * (xe.abs() + mean.abs())) * acc
    e0 = r / m * gsum((a * dz).abs()) / r * acc + mean.abs() * e1
    bound = (ulp_t(ref, dtype) + 2.0 ** -20 * ((a * dz).abs() + (k1 * xe).abs() + k0.abs() + (ad.abs() if add is not None else 0.0))
             + xe.abs() * e1 + e0)
    return ref, bound


def gn_affine_restate(x, gamma, beta, eps: float, film=None, add=None):
    """float64 GroupNorm32 (+ FiLM (1 + scale), shift) of x [n, h, w, c] (+ add[:, None, None, :]) -> (y, mean [n, 32], rstd)."""
    n, h, w, c = x.shape
    xe = x.double() if add is None else x.double() + add.double()[:, None, None, :]
    g = xe.reshape(n, h * w, 32, c // 32)
    mean = g.mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((g - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(n, h, w, c) * gamma.double() + beta.double()
    if film is not None:
        y = y * (1 + film[:, None, None, :c].double()) + film[:, None, None, c:2 * c].double()
    return y, mean, rstd
