"""Guarded operands for direct launches of library symbols, the case tables of tests/test_hip_guarded_launches.py and the
comparisons they share with tests/test_hip_launch_replay.py and tests/test_guarded_host.py.

Carves.  Every tensor a kernel takes a pointer to is a view of `shape` inside a larger test-owned buffer:
  output carve   the interior is NaN, a front and a back margin hold SENTINEL.  After the launch both margins are bitwise intact
                 (nothing was written before the start or past the end) and every interior element is finite (every element was
                 written, and from finite operands) -- on the whole tensor, not on samples.  A region that a kernel documents as
                 never written is exempted only by a named mask (`exempt=(why, mask)`, `why` citing the header or kernel comment).
  input carve    the same layout with NaN in both margins.  The float64 restatements read the interior only; a kernel whose
                 over-read reaches a stored value -- even multiplied by zero, 0 x NaN = NaN -- leaves a non-finite output, which
                 the check above reports.  After the launch the margins are still NaN (an input was not written to).
The view stays 16-byte aligned (the library refuses anything else): the front margin is a multiple of 8 elements for the 16-bit
types and of 4 for fp32; check() asserts the alignment.

Margins, in elements:
  GUARD = 4096                                         the default: vectors, statistics, workspaces of vectors
  margin_rows(width) = max(4096, 256 x width)          activations, residuals, fold operands, split-K workspaces and qkv / kv / out /
                                                       dout: one 256-pixel tile, or 256 token rows, of that operand -- the farthest a
                                                       tile loop that runs one tile or one row block too far can reach
  WEIGHT_MARGIN = 32 x 384 = 12288                     packed weights: one K-step (32 channels of one tap) of one Cout block in the
                                                       packed order [cin / 32][taps][cout / 16][64 lanes][8], at the widest block
                                                       (384 columns, the resident 1x1 kernel): what the three-ahead weight ring
                                                       fetches beyond the last step

What this cannot see: an over-read whose value is discarded -- a prefetch for a tile that does not exist, a masked lane whose
load is issued and dropped.  Only an address sanitizer sees those; the margins here are mapped memory on purpose, and nothing
places a buffer against unmapped pages.
"""
from __future__ import annotations

import ctypes as C

import torch

import launch_replay as lr

SENTINEL = -7.0
GUARD = 4096
WEIGHT_MARGIN = 32 * 384
NAN = float("nan")
F32 = torch.float32
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def margin_rows(width: int) -> int:
    return max(GUARD, 256 * int(width))


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Carve:
    """One guarded operand: `view` (shape) inside `buf` = [front margin | interior | back margin]."""

    def __init__(self, what, shape, dtype, device, margin=GUARD, front=None, output=True, fill=NAN, exempt=None):
        self.what, self.output, self.exempt = what, output, exempt
        self.numel = _numel(shape)
        self.front = margin if front is None else front
        self.back = margin
        self.buf = torch.full((self.front + self.numel + self.back,), SENTINEL if output else NAN, dtype=dtype, device=device)
        self.view = self.buf[self.front:self.front + self.numel].view(tuple(shape))
        self.view.fill_(fill)

    def data_ptr(self):
        return self.view.data_ptr()

    def _margins(self):
        return self.buf[:self.front], self.buf[self.front + self.numel:]

    def guard_ok(self):
        """The alignment of the view and both margins, bitwise."""
        assert self.view.data_ptr() % 16 == 0, f"{self.what}: the carve is not 16-byte aligned"
        bits = _BITS[self.buf.element_size()]
        for side, m in zip(("before the start", "past the end"), self._margins()):
            if self.output:
                want = torch.full((1,), SENTINEL, dtype=self.buf.dtype, device=self.buf.device).view(bits)
                bad = m.view(bits) != want
                msg = f"{self.what}: the guard {side} was written"
            else:
                bad = ~torch.isnan(m)
                msg = f"{self.what}: the margin {side} of an input was written"
            if bool(bad.any()):
                j = int(bad.nonzero()[0])
                raise AssertionError(f"{msg} ({int(bad.sum())} elements, the first at margin offset {j})")

    def finite_ok(self):
        """Every interior element of an output was written with a finite value (the exempted region aside)."""
        if not self.output:
            return
        bad = ~torch.isfinite(self.view)
        if self.exempt is not None:
            bad = bad & ~self.exempt[1].to(bad.device)
        if bool(bad.any()):
            idx = tuple(int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{self.what}: {int(bad.sum())} of {bad.numel()} elements are not finite (unwritten, or computed from "
                                 f"a value outside an operand), the first at {idx}")

    def check(self):
        self.guard_ok()
        self.finite_ok()


class Guarded:
    """The carves of one launch (or of one chain of launches): out() / inp() hand out views, check() holds all of them."""

    def __init__(self, device, guard_inputs=True):
        self.device, self.guard_inputs, self.carves = device, guard_inputs, []

    def out(self, what, shape, dtype, margin=GUARD, front=None, fill=NAN, exempt=None):
        c = Carve(what, shape, dtype, self.device, margin, front, True, fill, exempt)
        self.carves.append(c)
        return c.view

    def inp(self, what, t, margin=GUARD):
        """A copy of tensor t behind NaN margins (None stays None; with guard_inputs off, t itself)."""
        if t is None or not self.guard_inputs:
            return t
        c = Carve(what, t.shape, t.dtype, self.device, margin, None, False, 0.0)
        c.view.copy_(t)
        self.carves.append(c)
        return c.view

    def check(self):
        for c in self.carves:
            c.check()


def owned(shape, dtype, fill=NAN, device="cuda:0", what="output"):
    """A single output carve with the default margin -> (carve, view); carve.data_ptr() is the view's."""
    c = Carve(what, shape, dtype, device, GUARD, None, True, fill)
    return c, c.view


def guard_ok(carve, what):
    carve.what = what
    carve.guard_ok()


# ------------------------------------------------------------------ conv: operands, comparison
def conv_dict(label, n, h, w, c0, cout, taps=9, c1=0, prologue=0, res=False, stats=False, variant=0, expect=None, slabs=None,
              out_mode=0, out_scale=0.0, ksplit=1, up_phase=0, in_up=0, res_up=0, geglu=0, fc0=0, fc1=0, host_n=None):
    """One adm_conv case as the record dict of launch_replay.conv_record; h x w is what adm_conv_args holds (the output map, the
    source map for up_phase).  expect: the variant adm_conv_pick_variant must answer; slabs: adm_conv_stat_slabs' answer where it
    is asserted (the resident kernel); host_n: the batch of the host emulation (the persistent walks)."""
    return dict(label=label, n=n, h=h, w=w, c0=c0, c1=c1, cout=cout, taps=taps, prologue=prologue, out_mode=out_mode,
                out_scale=float(out_scale), variant=variant, ksplit=ksplit, up_phase=up_phase, in_up=in_up, res_up=res_up,
                geglu=geglu, fc0=fc0, fc1=fc1, has_in1=c1 > 0, has_res=bool(res) or prologue == 3, has_aff_a=prologue != 0,
                has_fold0=fc0 > 0, has_fold1=fc1 > 0, has_out_stats=bool(stats) or prologue == 3, has_w_packed32=False,
                has_ws=ksplit > 1, expect=expect, expect_slabs=slabs, host_n=host_n)


def conv_operands(ops, d, T, seed, device, g=None):
    """Seeded operands of one adm_conv record -> (t, packed, w32p, out).  t: the operands as the restatement reads them; packed /
    w32p: the packed weights (None without `ops`: the host emulation packs nothing).  g: the launch's Guarded -- outputs are
    always carved from it, inputs where it guards them."""
    g = g or Guarded(device, guard_inputs=False)
    torch.manual_seed(seed)
    n, h, w, c0, c1, cout, taps = d["n"], d["h"], d["w"], d["c0"], d["c1"], d["cout"], d["taps"]
    up = d["up_phase"]
    if up not in (0, 5) or d["prologue"] not in (0, 1, 2, 3):
        raise NotImplementedError(f"the restatement does not express up_phase {up} / prologue {d['prologue']}")
    hi, wi = (h // 2, w // 2) if d["in_up"] else (h, w)
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    cin, k = c0 + c1, (3 if taps == 9 else 1)
    t = {"x0": torch.randn(n, hi, wi, c0, device=device).to(T), "x1": torch.randn(n, hi, wi, c1, device=device).to(T) if d["has_in1"] else None}
    w32 = torch.randn(cout, cin, k, k, device=device) * (cin * taps) ** -0.5
    bias = 0.1 * torch.randn(cout, device=device) if d["prologue"] != 3 else torch.zeros(cout, device=device)  # backward-data convs: no bias
    packed = w32p = None
    if up:
        t["w"] = lr.round_t(up_phase_weights(w32), T)
        if ops is not None:
            packed = ops.pack_conv_weight_up(w32, T)
    elif d["geglu"]:
        wi_, bias = geglu_interleave(w32[:, :, 0, 0], bias)
        t["w"] = lr.round_t(wi_[:, :, None, None], T)
        if ops is not None:
            packed = ops.pack_conv_weight(wi_[:, :, None, None], T)
    else:
        t["w"] = lr.round_t(w32, T)
        if ops is not None:
            packed = ops.pack_conv_weight(w32, T)
            if d["has_w_packed32"]:
                w32p = ops.pack_conv_weight32(w32, T)
    if d["has_fold0"]:
        fc = d["fc0"] + d["fc1"]
        w1 = torch.randn(cout, fc, device=device) * fc ** -0.5
        if ops is not None:
            packed = ops.fold_weights(packed, ops.pack_conv_weight(w1, T))
        t["w1"] = lr.round_t(w1, T)
        t["f0"] = torch.randn(n, h, w, d["fc0"], device=device).to(T)
        t["f1"] = torch.randn(n, h, w, d["fc1"], device=device).to(T) if d["has_fold1"] else None
    t["bias"] = bias
    if d["prologue"] in (1, 2):
        t["a"], t["b"] = 1 + 0.2 * torch.randn(n, cin, device=device), 0.2 * torch.randn(n, cin, device=device)
    if d["prologue"] == 3:
        t["gnb_a"], t["gnb_b"] = 1 + 0.2 * torch.randn(n, cout, device=device), 0.2 * torch.randn(n, cout, device=device)
    if d["has_res"]:
        t["res"] = torch.randn(n, h // 2 if d["res_up"] else ho, w // 2 if d["res_up"] else wo, cout, device=device).to(T)
    # every operand behind NaN margins (a no-op where g does not guard inputs)
    for key in ("x0", "x1", "f0", "f1", "res"):
        if t.get(key) is not None:
            t[key] = g.inp(key, t[key], margin_rows(t[key].shape[-1]))
    for key in ("bias", "a", "b", "gnb_a", "gnb_b"):
        if key in t:
            t[key] = g.inp(key, t[key])
    packed, w32p = g.inp("w_packed", packed, WEIGHT_MARGIN), g.inp("w_packed32", w32p, WEIGHT_MARGIN)
    if d["out_mode"] == 1:
        out = g.out("out", (n, cout, h, w), F32, margin_rows(w))
    else:
        co = cout // 2 if d["geglu"] else cout
        out = g.out("out", (n, ho, wo, co), T, margin_rows(co))
    return t, packed, w32p, out


def up_phase_weights(w32):
    from autodiffusion_amd import ops
    return ops.up_phase_weights(w32)


def geglu_interleave(w, b):
    from autodiffusion_amd import ops
    return ops.geglu_interleave(w, b)


def conv_args(d, t, packed, w32p, out):
    """adm_conv_args of a record with every pointer but out_stats / ws set."""
    from autodiffusion_amd._lib import ConvArgs
    a = ConvArgs()
    for name, _ in ConvArgs._fields_:
        if name in d:
            setattr(a, name, d[name])
    a.in0, a.in1 = t["x0"].data_ptr(), (t["x1"].data_ptr() if t["x1"] is not None else None)
    a.w_packed, a.bias, a.out = packed.data_ptr(), t["bias"].data_ptr(), out.data_ptr()
    a.w_packed32 = w32p.data_ptr() if w32p is not None else None
    if "a" in t:
        a.aff_a, a.aff_b = t["a"].data_ptr(), t["b"].data_ptr()
    if "gnb_a" in t:
        a.aff_a, a.aff_b = t["gnb_a"].data_ptr(), t["gnb_b"].data_ptr()
    a.res = t["res"].data_ptr() if "res" in t else None
    if d["has_fold0"]:
        a.fold0, a.fold1 = t["f0"].data_ptr(), (t["f1"].data_ptr() if t["f1"] is not None else None)
    return a


REFUSALS = (-1, -2, -3)   # ADM_E_ARG, ADM_E_SHAPE, ADM_E_ALIGN (include/adm_hip.h): answered before anything is launched


def submit_conv(lib, fn, d, t, packed, w32p, out, g):
    """adm_conv through the library symbol `fn` with out_stats and the split-K workspace carved from g -> (status, stats | None,
    adm_conv_stat_slabs' answer | None).  Where that answer is 0 the request still goes out, with one slab carved: whether adm_conv
    then refuses it is the caller's question."""
    a = conv_args(d, t, packed, w32p, out)
    stats = slabs = None
    if d["has_out_stats"]:
        slabs = lib.adm_conv_stat_slabs(C.byref(a))
        stats = g.out("out_stats", (d["n"], max(1, slabs), d["cout"], 2), F32)
        a.out_stats = stats.data_ptr()
    if d["ksplit"] > 1:
        ws = g.out("ws", (d["ksplit"], d["n"] * d["h"] * d["w"], d["cout"]), F32, margin_rows(d["cout"]))
        a.ws = ws.data_ptr()
    rc = fn(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, stats, slabs


def launch_conv(lib, fn, d, t, packed, w32p, out, g):
    """submit_conv for a case that must run -> stats | None."""
    from autodiffusion_amd._lib import check
    a = conv_args(d, t, packed, w32p, out)
    assert not d["has_out_stats"] or lib.adm_conv_stat_slabs(C.byref(a)) > 0, d
    rc, stats, _ = submit_conv(lib, fn, d, t, packed, w32p, out, g)
    check(rc, "adm_conv (replay)")
    return stats


def compare_conv(d, T, t, out, stats, seed, rec=None):
    """The launch's output against conv_restate at launch_replay.sample_pixels (every pixel on maps <= 256 pixels), and the fused
    statistics against sums of the stored output -> (worst err / bound, relative Frobenius error)."""
    dev = out.device
    n = d["n"]
    ho, wo = (out.shape[2], out.shape[3]) if d["out_mode"] == 1 else (out.shape[1], out.shape[2])
    img, oy, ox = lr.sample_pixels(n, ho, wo, seed)
    cin = d["c0"] + d["c1"]
    per = max(1, (1 << 25) // max(1, (ho * wo * cin)))   # images per reference chunk
    worst, num, den = 0.0, 0.0, 0.0
    outv = out.permute(0, 2, 3, 1) if d["out_mode"] == 1 else out
    for i0 in range(0, n, per):
        sel = (img >= i0) & (img < i0 + per)
        ref, bound = lr.conv_restate(d, T, t, img[sel], oy[sel], ox[sel])
        got = outv[img[sel].to(dev), oy[sel].to(dev), ox[sel].to(dev)].double()
        assert torch.isfinite(got).all(), f"non-finite output {rec or d}"
        err = (got - ref).abs()
        r = err / bound
        if r.max().item() > 1.0:   # the worst element, for the failure report
            j = int(r.argmax())
            p, c = j // r.shape[1], j % r.shape[1]
            print(f"  worst element img {int(img[sel][p])} y {int(oy[sel][p])} x {int(ox[sel][p])} ch {c}: got {got[p, c].item():.8g} "
                  f"ref {ref[p, c].item():.8g} bound {bound[p, c].item():.4g} ulp_T(ref) {lr.ulp_t(ref[p, c], T).item():.4g}")
        worst = max(worst, r.max().item())
        num += (err ** 2).sum().item()
        den += (ref ** 2).sum().item()
    fro = (num / max(den, 1e-300)) ** 0.5
    if stats is not None:   # fused output statistics: per (image, channel) sums over the stored tensor
        y = outv.double()
        if d["prologue"] == 3:
            s1, s2 = y.sum((1, 2)), (y * t["res"].double()).sum((1, 2))
            a1, a2 = y.abs().sum((1, 2)), (y * t["res"].double()).abs().sum((1, 2))
        else:
            s1, s2 = y.sum((1, 2)), (y * y).sum((1, 2))
            a1, a2 = y.abs().sum((1, 2)), s2
        tot = stats.double().sum(1)
        tol = (256 + stats.shape[1] + 8) * 2.0 ** -24
        se = max(((tot[..., 0] - s1).abs() / (tol * a1 + 1e-30)).max().item(), ((tot[..., 1] - s2).abs() / (tol * a2 + 1e-30)).max().item())
        worst = max(worst, se)
    return worst, fro


# ------------------------------------------------------------------ the library symbols, called directly
def _p(t):
    return None if t is None else t.data_ptr()


class Hip:
    """The backend of the GPU tests: every method is one library symbol (or the chain of one GroupNorm pass) on the caller's
    tensors; nothing is allocated here but what `g` carves."""

    def __init__(self, ops, conv_fn=None):
        self.ops, self.conv_fn = ops, conv_fn

    def call(self, T, name, *args):
        from autodiffusion_amd import _lib
        _lib.check(getattr(_lib.load(lr.KIND_OF_DTYPE[T]), name)(*args, torch.cuda.current_stream().cuda_stream), name + " (guarded)")
        torch.cuda.synchronize()

    def conv(self, d, T, t, packed, w32p, out, g):
        from autodiffusion_amd import _lib
        lib = _lib.load(lr.KIND_OF_DTYPE[T])
        a = conv_args(d, t, packed, w32p, out)
        if d.get("expect") is not None:
            got = lib.adm_conv_pick_variant(C.byref(a))
            assert got == d["expect"], f"{d['label']}: adm_conv_pick_variant answers {got}, the case is meant for variant {d['expect']}"
        if d.get("expect_slabs") is not None:
            got = lib.adm_conv_stat_slabs(C.byref(a))
            assert got == d["expect_slabs"], f"{d['label']}: adm_conv_stat_slabs answers {got}, not {d['expect_slabs']}"
        return launch_conv(lib, self.conv_fn or lib.adm_conv, d, t, packed, w32p, out, g)

    def conv_try(self, d, T, t, packed, w32p, out, g):
        """The same launch where a refusal is an answer -> (accepted, stats | None, adm_conv_stat_slabs' answer | None,
        adm_conv_pick_variant's answer).  Any status but 0 and the three refusals raises."""
        from autodiffusion_amd import _lib
        lib = _lib.load(lr.KIND_OF_DTYPE[T])
        variant = lib.adm_conv_pick_variant(C.byref(conv_args(d, t, packed, w32p, out)))
        rc, stats, slabs = submit_conv(lib, self.conv_fn or lib.adm_conv, d, t, packed, w32p, out, g)
        if rc not in REFUSALS:
            _lib.check(rc, "adm_conv (envelope)")
        return rc == 0, stats, slabs, variant

    def attention_lse(self, qkv, out, lse, heads, d, new_order):
        n, t, _ = qkv.shape
        self.call(qkv.dtype, "adm_attention_lse", _p(qkv), _p(out), _p(lse), n, t, heads, d, int(new_order))

    def attention_1h512(self, qkv, out):
        self.call(qkv.dtype, "adm_attention_1h512", _p(qkv), _p(out), qkv.shape[0], qkv.shape[1])

    def attention_cross(self, q, q_stride, kv, kv_stride, kv_rows, out, n, tq, tk, heads, d, scale):
        self.call(q.dtype, "adm_attention_cross", _p(q), q_stride, _p(kv), kv_stride, kv_rows, _p(out), n, tq, tk, heads, d, float(scale))

    def attention_bwd(self, qkv, out, dout, lse, delta, dqkv, heads, d, new_order):
        n, t, _ = qkv.shape
        self.call(qkv.dtype, "adm_attention_bwd", _p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), n, t, heads, d, int(new_order))

    def gn_forward(self, mode, x0, x1, gamma, beta, film, film_stride, add, partial, partial1, a, b, stats, slabs, eps):
        n, h, w, c0 = x0.shape
        c1 = 0 if x1 is None else x1.shape[3]
        T, hw = x0.dtype, h * w
        if mode == "finalize2":   # each part of the concat carries its own sums
            self.call(T, "adm_gn_partial", _p(x0), c0, None, 0, _p(partial), n, hw, slabs)
            if x1 is not None:
                self.call(T, "adm_gn_partial", _p(x1), c1, None, 0, _p(partial1), n, hw, slabs)
            self.call(T, "adm_gn_finalize2", _p(partial), c0, slabs, _p(partial1), c1, slabs if x1 is not None else 0, _p(gamma), _p(beta),
                      _p(film), film_stride, _p(a), _p(b), _p(stats), n, hw, eps)
            return
        self.call(T, "adm_gn_partial", _p(x0), c0, _p(x1), c1, _p(partial), n, hw, slabs)
        if mode == "finalize_add":
            self.call(T, "adm_gn_finalize_add", _p(partial), _p(gamma), _p(beta), _p(add), add.stride(0), _p(a), _p(b), _p(stats),
                      n, c0 + c1, hw, slabs, eps)
        else:
            self.call(T, "adm_gn_finalize", _p(partial), _p(gamma), _p(beta), _p(film), film_stride, _p(a), _p(b), _p(stats),
                      n, c0 + c1, hw, slabs, eps)

    def gn_backward(self, x, dy, a, b, stats, e, add, partial, k1, k0, out, silu, dy_half, add_half, slabs, partial_given=False):
        n, h, w, c = x.shape
        T = x.dtype
        if not partial_given:
            self.call(T, "adm_gn_bwd_partial", _p(x), _p(dy), _p(a), _p(b), _p(partial), n, h, w, c, slabs, int(silu), int(dy_half))
        self.call(T, "adm_gn_bwd_finalize", _p(partial), _p(a), _p(stats), _p(e), 0 if e is None else e.stride(0), _p(k1), _p(k0),
                  n, c, h * w, slabs)
        self.call(T, "adm_gn_bwd_apply", _p(x), _p(dy), _p(a), _p(b), _p(k1), _p(k0), _p(add), _p(out), n, h, w, c, int(silu),
                  int(dy_half), int(add_half))


# ------------------------------------------------------------------ case runners (backend: Hip, or the host emulation)
def judge_conv(g, d, T, t, out, stats, seed):
    """What an accepted launch is held to: margins intact and every element of every output finite (Guarded.check), then the
    restatement's bounds -> (worst err / bound, relative Frobenius error, ok)."""
    g.check()
    worst, fro = compare_conv(d, T, t, out, stats, seed)
    u = lr.U[T]
    return worst, fro, worst <= 1.0 and fro <= lr.fro_bound(lr.conv_roundings(d), u)


def run_conv(be, ops, d, T, device, seed):
    g = Guarded(device)
    t, packed, w32p, out = conv_operands(ops, d, T, seed, device, g)
    stats = be.conv(d, T, t, packed, w32p, out, g)
    return judge_conv(g, d, T, t, out, stats, seed)


def untouched(g):
    """What a refused launch is held to: nothing was launched -- every output carve is NaN in every interior element still, and
    all margins (the inputs' too) are intact."""
    for c in g.carves:
        c.guard_ok()
        if c.output:
            written = ~torch.isnan(c.view)
            if bool(written.any()):
                idx = tuple(int(i) for i in written.nonzero()[0])
                raise AssertionError(f"{c.what}: the refused launch wrote {int(written.sum())} of {written.numel()} elements, the first at {idx}")


def try_conv(be, ops, d, T, device, seed, must=False):
    """One adm_conv request whose acceptance is the question.  Exactly two outcomes pass -> ("accepted", worst, fro) with
    judge_conv's conditions, or ("refused", None, None) with untouched()'s.  Besides: adm_conv_pick_variant answers d["expect"]
    where the case names one, adm_conv_stat_slabs answers > 0 exactly where the request with out_stats is accepted, and a `must`
    case is not refused."""
    g = Guarded(device)
    t, packed, w32p, out = conv_operands(ops, d, T, seed, device, g)
    accepted, stats, slabs, variant = be.conv_try(d, T, t, packed, w32p, out, g)
    where = f"{d['label']} {d['h']}x{d['w']}"
    if d.get("expect") is not None:
        assert variant == d["expect"], f"{where}: adm_conv_pick_variant answers {variant}, the case is meant for variant {d['expect']}"
    if d["has_out_stats"]:
        assert (slabs > 0) == accepted, (f"{where}: adm_conv_stat_slabs answers {slabs} and adm_conv "
                                         f"{'accepts' if accepted else 'refuses'} the request with out_stats")
    if not accepted:
        assert not must, f"{where}: a must-accept case was refused"
        untouched(g)
        return "refused", None, None
    worst, fro, ok = judge_conv(g, d, T, t, out, stats, seed)
    assert ok, f"{where}: worst err/bound {worst:.3f}, fro/u {fro / lr.U[T]:.3f} (bound {lr.fro_bound(lr.conv_roundings(d), 1.0):.3f})"
    return "accepted", worst, fro


def _heads_of(x, heads, d):
    """[t, >= heads d] rows -> [heads, t, d]."""
    return x[:, :heads * d].reshape(x.shape[0], heads, d).permute(1, 0, 2)


def compare_attention(q, k, v, scale, T, out, lse=None):
    """q / k / v [B, t, d] of one image, out [B, tq, d], lse [B, tq] | None -> (worst err / bound, sum err^2, sum ref^2)."""
    ref, bound = lr.attention_restate(q, k, v, scale, T)
    worst, e2, r2, _ = lr.worst_ratio(out, ref, bound)
    if lse is not None:
        lref, lb = lr.lse_restate(q, k, scale, T)
        worst = max(worst, lr.worst_ratio(lse, lref, lb)[0])
    return worst, e2, r2


def run_attention_lse(be, n, t, heads, d, new_order, T, device, seed):
    g = Guarded(device)
    torch.manual_seed(seed)
    c = heads * d
    qkv = g.inp("qkv", torch.randn(n, t, 3 * c, device=device).to(T), margin_rows(3 * c))
    out = g.out("out", (n, t, c), T, margin_rows(c))
    lse = g.out("lse", (n, heads, t), F32)
    be.attention_lse(qkv, out, lse, heads, d, new_order)
    g.check()
    worst, num, den = 0.0, 0.0, 0.0
    for j in range(n):
        qh, kh, vh = lr.split_qkv(qkv[j:j + 1], heads, new_order)
        w, e2, r2 = compare_attention(qh, kh, vh, d ** -0.5, T, _heads_of(out[j], heads, d), lse[j])
        worst, num, den = max(worst, w), num + e2, den + r2
    fro = (num / den) ** 0.5
    return worst, fro, worst <= 1.0 and fro <= lr.fro_bound(2, lr.U[T])


def run_attention_1h512(be, n, t, T, device, seed):
    g = Guarded(device)
    torch.manual_seed(seed)
    qkv = g.inp("qkv", torch.randn(n, t, 1536, device=device).to(T), margin_rows(1536))
    out = g.out("out", (n, t, 512), T, margin_rows(512))
    be.attention_1h512(qkv, out)
    g.check()
    worst, num, den = 0.0, 0.0, 0.0
    for j in range(n):
        q, k, v = (qkv[j:j + 1, :, i * 512:(i + 1) * 512] for i in range(3))
        w, e2, r2 = compare_attention(q, k, v, 512 ** -0.5, T, out[j:j + 1])
        worst, num, den = max(worst, w), num + e2, den + r2
    fro = (num / den) ** 0.5
    return worst, fro, worst <= 1.0 and fro <= lr.fro_bound(2, lr.U[T])


def run_attention_cross(be, n, tq, tk, kv_rows, heads, d, alias, T, device, seed):
    """alias: self-attention over a fused [q | k | v] projection, kv = the same storage from column heads d on.  Otherwise q
    [n, tq, heads d] and kv [n, kv_rows, 2 heads d]; the rows tk .. kv_rows of every image are NaN (they are not attended to), and
    with kv_rows == tk the rows behind the last image's are the margin."""
    g = Guarded(device)
    torch.manual_seed(seed)
    hd = heads * d
    scale = d ** -0.5
    if alias:
        buf = g.inp("qkv", torch.randn(n, tq, 3 * hd, device=device).to(T), margin_rows(3 * hd))
        q, qs, kvs = buf, 3 * hd, 3 * hd
        kv_ptr = buf.reshape(-1)[hd:]          # the pointer the model passes: K at column heads d of the same rows
        kvv = buf[:, :, hd:]
    else:
        q = g.inp("q", torch.randn(n, tq, hd, device=device).to(T), margin_rows(hd))
        kv0 = torch.randn(n, kv_rows, 2 * hd, device=device)
        kv0[:, tk:] = NAN
        kvv = g.inp("kv", kv0.to(T), margin_rows(2 * hd))
        qs, kvs, kv_ptr = hd, 2 * hd, kvv
    out = g.out("out", (n, tq, hd), T, margin_rows(hd))
    be.attention_cross(q, qs, kv_ptr, kvs, kv_rows, out, n, tq, tk, heads, d, scale)
    g.check()
    worst, num, den = 0.0, 0.0, 0.0
    for j in range(n):
        qh = _heads_of(q[j], heads, d)
        kh = _heads_of(kvv[j, :tk], heads, d)
        vh = _heads_of(kvv[j, :tk, hd:], heads, d)
        w, e2, r2 = compare_attention(qh, kh, vh, scale, T, _heads_of(out[j], heads, d))
        worst, num, den = max(worst, w), num + e2, den + r2
    fro = (num / den) ** 0.5
    return worst, fro, worst <= 1.0 and fro <= lr.fro_bound(2, lr.U[T])


def compare_attention_bwd(qkv, out, dout, dqkv, heads, new_order, T, images):
    n, t, c3 = qkv.shape
    d = c3 // 3 // heads
    worst = 0.0
    for j in images:
        qh, kh, vh = lr.split_qkv(qkv[j:j + 1], heads, new_order)
        oh, doh = _heads_of(out[j], heads, d), _heads_of(dout[j], heads, d)
        refs, bounds = lr.attention_bwd_restate(qh, kh, vh, oh, doh, d ** -0.5, T)
        for got, r, b in zip(lr.split_qkv(dqkv[j:j + 1], heads, new_order), refs, bounds):
            assert torch.isfinite(got).all(), (n, t, heads, d)
            worst = max(worst, ((got.double() - r).abs() / b).max().item())
    return worst


def run_attention_bwd(be, n, t, heads, d, new_order, T, device, seed):
    """The forward (output and log-sum-exp, guarded as well) feeds the backward, as in the model."""
    g = Guarded(device)
    torch.manual_seed(seed)
    c = heads * d
    qkv = g.inp("qkv", torch.randn(n, t, 3 * c, device=device).to(T), margin_rows(3 * c))
    dout = g.inp("dout", torch.randn(n, t, c, device=device).to(T), margin_rows(c))
    out = g.out("out", (n, t, c), T, margin_rows(c))
    lse = g.out("lse", (n, heads, t), F32)
    be.attention_lse(qkv, out, lse, heads, d, new_order)
    g.check()
    g2 = Guarded(device)
    o_in, lse_in = g2.inp("out", out, margin_rows(c)), g2.inp("lse", lse)
    delta = g2.out("delta_ws", (n, heads, t), F32)
    dqkv = g2.out("dqkv", (n, t, 3 * c), T, margin_rows(3 * c))
    be.attention_bwd(qkv, o_in, dout, lse_in, delta, dqkv, heads, d, new_order)
    g.check()
    g2.check()
    worst = compare_attention_bwd(qkv, o_in, dout, dqkv, heads, new_order, T, range(n))
    return worst, None, worst <= 1.0


GN_FWD_MODES = ("finalize", "finalize2", "finalize_add")


def run_gn_forward(be, mode, n, h, w, c0, c1, film_pad, slabs, T, device, seed, eps=1e-5):
    """adm_gn_partial + one of the three finalize kernels -> y = a x + b against float64 GroupNorm, and (mean, rstd).
    film_pad: None = no FiLM; else film_stride = 2 c + film_pad.  finalize_add takes one source and no FiLM."""
    g = Guarded(device)
    torch.manual_seed(seed)
    c = c0 + c1
    x0 = g.inp("x0", (0.3 + torch.randn(n, h, w, c0, device=device)).to(T), margin_rows(c0))
    x1 = g.inp("x1", (0.3 + torch.randn(n, h, w, c1, device=device)).to(T), margin_rows(c1)) if c1 else None
    gamma, beta = g.inp("gamma", 1 + 0.2 * torch.randn(c, device=device)), g.inp("beta", 0.2 * torch.randn(c, device=device))
    film = add = None
    film_stride = 0
    if mode == "finalize_add":
        add = g.inp("add", 0.3 * torch.randn(n, c, device=device))
    elif film_pad is not None:
        film_stride = 2 * c + film_pad
        full = torch.full((n, film_stride), NAN, device=device)     # the columns >= 2 c of a row are another layer's: never read
        full[:, :2 * c] = 0.3 * torch.randn(n, 2 * c, device=device)
        film = g.inp("film", full)
    two = mode == "finalize2"
    partial = g.out("partial", (n, slabs, c0 if two else c, 2), F32)
    partial1 = g.out("partial1", (n, slabs, c1, 2), F32) if two and c1 else None
    a, b, stats = g.out("aff_a", (n, c), F32), g.out("aff_b", (n, c), F32), g.out("stats", (n, 32, 2), F32)
    be.gn_forward(mode, x0, x1, gamma, beta, film, film_stride, add, partial, partial1, a, b, stats, slabs, eps)
    g.check()
    x = x0 if x1 is None else torch.cat([x0, x1], 3)
    y, mean, rstd = lr.gn_affine_restate(x, gamma, beta, eps, film=None if film is None else film[:, :2 * c], add=add)
    got = a.double()[:, None, None, :] * x.double() + b.double()[:, None, None, :]
    worst = ((got - y).abs() / (lr.U[T] / 8 * (1 + y.abs()))).max().item()
    st = stats.double()
    worst = max(worst, ((st[..., 0] - mean).abs() / (2.0 ** -20 * (mean.abs() + 1 / rstd))).max().item(),
                ((st[..., 1] - rstd).abs() / (2.0 ** -20 * rstd)).max().item())
    return worst, None, worst <= 1.0


def run_gn_backward(be, n, h, w, c, silu, dy_half, has_add, add_half, norm_add, T, device, seed):
    g = Guarded(device)
    torch.manual_seed(seed)
    x = torch.randn(n, h, w, c, device=device).to(T)
    e = 0.3 * torch.randn(n, c, device=device) if norm_add else None
    _, mean, rstd = lr.gn_affine_restate(x, torch.ones(c, device=device), torch.zeros(c, device=device), 1e-5, add=e)
    stats = g.inp("stats", torch.stack([mean, rstd], -1).float())
    a, b = g.inp("aff_a", 1 + 0.2 * torch.randn(n, c, device=device)), g.inp("aff_b", 0.2 * torch.randn(n, c, device=device))
    hs, ws_ = h // 2, w // 2
    dy = g.inp("dy", torch.randn(n, hs if dy_half else h, ws_ if dy_half else w, c, device=device).to(T), margin_rows(c))
    add = g.inp("add", torch.randn(n, hs if add_half else h, ws_ if add_half else w, c, device=device).to(T), margin_rows(c)) if has_add else None
    x, e = g.inp("x", x, margin_rows(c)), g.inp("norm_add", e)
    slabs = max(1, h * w // 256)      # ops.gn_bwd's rule (GN_BWD_SLAB_PIXELS)
    partial = g.out("partial", (n, slabs, c, 2), F32)
    k1, k0 = g.out("k1", (n, c), F32), g.out("k0", (n, c), F32)
    out = g.out("dx", (n, h, w, c), T, margin_rows(c))
    be.gn_backward(x, dy, a, b, stats, e, add, partial, k1, k0, out, silu, dy_half, add_half, slabs)
    g.check()
    ref, bound = lr.gn_bwd_restate(x, dy, a, b, stats, silu, dy_half, add, add_half, e, T)
    worst = lr.worst_ratio(out, ref, bound)[0]
    return worst, None, worst <= 1.0


# ------------------------------------------------------------------ the case tables
def _staged_convs():
    c = conv_dict
    cases = []
    for cout, v in ((200, 6), (328, 5)):   # 256-pixel tiles; 200: the second 128-wide block ends on a ragged 16-column tile (cout % 16 == 8)
        cases += [c(f"3x3 v{v} 256-pixel tiles", 3, 16, 16, 32, cout, expect=v),
                  c(f"3x3 v{v} + residual + statistics", 3, 16, 16, 32, cout, res=True, stats=True, expect=v),
                  c(f"3x3 v{v} GroupNorm + SiLU prologue", 3, 16, 16, 32, cout, prologue=2, expect=v)]
    cases += [
        c("3x3 16x32 map, concat input", 1, 16, 32, 32, 72, c1=32, expect=6),
        c("3x3 32x16 map", 1, 32, 16, 32, 72, expect=6),
        c("3x3 8x8 maps, two images per tile, odd n", 3, 8, 8, 64, 72, expect=6),
        c("1x1 8x8 maps, two images per tile, odd n", 3, 8, 8, 64, 72, taps=1, expect=6),
        c("1x1 pad steps K 160", 3, 8, 8, 160, 96, taps=1, expect=6),
        c("1x1 pad steps K 224", 3, 8, 8, 224, 96, taps=1, expect=6),
        c("1x1 8x16 map, two images per 256-pixel tile", 3, 8, 16, 64, 40, taps=1, expect=6),
        c("variant 3, 16-bit output", 2, 16, 16, 32, 8, expect=3),
        c("variant 3, fp32 NCHW, out_scale 2^-10", 2, 16, 16, 32, 6, out_mode=1, out_scale=2.0 ** -10, expect=3),
        c("split-K 3x3 ksplit 2 + residual + statistics", 2, 16, 16, 256, 72, ksplit=2, res=True, stats=True, expect=6),
        c("split-K 3x3 ksplit 4", 3, 8, 8, 512, 72, ksplit=4, expect=6),
        c("split-K 1x1 ksplit 8", 3, 8, 8, 1024, 200, taps=1, ksplit=8, expect=6),
        c("GroupNorm-backward epilogue", 2, 16, 16, 32, 40, prologue=3, expect=6),
        c("skip-connection fold 8x8", 3, 8, 8, 64, 72, prologue=2, fc0=32, fc1=32, expect=6),
        c("skip-connection fold 16x16", 2, 16, 16, 64, 72, prologue=2, fc0=32, fc1=32, expect=6),
        c("in_up", 2, 16, 16, 32, 40, in_up=1, expect=6),
        c("res_up", 2, 16, 16, 32, 40, res=True, res_up=1, expect=6),
        c("in_up + res_up", 2, 16, 16, 32, 40, in_up=1, res=True, res_up=1, expect=6),
        c("up_phase 5 + statistics", 1, 16, 16, 32, 40, up_phase=5, stats=True, expect=6),
        c("1x1 small_tiles_16 128-pixel tiles", 3, 16, 16, 1280, 200, taps=1, expect=6, slabs=4),   # four 64-pixel groups: the 128-pixel tiles
    ]
    return cases


def _resident_convs():
    c = conv_dict
    return [
        c("resident 128-pixel tiles", 3, 8, 16, 64, 264, taps=1, stats=True, expect=10, slabs=1),
        c("resident 64-pixel tiles, second Cout block 8 wide", 3, 8, 8, 128, 392, taps=1, stats=True, expect=10, slabs=1),
        c("resident 64-pixel tiles, second Cout block 8 wide + residual", 3, 8, 8, 128, 392, taps=1, res=True, stats=True, expect=10, slabs=1),
        c("resident 2x4 wave layout", 1, 16, 16, 64, 72, taps=1, c1=64, variant=10, stats=True, expect=10, slabs=4),
        c("resident 32-pixel tiles", 3, 8, 8, 1280, 200, taps=1, variant=10, stats=True, expect=10, slabs=2),
        # with variant 0 the library keeps outputs narrower than 256 on the staged kernel, which has no GEGLU epilogue: asked for by name
        c("resident GEGLU epilogue", 2, 8, 8, 64, 208, taps=1, geglu=1, variant=10, expect=10),
        c("resident csplit, three Cout blocks", 3, 8, 8, 128, 776, taps=1, expect=10),
        c("resident csplit, five Cout blocks in 3 parts of 2", 3, 8, 8, 128, 1544, taps=1, expect=10),
    ]


CONV_CASES = _staged_convs() + _resident_convs()


def walk_cases(cus: int):
    """The persistent tile walks at a device of `cus` compute units -> [(case, tiles, slots per round)].  The staged kernels run
    at most 2 blocks per CU, the resident kernel one."""
    want = 5 * cus + 3
    nbp = (392 + 127) // 128                       # 32 -> 392 runs on variant 6: four 128-wide Cout blocks per pixel tile
    n3 = -(-want // nbp)                           # pixel tiles x 4 cannot equal an odd 5 CUs + 3: the next multiple of 4 above it
    n1 = 2 * want - 1                              # 8x8: two images per tile, the last tile half empty
    nr = 2 * cus + cus // 2 + 3
    return [(conv_dict("walk: staged 3x3", n3, 16, 16, 32, 392, expect=6, host_n=2), n3 * nbp, 2 * cus),
            (conv_dict("walk: staged 1x1 at 8x8", n1, 8, 8, 64, 72, taps=1, expect=6, host_n=3), (n1 + 1) // 2, 2 * cus),
            (conv_dict("walk: resident 1x1", nr, 8, 8, 128, 392, taps=1, stats=True, expect=10, slabs=1, host_n=3), nr, cus)]


ATTN_T = (1, 63, 65, 129, 200)
ATTN_LSE_CASES = ([(t, 3, 64, no) for t in ATTN_T for no in (True, False)]
                  + [(t, 2, d, True) for t in ATTN_T for d in (32, 80, 160)])                      # (t, heads, d, new_order)
ATTN_CROSS_CASES = [("tq 130 tk 77 rows 77", 130, 77, 77, 2, 48, False), ("tq 130 tk 77 rows 128", 130, 77, 128, 2, 48, False),
                    ("fused-projection alias", 130, 130, 130, 2, 64, True)]          # (label, tq, tk, kv_rows, heads, d, alias)
ATTN_1H512_T = (1, 65, 200)
ATTN_BWD_CASES = [(t, 2, d) for t in ATTN_T for d in (32, 64)]
GN_FWD_SHAPES = [(3, 3, 5, 32, 0), (2, 1, 1, 64, 0), (2, 8, 8, 32, 32), (1, 16, 16, 2048, 0)]        # (n, h, w, c0, c1)
# (label, mode, n, h, w, c0, c1, film_pad, slabs); slabs None: ops.gn_slabs' rule
GN_FWD_CASES = ([(f"{m} {s}", m, *s, None, None) for s in GN_FWD_SHAPES for m in GN_FWD_MODES if not (m == "finalize_add" and s[4])]
                + [("finalize, slabs 4 do not divide hw 15", "finalize", 3, 3, 5, 32, 0, None, 4),
                   ("finalize, FiLM at film_stride 2 c + 24", "finalize", 2, 8, 8, 32, 32, 24, None),
                   ("finalize2, FiLM at film_stride 2 c + 24", "finalize2", 2, 8, 8, 32, 32, 24, None)])
# (n, h, w, c, dy_half, has_add, add_half)
GN_BWD_SHAPES = [(3, 6, 10, 32, False, False, False), (2, 8, 8, 64, True, False, False), (2, 8, 8, 64, False, True, True),
                 (1, 2, 2, 2048, False, False, False)]
GN_BWD_CASES = [s + (silu, na) for s in GN_BWD_SHAPES for silu in (False, True) for na in (False, True)]


def gn_slabs(hw: int) -> int:
    return max(1, min(64, hw // 64))
