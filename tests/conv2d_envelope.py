"""The envelope of the kernels of csrc/adm_convg.hip -- adm_conv2d, adm_pool2d, adm_global_avgpool_f32, adm_resize_bilinear --
at shapes no model launches: the sibling of tests/conv_envelope.py.

The contract is the same: whatever a symbol accepts it computes on every element within the replay's bounds; whatever it cannot
compute it refuses (ADM_E_ARG / ADM_E_SHAPE / ADM_E_ALIGN) before the first launch and writes nothing.  Here the tables also say
WHICH of the two every row must be: an accepted-table row that is refused fails, and so does a refusal row that is answered 0.
tests/test_hip_conv2d_envelope.py walks the tables on the library symbols, tests/test_conv2d_envelope_host.py on a float32 host
stand-in (Host below) with planted defects.

No restatement or bound is new: the rows are records in the format of inception_replay.conv2d_record (and the pool, gap and
resize records) and go to inception_replay.compare_conv / compare_pool / compare_gap / compare_resize and
clip_image_replay.bicubic_restate, whole tensor, unchanged bounds.  What differs from inception_replay.conv_operands is the
operands' surroundings: channels cin .. cin_pad of the input are zero (the ABI), everything else the kernel has no business
reading is NaN -- channels cin_pad .. in_stride, the channels of a wider parent tensor around an input slice, and guarded.py's
margins around input, weights, bias and the output's parent.  A read of any of it, even times a zero weight, leaves a
non-finite output.  The parent of an output slice holds inception_replay.SENTINEL outside the slice, bit for bit afterwards.

conv2d accepted table (CONV_FAMILIES), a union of one-axis walks around one small base case, not a product:
  cout      the kernel pick by cout and the partial channel tiles: 4 8 28 32 on convg_kernel<2>; 36 64 132 192 260 on
            convg_lds_kernel<4,1> (132 and 260: a last 64-wide block of 4 channels; 192: grid.y 3); 68 128 196 256 on
            convg_lds_kernel<2,2> (68 and 196: the last 128-wide block holds 68, its second wave column 4 channels).  "Least
            padding" sends 68 and 196 to the 128-wide blocks and 132 and 260 to the 64-wide ones, not the other way round: the
            pick of every row is asserted against inception_replay.conv_kernel_pick, so a change of the rule cannot silently
            empty a family.
  K-steps   steps = kh kw cin_pad / 32 of 1, 2 (two ways), 3, 4, 5, 6, 7, 27, 49, 196 on each pick (cout 28 / 132 / 68): the
            short prologues of the LDS kernel's 3-stage ring, its first wraps, and long rings.
  M         M = n oh ow of 1 63 64 65 127 128 129 255 256 257 on each pick (cout 32 / 64 / 128), 3x3 with padding so that image
            borders fall inside the tiles; 129 is n = 3 maps of 43 pixels: two image boundaries in one 64-pixel wave tile.
            127, 257 and 43 are primes: those maps are single rows or columns (1x127, 257x1, 43x1) -- longer than the 20 pixels
            every other map keeps to, still below 400 pixels.
  geometry  kernels 1x1 3x3 5x5 2x2 1x7 7x1 1x3 3x1, 14x14 at stride 14; strides 1 2 3 on maps they do not divide; pads (0,0)
            (1,1) (0,3) (3,0) (2,1); a 5x5 window on a 2x2 image; h != w; h = 1; w = 1.
  layout    cin 3 31 32 (33) at cin_pad 32 and 64; in_stride = cin_pad, + 8, + 40; the input a channel slice of a wider tensor;
            out_off 0 4 12 in out_stride cout + 16; out_stride cout + 4; bias and ReLU on and off.
Refusal tables go through the same symbols on operands allocated for the output the library computed BEFORE the output-size
fix (C division truncates: h = 2, k = 3, stride 2 gave oh = 1), so that a library which launches such a request writes inside the
allocation and fails on its status.

Frobenius check.  ||got - ref|| / ||ref|| <= launch_replay.fro_bound(1, u) = 0.6 u is the only check that sees a truncating
output conversion (0.85 u), and an RMS over few elements is noise: it is applied to conv cases of at least FRO_MIN_ELEMS = 72
output elements.  Chosen on the host: the correctly rounded float32 stand-in (Host) ran every accepted conv row at 8 seeds and
every row below 600 elements at 2000 more, in both types.  The cases of 32 elements left the bound on 17 of 4000 draws (worst
fro / u 0.667), those of 64 elements on 2 of 4000 (0.638); from 72 elements on none did: worst 0.594 at 72, 0.553 at 128, 0.531 at
280 .. 864, 0.452 from 1024 on.  72 is the smallest count that stayed inside on every case and seed tried.  Every kernel pick
keeps far more than five checked cases (tests/test_conv2d_envelope_host.py asserts it).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

import clip_image_replay as cr
import guarded as gd
import inception_replay as ir
import launch_replay as lr

FRO_MIN_ELEMS = 72
K2, L41, L22 = "convg_kernel<2>", "convg_lds_kernel<4,1>", "convg_lds_kernel<2,2>"
PICKS = (K2, L41, L22)
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


# ------------------------------------------------------------------ rows
def conv_d(**kw):
    """One conv2d record (inception_replay.conv2d_record's keys, and in_off: the input is channels in_off .. of a tensor
    in_stride wide) around the base case: n 2, 5x7 map (M = 70: one 64-pixel tile and a ragged second), 27 of 32 channels, 3x3
    pad 1, bias, no ReLU."""
    d = dict(n=2, h=5, w=7, cin=None, cin_pad=32, in_stride=None, in_off=0, cout=36, kh=3, kw=3, stride=1, ph=1, pw=1, relu=False,
             has_bias=True, out_stride=None, out_off=0)
    d.update(kw)
    if d["cin"] is None:
        d["cin"] = d["cin_pad"] - 5
    if d["in_stride"] is None:
        d["in_stride"] = d["cin_pad"] + d["in_off"]
    if d["out_stride"] is None:
        d["out_stride"] = d["cout"] + d["out_off"]
    return d


def row(name, d, expect="accepted", over=None, ptr=None, pick=None):
    """name; the record the operands are built for; what the symbol must answer; for refusal rows the request fields that differ
    from the record (over) and the pointers that do (ptr: field -> byte offset, or None for a null pointer)."""
    return dict(name=name, d=d, expect=expect, over=over or {}, ptr=ptr or {}, pick=pick)


def _conv_cout():
    picks = [(c, K2) for c in (4, 8, 28, 32)] + [(c, L41) for c in (36, 64, 132, 192, 260)] + [(c, L22) for c in (68, 128, 196, 256)]
    return [row(f"cout{c}", conv_d(cout=c), pick=p) for c, p in picks]


# steps -> (kh, kw, cin_pad)
K_STEPS = [("1", 1, 1, 32), ("2:1x1c64", 1, 1, 64), ("2:1x2c32", 1, 2, 32), ("3", 1, 3, 32), ("4", 2, 2, 32), ("5", 5, 1, 32),
           ("6", 1, 3, 64), ("7", 7, 1, 32), ("27", 3, 3, 96), ("49", 7, 7, 32), ("196", 14, 14, 32)]
K_COUT = {K2: 28, L41: 132, L22: 68}


def _conv_ksteps():
    rows = []
    for pick in PICKS:
        for label, kh, kw, cp in K_STEPS:
            d = conv_d(n=2, h=6, w=6, cin_pad=cp, cout=K_COUT[pick], kh=kh, kw=kw, ph=kh // 2, pw=kw // 2)
            rows.append(row(f"K{label}/{K_COUT[pick]}", d, pick=pick))
    return rows


# M -> (n, h, w) of a 3x3 pad-1 stride-1 conv (oh = h, ow = w)
M_MAPS = [(1, 1, 1, 1), (63, 1, 7, 9), (64, 1, 8, 8), (65, 1, 5, 13), (127, 1, 1, 127), (128, 2, 8, 8), (129, 3, 43, 1), (255, 1, 15, 17),
          (256, 1, 16, 16), (257, 1, 257, 1)]
M_COUT = {K2: 32, L41: 64, L22: 128}


def _conv_m():
    return [row(f"M{m}/{M_COUT[p]}", conv_d(n=n, h=h, w=w, cout=M_COUT[p]), pick=p) for p in PICKS for m, n, h, w in M_MAPS]


def _conv_geometry():
    g = lambda name, **kw: row(name, conv_d(**{**dict(h=7, w=10), **kw}), pick=ir.conv_kernel_pick(kw.get("cout", 36)))  # noqa: E731
    return [
        g("1x1", kh=1, kw=1, ph=0, pw=0), g("3x3", ), g("5x5", kh=5, kw=5, ph=2, pw=2), g("2x2", kh=2, kw=2, ph=0, pw=0),
        g("1x7", kh=1, kw=7, ph=0, pw=3), g("7x1", kh=7, kw=1, ph=3, pw=0), g("1x3", kh=1, kw=3, ph=0, pw=1),
        g("3x1", kh=3, kw=1, ph=1, pw=0),
        g("14x14s14", h=14, w=14, kh=14, kw=14, stride=14, ph=0, pw=0),
        g("14x14s14p4", h=20, w=17, kh=14, kw=14, stride=14, ph=4, pw=4),                  # 2 x 1 outputs
        g("s2", stride=2), g("s3", stride=3), g("s2p0", stride=2, ph=0, pw=0),             # 7x10: neither stride divides both axes
        g("5x5s3p0", h=10, w=9, kh=5, kw=5, stride=3, ph=0, pw=0), g("1x1s2", kh=1, kw=1, ph=0, pw=0, stride=2),
        g("p0,0", ph=0, pw=0), g("p0,3", ph=0, pw=3), g("p3,0", ph=3, pw=0), g("p2,1", ph=2, pw=1),
        g("p2,1s2", ph=2, pw=1, stride=2),
        g("5x5on2x2", h=2, w=2, kh=5, kw=5, ph=2, pw=2),
        g("h1", h=1, w=9), g("w1", h=9, w=1), g("h1s2", h=1, w=9, stride=2),
        g("5x5s2/8", kh=5, kw=5, ph=2, pw=2, stride=2, cout=8), g("5x5s2/132", kh=5, kw=5, ph=2, pw=2, stride=2, cout=132),
        g("1x7/8", kh=1, kw=7, ph=0, pw=3, cout=8), g("7x1/132", kh=7, kw=1, ph=3, pw=0, cout=132),
    ]


def _conv_layout():
    r = lambda name, **kw: row(name, conv_d(**kw), pick=ir.conv_kernel_pick(kw.get("cout", 36)))  # noqa: E731
    rows = [r(f"cin{c}/{cp}", cin=c, cin_pad=cp) for cp, cs in ((32, (3, 31, 32)), (64, (3, 31, 32, 33))) for c in cs]
    rows += [r(f"in_stride+{e}/{cp}", cin_pad=cp, in_stride=cp + e) for cp in (32, 64) for e in (0, 8, 40)]
    rows += [r(f"in_off{o}", in_off=o, in_stride=32 + 40) for o in (8, 24)]
    rows += [r("in_off16/132", in_off=16, in_stride=64 + 16, cin_pad=64, cout=132), r("in_off8/8", in_off=8, in_stride=48, cout=8)]
    rows += [r(f"out_off{o}", out_off=o, out_stride=36 + 16) for o in (0, 4, 12)]
    rows += [r("out_off12/8", out_off=12, out_stride=8 + 16, cout=8), r("out_off12/132", out_off=12, out_stride=132 + 16, cout=132),
             r("out_off4/4", out_off=4, out_stride=4 + 16, cout=4)]
    rows += [r("out_stride+4", out_stride=40), r("out_stride+4/4", cout=4, out_stride=8), r("out_stride+4/132", cout=132, out_stride=136)]
    rows += [r(f"bias{int(b)}relu{int(a)}", has_bias=b, relu=a) for b in (True, False) for a in (True, False)]
    rows += [r("bias0relu1/8", has_bias=False, relu=True, cout=8), r("bias0relu1/132", has_bias=False, relu=True, cout=132)]
    return rows


# the truncation family: -stride < h + 2 pad - k < 0 on one or both axes (C division gave an output size of 1)
TRUNCATION = [("h2k3s2", dict(h=2, w=2, stride=2)), ("h1k3s3", dict(h=1, w=1, stride=3)), ("w2k3s2", dict(h=5, w=2, stride=2)),
              ("w1k3s3", dict(h=5, w=1, stride=3))]


def _conv_refusals():
    base = conv_d()
    ref = lambda name, over=None, ptr=None, d=base: row(name, d, "refused", over, ptr)  # noqa: E731
    rows = [ref("cin_pad48", dict(cin_pad=48), d=conv_d(cin_pad=64, in_stride=64)),
            ref("in_stride<cin_pad", dict(in_stride=24)), ref("in_stride36", dict(in_stride=36), d=conv_d(in_stride=40)),
            ref("cout6", dict(cout=6), d=conv_d(cout=8)), ref("out_stride<cout", dict(out_stride=32)),
            ref("out_stride38", dict(out_stride=38), d=conv_d(out_stride=40)),
            ref("in+8B", ptr=dict(in_=8)), ref("w+8B", ptr=dict(w=8)), ref("out+4B", ptr=dict(out=4)), ref("bias+8B", ptr=dict(bias=8)),
            ref("null in", ptr=dict(in_=None)), ref("null w", ptr=dict(w=None)), ref("null out", ptr=dict(out=None))]
    for f in ("n", "h", "w_in", "kh", "kw", "stride"):
        rows += [ref(f"{f}=0", {f: 0}), ref(f"{f}=-1", {f: -1})]
    rows += [ref("pad_h=-1", dict(pad_h=-1)), ref("pad_w=-1", dict(pad_w=-1))]
    rows.append(ref("empty h2k3s1", d=conv_d(h=2, w=2, ph=0, pw=0)))
    rows += [ref(f"trunc {name}", d=conv_d(ph=0, pw=0, **kw)) for name, kw in TRUNCATION]
    return rows


CONV_FAMILIES = {"conv2d cout": _conv_cout, "conv2d K-steps": _conv_ksteps, "conv2d M": _conv_m, "conv2d geometry": _conv_geometry,
                 "conv2d layout": _conv_layout, "conv2d refusals": _conv_refusals}


def pool_d(**kw):
    d = dict(n=2, h=5, w=3, c=8, in_stride=None, in_off=0, k=3, stride=1, pad=1, mode="max", out_stride=None, out_off=0)
    d.update(kw)
    if d["in_stride"] is None:
        d["in_stride"] = d["c"] + d["in_off"]
    if d["out_stride"] is None:
        d["out_stride"] = d["c"] + d["out_off"]
    return d


POOL_MAPS = [(1, 1), (1, 7), (5, 3), (9, 9)]
# (c, in_off, in_stride - in_off - c, out_off, out_stride - out_off - c), rotated over the rows
POOL_SLICES = [(8, 0, 0, 0, 0), (24, 8, 8, 16, 0), (64, 0, 16, 8, 8), (8, 16, 0, 0, 24), (24, 0, 0, 8, 0), (64, 8, 8, 0, 0)]


def _pool():
    """k x stride x pad < k x map x mode; the channel count and the slices rotate.  Rows whose window does not fit the padded
    image (h + 2 pad < k) must be refused: with stride > 1 they are the truncation family."""
    rows, i = [], 0
    for k in (1, 2, 3, 5):
        for stride in (1, 2, 3):
            for pad in range(k):
                for h, w in POOL_MAPS:
                    for mode in ("max", "avg"):
                        c, io, ie, oo, oe = POOL_SLICES[i % len(POOL_SLICES)]
                        i += 1
                        d = pool_d(h=h, w=w, c=c, in_off=io, in_stride=io + c + ie, k=k, stride=stride, pad=pad, mode=mode, out_off=oo,
                                   out_stride=oo + c + oe)
                        fits = h + 2 * pad >= k and w + 2 * pad >= k
                        rows.append(row(f"{mode}{k}/{stride}/{pad}@{h}x{w}c{c}", d, "accepted" if fits else "refused"))
    return rows


def _pool_refusals():
    base = pool_d(c=8, in_stride=16, out_stride=16)
    ref = lambda name, over=None, ptr=None, d=base: row(name, d, "refused", over, ptr)  # noqa: E731
    rows = [ref("c12", dict(c=12)), ref("in_stride12", dict(in_stride=12)), ref("out_stride12", dict(out_stride=12)),
            ref("pad=k", dict(pad=3)), ref("pad>k", dict(pad=4)), ref("mode2", dict(mode=2)), ref("in+8B", ptr=dict(in_=8)),
            ref("out+8B", ptr=dict(out=8)), ref("null in", ptr=dict(in_=None)), ref("null out", ptr=dict(out=None)),
            ref("empty h2k3s1", d=pool_d(h=2, w=2, pad=0))]
    rows += [ref(f"trunc {name} {mode}", d=pool_d(pad=0, mode=mode, **kw)) for name, kw in TRUNCATION for mode in ("max", "avg")]
    return rows


GAP_HW = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (17, 17)]      # hw 1 2 63 64 65 289


def _gap():
    rows = []
    for n in (1, 3, 33):
        for c in (8, 40, 64, 2048):
            for h, w in GAP_HW:
                if (c == 64) != (n == 33) and c == 64:      # c 64 with n 33 only: n c / 8 = 264 threads cross one 256-thread block
                    continue
                if n * h * w * c > 1 << 22:                  # 33 images of 2048 channels: the one- and two-pixel maps only
                    continue
                rows.append(row(f"n{n}c{c}hw{h * w}", dict(n=n, h=h, w=w, c=c)))
    rows.append(row("c12", dict(n=2, h=3, w=3, c=16), "refused", dict(c=12)))
    return rows


RESIZE_PAIRS = [((1, 1), (1, 1)), ((1, 5), (4, 4)), ((5, 1), (4, 4)), ((7, 5), (1, 1)), ((7, 5), (1, 9)), ((4, 4), (9, 7)), ((20, 17), (5, 6))]


def resize_d(kind, hp, src, dst, cpad):
    scale, shift = (2 / 255.0, -1.0) if kind == 0 else (2.0, -1.0)
    return dict(n=2, h=src[0], w=src[1], oh=dst[0], ow=dst[1], cpad=cpad, kind=kind, half_pixel=hp, scale=scale, shift=shift)


def _resize():
    return [row(f"{ir.LAYOUTS[kind]} hp{hp} {s[0]}x{s[1]}>{o[0]}x{o[1]} c{cpad}", resize_d(kind, hp, s, o, cpad))
            for kind in (0, 1, 2) for hp in (0, 1, 2) for s, o in RESIZE_PAIRS for cpad in (8, 32)]


def _resize_refusals():
    base = resize_d(2, 1, (7, 5), (4, 4), 8)
    return [row("half_pixel3", base, "refused", dict(half_pixel=3)), row("kind3", base, "refused", dict(kind=3)),
            row("cpad4", base, "refused", dict(cpad=4)), row("out+8B", base, "refused", ptr=dict(out=8)),
            row("null in", base, "refused", ptr=dict(in_=None)), row("null out", base, "refused", ptr=dict(out=None))]


FAMILIES = dict(CONV_FAMILIES, **{"pool2d": _pool, "pool2d refusals": _pool_refusals, "global_avgpool_f32": _gap, "resize": _resize,
                                  "resize refusals": _resize_refusals})
FAMILY_LABELS = list(FAMILIES)
CONV_ACCEPTED = [f for f in CONV_FAMILIES if f != "conv2d refusals"]


def rows_of(label):
    return FAMILIES[label]()


def find(label, name):
    return next(r for r in rows_of(label) if r["name"] == name)


# ------------------------------------------------------------------ output sizes
def fits(size, k, pad):
    """The window fits the padded image."""
    return size + 2 * pad >= k


def c_out_size(size, k, stride, pad):
    """The output size as C computes it without the fit test: division truncates toward zero."""
    num = size + 2 * pad - k
    return (num // stride if num >= 0 else -((-num) // stride)) + 1


def alloc_size(size, k, stride, pad):
    """The output extent the operands are allocated for: the real one, or what a library without the fit test would write."""
    return max(1, c_out_size(size, k, stride, pad))


# ------------------------------------------------------------------ operands
def _carve_of(g, view):
    return next(c for c in g.carves if c.view.data_ptr() == view.data_ptr() and c.numel == view.numel())


def _flat_from(g, view, off):
    """The memory from element `off` of a carved view on, the back margin included: what a pointer to it addresses."""
    c = _carve_of(g, view)
    return c.buf[c.front + off:]


def _slice_in(g, what, n, h, w, width, off, cin, cpad, T, gen, device):
    """An input of `cin` random channels at channel `off` of a [n, h, w, width] parent: zero up to cpad, NaN everywhere else."""
    parent = torch.full((n, h, w, width), gd.NAN, dtype=T, device=device)
    parent[..., off:off + cin] = torch.randn((n, h, w, cin), generator=gen, device=device).to(T)
    parent[..., off + cin:off + cpad] = 0
    return g.inp(what, parent, gd.margin_rows(width))


def _slice_out(g, what, n, oh, ow, width, off, c, T):
    """The NaN output slice at channel `off` of a guarded [n, oh, ow, width] parent that holds the sentinel elsewhere."""
    parent = g.out(what, (n, oh, ow, width), T, gd.margin_rows(width))
    parent[..., :off] = ir.SENTINEL
    parent[..., off + c:] = ir.SENTINEL
    return parent, parent[..., off:off + c]


def _ptrs(q, r):
    for field, tweak in r["ptr"].items():
        q[field] = None if tweak is None else q[field] + tweak
    return q


def conv_request(be, r, T, seed, device, g):
    """Seeded operands of a conv2d row -> (the request: adm_conv2d_args' fields and, under "_t", the memory behind each pointer
    for the host stand-in; x [n, h, w, cin_pad ..] as the restatement reads it; packed weights; bias; parent; out slice)."""
    d = r["d"]
    gen = torch.Generator(device=device).manual_seed(seed)
    n, h, w, cin, cp, cs, cout, io = d["n"], d["h"], d["w"], d["cin"], d["cin_pad"], d["in_stride"], d["cout"], d["in_off"]
    assert cin <= cp and io + cp <= cs and io % 8 == 0 and d["out_off"] + cout <= d["out_stride"], d
    xp = _slice_in(g, "in", n, h, w, cs, io, cin, cp, T, gen, device)
    w32 = torch.randn((cout, cin, d["kh"], d["kw"]), generator=gen, device=device) * (cin * d["kh"] * d["kw"]) ** -0.5
    scale = 1 + 0.2 * torch.randn((cout,), generator=gen, device=device)
    bias = 0.3 * torch.randn((cout,), generator=gen, device=device) if d["has_bias"] else None
    packed = be.pack(w32, scale, cp, T)
    assert tuple(packed.shape) == (cout, d["kh"] * d["kw"], cp) and ir.packing_errors(packed, w32, scale, T) == 0, f"{r['name']}: packing"
    packed, bias = g.inp("w", packed, gd.WEIGHT_MARGIN), g.inp("bias", bias)
    oh, ow = alloc_size(h, d["kh"], d["stride"], d["ph"]), alloc_size(w, d["kw"], d["stride"], d["pw"])
    parent, out = _slice_out(g, "out", n, oh, ow, d["out_stride"], d["out_off"], cout, T)
    t = dict(x=_flat_from(g, xp, io), w=packed, bias=bias, out=_flat_from(g, parent, d["out_off"]), out_base=_flat_from(g, parent, 0))
    q = dict(in_=t["x"].data_ptr(), w=packed.data_ptr(), bias=None if bias is None else bias.data_ptr(), out=t["out"].data_ptr(),
             n=n, h=h, w_in=w, cin_pad=cp, in_stride=cs, cout=cout, out_stride=d["out_stride"], kh=d["kh"], kw=d["kw"],
             stride=d["stride"], pad_h=d["ph"], pad_w=d["pw"], relu=int(d["relu"]), _t=t)
    q.update(r["over"])
    return _ptrs(q, r), xp[..., io:], packed, bias, parent, out


def pool_request(r, T, seed, device, g):
    d = r["d"]
    gen = torch.Generator(device=device).manual_seed(seed)
    n, h, w, c, io = d["n"], d["h"], d["w"], d["c"], d["in_off"]
    xp = _slice_in(g, "in", n, h, w, d["in_stride"], io, c, c, T, gen, device)
    oh, ow = alloc_size(h, d["k"], d["stride"], d["pad"]), alloc_size(w, d["k"], d["stride"], d["pad"])
    parent, out = _slice_out(g, "out", n, oh, ow, d["out_stride"], d["out_off"], c, T)
    t = dict(x=_flat_from(g, xp, io), out=_flat_from(g, parent, d["out_off"]))
    q = dict(in_=t["x"].data_ptr(), out=t["out"].data_ptr(), n=n, h=h, w=w, c=c, in_stride=d["in_stride"], out_stride=d["out_stride"],
             k=d["k"], stride=d["stride"], pad=d["pad"], mode={"max": 0, "avg": 1}[d["mode"]], _t=t)
    q.update(r["over"])
    return _ptrs(q, r), xp[..., io:io + c], parent, out


def gap_request(r, T, seed, device, g):
    d = r["d"]
    gen = torch.Generator(device=device).manual_seed(seed)
    x = g.inp("in", torch.randn((d["n"], d["h"], d["w"], d["c"]), generator=gen, device=device).to(T), gd.margin_rows(d["c"]))
    out = g.out("out", (d["n"], d["c"]), gd.F32)
    t = dict(x=_flat_from(g, x, 0), out=_flat_from(g, out, 0))
    q = dict(in_=x.data_ptr(), out=out.data_ptr(), n=d["n"], hw=d["h"] * d["w"], c=d["c"], _t=t)
    q.update(r["over"])
    return _ptrs(q, r), x, out


def resize_request(r, T, seed, device, g):
    """uint8 images cannot hold NaN: only the fp32 layouts sit behind margins."""
    d = r["d"]
    images = ir.resize_images(d, False, seed, device)
    if d["kind"] != 0:
        images = g.inp("in", images)
    out = g.out("out", (d["n"], d["oh"], d["ow"], d["cpad"]), T, gd.margin_rows(d["cpad"]))
    t = dict(x=images, out=_flat_from(g, out, 0))
    q = dict(in_=images.data_ptr(), out=out.data_ptr(), n=d["n"], h=d["h"], w=d["w"], oh=d["oh"], ow=d["ow"], cpad=d["cpad"],
             kind=d["kind"], half_pixel=int(d["half_pixel"]), scale=d["scale"], shift=d["shift"], _t=t)
    q.update(r["over"])
    return _ptrs(q, r), images, out


# ------------------------------------------------------------------ the library symbols
class Hip:
    """Every method is one library symbol on the request's pointers -> its status, unchecked."""

    def __init__(self, ops):
        self.ops = ops

    def pack(self, w32, scale, cin_pad, T):
        """adm_pack_conv2d_weight itself: ops.pack_conv2d_weight pads cin to the next 32 only, the rows also ask for 3 in 64."""
        from autodiffusion_amd._lib import check
        cout, cin, kh, kw = w32.shape
        out = torch.empty((cout, kh * kw, cin_pad), dtype=T, device=w32.device)
        check(self._lib(T).adm_pack_conv2d_weight(w32.contiguous().data_ptr(), scale.contiguous().data_ptr(), out.data_ptr(), cout, cin, kh, kw,
                                                  cin_pad, torch.cuda.current_stream().cuda_stream), "adm_pack_conv2d_weight")
        return out

    @staticmethod
    def _lib(T):
        from autodiffusion_amd import _lib
        return _lib.load(lr.KIND_OF_DTYPE[T])

    @staticmethod
    def _done(rc):
        torch.cuda.synchronize()
        return rc

    def conv2d(self, T, q):
        from autodiffusion_amd._lib import Conv2dArgs
        a = Conv2dArgs()
        for name, _ in Conv2dArgs._fields_:
            setattr(a, name, q[name])
        return self._done(self._lib(T).adm_conv2d(C.byref(a), torch.cuda.current_stream().cuda_stream))

    def pool2d(self, T, q):
        return self._done(self._lib(T).adm_pool2d(q["in_"], q["out"], q["n"], q["h"], q["w"], q["c"], q["in_stride"], q["out_stride"], q["k"],
                                                  q["stride"], q["pad"], q["mode"], torch.cuda.current_stream().cuda_stream))

    def gap(self, T, q):
        return self._done(self._lib(T).adm_global_avgpool_f32(q["in_"], q["out"], q["n"], q["hw"], q["c"], torch.cuda.current_stream().cuda_stream))

    def resize(self, T, q):
        return self._done(self._lib(T).adm_resize_bilinear(q["in_"], q["out"], q["n"], q["h"], q["w"], q["oh"], q["ow"], q["cpad"], q["kind"],
                                                           q["half_pixel"], q["scale"], q["shift"], torch.cuda.current_stream().cuda_stream))


def truncate_t(v, dtype):
    """fp32 -> T toward zero."""
    r = v.to(dtype)
    bits = r.view(torch.int16)
    return torch.where(r.float().abs() > v.abs(), bits - 1, bits).view(dtype)   # sign-magnitude: one step toward zero


def _nhwc(flat, n, h, w, c, stride):
    return torch.as_strided(flat, (n, h, w, c), (h * w * stride, w * stride, stride, 1))


DEFECTS = ("a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k", "l")


class Host:
    """The host stand-in for the library symbols: the argument checks of csrc/adm_convg.hip restated (with the output-size rule
    as include/adm_hip.h states it: the window must fit the padded image), float32 torch arithmetic, one rounding to T, written
    through the request's pointers.  defect: one of the planted defects of tests/test_conv2d_envelope_host.py."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def pack(self, w32, scale, cin_pad, T):
        return ir.reference_weights(w32, scale, cin_pad, T).to(T)

    def _out_hw(self, h, w, kh, kw, stride, ph, pw):
        """-> (oh, ow) or None where the request is refused."""
        if self.defect != "a" and not (fits(h, kh, ph) and fits(w, kw, pw)):
            return None
        oh, ow = c_out_size(h, kh, stride, ph), c_out_size(w, kw, stride, pw)
        return (oh, ow) if oh > 0 and ow > 0 else None

    def conv2d(self, T, q):
        t = q["_t"]
        if not (q["in_"] and q["w"] and q["out"]):
            return E_ARG
        if not (q["n"] > 0 and q["h"] > 0 and q["w_in"] > 0 and q["kh"] > 0 and q["kw"] > 0 and q["stride"] > 0 and q["pad_h"] >= 0 and q["pad_w"] >= 0):
            return E_ARG
        cp, cs, cout, os_ = q["cin_pad"], q["in_stride"], q["cout"], q["out_stride"]
        if not (cp > 0 and cp % 32 == 0 and cs >= cp and cs % 8 == 0):
            return E_SHAPE
        if not (cout > 0 and cout % 4 == 0 and os_ >= cout and os_ % 4 == 0):
            return E_SHAPE
        n, h, w, kh, kw, s, ph, pw = q["n"], q["h"], q["w_in"], q["kh"], q["kw"], q["stride"], q["pad_h"], q["pad_w"]
        ohw = self._out_hw(h, w, kh, kw, s, ph, pw)
        if ohw is None:
            return E_SHAPE
        if q["in_"] % 16 or q["w"] % 16 or q["out"] % 8 or (q["bias"] or 0) % 16:
            return E_ALIGN
        oh, ow = ohw
        x = _nhwc(t["x"], n, h, w, cp, cs).float()
        m = torch.arange(n * oh * ow)
        img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
        taps, chunks = kh * kw, cp // 32
        cols = []
        for tap in range(taps):
            ky, kx = divmod(tap, kw)
            if self.defect == "d" and kh != kw:
                ky, kx = kx, ky
            iy, ix = oy * s - ph + ky, ox * s - (ph if self.defect == "e" else pw) + kx
            ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
            cols.append(torch.where(ok[:, None], x[img, iy.clamp(0, h - 1), ix.clamp(0, w - 1)], torch.zeros(())))
        steps = taps * chunks
        pa = torch.stack(cols, 1).reshape(m.numel(), steps, 32)       # K-step = (tap, 32-channel chunk), as the kernels walk it
        if self.defect == "b" and steps <= 2:
            pa[:, steps - 1] = 0
        if self.defect == "c" and steps >= 3:
            pa[:, [0, 2]] = pa[:, [2, 0]]
        z = pa.reshape(m.numel(), -1) @ t["w"].float().reshape(cout, -1).T
        if self.defect == "h" and cs > cp:
            z = z + 0 * _nhwc(t["x"], n, h, w, cs, cs).float()[img, oy.clamp(0, h - 1), ox.clamp(0, w - 1), cp][:, None]
        if t["bias"] is not None:
            z = z + t["bias"]
        if q["relu"]:
            z = torch.where(z < 0, torch.zeros(()), z)               # NaN stays NaN
        y = truncate_t(z, T) if self.defect == "j" else z.to(T)
        outv = _nhwc(t["out_base"] if self.defect == "g" else t["out"], n, oh, ow, cout, os_)
        keep_c = cout & ~15 if self.defect == "f" else cout
        keep_m = (m % 64 != 63) if self.defect == "i" else torch.ones_like(m, dtype=torch.bool)
        outv[img[keep_m], oy[keep_m], ox[keep_m], :keep_c] = y[keep_m, :keep_c]
        return 0

    def pool2d(self, T, q):
        t = q["_t"]
        if not (q["in_"] and q["out"]):
            return E_ARG
        n, h, w, c, k, s, pad, mode = q["n"], q["h"], q["w"], q["c"], q["k"], q["stride"], q["pad"], q["mode"]
        if not (n > 0 and h > 0 and w > 0 and k > 0 and s > 0 and 0 <= pad < k and mode in (0, 1)):
            return E_ARG
        if not (c > 0 and c % 8 == 0 and q["in_stride"] >= c and q["out_stride"] >= c and q["in_stride"] % 8 == 0 and q["out_stride"] % 8 == 0):
            return E_SHAPE
        if q["in_"] % 16 or q["out"] % 16:
            return E_ALIGN
        ohw = self._out_hw(h, w, k, k, s, pad, pad)
        if ohw is None:
            return E_SHAPE
        oh, ow = ohw
        x = F.pad(_nhwc(t["x"], n, h, w, c, q["in_stride"]).float(), (0, 0, pad, k, pad, k), value=float("-inf") if mode == 0 else 0.0)
        ones = F.pad(torch.ones(1, h, w, 1), (0, 0, pad, k, pad, k))
        acc = cnt = None
        for ky in range(k):
            for kx in range(k):
                sl = (slice(None), slice(ky, ky + (oh - 1) * s + 1, s), slice(kx, kx + (ow - 1) * s + 1, s))
                if mode == 0:
                    acc = x[sl] if acc is None else torch.maximum(acc, x[sl])
                else:
                    acc = x[sl] if acc is None else acc + x[sl]
                    cnt = ones[sl] if cnt is None else cnt + ones[sl]
        if mode == 1:
            acc = acc * (1.0 / (torch.full_like(cnt, float(k * k)) if self.defect == "k" else cnt))
        _nhwc(t["out"], n, oh, ow, c, q["out_stride"]).copy_(acc.to(T))
        return 0

    def gap(self, T, q):
        t = q["_t"]
        if not (q["in_"] and q["out"]):
            return E_ARG
        n, hw, c = q["n"], q["hw"], q["c"]
        if not (n > 0 and hw > 0 and c > 0 and c % 8 == 0):
            return E_SHAPE
        if q["in_"] % 16:
            return E_ALIGN
        t["out"][:n * c].view(n, c).copy_(t["x"][:n * hw * c].view(n, hw, c).float().mean(1))
        return 0

    def resize(self, T, q):
        t = q["_t"]
        if not (q["in_"] and q["out"]):
            return E_ARG
        n, h, w, oh, ow, cpad, kind, hp = q["n"], q["h"], q["w"], q["oh"], q["ow"], q["cpad"], q["kind"], q["half_pixel"]
        if not (n > 0 and h > 0 and w > 0 and oh > 0 and ow > 0 and cpad >= 8 and cpad % 8 == 0 and 0 <= kind <= 2 and 0 <= hp <= 2):
            return E_ARG
        if q["out"] % 16:
            return E_ALIGN
        px = (t["x"].permute(0, 2, 3, 1) if kind == 1 else t["x"]).float()
        sc, sh = torch.tensor(q["scale"], dtype=torch.float32), torch.tensor(q["shift"], dtype=torch.float32)
        if hp == 2:
            if self.defect == "l":                                      # out == 1 samples the centre row / column, not index 0
                px = px[:, h // 2:h // 2 + 1] if oh == 1 else px
                px = px[:, :, w // 2:w // 2 + 1] if ow == 1 else px
            v = F.interpolate(px.permute(0, 3, 1, 2), (oh, ow), mode="bicubic", align_corners=True).permute(0, 2, 3, 1) * sc + sh
        else:
            y0, y1, fy = ir.resize_coords(h, oh, bool(hp), "cpu")
            x0, x1, fx = ir.resize_coords(w, ow, bool(hp), "cpu")
            fy, fx = fy.float().view(1, -1, 1, 1), fx.float().view(1, 1, -1, 1)
            top = px[:, y0][:, :, x0] * (1 - fx) + px[:, y0][:, :, x1] * fx
            bot = px[:, y1][:, :, x0] * (1 - fx) + px[:, y1][:, :, x1] * fx
            v = (top * (1 - fy) + bot * fy) * sc + sh
        t["out"][:n * oh * ow * cpad].view(n, oh, ow, cpad).copy_(F.pad(v.to(T), (0, cpad - 3)))
        return 0


# ------------------------------------------------------------------ one row
def _untouched(g, parent, out, where):
    """What a refused request is held to: the output NaN in every element, the parent's sentinel and every margin intact."""
    for c in g.carves:
        c.guard_ok()
    written = ~torch.isnan(out)
    assert not bool(written.any()), f"{where}: the refused request wrote {int(written.sum())} of {written.numel()} output elements"
    if parent is not None:
        off = out.storage_offset() - parent.storage_offset()
        assert ir.sentinel_intact(parent, off, out.shape[3]), f"{where}: the refused request wrote outside the output slice"


def _answer(r, rc, where):
    """-> whether the request was accepted; asserts that it is what the table says."""
    assert rc == 0 or rc in gd.REFUSALS, f"{where}: status {rc} is neither 0 nor a refusal"
    got = "accepted" if rc == 0 else "refused"
    assert got == r["expect"], f"{where}: {got} (status {rc}), the table says {r['expect']}"
    return rc == 0


def try_conv2d(be, r, T, device, seed):
    """-> ("accepted", worst err / bound, fro / u, whether the Frobenius bound was applied) | ("refused", None, None, False)."""
    where = f"conv2d {r['name']}"
    d = r["d"]
    if r["pick"] is not None:
        assert ir.conv_kernel_pick(d["cout"]) == r["pick"], f"{where}: the table means {r['pick']}, cout {d['cout']} picks {ir.conv_kernel_pick(d['cout'])}"
    g = gd.Guarded(device)
    q, x, packed, bias, parent, out = conv_request(be, r, T, seed, device, g)
    if not _answer(r, be.conv2d(T, q), where):
        _untouched(g, parent, out, where)
        return "refused", None, None, False
    g.check()
    assert ir.sentinel_intact(parent, d["out_off"], d["cout"]), f"{where}: wrote outside its channel slice"
    oh, ow = ir.conv_out_hw(d)
    assert tuple(out.shape) == (d["n"], oh, ow, d["cout"]) and out.numel() < ir.FULL_BELOW
    worst, fro, report = ir.compare_conv(x, packed, bias, d, T, out, torch.arange(d["n"] * oh * ow))
    checked = out.numel() >= FRO_MIN_ELEMS
    u = lr.U[T]
    assert worst <= 1.0, f"{where}: worst err/bound {worst:.3f} at {report}"
    assert not checked or fro <= lr.fro_bound(1, u), f"{where}: fro/u {fro / u:.3f} over {out.numel()} elements (bound {lr.FRO_U})"
    return "accepted", worst, fro / u, checked


def try_pool2d(be, r, T, device, seed):
    where = f"pool2d {r['name']}"
    d = r["d"]
    g = gd.Guarded(device)
    q, x, parent, out = pool_request(r, T, seed, device, g)
    if not _answer(r, be.pool2d(T, q), where):
        _untouched(g, parent, out, where)
        return "refused", None, None, False
    g.check()
    assert ir.sentinel_intact(parent, d["out_off"], d["c"]), f"{where}: wrote outside its channel slice"
    worst = ir.compare_pool(x, d, T, out)
    assert worst <= 1.0, f"{where}: worst err/bound {worst:.3f}" + (" (max pooling is exact)" if d["mode"] == "max" else "")
    return "accepted", worst, None, False


def try_gap(be, r, T, device, seed):
    where = f"global_avgpool_f32 {r['name']}"
    g = gd.Guarded(device)
    q, x, out = gap_request(r, T, seed, device, g)
    if not _answer(r, be.gap(T, q), where):
        _untouched(g, None, out, where)
        return "refused", None, None, False
    g.check()
    worst = ir.compare_gap(x, out)
    assert worst <= 1.0, f"{where}: worst err/bound {worst:.3f}"
    return "accepted", worst, None, False


def try_resize(be, r, T, device, seed):
    where = f"resize {r['name']}"
    d = r["d"]
    g = gd.Guarded(device)
    q, images, out = resize_request(r, T, seed, device, g)
    if not _answer(r, be.resize(T, q), where):
        _untouched(g, None, out, where)
        return "refused", None, None, False
    g.check()
    if d["half_pixel"] == 2:
        assert bool((out[..., 3:] == 0).all()), f"{where}: channels 3.. are not exactly zero"
        ref, bound = cr.bicubic_restate(images, d["kind"], d["scale"], d["shift"], d["oh"], d["ow"], T)
        worst = float(((out[..., :3].double() - ref).abs() / bound).max())
    else:
        worst = ir.compare_resize(images, d, T, out, range(d["n"]))
    assert worst <= 1.0, f"{where}: worst err/bound {worst:.3f}"
    return "accepted", worst, None, False


def try_row(be, label, r, T, device, seed):
    fn = try_conv2d if label in CONV_FAMILIES else try_pool2d if label.startswith("pool2d") else try_gap if label.startswith("global") else try_resize
    return fn(be, r, T, device, seed)


# ------------------------------------------------------------------ the walk
def walk(be, label, T, device, seed0=100):
    """Every row of one family -> (outcomes [(name, "accepted" | "refused" | "FAILED", worst | None, fro / u | None, Frobenius
    applied, kernel pick | None)], the failed checks' messages).  A failed check does not end the walk."""
    outcomes, failures = [], []
    for i, r in enumerate(rows_of(label)):
        try:
            o, worst, fro, checked = try_row(be, label, r, T, device, seed0 + i)
        except AssertionError as e:
            o, worst, fro, checked = "FAILED", None, None, False
            failures.append(str(e))
        outcomes.append((r["name"], o, worst, fro, checked, r["pick"]))
    return outcomes, failures


def matrix_line(label, kind, outcomes):
    names = {o: [n for n, oo, *_ in outcomes if oo == o] for o in ("accepted", "refused", "FAILED")}
    worst = max([x[2] for x in outcomes if x[1] == "accepted"], default=0.0)
    fro = max([x[3] for x in outcomes if x[4]], default=0.0)
    failed = f" | FAILED {len(names['FAILED'])}: {' '.join(names['FAILED'])}" if names["FAILED"] else ""
    return (f"ENVELOPE {label} | {kind} | accepted {len(names['accepted'])}: {' '.join(names['accepted']) or '-'} | "
            f"refused {len(names['refused'])}: {' '.join(names['refused']) or '-'} | worst err/bound {worst:.3f} | "
            f"worst fro/u {fro:.3f} on {sum(1 for x in outcomes if x[4])} cases{failed}")


def pick_lines(label, kind, outcomes):
    """Per kernel pick of a conv2d family: cases, Frobenius-checked cases, worst err/bound and worst checked fro/u."""
    lines = []
    for p in PICKS:
        mine = [x for x in outcomes if x[5] == p and x[1] == "accepted"]
        if mine:
            lines.append(f"ENVELOPE {label} | {kind} | {p} | cases {len(mine)} | fro-checked {sum(1 for x in mine if x[4])} | "
                         f"worst err/bound {max(x[2] for x in mine):.3f} | worst fro/u {max([x[3] for x in mine if x[4]], default=0.0):.3f}")
    return lines
