"""The guarded-launch harness of tests/guarded.py on the host: emulation and defects.

Emulation: every small case of tests/test_hip_guarded_launches.py runs with the float64 restatement, rounded to T, written through
the carves as if it were the kernel (the persistent walks at a reduced batch).  It must pass every check: the reference alone
satisfies the conditions the kernels are held to.  Defects: one element written past the end, one before the start, one interior
element left unwritten, an input row read past its end and multiplied by zero, and an output carve that is not 16-byte aligned
must each fail.
"""
import pytest
import torch

import guarded as gd
import launch_replay as lr

CPU = "cpu"
TYPES = [torch.bfloat16, torch.float16]
_ids = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _carve_of(g, view):
    return next(c for c in g.carves if c.view.data_ptr() == view.data_ptr())


def _merge_qkv(parts, n, heads, new_order):
    """The inverse of launch_replay.split_qkv: three [n heads, t, d] -> [n, t, 3 heads d]."""
    _, t, d = parts[0].shape
    x = torch.stack([p.reshape(n, heads, t, d) for p in parts], 0)     # [3, n, heads, t, d]
    x = x.permute(1, 3, 0, 2, 4) if new_order else x.permute(1, 3, 2, 0, 4)
    return x.reshape(n, t, 3 * heads * d)


class Emulated:
    """The backend of guarded.run_*: the restatements written through the carves.  defect: what a wrong kernel would do."""

    def __init__(self, defect=None):
        self.defect = defect

    def _spoil(self, g, out, src):
        """out: the launch's main output; src: an input carve's view whose row width is its last dimension."""
        c = _carve_of(g, out)
        if self.defect == "past the end":
            c.buf[c.front + c.numel] = 1.0
        elif self.defect == "before the start":
            c.buf[c.front - 1] = 1.0
        elif self.defect == "unwritten":
            out.view(-1)[out.numel() // 2] = float("nan")
        elif self.defect == "masked over-read":   # the row behind the operand's last, loaded and multiplied by zero
            s = _carve_of(g, src)
            row = s.buf[s.front + s.numel:s.front + s.numel + src.shape[-1]]
            out.view(-1)[-1] += (0.0 * row.float()).sum().to(out.dtype)

    def conv(self, d, T, t, packed, w32p, out, g):
        n = d["n"]
        ho, wo = (out.shape[2], out.shape[3]) if d["out_mode"] == 1 else (out.shape[1], out.shape[2])
        img, oy, ox = (v.reshape(-1) for v in torch.meshgrid(torch.arange(n), torch.arange(ho), torch.arange(wo), indexing="ij"))
        ref, _ = lr.conv_restate(d, T, t, img, oy, ox)
        ref = ref.reshape(n, ho, wo, -1)
        if d["out_mode"] == 1:
            out.copy_(ref.permute(0, 3, 1, 2).float())
        else:
            out.copy_(ref.to(T))
        stats = None
        if d["has_out_stats"]:   # the sums of the stored output, all in the first slab
            stats = g.out("out_stats", (n, d["expect_slabs"] or 1, d["cout"], 2), torch.float32)
            y = out.double()
            stats.zero_()
            stats[:, 0, :, 0] = y.sum((1, 2)).float()
            stats[:, 0, :, 1] = ((y * t["res"].double()) if d["prologue"] == 3 else y * y).sum((1, 2)).float()
        if d["ksplit"] > 1:
            g.out("ws", (d["ksplit"], n * d["h"] * d["w"], d["cout"]), torch.float32, gd.margin_rows(d["cout"])).zero_()
        self._spoil(g, out, t["x0"])
        return stats

    def conv_try(self, d, T, t, packed, w32p, out, g):
        """guarded.Hip.conv_try's answers from the emulation, which accepts everything; the envelope's defects refuse, or leave
        the columns behind the 16-pixel tile row unwritten."""
        slabs = (d["expect_slabs"] or 1) if d["has_out_stats"] else None
        if self.defect == "refused":
            return False, None, 0 if slabs else None, d["expect"]
        if self.defect == "slabs offered, then refused":
            return False, None, slabs, d["expect"]
        if self.defect == "refused after a partial write":
            out.view(-1)[:8] = 0.0
            return False, None, 0 if slabs else None, d["expect"]
        stats = self.conv(d, T, t, packed, w32p, out, g)
        if self.defect == "columns >= 16 unwritten":
            (out[..., 16:] if d["out_mode"] == 1 else out[:, :, 16:]).fill_(float("nan"))
        return True, stats, slabs, d["expect"]

    def attention_lse(self, qkv, out, lse, heads, d, new_order):
        n = qkv.shape[0]
        q, k, v = lr.split_qkv(qkv, heads, new_order)
        ref, _ = lr.attention_restate(q, k, v, d ** -0.5, qkv.dtype)
        out.copy_(lr.merge_heads(ref, n, heads).to(qkv.dtype))
        if lse is not None:
            lse.copy_(lr.lse_restate(q, k, d ** -0.5, qkv.dtype)[0].reshape(n, heads, -1).float())

    def attention_1h512(self, qkv, out):
        q, k, v = (qkv[:, :, i * 512:(i + 1) * 512] for i in range(3))
        out.copy_(lr.attention_restate(q, k, v, 512 ** -0.5, qkv.dtype)[0].to(qkv.dtype))

    def attention_cross(self, q, q_stride, kv, kv_stride, kv_rows, out, n, tq, tk, heads, d, scale):
        hd = heads * d
        kvv = torch.as_strided(kv, (n, kv_rows, 2 * hd), (kv_rows * kv_stride, kv_stride, 1))

        def split(x):
            return x.reshape(n, x.shape[1], heads, d).permute(0, 2, 1, 3).reshape(n * heads, x.shape[1], d)
        qh, kh, vh = split(q[:, :, :hd]), split(kvv[:, :tk, :hd]), split(kvv[:, :tk, hd:])
        ref, _ = lr.attention_restate(qh, kh, vh, scale, q.dtype)
        if self.defect == "masked over-read" and kv_rows > tk:   # the key tile's rows >= tk, loaded and weighted with zero
            ref = ref + (0.0 * split(kvv[:, tk:tk + 1, hd:]).double())
        out.copy_(lr.merge_heads(ref, n, heads).to(q.dtype))

    def attention_bwd(self, qkv, out, dout, lse, delta, dqkv, heads, d, new_order):
        n, t, _ = qkv.shape
        q, k, v = lr.split_qkv(qkv, heads, new_order)

        def split(x):
            return x.reshape(n, t, heads, d).permute(0, 2, 1, 3).reshape(n * heads, t, d)
        refs, _ = lr.attention_bwd_restate(q, k, v, split(out), split(dout), d ** -0.5, qkv.dtype)
        dqkv.copy_(_merge_qkv(refs, n, heads, new_order).to(qkv.dtype))
        delta.copy_((split(out).double() * split(dout).double()).sum(-1).reshape(n, heads, t).float())

    def gn_forward(self, mode, x0, x1, gamma, beta, film, film_stride, add, partial, partial1, a, b, stats, slabs, eps):
        x = x0 if x1 is None else torch.cat([x0, x1], 3)
        c = x.shape[3]
        _, mean, rstd = lr.gn_affine_restate(x, gamma, beta, eps, film=None if film is None else film[:, :2 * c], add=add)
        m, r = mean.repeat_interleave(c // 32, 1), rstd.repeat_interleave(c // 32, 1)
        ga, be = gamma.double(), beta.double()
        if add is not None:
            aa, bb = r * ga, be + (add.double() - m) * r * ga
        else:
            sc, sh = (film[:, :c].double(), film[:, c:2 * c].double()) if film is not None else (0.0, 0.0)
            aa, bb = r * ga * (1 + sc), (be - m * r * ga) * (1 + sc) + sh
        a.copy_(aa.float())
        b.copy_(bb.float())
        stats.copy_(torch.stack([mean, rstd], -1).float())
        for p in (partial, partial1):
            if p is not None:
                p.zero_()

    def gn_backward(self, x, dy, a, b, stats, e, add, partial, k1, k0, out, silu, dy_half, add_half, slabs, partial_given=False):
        ref, _ = lr.gn_bwd_restate(x, dy, a, b, stats, silu, dy_half, add, add_half, e, x.dtype)
        out.copy_(ref.to(x.dtype))
        for p in (partial, k1, k0):
            p.zero_()


def _ok(result):
    worst, fro, ok = result
    assert ok, (worst, fro)


def _host(d):
    return dict(d, n=d["host_n"]) if d["host_n"] else d


ALL_CONVS = gd.CONV_CASES + [c for c, _, _ in gd.walk_cases(256)]


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("case", ALL_CONVS, ids=lambda d: d["label"])
def test_conv_cases_hold_for_the_restatement(case, T):
    _ok(gd.run_conv(Emulated(), None, _host(case), T, CPU, 11))


def test_walk_cases_exceed_one_round_with_a_partly_filled_last_one():
    for cus in (256, 304, 64):
        for case, tiles, slots in gd.walk_cases(cus):
            assert tiles > slots and tiles % slots != 0 and tiles % cus != 0, (case["label"], cus, tiles, slots)


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
def test_attention_cases_hold_for_the_restatement(T):
    be = Emulated()
    for t, heads, d, new_order in gd.ATTN_LSE_CASES:
        _ok(gd.run_attention_lse(be, 2, t, heads, d, new_order, T, CPU, 13 + t))
    for _, tq, tk, rows, heads, d, alias in gd.ATTN_CROSS_CASES:
        _ok(gd.run_attention_cross(be, 2, tq, tk, rows, heads, d, alias, T, CPU, 14))
    for t in gd.ATTN_1H512_T:
        _ok(gd.run_attention_1h512(be, 2, t, T, CPU, 15 + t))
    for t, heads, d in gd.ATTN_BWD_CASES:
        for new_order in (True, False):
            _ok(gd.run_attention_bwd(be, 2, t, heads, d, new_order, T, CPU, 16 + t))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
def test_groupnorm_cases_hold_for_the_restatement(T):
    be = Emulated()
    for label, mode, n, h, w, c0, c1, film_pad, slabs in gd.GN_FWD_CASES:
        _ok(gd.run_gn_forward(be, mode, n, h, w, c0, c1, film_pad, gd.gn_slabs(h * w) if slabs is None else slabs, T, CPU, 17))
    for n, h, w, c, dy_half, has_add, add_half, silu, norm_add in gd.GN_BWD_CASES:
        _ok(gd.run_gn_backward(be, n, h, w, c, silu, dy_half, has_add, add_half, norm_add, T, CPU, 18))


DEFECTS = {"past the end": "guard past the end was written", "before the start": "guard before the start was written",
           "unwritten": "not finite", "masked over-read": "not finite"}


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("case", [gd.CONV_CASES[1], gd.CONV_CASES[9]], ids=lambda d: d["label"])
def test_conv_defects_fail(case, defect, T):
    with pytest.raises(AssertionError, match=DEFECTS[defect]):
        gd.run_conv(Emulated(defect), None, case, T, CPU, 11)


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
def test_masked_key_rows_behind_tk_fail(T):
    """kv_rows 128 > tk 77: a key tile that loads the NaN pad rows and weights them with zero leaves NaN in the output."""
    _, tq, tk, rows, heads, d, alias = gd.ATTN_CROSS_CASES[1]
    with pytest.raises(AssertionError, match="not finite"):
        gd.run_attention_cross(Emulated("masked over-read"), 2, tq, tk, rows, heads, d, alias, T, CPU, 14)


@pytest.mark.parametrize("T", TYPES + [torch.float32], ids=str)
def test_misaligned_output_carve_fails(T):
    g = gd.Guarded(CPU)
    out = g.out("out", (3, 8), T, front=gd.GUARD + 1)
    out.zero_()
    with pytest.raises(AssertionError, match="not 16-byte aligned"):
        g.check()
    g = gd.Guarded(CPU)
    g.out("out", (3, 8), T).zero_()
    g.check()


def test_margins_follow_the_written_rules():
    assert gd.margin_rows(8) == 4096 and gd.margin_rows(392) == 256 * 392 and gd.WEIGHT_MARGIN == 32 * 384
    g = gd.Guarded(CPU)
    x = g.inp("x", torch.ones(2, 3, 16), gd.margin_rows(16))
    c = g.carves[0]
    assert c.front == c.back == 4096 and c.front % 8 == 0 and bool(torch.isnan(c.buf[:c.front]).all()) and bool((x == 1).all())
    x.view(-1)[0] = 2.0
    g.check()                        # an input's interior is the test's to set
    c.buf[c.front + c.numel + 5] = 0.0
    with pytest.raises(AssertionError, match="margin past the end of an input was written"):
        g.check()


def test_an_exempted_region_is_named_and_nothing_else_is_excused():
    g = gd.Guarded(CPU)
    mask = torch.zeros(2, 4, dtype=torch.bool)
    mask[:, 3:] = True
    out = g.out("out", (2, 4), torch.float32, exempt=("rows >= t of the padded pitch are never written (include/adm_hip.h)", mask))
    out[:, :3] = 1.0
    g.check()
    out[0, 1] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        g.check()
