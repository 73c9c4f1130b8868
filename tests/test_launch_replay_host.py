"""CPU checks of tests/launch_replay.py's float64 restatements against compositions of plain torch ops (F.conv2d, F.interpolate,
F.silu, torch.cat, an explicit softmax), for every flag the replay uses, and of its pixel sampler: a wrong reference would
otherwise pass unnoticed on the GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import launch_replay as lr

BF = torch.bfloat16


def _rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rec(**kw):
    d = dict(taps=9, prologue=0, out_mode=0, ksplit=1, up_phase=0, in_up=0, res_up=0, geglu=0, out_scale=0.0,
             has_fold0=False, has_res=False)
    d.update(kw)
    return d


def _case(n=2, hs=16, c0=32, c1=0, cout=24, taps=9, pro=0, dtype=BF, seed=0):
    t = {"x0": lr.round_t(_rnd((n, hs, hs, c0), seed), dtype), "x1": lr.round_t(_rnd((n, hs, hs, c1), seed + 1), dtype) if c1 else None,
         "a": 1 + 0.2 * _rnd((n, c0 + c1), seed + 2), "b": 0.2 * _rnd((n, c0 + c1), seed + 3),
         "bias": 0.1 * _rnd((cout,), seed + 4)}
    k = 3 if taps == 9 else 1
    t["w"] = lr.round_t(_rnd((cout, c0 + c1, k, k), seed + 5, (c0 + c1) ** -0.5), dtype)
    return t


def _act(t, pro, dtype):
    x = t["x0"] if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 3)
    x = x.permute(0, 3, 1, 2)
    if pro:
        x = t["a"][:, :, None, None] * x + t["b"][:, :, None, None]
        if pro == 2:
            x = F.silu(x)
        x = lr.round_t(x, dtype)
    return x.double()


def _all_pixels(n, h, w):
    return lr.sample_pixels(n, h, w, 0) if h * w <= 256 else tuple(
        g.reshape(-1) for g in torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij"))


def _at(ref_nchw, img, y, x):
    return ref_nchw.permute(0, 2, 3, 1)[img, y, x]


@pytest.mark.parametrize("dtype", [BF, torch.float16])
@pytest.mark.parametrize("taps,pro,c1", [(9, 0, 0), (9, 1, 32), (9, 2, 0), (1, 2, 64), (1, 0, 0)])
def test_conv_restatement_matches_torch(dtype, taps, pro, c1):
    n, hs, cout = 2, 16, 24
    t = _case(n, hs, 32, c1, cout, taps, pro, dtype)
    ref = F.conv2d(_act(t, pro, dtype), t["w"].double(), t["bias"].double(), padding=1 if taps == 9 else 0)
    img, y, x = _all_pixels(n, hs, hs)
    got, bound = lr.conv_restate(_rec(taps=taps, prologue=pro), dtype, t, img, y, x)
    err = (got - _at(ref, img, y, x)).abs()
    # the composition's prologue (a * x, then + b) may round one fp32 ulp off the restatement's fused multiply-add: a value at a
    # T midpoint then rounds the other way -- the case the bound's rounding-risk term covers
    assert (err <= bound).all() and (err <= 1e-9).float().mean() >= 0.95, err.max()
    # residual and the fp32 NCHW epilogue with out_scale
    t["res"] = lr.round_t(_rnd((n, hs, hs, cout), 9), dtype)
    base = got
    got, _ = lr.conv_restate(_rec(taps=taps, prologue=pro, has_res=True), dtype, t, img, y, x)
    torch.testing.assert_close(got, base + t["res"][img, y, x].double(), rtol=1e-12, atol=1e-12)
    got, _ = lr.conv_restate(_rec(taps=taps, prologue=pro, out_mode=1, out_scale=2.0 ** -10), dtype, t, img, y, x)
    torch.testing.assert_close(got, base * 2.0 ** -10, rtol=1e-12, atol=1e-15)


def test_conv_restatement_virtual_upsample():
    n, hs, cout = 2, 8, 16
    t = _case(n, hs, 32, 0, cout, 9, 2)
    t["res"] = lr.round_t(_rnd((n, hs, hs, cout), 9), BF)
    up = F.interpolate(_act(t, 2, BF), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, t["w"].double(), t["bias"].double(), padding=1) + F.interpolate(t["res"].permute(0, 3, 1, 2).double(),
                                                                                     scale_factor=2, mode="nearest")
    img, y, x = _all_pixels(n, 2 * hs, 2 * hs)
    got, _ = lr.conv_restate(_rec(prologue=2, in_up=1, res_up=1, has_res=True), BF, t, img, y, x)
    torch.testing.assert_close(got, _at(ref, img, y, x), rtol=1e-9, atol=1e-9)


def test_conv_restatement_up_phases():
    """up_phase 5 with the phase weights of ops.up_phase_weights: equal to conv3x3(upsample(x)) when the pre-summed taps are exact
    (small-integer weights)."""
    from autodiffusion_amd.ops import up_phase_weights
    n, hs, cout = 2, 8, 16
    t = _case(n, hs, 32, 0, cout, 9, 1)
    w = torch.randint(-3, 4, (cout, 32, 3, 3), generator=torch.Generator().manual_seed(3)).float()
    t["w"] = up_phase_weights(w)
    up = F.interpolate(_act(t, 1, BF), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, w.double(), t["bias"].double(), padding=1)
    img, y, x = _all_pixels(n, 2 * hs, 2 * hs)
    got, _ = lr.conv_restate(_rec(prologue=1, up_phase=5), BF, t, img, y, x)
    torch.testing.assert_close(got, _at(ref, img, y, x), rtol=1e-9, atol=1e-9)


def test_conv_restatement_fold_geglu_and_gn_backward_epilogue():
    n, hs, cout = 2, 8, 32
    t = _case(n, hs, 32, 0, cout, 9, 2)
    t["f0"], t["f1"] = lr.round_t(_rnd((n, hs, hs, 32), 11), BF), lr.round_t(_rnd((n, hs, hs, 64), 12), BF)
    t["w1"] = lr.round_t(_rnd((cout, 96), 13, 0.1), BF)
    xs = torch.cat([t["f0"], t["f1"]], 3).permute(0, 3, 1, 2).double()
    base = F.conv2d(_act(t, 2, BF), t["w"].double(), t["bias"].double(), padding=1)
    ref = base + F.conv2d(xs, t["w1"].double()[:, :, None, None])
    img, y, x = _all_pixels(n, hs, hs)
    got, _ = lr.conv_restate(_rec(prologue=2, has_fold0=True), BF, t, img, y, x)
    torch.testing.assert_close(got, _at(ref, img, y, x), rtol=1e-9, atol=1e-9)
    # GEGLU: rows interleaved (value m, gate m), as ops.geglu_interleave lays them out
    from autodiffusion_amd.ops import geglu_interleave
    t1 = _case(n, hs, 64, 0, 2 * cout, 1, 0)
    wi, bi = geglu_interleave(t1["w"][:, :, 0, 0], t1["bias"])
    t1["w"], t1["bias"] = wi[:, :, None, None], bi
    u = F.conv2d(_act(t1, 0, BF), t1["w"].double()[:cout * 2], t1["bias"].double())   # interleaved channels
    val, gate = u[:, 0::2], u[:, 1::2]
    gl = val * F.gelu(gate)
    got, _ = lr.conv_restate(_rec(taps=1, geglu=1), BF, t1, img, y, x)
    torch.testing.assert_close(got, _at(gl, img, y, x), rtol=1e-9, atol=1e-9)
    # prologue 3: dz = conv * SiLU'(a x + b) with x = res
    t3 = _case(n, hs, 32, 0, cout, 9, 0)
    t3["res"] = lr.round_t(_rnd((n, hs, hs, cout), 14), BF)
    t3["gnb_a"], t3["gnb_b"] = 1 + 0.2 * _rnd((n, cout), 15), 0.2 * _rnd((n, cout), 16)
    z = (t3["gnb_a"].double()[:, :, None, None] * t3["res"].permute(0, 3, 1, 2).double()
         + t3["gnb_b"].double()[:, :, None, None]).requires_grad_()
    F.silu(z).sum().backward()
    ref3 = F.conv2d(_act(t3, 0, BF), t3["w"].double(), t3["bias"].double(), padding=1) * z.grad
    got, _ = lr.conv_restate(_rec(prologue=3, has_res=True), BF, t3, img, y, x)
    torch.testing.assert_close(got, _at(ref3, img, y, x), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("new_order", [True, False])
def test_attention_restatement_matches_explicit_softmax(new_order):
    from oracle import nets
    n, heads, d, t = 2, 3, 16, 20
    qkv = lr.round_t(_rnd((n, t, 3 * heads * d), 1), BF)
    q, k, v = lr.split_qkv(qkv, heads, new_order)
    ref, bound = lr.attention_restate(q, k, v, d ** -0.5, BF)
    s = q.double() @ k.double().transpose(1, 2) / math.sqrt(d)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    mine = (e / e.sum(-1, keepdim=True)) @ v.double()
    torch.testing.assert_close(ref, mine, rtol=1e-12, atol=1e-12)
    orc = nets.qkv_attention(qkv.permute(0, 2, 1).double(), heads, new_order).permute(0, 2, 1)   # [n, t, H D]
    torch.testing.assert_close(lr.merge_heads(ref, n, heads), orc, rtol=1e-5, atol=1e-5)   # its softmax runs in fp32
    assert (bound >= lr.C_ATTN * lr.U[BF] * v.abs().amax(1, keepdim=True)).all()


def test_sampler_hits_every_tile_corner():
    for h, w, tile in ((64, 64, 16), (48, 32, 16), (256, 256, 16), (16, 8, 8), (40, 24, 16)):
        img, y, x = lr.sample_pixels(3, h, w, 5)
        got = set(zip(img.tolist(), y.tolist(), x.tolist()))
        for i in range(3):
            for ty in range(0, h, tile):
                for tx in range(0, w, tile):
                    y1, x1 = min(h, ty + tile) - 1, min(w, tx + tile) - 1
                    for c in ((ty, tx), (ty, x1), (y1, tx), (y1, x1)):
                        assert (i,) + c in got, (h, w, i, c)
        assert (img < 3).all() and (y < h).all() and (x < w).all()
    img, y, x = lr.sample_pixels(2, 8, 8, 0)     # small maps: every pixel
    assert img.numel() == 2 * 64


def test_ulp_and_prologue_risk():
    v = torch.tensor([1.0, 1.5, 2.0, 3.0e-6, 0.0], dtype=torch.float64)
    assert lr.ulp_t(v, BF).tolist()[:3] == [2 ** -7, 2 ** -7, 2 ** -6]
    assert lr.ulp_t(v, torch.float16)[:3].tolist() == [2 ** -10, 2 ** -10, 2 ** -9]
    assert lr.ulp_t(v, torch.float16)[3].item() == 2 ** -24 and lr.ulp_t(v, torch.float16)[4].item() == 2 ** -24
    # a value one fp32 ulp from a bf16 rounding midpoint is at risk, one far from it is not
    mid = torch.tensor([1.0 + 2 ** -8 + 2 ** -23, 1.0 + 2 ** -10, 2.0 - 2 ** -8 + 2 ** -22])
    r, risk = lr.prologue(mid, torch.ones(3), torch.zeros(3), 1, BF)
    assert risk[0].item() == 2 ** -7 and risk[1].item() == 0.0
    # just above the midpoint below a power of two: rounds up to 2.0, one fp32 ulp less rounds down by the smaller step
    assert r[2].item() == 2.0 and risk[2].item() == 2 ** -7


def test_families_cover_labels():
    from autodiffusion_amd._lib import ConvArgs
    a = ConvArgs()
    a.n, a.h, a.w, a.c0, a.cout, a.taps, a.variant, a.ksplit, a.out_mode, a.out_scale = 2, 8, 8, 64, 64, 9, 5, 2, 0, 0.0
    f = lr.families(lr.conv_record("f16", a))
    assert f == {("f16", "variant 5"), ("f16", "ksplit > 1"), ("f16", "8x8 map")}
    assert lr.families(("attention_cross", "bf16", 1, 64, 3 * 480, 64, 3 * 480, 64, 10, 48, 0.15)) == {("bf16", "attention_cross d 48 (self)")}


def test_attention_backward_and_lse_restatements_match_autograd():
    n, t, d = 3, 24, 16
    q, k, v, do = (_rnd((n, t, d), s_) for s_ in (1, 2, 3, 4))
    q, k, v = (x.double().requires_grad_() for x in (q, k, v))
    scale = d ** -0.5
    o = torch.softmax(q @ k.transpose(1, 2) * scale, -1) @ v
    o.backward(do.double())
    (dq, dk, dv), bounds = lr.attention_bwd_restate(q.detach(), k.detach(), v.detach(), o.detach(), do, scale, BF)
    for got, ref in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-10)
    assert all((b > 0).all() for b in bounds)
    lse, lb = lr.lse_restate(q.detach(), k.detach(), scale, BF)
    torch.testing.assert_close(lse * math.log(2.0), torch.logsumexp(q.detach() @ k.detach().transpose(1, 2) * scale, -1))


@pytest.mark.parametrize("silu,dy_half,add_half,with_e", [(True, False, False, False), (False, True, True, True), (True, True, False, True)])
def test_gn_backward_restatement_matches_autograd(silu, dy_half, add_half, with_e):
    """dx of act(GroupNorm(x + e) * g + s) by autograd against the restatement fed (a, b) = the layer's affine on the stored x and the
    float64 (mean, rstd) of x + e."""
    n, h, w, c = 2, 4, 4, 64
    x = lr.round_t(_rnd((n, h, w, c), 1), BF).double()
    e = 0.5 * _rnd((n, c), 2).double() if with_e else None
    g, sft = (1 + 0.2 * _rnd((n, c), 3)).double(), 0.2 * _rnd((n, c), 4).double()
    dy = lr.round_t(_rnd((n, h // 2, w // 2, c) if dy_half else (n, h, w, c), 5), BF).double()
    add = lr.round_t(_rnd((n, h // 2, w // 2, c) if add_half else (n, h, w, c), 6), BF).double()
    xr = x.clone().requires_grad_()
    xe = xr if e is None else xr + e[:, None, None, :]
    y = F.group_norm(xe.permute(0, 3, 1, 2), 32, eps=1e-5).permute(0, 2, 3, 1) * g[:, None, None, :] + sft[:, None, None, :]
    if silu:
        y = F.silu(y)
    dyf = lr._half_up(dy, h, w) if dy_half else dy
    y.backward(dyf)
    ref = xr.grad + (lr._half_up(add, h, w) if add_half else add)
    _, mean, rstd = lr.gn_affine_restate(x, torch.ones(c), torch.zeros(c), 1e-5, add=e)
    r_c, m_c = rstd.repeat_interleave(2, 1), mean.repeat_interleave(2, 1)
    a = g * r_c
    b = sft - m_c * a + (a * e if e is not None else 0)
    got, bound = lr.gn_bwd_restate(x, dy, a, b, torch.stack([mean, rstd], -1), silu, dy_half, add, add_half, e, BF)
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-9)
    assert (bound > 0).all()


def test_gn_affine_restatement_matches_group_norm():
    n, h, w, c = 2, 4, 4, 64
    x = _rnd((n, h, w, c), 1).double()
    gamma, beta, film, add = 1 + 0.2 * _rnd((c,), 2), 0.1 * _rnd((c,), 3), 0.3 * _rnd((n, 2 * c), 4), 0.5 * _rnd((n, c), 5)
    y, _, _ = lr.gn_affine_restate(x, gamma, beta, 1e-5, film=film)
    ref = F.group_norm(x.permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 3, 1)
    torch.testing.assert_close(y, ref * (1 + film[:, None, None, :c].double()) + film[:, None, None, c:].double())
    y, _, _ = lr.gn_affine_restate(x, gamma, beta, 1e-6, add=add)
    xe = (x + add.double()[:, None, None, :]).permute(0, 3, 1, 2)
    torch.testing.assert_close(y, F.group_norm(xe, 32, gamma.double(), beta.double(), eps=1e-6).permute(0, 2, 3, 1))
