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


# ------------------------------------------------------------------ the census and the coverage table
def test_symbol_coverage_names_every_launch_symbol_and_nothing_else():
    from autodiffusion_amd import _lib
    syms = lr.launch_symbols()
    assert set(syms) == set(lr.SYMBOL_COVERAGE), set(syms) ^ set(lr.SYMBOL_COVERAGE)
    assert "adm_conv" in syms and "adm_layernorm" in syms and "adm_vae_image_out" in syms
    # not launches: no stream argument, or stream management
    for name in ("adm_abi_version", "adm_conv_stat_slabs", "adm_conv_pick_variant", "adm_packed_weight_elems", "adm_stream_destroy",
                 "adm_stream_probe"):
        assert name in _lib.SIGNATURES and name not in syms
    for sym, cov in lr.SYMBOL_COVERAGE.items():
        if cov[0] == "elsewhere":
            assert len(cov) == 2 and cov[1].startswith("tests/") and "::" in cov[1], (sym, cov)
        else:
            assert set(cov) <= lr.REPLAYED, (sym, cov)
    # every new record kind is a required family and replays some symbol
    kinds = {k for cov in lr.SYMBOL_COVERAGE.values() if cov[0] != "elsewhere" for k in cov}
    assert set(lr.NEW_KINDS) <= kinds and set(lr.NEW_KINDS) <= set(lr.REQUIRED_FAMILIES) and kinds == lr.REPLAYED


def test_every_test_named_elsewhere_exists():
    import ast
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    defs = {}
    for cov in lr.SYMBOL_COVERAGE.values():
        if cov[0] != "elsewhere":
            continue
        path, name = cov[1].split("::")
        if path not in defs:
            with open(os.path.join(root, path)) as f:
                defs[path] = {n.name for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.FunctionDef)}
        assert name.startswith("test_") and name in defs[path], cov


def _fake_records():
    """One record per new kind and library (the classifier heads' from _fake_head_records), and the VAE's / CLIP's conv and attention
    families, shaped as the recorder shapes them."""
    from autodiffusion_amd._lib import ConvArgs
    recs = {}
    for kind in ("bf16", "f16"):
        a = ConvArgs()
        a.n, a.h, a.w, a.c0, a.cout, a.taps, a.variant = 3, 8, 16, 768, 2304, 1, 10
        recs[("clip conv", kind)] = lr.conv_record(kind, a)
        recs[("vae attention", kind)] = ("attention", kind, 1, 4096, 1536, 1, True, False)
        recs[("layernorm", kind)] = ("layernorm", kind, 384, 768, 1e-5)
        recs[("layernorm_f32out", kind)] = ("layernorm_f32out", kind, 3, 77, 128, 768, 1e-5)
        recs[("geglu", kind)] = ("geglu", kind, 1536, 5120)
        recs[("quick_gelu", kind)] = ("quick_gelu", kind, 384, 3072)
        recs[("attention_causal", kind)] = ("attention_causal", kind, 3, 77, 128, 12)
        recs[("clip_embed", kind)] = ("clip_embed", kind, 3, 77, 128, 768, 49408, 77)
        recs[("resample", kind)] = ("resample", kind, 2, 16, 16, 256, 1, True)
        recs[("nchw_to_nhwc_pad", kind)] = ("nchw_to_nhwc_pad", kind, 2, 3, 64, 64, 32)
        recs[("vae_latent_in", kind)] = ("vae_latent_in", kind, 1, 4, 4, 64, 64)
        recs[("conv2d", kind)] = ("conv2d", kind, ("cin", 320), ("cout", 320))
        recs[("stem_conv3x3", kind)] = ("stem_conv3x3", kind, 1, 3, 512, 512, 128)
    recs[("vae_image_out", "bf16")] = ("vae_image_out", "bf16", 1, 512, 512, True, True)
    recs.update(_fake_head_records())
    return recs


def test_coverage_guard_fails_when_a_model_or_a_hook_is_removed():
    """With a stubbed census (every replayed symbol called on both libraries): the full record set passes; without any one new
    hook's records, without the VAE's or without the CLIP encoder's, the guard names what is missing."""
    recs = _fake_records()
    here = {s: cov for s, cov in lr.SYMBOL_COVERAGE.items() if cov[0] != "elsewhere" and set(cov) & set(lr.NEW_KINDS)}
    one_library = {"adm_" + f for f, k in lr.ONE_LIBRARY_FAMILIES.items() if k == "bf16"}   # fp32 kernels on the bf16 library alone
    census = {(s, k) for s in here for k in ("bf16", "f16") if not (s in one_library and k == "f16")}
    census |= {("adm_stem_conv3x3", k) for k in ("bf16", "f16")}   # the KL-f8 encoder's conv_in: a record kind of its own
    assert lr.coverage_gaps(census, recs.values(), lr.REPLAYED) == []
    left = [r for r in recs.values() if r[0] != "stem_conv3x3"]          # its hook removed from the recorder
    gaps = lr.coverage_gaps(census, left, lr.REPLAYED)
    assert len(gaps) == 2 and all("adm_stem_conv3x3" in g and "no stem_conv3x3 record" in g for g in gaps), gaps
    assert "not replayed" in lr.coverage_gaps({("adm_stem_conv3x3", "bf16")}, recs.values(), lr.REPLAYED - {"stem_conv3x3"})[0]
    new = set(lr.NEW_KINDS) | {"attention d 512", "non-square map"}
    assert not [m for m in lr.missing_families(recs.values()) if m[1] in new]
    for kind in lr.NEW_KINDS:   # one hook removed from the recorder
        left = [r for r in recs.values() if r[0] != kind]
        gaps = lr.coverage_gaps(census, left, lr.REPLAYED)
        assert gaps and all(kind in g for g in gaps), (kind, gaps)
        assert {m[1] for m in lr.missing_families(left)} & new == {kind}
    vae = {"vae attention", "vae_latent_in", "vae_image_out"}
    left = [r for k, r in recs.items() if k[0] not in vae]
    assert {m[1] for m in lr.missing_families(left)} & new == {"attention d 512", "vae_latent_in", "vae_image_out"}
    assert len(lr.coverage_gaps(census, left, lr.REPLAYED)) == 3   # adm_vae_latent_in on both libraries, adm_vae_image_out
    clip = {"clip conv", "layernorm_f32out", "quick_gelu", "attention_causal", "clip_embed"}
    left = [r for k, r in recs.items() if k[0] not in clip]
    assert {m[1] for m in lr.missing_families(left)} & new == {"non-square map", "layernorm_f32out", "quick_gelu", "attention_causal", "clip_embed"}
    # a launch symbol nobody listed, and a kind the replay does not take
    assert "no entry" in lr.coverage_gaps({("adm_brand_new", "bf16")}, recs.values(), lr.REPLAYED)[0]
    assert "not replayed" in lr.coverage_gaps({("adm_geglu", "bf16")}, recs.values(), lr.REPLAYED - {"geglu"})[0]
    # a record taken on the other library does not stand in
    assert lr.coverage_gaps({("adm_geglu", "f16")}, [recs[("geglu", "bf16")]], lr.REPLAYED)


def test_recorder_notes_every_launch_symbol_on_both_libraries():
    """The census hook sits on every launch symbol of both libraries and passes the call through: a call with null pointers is
    refused by the library's own argument check (no GPU needed) and is noted all the same."""
    from autodiffusion_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        for kind in ("bf16", "f16"):
            lib = _lib.load(kind)
            assert lib.adm_layernorm(None, None, None, None, 4, 64, 1e-5, None) != 0
            assert lib.adm_vae_image_out(None, None, None, 1, 8, 8, None) != 0
            assert type(lib.adm_conv_stat_slabs).__name__ == "_FuncPtr"   # not a launch: left alone
        assert rec.census == {(s, k) for s in ("adm_layernorm", "adm_vae_image_out") for k in ("bf16", "f16")}
        assert rec.records == set()
    assert _lib.load().adm_layernorm.argtypes is not None   # the patch is undone: the ctypes function is back


# ------------------------------------------------------------------ fp32 emulations of the kernels' arithmetic
TYPES = [BF, torch.float16]
F32 = torch.float32


def _truncate(y32, dtype):
    """Conversion to T that truncates towards zero instead of rounding to nearest (the defect the Frobenius bound catches)."""
    r = y32.to(dtype)
    over = r.float().abs() > y32.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)


def _layernorm_emulated(x, gamma, beta, eps, c_minus_one=False):
    """adm_layernorm's fp32 arithmetic in its own order: lane l of 64 adds the 8 values of its segments l, l + 64, ..., six butterfly
    steps follow; mean, then the variance of the centred values the same way."""
    rows, c = x.shape
    segs = (c // 8 + 63) // 64
    xp = F.pad(x.to(F32), (0, segs * 512 - c)).reshape(rows, segs, 64, 8).permute(0, 2, 1, 3).reshape(rows, 64, segs * 8)
    live = F.pad(torch.ones(c), (0, segs * 512 - c)).reshape(segs, 64, 8).permute(1, 0, 2).reshape(64, segs * 8).bool()

    def wave_sum(v):   # v [rows, 64, segs * 8] -> [rows, 1, 1]
        s = torch.zeros(rows, 64, dtype=F32)
        for j in range(v.shape[2]):
            s = s + v[:, :, j]
        lanes = torch.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ off]
        return s[:, :1, None]
    inv_c = torch.tensor(1.0 / c, dtype=F32)
    mean = wave_sum(xp) * inv_c
    d = torch.where(live, xp - mean, torch.zeros(()))
    var = wave_sum(d * d) * (torch.tensor(1.0 / (c - 1), dtype=F32) if c_minus_one else inv_c)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    y = (xp - mean) * rstd
    y = y.reshape(rows, 64, segs, 8).permute(0, 2, 1, 3).reshape(rows, segs * 512)[:, :c]
    return y * gamma.to(F32) + beta.to(F32)


def _ln_case(rows, c, ratio, dtype, seed, std=1.0):
    x = lr.round_t((_rnd((rows, c), seed) + ratio) * std, dtype)
    return x, 1 + 0.2 * _rnd((c,), seed + 1), 0.1 * _rnd((c,), seed + 2)


def test_layernorm_restatement_matches_torch():
    x, g, b = _ln_case(9, 320, 0.5, BF, 1)
    ref, bound = lr.layernorm_restate(x, g, b, 1e-5, BF)
    torch.testing.assert_close(ref, F.layer_norm(x.double(), (320,), g.double(), b.double(), 1e-5), rtol=1e-12, atol=1e-12)
    ref32, bound32 = lr.layernorm_restate(x, g, b, 1e-5, BF, f32out=True)
    assert torch.equal(ref, ref32) and (bound32 < bound).all() and (bound32 > 0).all()
    torch.testing.assert_close(bound - bound32, 0.5 * lr.ulp_t(ref, BF), rtol=1e-9, atol=0)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("c", [64, 320, 768, 1280, 2048])
def test_layernorm_emulation_stays_within_the_bound_and_defects_do_not(c, dtype):
    u = lr.U[dtype]
    for ratio in (0.25, 8, 32):
        x, g, b = _ln_case(16, c, ratio, dtype, c + int(ratio))
        ref, bound = lr.layernorm_restate(x, g, b, 1e-5, dtype)
        y32 = _layernorm_emulated(x, g, b, 1e-5)
        err = (y32.to(dtype).double() - ref).abs()
        assert (err <= bound).all(), (c, ratio, (err / bound).max())
        assert (bound / (0.5 * lr.ulp_t(ref, dtype))).median() <= 1.34   # the bound stays close to a bare half ulp
        fro = (err.norm() / ref.norm()).item()
        assert fro <= lr.fro_bound(1, u), fro / u
        # fp32 output: the same arithmetic without the rounding to T
        ref32, bound32 = lr.layernorm_restate(x, g, b, 1e-5, dtype, f32out=True)
        assert ((y32.double() - ref32).abs() <= bound32).all()
        # a variance over c - 1
        bad = _layernorm_emulated(x, g, b, 1e-5, c_minus_one=True)
        assert ((bad.to(dtype).double() - ref).abs() > bound).any() and ((bad.double() - ref32).abs() > bound32).any()
        # a store that truncates: inside the per-element bound or not, the Frobenius bound refuses it
        tr = (_truncate(y32, dtype).double() - ref).norm() / ref.norm()
        assert tr > lr.fro_bound(1, u), tr / u
    # eps 1e-6 where 1e-5 is meant shows where the variance is small
    x, g, b = _ln_case(16, c, 0.25, dtype, 5, std=2.0 ** -8)
    ref, bound = lr.layernorm_restate(x, g, b, 1e-5, dtype)
    assert ((_layernorm_emulated(x, g, b, 1e-5).to(dtype).double() - ref).abs() <= bound).all()
    assert ((_layernorm_emulated(x, g, b, 1e-6).to(dtype).double() - ref).abs() > bound).any()


@pytest.mark.parametrize("dtype", TYPES)
def test_geglu_restatement_emulation_and_defects(dtype):
    inner = 96
    u16 = lr.round_t(_rnd((40, 2 * inner), 3, 1.5), dtype)
    ref, bound = lr.geglu_restate(u16, dtype)
    v, g = u16.double().chunk(2, -1)
    torch.testing.assert_close(ref, v * F.gelu(g), rtol=1e-12, atol=1e-12)
    v32, g32 = u16.to(F32).chunk(2, -1)
    emu = v32 * (0.5 * g32 * (1.0 + torch.erf(g32 * 0.70710678118654752)))
    err = (emu.to(dtype).double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max()
    assert err.norm() / ref.norm() <= lr.fro_bound(1, lr.U[dtype])
    tanh = v32 * F.gelu(g32, approximate="tanh")
    assert ((tanh.to(dtype).double() - ref).abs() > bound).any()
    gate_first = v32 * lr.round_t(F.gelu(g32), dtype)          # the gate rounded to T before the product
    assert ((gate_first.to(dtype).double() - ref).abs() > bound).any()
    assert (_truncate(emu, dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, lr.U[dtype])


@pytest.mark.parametrize("dtype", TYPES)
def test_quick_gelu_restatement_emulation_and_defects(dtype):
    a = _rnd((64, 128), 4, 4.0)
    a.view(-1)[:8] = torch.tensor(lr.QUICK_GELU_SPECIALS)
    a = lr.round_t(a, dtype)
    ref, bound = lr.quick_gelu_restate(a, dtype)
    torch.testing.assert_close(ref, a.double() * torch.sigmoid(1.702 * a.double()), rtol=0, atol=0)
    torch.testing.assert_close(ref, (a.double() * torch.sigmoid(1.702 * a.double())), rtol=1e-12, atol=1e-300)
    a32 = a.to(F32)
    k = torch.tensor(-1.702, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)
    emu = a32 * (1.0 / (1.0 + torch.exp2(a32 * k)))
    err = (emu.to(dtype).double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max()
    assert err.norm() / ref.norm() <= lr.fro_bound(1, lr.U[dtype])
    bad = a32 * torch.sigmoid(1.7 * a32)
    assert ((bad.to(dtype).double() - ref).abs() > bound).any()
    assert (_truncate(emu, dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, lr.U[dtype])


def _causal_emulated(q, k, v, dtype, shift=0):
    """fp32 logits, exp2 of the scaled distance to the row maximum, P rounded to T for the PV product, the row sum of the fp32 P;
    shift = -1 drops the diagonal key, +1 admits one key above it."""
    t = q.shape[1]
    s = q.to(F32) @ k.to(F32).transpose(1, 2)
    dead = torch.ones(t, t, dtype=torch.bool).triu(1 + shift)
    s = s.masked_fill(dead, -1e30)
    c = torch.tensor(1.4426950408889634 * 0.125, dtype=F32)
    p = torch.exp2((s - s.amax(-1, keepdim=True)) * c).masked_fill(dead, 0.0)
    o = (lr.round_t(p, dtype) @ v.to(F32)) / p.sum(-1, keepdim=True)
    return o.to(dtype)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("t", [1, 17, 77, 256])
def test_causal_attention_restatement_emulation_and_defects(t, dtype):
    heads = 2
    q, k, v = (lr.round_t(_rnd((heads, t, 64), 10 + i), dtype) for i in range(3))
    ref, bound = lr.attention_restate(q, k, v, 0.125, dtype, causal=True)
    s = q.double() @ k.double().transpose(1, 2) * 0.125
    keep = torch.ones(t, t, dtype=torch.bool).tril()
    e = torch.where(keep, torch.exp(s - torch.where(keep, s, torch.full_like(s, -1e300)).amax(-1, keepdim=True)), torch.zeros_like(s))
    torch.testing.assert_close(ref, (e / e.sum(-1, keepdim=True)) @ v.double(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref[:, 0], v.double()[:, 0], rtol=0, atol=0)          # the first query sees its own key only
    # the bound of a row is the plain bound of that row's prefix
    for i in (0, t // 2, t - 1):
        r1, b1 = lr.attention_restate(q[:, i:i + 1], k[:, :i + 1], v[:, :i + 1], 0.125, dtype)
        torch.testing.assert_close(ref[:, i:i + 1], r1, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(bound[:, i:i + 1], b1, rtol=1e-9, atol=0)
    got = _causal_emulated(q, k, v, dtype).double()
    err = (got - ref).abs()
    assert (err <= bound).all(), (err / bound).max()
    assert err.norm() / ref.norm() <= lr.fro_bound(2, lr.U[dtype])
    if t > 1:
        for shift in (-1, 1):   # the mask off by one, either way
            bad = _causal_emulated(q, k, v, dtype, shift).double()[:, 1:]
            assert ((bad - ref[:, 1:]).abs() > bound[:, 1:]).any(), shift


@pytest.mark.parametrize("dtype", TYPES)
def test_clip_embed_restatement_and_a_shifted_position_row(dtype):
    n, t, pitch, c, vocab = 2, 20, 64, 32, 50
    tok, pos = _rnd((vocab, c), 1), _rnd((77, c), 2, 0.3)
    ids = torch.randint(0, vocab, (n, t), generator=torch.Generator().manual_seed(3))
    ref = lr.clip_embed_restate(ids, tok, pos, pitch, dtype)
    assert ref.shape == (n, pitch, c) and ref.dtype == dtype
    assert torch.equal(ref[:, :t], (F.embedding(ids, tok) + pos[:t]).to(dtype)) and bool((ref[:, t:] == 0).all())
    shifted = (F.embedding(ids, tok) + pos[1:t + 1]).to(dtype)
    assert not torch.equal(ref[:, :t], shifted)
    assert not torch.equal(ref[:, :t], (F.embedding(ids, tok).to(dtype) + pos[:t].to(dtype)))   # rounding the operands first


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("with_aff", [False, True])
def test_resample_restatement_emulation_and_defects(with_aff, dtype):
    n, h, w, c = 2, 6, 4, 16
    u = lr.U[dtype]
    x = lr.round_t(_rnd((n, h, w, c), 5), dtype)
    aff = (1 + 0.2 * _rnd((n, c), 6), 0.2 * _rnd((n, c), 7)) if with_aff else None
    xc = x.permute(0, 3, 1, 2).double()
    if with_aff:
        xc = F.silu(aff[0].double()[:, :, None, None] * xc + aff[1].double()[:, :, None, None])
    x32 = x.to(F32)
    s32 = F.silu(aff[0][:, None, None, :] * x32 + aff[1][:, None, None, :]) if with_aff else x32
    plain = {1: F.avg_pool2d(xc, 2), 2: F.interpolate(xc, scale_factor=2, mode="nearest"), 3: xc[:, :, ::2, ::2],
             4: F.conv_transpose2d(xc, torch.ones(c, 1, 1, 1, dtype=torch.float64), stride=2, groups=c, output_padding=1)}
    emu = {1: (((s32[:, 0::2, 0::2] + s32[:, 0::2, 1::2]) + s32[:, 1::2, 0::2]) + s32[:, 1::2, 1::2]) * 0.25,
           2: s32.repeat_interleave(2, 1).repeat_interleave(2, 2), 3: s32[:, ::2, ::2]}
    for mode in (1, 2, 3) + (() if with_aff else (4,)):
        ref, bound = lr.resample_restate(x, mode, aff, dtype)
        torch.testing.assert_close(ref, plain[mode].permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        if mode != 1 and not with_aff:
            assert bound is None and torch.equal(ref.to(dtype).double(), ref)      # a copy of T values: bitwise
            continue
        err = (emu[mode].to(dtype).double() - ref).abs()
        assert (err <= bound).all(), (mode, (err / bound).max())
        assert (bound <= 1.01 * 0.5 * lr.ulp_t(ref, dtype) + 2.0 ** -19 * (1 + ref.abs())).all()
        assert err.norm() / ref.norm() <= lr.fro_bound(1, u)
        assert (_truncate(emu[mode], dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, u)
    # the taps rounded to T before the mean (with the affine), or a sum of four without the 1 / 4
    ref, bound = lr.resample_restate(x, 1, aff, dtype)
    bad = emu[1] * 4 if not with_aff else F.avg_pool2d(lr.round_t(s32, dtype).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert ((bad.to(dtype).double() - ref).abs() > bound).any()
    with pytest.raises(NotImplementedError):
        lr.resample_restate(x, 4, (torch.ones(n, c), torch.zeros(n, c)), dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_nchw_to_nhwc_pad_restatement(dtype):
    x = _rnd((2, 3, 5, 7), 8, 1.5)
    ref = lr.nchw_to_nhwc_pad_restate(x, 32, dtype)
    assert ref.shape == (2, 5, 7, 32) and ref.dtype == dtype
    assert torch.equal(ref, F.pad(x.permute(0, 2, 3, 1), (0, 29)).to(dtype))
    assert not torch.equal(ref, _truncate(F.pad(x.permute(0, 2, 3, 1), (0, 29)), dtype))


@pytest.mark.parametrize("dtype", TYPES)
def test_vae_latent_in_restatement_emulation_and_defects(dtype):
    import numpy as np
    n, e, zc, h, w = 2, 4, 4, 9, 5
    inv = float(np.float32(1.0 / 0.18215))
    z, wt, b = _rnd((n, e, h, w), 1, 4 * 0.18215), _rnd((zc, e, 1, 1), 2, 0.5), _rnd((zc,), 3, 0.1)
    ref, bound = lr.vae_latent_in_restate(z, wt, b, inv, dtype)
    torch.testing.assert_close(ref, F.conv2d(z.double() * inv, wt.double(), b.double()).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    zs = (torch.tensor(inv, dtype=F32) * z).permute(0, 2, 3, 1)                # one fp32 product, then e fused multiply-adds
    acc = torch.zeros(n, h, w, zc, dtype=F32)
    for j in range(e):
        acc = (wt[:, j, 0, 0].double() * zs[..., j:j + 1].double() + acc.double()).to(F32)
    emu = acc + b
    err = (emu.to(dtype).double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max()
    assert err.norm() / ref.norm() <= lr.fro_bound(1, lr.U[dtype])
    bad = F.conv2d(lr.round_t(z * inv, dtype), wt, b).permute(0, 2, 3, 1)      # the scaled latent rounded to T in front of the conv
    assert ((bad.to(dtype).double() - ref).abs() > bound).any()
    assert (_truncate(emu, dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, lr.U[dtype])


def test_vae_image_out_restatement():
    import numpy as np
    x = _rnd((2, 3, 9, 11), 6, 1.2)
    x.view(-1)[:len(lr.IMAGE_OUT_SPECIALS)] = torch.tensor(lr.IMAGE_OUT_SPECIALS)
    unit, u8 = lr.vae_image_out_restate(x)
    want = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)
    assert torch.equal(unit, want) and unit.dtype == torch.float32
    assert np.array_equal(u8.numpy(), (255.0 * want).permute(0, 2, 3, 1).numpy().astype(np.uint8)) and u8.dtype == torch.uint8
    assert unit.min() == 0.0 and unit.max() == 1.0
    assert not np.array_equal(u8.numpy(), np.rint((255.0 * want).permute(0, 2, 3, 1).numpy()).astype(np.uint8))   # rounding, not truncation


def test_compared_images_and_worst_ratio():
    assert lr.compared_images(5, lr.BIG, 1) == [0, 1, 2, 3, 4]
    sel = lr.compared_images(64, lr.BIG + 1, 1)
    assert sel[0] == 0 and sel[-1] == 63 and 2 <= len(sel) <= 3 and sel == lr.compared_images(64, lr.BIG + 1, 1)
    got, ref = torch.tensor([[1.0, 2.0], [3.0, float("nan")]]), torch.tensor([[1.0, 2.5], [3.0, 4.0]], dtype=torch.float64)
    w, e2, r2, rep = lr.worst_ratio(got, ref, torch.full((2, 2), 0.25, dtype=torch.float64))
    assert w == float("inf") and "(1, 1)" in rep
    w, e2, r2, rep = lr.worst_ratio(got[:1], ref[:1], torch.full((1, 2), 0.25, dtype=torch.float64))
    assert w == 2.0 and e2 == 0.25 and r2 == 7.25 and "(0, 1)" in rep


def test_families_of_the_new_records():
    recs = _fake_records()
    assert lr.families(recs[("clip conv", "bf16")]) == {("bf16", "variant 10"), ("bf16", "non-square map")}
    assert lr.families(recs[("vae attention", "f16")]) == {("f16", "attention d 512")}
    for kind in lr.NEW_KINDS + lr.ENCODER_KINDS:
        assert lr.families(recs[(kind, "bf16")]) == {("bf16", kind)}


# ------------------------------------------------------------------ classifier heads and gradient helpers
def _fake_head_records():
    """One record per classifier-head kind, shaped as the recorder shapes them: the attention pool and the 16-bit head kernels on
    both libraries, the fp32 vector kernels and the loss gradient on the bf16 library that ops launches them from."""
    recs = {}
    for kind in ("bf16", "f16"):
        recs[("pool_prep", kind)] = ("pool_prep", kind, 2, 64, 256, 128)
        recs[("pool_attn_fwd", kind)] = ("pool_attn_fwd", kind, 2, 65, 128, 4, 64)
        recs[("pool_attn_bwd", kind)] = ("pool_attn_bwd", kind, 2, 65, 128, 4, 64)
        recs[("pool_prep_bwd", kind)] = ("pool_prep_bwd", kind, 2, 64, 256, 128)
        recs[("channel_mean", kind)] = ("channel_mean", kind, 2, 64, 256, False, 448, 1024)
        recs[("bcast_add", kind)] = ("bcast_add", kind, 2, 64, 256, True, 448, 1024)
    recs[("vec_act", "bf16")] = ("vec_act", "bf16", 4096, 2, True)
    recs[("vec_gn", "bf16")] = ("vec_gn", "bf16", 2, 2048, 1e-5)
    recs[("vec_gn_bwd", "bf16")] = ("vec_gn_bwd", "bf16", 2, 2048)
    recs[("logsoftmax_grad", "bf16")] = ("logsoftmax_grad", "bf16", 2, 1000, 1024.0)
    return recs


SPATIAL_HEAD_KINDS = ("channel_mean", "bcast_add", "vec_act", "vec_gn", "vec_gn_bwd")
F32_LIBRARY_KINDS = ("vec_act", "vec_gn", "vec_gn_bwd", "logsoftmax_grad")


def test_head_kinds_are_listed_required_and_replayed():
    assert len(lr.HEAD_KINDS) == 10 and set(lr.HEAD_KINDS) <= set(lr.NEW_KINDS) and set(lr.HEAD_KINDS) <= set(lr.REQUIRED_FAMILIES)
    assert set(lr.HEAD_KINDS) <= lr.REPLAYED
    for k in lr.HEAD_KINDS:
        assert lr.SYMBOL_COVERAGE["adm_" + k] == (k,)
    assert {f for f, lib in lr.ONE_LIBRARY_FAMILIES.items() if lib == "bf16"} == {"vae_image_out"} | set(F32_LIBRARY_KINDS) | set(lr.EMBED_FAMILIES)
    assert lr.SYMBOL_COVERAGE["adm_grad_add"] == ("elsewhere", "tests/test_hip_launch_replay.py::test_grad_add_at_edges")
    recs = _fake_head_records()
    for (k, lib), r in recs.items():
        assert lr.families(r) == {(lib, k)}


def test_coverage_guard_fails_when_a_head_hook_or_the_spatial_head_classifiers_are_removed():
    recs = {**_fake_records(), **_fake_head_records()}
    census = {("adm_" + k, lib) for (k, lib) in _fake_head_records()}
    assert lr.coverage_gaps(census, recs.values(), lr.REPLAYED) == []
    heads = set(lr.HEAD_KINDS)
    assert not [m for m in lr.missing_families(recs.values()) if m[1] in heads]
    for kind in lr.HEAD_KINDS:   # one hook removed from the recorder
        left = [r for r in recs.values() if r[0] != kind]
        gaps = lr.coverage_gaps(census, left, lr.REPLAYED)
        assert gaps and all(kind in g for g in gaps), (kind, gaps)
        want = {("bf16", kind)} if kind in F32_LIBRARY_KINDS else {("bf16", kind), ("f16", kind)}
        assert {m for m in lr.missing_families(left) if m[1] in heads} == want
    # without the adaptive / spatial / spatial_v2 classifiers nothing launches the kernels of csrc/adm_clfhead.hip
    left = [r for r in recs.values() if r[0] not in SPATIAL_HEAD_KINDS]
    assert {m[1] for m in lr.missing_families(left) if m[1] in heads} == set(SPATIAL_HEAD_KINDS)
    # a record of the fp32 kernels taken under the other library's name does not stand in
    assert lr.coverage_gaps({("adm_vec_gn", "bf16")}, [("vec_gn", "f16", 2, 2048, 1e-5)], lr.REPLAYED)


def test_recorder_hooks_every_head_wrapper():
    """Each of the ten ops wrappers is replaced, and the hook records before it passes the call on (the call itself fails here:
    host tensors)."""
    from autodiffusion_amd import ops
    from autodiffusion_amd._lib import AdmError
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        h = torch.zeros(2, 8, 8, 64, dtype=torch.float16)
        v = torch.zeros(2, 96)
        calls = [lambda: ops.pool_prep(h, (v, v), v, 128), lambda: ops.pool_attn_fwd(torch.zeros(2, 128, 192, dtype=BF), 65, 1),
                 lambda: ops.pool_attn_bwd(torch.zeros(2, 128, 192, dtype=BF), v, v, 65, 1),
                 lambda: ops.pool_prep_bwd(torch.zeros(2, 128, 64, dtype=BF), 8, 8), lambda: ops.channel_mean(h, out=v, col=32),
                 lambda: ops.bcast_add(v, (2, 8, 8, 64), BF, 0.5, col=16), lambda: ops.vec_act(v, "relu", dy=v),
                 lambda: ops.vec_gn(v, v, v), lambda: ops.vec_gn_bwd(v, v, v, v),
                 lambda: ops.logsoftmax_grad(v, torch.zeros(2, dtype=torch.int64), 1024.0)]
        for call in calls:
            with pytest.raises(AdmError):
                call()
        assert rec.records == {("pool_prep", "f16", 2, 64, 64, 128), ("pool_attn_fwd", "bf16", 2, 65, 128, 1, 64),
                               ("pool_attn_bwd", "bf16", 2, 65, 128, 1, 64), ("pool_prep_bwd", "bf16", 2, 64, 64, 128),
                               ("channel_mean", "f16", 2, 64, 64, False, 32, 96), ("bcast_add", "bf16", 2, 64, 64, False, 16, 96),
                               ("vec_act", "bf16", 192, 2, True), ("vec_gn", "bf16", 2, 96, 1e-5), ("vec_gn_bwd", "bf16", 2, 96),
                               ("logsoftmax_grad", "bf16", 2, 96, 1024.0)}


# ------------------------------------------------------------------ the fp32 embedding path as record kinds
def _fake_embed_records():
    """The embedding path's records as the recorder shapes them, on the bf16 library that ops launches the fp32 kernels from: every
    emb_layers at batch 256 (matrix pipe), the attention pool's 1000-wide backward projection (GEMV), time_embed's second Linear
    with the label table, and the sinusoid."""
    return {("emb_layers", "bf16"): ("linear_f32", "bf16", 256, 768, 33792, True, True, False, True),
            ("pool backward", "bf16"): ("linear_f32", "bf16", 2, 1000, 512, False, False, False, True),
            ("label table", "bf16"): ("linear_f32", "bf16", 2, 768, 768, True, True, True, True),
            ("timestep_embedding", "bf16"): ("timestep_embedding", "bf16", 2, 192, 10000.0)}


def test_embedding_kinds_are_required_replayed_and_guarded():
    assert lr.SYMBOL_COVERAGE["adm_linear_f32"] == ("linear_f32",) and lr.SYMBOL_COVERAGE["adm_timestep_embedding"] == ("timestep_embedding",)
    assert set(lr.EMBED_KINDS) <= lr.REPLAYED and set(lr.EMBED_FAMILIES) <= set(lr.REQUIRED_FAMILIES)
    recs = _fake_embed_records()
    assert lr.families(recs[("emb_layers", "bf16")]) == {("bf16", "linear_f32"), ("bf16", "linear_f32 mfma")}
    assert lr.families(recs[("pool backward", "bf16")]) == {("bf16", "linear_f32"), ("bf16", "linear_f32 gemv")}
    assert lr.families(recs[("label table", "bf16")]) == {("bf16", "linear_f32"), ("bf16", "linear_f32 mfma"), ("bf16", "linear_f32 table")}
    assert lr.families(("linear_f32", "bf16", 2, 30, 8, False, True, False, True)) == {("bf16", "linear_f32"), ("bf16", "linear_f32 tile")}
    assert lr.families(("linear_f32", "bf16", 2, 32, 8, False, True, False, False)) == {("bf16", "linear_f32"), ("bf16", "linear_f32 tile")}
    assert lr.families(recs[("timestep_embedding", "bf16")]) == {("bf16", "timestep_embedding")}
    # the stubbed census: both symbols called on the bf16 library
    census = {("adm_linear_f32", "bf16"), ("adm_timestep_embedding", "bf16")}
    embed = set(lr.EMBED_FAMILIES)
    assert lr.coverage_gaps(census, recs.values(), lr.REPLAYED) == []
    assert not [m for m in lr.missing_families(recs.values()) if m[1] in embed]
    # one hook removed from the recorder: the census still sees the symbol, the guard names the missing record kind
    left = [r for r in recs.values() if r[0] != "linear_f32"]
    gaps = lr.coverage_gaps(census, left, lr.REPLAYED)
    assert len(gaps) == 1 and "adm_linear_f32" in gaps[0] and "no linear_f32 record" in gaps[0]
    assert {m for m in lr.missing_families(left) if m[1] in embed} == {("bf16", f) for f in embed - {"timestep_embedding"}}
    left = [r for r in recs.values() if r[0] != "timestep_embedding"]
    gaps = lr.coverage_gaps(census, left, lr.REPLAYED)
    assert len(gaps) == 1 and "adm_timestep_embedding" in gaps[0] and "no timestep_embedding record" in gaps[0]
    assert {m for m in lr.missing_families(left) if m[1] in embed} == {("bf16", "timestep_embedding")}
    # a model dropped: without the classifier's backward projection the GEMV family is missing, without the class-conditional
    # UNets the table's
    for gone, fam in (("pool backward", "linear_f32 gemv"), ("label table", "linear_f32 table")):
        left = [r for k, r in recs.items() if k[0] != gone]
        assert {m for m in lr.missing_families(left) if m[1] in embed} == {("bf16", fam)}
    # a kind the replay does not take
    assert "not replayed" in lr.coverage_gaps({("adm_linear_f32", "bf16")}, recs.values(), lr.REPLAYED - {"linear_f32"})[0]


def test_recorder_hooks_the_embedding_wrappers():
    """Both ops wrappers are replaced, and the hook records before it passes the call on (the call itself fails here: host tensors)."""
    from autodiffusion_amd import ops
    from autodiffusion_amd._lib import AdmError
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        x, w, b = torch.zeros(2, 20), torch.zeros(8, 20), torch.zeros(8)
        for call in (lambda: ops.linear_f32(x, w, b, silu_in=True), lambda: ops.linear_f32(x, w, None, table=torch.zeros(3, 8), idx=torch.zeros(2, dtype=torch.int64)),
                     lambda: ops.timestep_embedding(torch.zeros(3), 33), lambda: ops.timestep_embedding(torch.zeros(3), 32, 100)):
            with pytest.raises(AdmError):
                call()
        al = x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
        assert rec.records == {("linear_f32", "bf16", 2, 20, 8, True, True, False, al), ("linear_f32", "bf16", 2, 20, 8, False, False, True, al),
                               ("timestep_embedding", "bf16", 3, 33, 10000.0), ("timestep_embedding", "bf16", 3, 32, 100.0)}
    assert ops.linear_f32.__module__ == "autodiffusion_amd.ops"   # the patch is undone


def _silu32(z):
    return z * (1.0 / (1.0 + torch.exp2(z * torch.tensor(-1.4426950408889634, dtype=F32))))


def _seq_sum(v, dim=-1):
    """fp32 sum along dim in index order, one add at a time."""
    v = v.movedim(dim, 0)
    s = torch.zeros_like(v[0])
    for x in v:
        s = s + x
    return s


def _lane_sum(v, lanes):
    """The kernels' strided sums along the last axis: lane l adds elements l, l + lanes, ... in order, then the lanes are halved
    (lane l takes lane l + half: the butterfly's and the block tree's pairing for lane 0)."""
    pad = (-v.shape[-1]) % lanes
    v = F.pad(v, (0, pad)).reshape(*v.shape[:-1], -1, lanes)
    s = _seq_sum(v, -2)
    while s.shape[-1] > 1:
        half = s.shape[-1] // 2
        s = s[..., :half] + s[..., half:]
    return s[..., 0]


def _ratio(got, ref, bound):
    return ((got.double() - ref).abs() / bound).max().item()


def _pool_case(n, hw, c, dtype, seed):
    h = lr.round_t(_rnd((n, hw, c), seed), dtype)
    a, b = 1 + 0.2 * _rnd((n, c), seed + 1), 0.2 * _rnd((n, c), seed + 2)
    pos = _rnd((c, hw + 1), seed + 3, c ** -0.5) + 0.01 * torch.arange(c * (hw + 1)).reshape(c, hw + 1) / (c * (hw + 1))
    return h, a, b, pos


def _pool_prep_emulated(h, a, b, pos, tpad, dtype, pos_tc=False, div_t=False):
    n, hw, c = h.shape
    v = _silu32(a[:, None, :] * h.to(F32) + b[:, None, :])
    p = pos.reshape(hw + 1, c) if pos_tc else pos.t()
    tok = torch.zeros(n, tpad, c, dtype=dtype)
    tok[:, 1:hw + 1] = (v + p[None, 1:]).to(dtype)
    tok[:, 0] = (_seq_sum(v, 1) / torch.tensor(float(hw + 1 if div_t else hw), dtype=F32) + p[0]).to(dtype)
    return tok


@pytest.mark.parametrize("dtype", TYPES)
def test_pool_prep_restatement_emulation_and_defects(dtype):
    n, hw, c, tpad = 2, 64, 96, 128
    h, a, b, pos = _pool_case(n, hw, c, dtype, 1)
    ref, bound = lr.pool_prep_restate(h, a, b, pos, tpad, dtype)
    act = F.silu(a.double()[:, None] * h.double() + b.double()[:, None])
    plain = torch.cat([act.mean(1, keepdim=True), act], 1) + pos.double().t()[None]
    torch.testing.assert_close(ref, plain, rtol=1e-12, atol=1e-12)
    emu = _pool_prep_emulated(h, a, b, pos, tpad, dtype)
    r = _ratio(emu[:, :hw + 1], ref, bound)
    print(f"pool_prep {dtype}: emulation worst err/bound {r:.3f}")
    assert r <= 1.0 and bool((emu[:, hw + 1:] == 0).all())
    assert (bound / lr.half_ulp(ref, dtype)).median() <= 1.1           # the bound stays close to a bare half ulp
    for kw in (dict(pos_tc=True), dict(div_t=True)):
        bad = _pool_prep_emulated(h, a, b, pos, tpad, dtype, **kw)
        rb = _ratio(bad[:, :hw + 1], ref, bound)
        print(f"pool_prep {dtype}: defect {kw} {rb:.1f} x the bound")
        assert rb > 1.0, kw


def _pool_qkv(n, t, tpad, heads, d, dtype, seed, qk_scale=1.0):
    qkv = torch.full((n, tpad, 3 * heads * d), float("nan"))
    x = _rnd((n, t, 3 * heads * d), seed)
    x[..., :2 * heads * d] *= qk_scale
    qkv[:, :t] = x
    qkv[:, t:] = 0.0       # the pad rows hold the projection's bias in a model; zero keeps the pad-key defect's logits at 0
    return lr.round_t(qkv, dtype)


def _pool_fwd_emulated(qkv, t, heads, inv_d=False, pad_keys=False):
    n, tpad, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    x = qkv.to(F32).reshape(n, tpad, 3, heads, d)
    q0, k, v = x[:, 0, 0], x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)     # [n, H, d], [n, H, tpad, d]
    scale = torch.tensor(1.0 / d if inv_d else d ** -0.5, dtype=F32)
    tk = tpad if pad_keys else t
    lg = _seq_sum(q0[:, :, None, :] * k[:, :, :tk], -1) * scale
    e = torch.exp(lg - lg.amax(-1, keepdim=True))
    w = torch.zeros(n, heads, tpad)
    w[..., :tk] = e / _lane_sum(e, 64)[..., None]
    if pad_keys:
        w[..., t:] = 0.0
    a0 = _seq_sum(w[..., :t, None] * v[:, :, :t], 2)
    return w, a0.reshape(n, c)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n,heads,d,t,tpad,qk", [(2, 4, 64, 65, 128, 1.0), (1, 3, 32, 130, 192, 1.0), (2, 1, 8, 17, 24, 1.0),
                                                 (1, 2, 64, 65, 128, 2.7)])
def test_pool_attn_fwd_restatement_emulation_and_defects(n, heads, d, t, tpad, qk, dtype):
    qkv = _pool_qkv(n, t, tpad, heads, d, dtype, 3, qk)
    (w, a0), (bw, ba) = lr.pool_attn_fwd_restate(qkv, t, heads)
    q, k, v = lr.pool_split(qkv, t, heads)
    s = torch.einsum("nhd,nhtd->nht", q, k) / math.sqrt(d)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    torch.testing.assert_close(w, e / e.sum(-1, keepdim=True), rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(a0, torch.einsum("nht,nhtd->nhd", w, v).reshape(n, -1), rtol=1e-12, atol=1e-12)
    gw, ga = _pool_fwd_emulated(qkv, t, heads)
    rw, ra = _ratio(gw[..., :t], w, bw), _ratio(ga, a0, ba)
    print(f"pool_attn_fwd {dtype} d {d} T {t} qk x{qk}: logits span {s.min().item():.1f} .. {s.max().item():.1f}; emulation worst "
          f"err/bound weights {rw:.3f}, a0 {ra:.3f}")
    assert rw <= 1.0 and ra <= 1.0 and bool((gw[..., t:] == 0).all())
    assert ((gw[..., :t].double().sum(-1) - 1).abs() <= bw.sum(-1)).all()
    for kw in (dict(inv_d=True), dict(pad_keys=True)):
        bwd, bad = _pool_fwd_emulated(qkv, t, heads, **kw)
        rb = max(_ratio(bwd[..., :t], w, bw), _ratio(bad, a0, ba))
        print(f"pool_attn_fwd {dtype}: defect {kw} {rb:.1f} x the bound")
        assert rb > 1.0 or (kw == dict(pad_keys=True) and t == tpad), kw


def _pool_bwd_emulated(qkv, wts, da0, t, heads, dtype, no_delta=False, dq_row1=False, dk_w=False):
    n, tpad, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    x = qkv.to(F32).reshape(n, tpad, 3, heads, d)
    q0, k, v = x[:, 0, 0], x[:, :t, 1].permute(0, 2, 1, 3), x[:, :t, 2].permute(0, 2, 1, 3)
    w, da = wts[..., :t], da0.reshape(n, heads, d)
    dw = _seq_sum(da[:, :, None, :] * v, -1)
    delta = torch.zeros(n, heads, 1) if no_delta else _lane_sum(w * dw, 64)[..., None]
    dlg = w * (dw - delta) * torch.tensor(d ** -0.5, dtype=F32)
    out = torch.zeros(n, tpad, 3, heads, d, dtype=dtype)
    out[:, :t, 1] = ((w if dk_w else dlg)[..., None] * q0[:, :, None, :]).permute(0, 2, 1, 3).to(dtype)
    out[:, :t, 2] = (w[..., None] * da[:, :, None, :]).permute(0, 2, 1, 3).to(dtype)
    out[:, 0, 0] = _seq_sum(dlg[..., None] * k, 2).to(dtype)
    if dq_row1 and t > 1:
        out[:, 1, 0] = out[:, 0, 0]
    return out.reshape(n, tpad, c3)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n,heads,d,t,tpad", [(2, 4, 64, 65, 128), (1, 3, 32, 130, 192), (2, 1, 8, 17, 24), (3, 1, 32, 1, 64)])
@pytest.mark.parametrize("mag", [1e-3, 1.024])
def test_pool_attn_bwd_restatement_emulation_and_defects(n, heads, d, t, tpad, mag, dtype):
    qkv = _pool_qkv(n, t, tpad, heads, d, dtype, 5)
    wts, _ = _pool_fwd_emulated(qkv, t, heads)
    da0 = _rnd((n, heads * d), 6, mag)
    ref, bound = lr.pool_attn_bwd_restate(qkv, wts, da0, t, heads, dtype)
    # autograd of the float64 pool, with the stored weights' softmax replaced by its own (they agree to fp32 accuracy)
    x = qkv[:, :t].double().clone().requires_grad_()
    (_, a0), _ = lr.pool_attn_fwd_restate(x, t, heads)
    (a0 * da0.double()).sum().backward()
    torch.testing.assert_close(ref, x.grad, rtol=2e-5, atol=2e-6 * mag)
    got = _pool_bwd_emulated(qkv, wts, da0, t, heads, dtype)
    r = _ratio(got[:, :t], ref, bound)
    c = heads * d
    under = float(((got[:, :t, c:2 * c] == 0) & (ref[:, :, c:2 * c] != 0)).float().mean())
    print(f"pool_attn_bwd {dtype} d {d} T {t} |da0| {mag:g}: emulation worst err/bound {r:.3f}; dK flushed to zero {under:.1%}")
    assert r <= 1.0 and lr.pool_zero_rows_ok(got, t)
    if t == 1:
        assert bool((got[:, 0, :2 * c] == 0).all())      # a single key: weight 1, dK = 0 and dQ = 0, exactly (of either sign)
        return
    for kw in (dict(no_delta=True), dict(dk_w=True)):
        rb = _ratio(_pool_bwd_emulated(qkv, wts, da0, t, heads, dtype, **kw)[:, :t], ref, bound)
        print(f"pool_attn_bwd {dtype}: defect {kw} {rb:.1f} x the bound")
        assert rb > 1.0, kw
    bad = _pool_bwd_emulated(qkv, wts, da0, t, heads, dtype, dq_row1=True)
    assert _ratio(bad[:, :t], ref, bound) > 1.0 and not lr.pool_zero_rows_ok(bad, t)


@pytest.mark.parametrize("dtype", TYPES)
def test_pool_prep_bwd_restatement_emulation_and_defects(dtype):
    n, hw, c, tpad = 2, 64, 40, 128
    dtok = lr.round_t(_rnd((n, tpad, c), 7), dtype)
    ref, bound = lr.pool_prep_bwd_restate(dtok, hw, dtype)
    act = _rnd((n, hw, c), 8).double().requires_grad_()
    (torch.cat([act.mean(1, keepdim=True), act], 1) * dtok[:, :hw + 1].double()).sum().backward()
    torch.testing.assert_close(ref, act.grad, rtol=1e-12, atol=1e-12)
    x = dtok.to(F32)
    emu = (x[:, 1:hw + 1] + x[:, :1] / torch.tensor(float(hw), dtype=F32)).to(dtype)
    r = _ratio(emu, ref, bound)
    bad = (x[:, 1:hw + 1] + x[:, :1] / torch.tensor(float(hw + 1), dtype=F32)).to(dtype)
    rb = _ratio(bad, ref, bound)
    print(f"pool_prep_bwd {dtype}: emulation worst err/bound {r:.3f}; token 0 over T {rb:.1f} x the bound")
    assert r <= 1.0 and rb > 1.0


def test_pool_restatements_compose_to_the_oracle_attention_pool():
    """pool_prep -> a float64 qkv projection -> pool_attn_fwd against oracle.nets.attention_pool with an identity c_proj."""
    from types import SimpleNamespace
    from oracle import nets
    n, hw, c, heads = 2, 64, 64, 2
    h, a, b, pos = _pool_case(n, hw, c, BF, 11)
    tok, _ = lr.pool_prep_restate(h, a, b, pos, 128, BF)
    wq, bq = _rnd((3 * c, c), 12, c ** -0.5).double(), _rnd((3 * c,), 13, 0.1).double()
    (_, a0), _ = lr.pool_attn_fwd_restate(tok @ wq.t() + bq, hw + 1, heads)
    P = {"out.2.positional_embedding": pos.double(), "out.2.qkv_proj.weight": wq[:, :, None], "out.2.qkv_proj.bias": bq,
         "out.2.c_proj.weight": torch.eye(c, dtype=torch.float64)[:, :, None], "out.2.c_proj.bias": torch.zeros(c, dtype=torch.float64)}
    act = F.silu(a.double()[:, None] * h.double() + b.double()[:, None]).permute(0, 2, 1).reshape(n, c, 8, 8)
    orc = nets.attention_pool(P, SimpleNamespace(prefix="out", num_heads=heads), act)
    torch.testing.assert_close(a0, orc.double(), rtol=1e-5, atol=1e-5)   # the oracle's softmax runs in fp32


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("hw", [9, 64, 63])
def test_channel_mean_restatement_emulation_and_defects(hw, affine, dtype):
    n, c = 2, 40
    h, a, b, _ = _pool_case(n, hw, c, dtype, 21)
    aff = (a, b) if affine else None
    ref, bound = lr.channel_mean_restate(h, aff)
    v = F.silu(a.double()[:, None] * h.double() + b.double()[:, None]) if affine else h.double()
    torch.testing.assert_close(ref, v.mean(1), rtol=1e-12, atol=1e-12)
    v32 = _silu32(a[:, None] * h.to(F32) + b[:, None]) if affine else h.to(F32)
    lanes = F.pad(v32, (0, 0, 0, (-hw) % 4)).reshape(n, -1, 4, c)
    r4 = _seq_sum(lanes, 1)
    tot = ((r4[:, 0] + r4[:, 1]) + r4[:, 2]) + r4[:, 3]
    emu = tot / torch.tensor(float(hw), dtype=F32)
    r = _ratio(emu, ref, bound)
    bad = tot / torch.tensor(float((hw + 3) // 4), dtype=F32)        # divided by one lane's pixels
    rb = _ratio(bad, ref, bound)
    print(f"channel_mean {dtype} hw {hw} affine {affine}: emulation worst err/bound {r:.3f}; one lane's count {rb:.3g} x the bound")
    assert r <= 1.0 and rb > 1.0


@pytest.mark.parametrize("dtype", TYPES)
def test_bcast_add_restatement_emulation_and_defects(dtype):
    n, hw, c, col, scale = 3, 16, 24, 8, 1.0 / 64
    v = _rnd((n, 64), 31)
    add = lr.round_t(_rnd((n, hw, c), 32), dtype)
    win = v[:, col:col + c]
    ref, bound = lr.bcast_add_restate(win, scale, add, hw, dtype)
    torch.testing.assert_close(ref, add.double() + win.double()[:, None] * scale, rtol=1e-12, atol=1e-12)
    emu = (win[:, None] * torch.tensor(scale, dtype=F32) + add.to(F32)).to(dtype)
    r = _ratio(emu, ref, bound)
    bad = (v[:, None, :c] * torch.tensor(scale, dtype=F32) + add.to(F32)).to(dtype)           # col ignored
    rb = _ratio(bad, ref, bound)
    print(f"bcast_add {dtype}: emulation worst err/bound {r:.3f}; col ignored {rb:.1f} x the bound")
    assert r <= 1.0 and rb > 1.0
    exact, none = lr.bcast_add_restate(win, 1.0 / 3, None, hw, dtype)
    assert none is None and exact.dtype == dtype and exact.shape == (n, hw, c)
    assert torch.equal(exact[:, 5], (win * torch.tensor(1.0 / 3, dtype=F32)).to(dtype))
    assert not torch.equal(exact[:, 5], (v[:, :c] * torch.tensor(1.0 / 3, dtype=F32)).to(dtype))


VEC_SPECIALS = (0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e-3, -1.2784645)


def _vec_act_emulated(x, mode, dy=None, plain_sigmoid=False, relu_at_zero=False):
    if mode == 2:
        if dy is None:
            return torch.clamp(x, min=0.0)
        return dy * ((x >= 0) if relu_at_zero else (x > 0)).to(F32)
    s = 1.0 / (1.0 + torch.exp(-x))
    if dy is None:
        return x / (1.0 + torch.exp(-x))
    return dy * (s if plain_sigmoid else s * (1.0 + x * (1.0 - s)))


def test_vec_act_restatement_emulation_and_defects():
    x = _rnd((5 * 2048,), 41, 3.0)
    x[:len(VEC_SPECIALS)] = torch.tensor(VEC_SPECIALS)
    dy = _rnd((5 * 2048,), 42)
    xd = x.double().requires_grad_()
    F.silu(xd).backward(dy.double())
    ref, bound = lr.vec_act_restate(x, 1)
    torch.testing.assert_close(ref, F.silu(x.double()), rtol=1e-12, atol=1e-300)
    refb, boundb = lr.vec_act_restate(x, 1, dy)
    torch.testing.assert_close(refb, xd.grad, rtol=1e-12, atol=1e-15)
    r, rb = _ratio(_vec_act_emulated(x, 1), ref, bound), _ratio(_vec_act_emulated(x, 1, dy), refb, boundb)
    bad = _ratio(_vec_act_emulated(x, 1, dy, plain_sigmoid=True), refb, boundb)
    print(f"vec_act: emulation worst err/bound SiLU {r:.3f}, SiLU' {rb:.3f}; SiLU' without z (1 - s) {bad:.3g} x the bound")
    assert r <= 1.0 and rb <= 1.0 and bad > 1.0
    assert torch.isfinite(_vec_act_emulated(x, 1)).all() and torch.isfinite(_vec_act_emulated(x, 1, dy)).all()
    ref, none = lr.vec_act_restate(x, 2)
    refb, noneb = lr.vec_act_restate(x, 2, dy)
    assert none is None and noneb is None
    assert torch.equal(ref, F.relu(x.double())) and torch.equal(refb, dy.double() * (x > 0))
    assert torch.equal(_vec_act_emulated(x, 2).double(), ref) and torch.equal(_vec_act_emulated(x, 2, dy).double(), refb)
    assert refb[0] == 0 and refb[1] == 0                                   # ReLU'(+-0) = 0
    assert not torch.equal(_vec_act_emulated(x, 2, dy, relu_at_zero=True).double(), refb)


def _vec_gn_emulated(x, gamma, beta, eps, unbiased=False):
    n, c = x.shape
    cpg = c // 32
    g = x.reshape(n, 32, cpg)
    fc = torch.tensor(float(cpg), dtype=F32)
    mean = (_lane_sum(g, 8) / fc)[..., None]
    d = g - mean
    ss = _lane_sum(d * d, 8)
    rstd = (1.0 / torch.sqrt(ss / (fc - 1 if unbiased else fc) + torch.tensor(eps, dtype=F32)))[..., None]
    y = gamma.reshape(1, 32, cpg) * d * rstd + beta.reshape(1, 32, cpg)
    return y.reshape(n, c), torch.cat([mean, rstd], -1)


def _vec_gn_bwd_emulated(x, gamma, stats, dz, no_xhat=False):
    n, c = x.shape
    cpg = c // 32
    fc = torch.tensor(float(cpg), dtype=F32)
    mean, rstd = stats[..., :1], stats[..., 1:]
    g = (gamma[None] * dz).reshape(n, 32, cpg)
    xh = (x.reshape(n, 32, cpg) - mean) * rstd
    s1, s2 = (_lane_sum(g, 8) / fc)[..., None], (_lane_sum(g * xh, 8) / fc)[..., None]
    return (rstd * (g - s1 - (0 if no_xhat else xh * s2))).reshape(n, c)


def _vec_rows(n, c, seed, offset=0.0, std=1.0):
    return _rnd((n, c), seed, std) + offset, 1 + 0.2 * _rnd((c,), seed + 1), 0.1 * _rnd((c,), seed + 2)


@pytest.mark.parametrize("n,c,offset,std", [(5, 2048, 0.3, 1.0), (1, 32, 0.3, 1.0), (3, 96, 0.0, 1.0), (2, 288, 0.0, 2.0), (4, 2048, 100.0, 0.1)])
def test_vec_gn_restatements_emulation_and_defects(n, c, offset, std):
    x, gamma, beta = _vec_rows(n, c, 51, offset, std)
    (y, mean, rstd), (by, bm, br) = lr.vec_gn_restate(x, gamma, beta, 1e-5)
    plain = (F.group_norm(x.double(), 32, gamma.double(), beta.double(), float(torch.tensor(1e-5, dtype=F32))) if c > 32
             else beta.double()[None].expand(n, -1))           # one value per group: torch refuses it, the result is beta
    torch.testing.assert_close(y, plain, rtol=1e-10, atol=1e-10)
    ye, st = _vec_gn_emulated(x, gamma, beta, 1e-5)
    r = max(_ratio(ye, y, by), _ratio(st[..., 0], mean, bm), _ratio(st[..., 1], rstd, br))
    print(f"vec_gn n {n} c {c} mean {offset} std {std}: emulation worst err/bound {r:.3f}")
    assert r <= 1.0
    dz = _rnd((n, c), 54)
    ref, bound = lr.vec_gn_bwd_restate(x, gamma, st, dz)
    rbw = _ratio(_vec_gn_bwd_emulated(x, gamma, st, dz), ref, bound)
    print(f"vec_gn_bwd n {n} c {c}: emulation worst err/bound {rbw:.3f}")
    assert rbw <= 1.0
    if c == 32:   # one value per group: y = beta and dx = 0, both exactly
        assert torch.equal(ye, beta[None].expand(n, -1)) and not bool(_vec_gn_bwd_emulated(x, gamma, st, dz).view(torch.int32).any())
        return
    # the backward restatement against autograd through the float64 GroupNorm (its own float64 statistics)
    xd = x.double().requires_grad_()
    F.group_norm(xd, 32, gamma.double(), beta.double(), float(torch.tensor(1e-5, dtype=F32))).backward(dz.double())
    st64 = torch.stack([mean, rstd], -1)
    torch.testing.assert_close(lr.vec_gn_bwd_restate(x, gamma, st64, dz)[0], xd.grad, rtol=1e-8, atol=1e-8)
    bad_y = _ratio(_vec_gn_emulated(x, gamma, beta, 1e-5, unbiased=True)[0], y, by)
    bad_dx = _ratio(_vec_gn_bwd_emulated(x, gamma, st, dz, no_xhat=True), ref, bound)
    print(f"vec_gn: variance over cpg - 1 {bad_y:.3g} x the bound; vec_gn_bwd without the xhat term {bad_dx:.3g} x the bound")
    assert bad_dx > 1.0 and (bad_y > 1.0 or offset == 100.0)


def _logsoftmax_emulated(logits, y, scale, onehot_unscaled=False):
    n, k = logits.shape
    mx = logits.amax(-1, keepdim=True)
    e = torch.exp(logits - mx)
    total = _lane_sum(e, 256)[..., None]
    sm = e / total
    one = torch.zeros(n, k)
    one[torch.arange(n), y] = 1.0
    sc = torch.tensor(scale, dtype=F32)
    dl = (one - sc * sm) if onehot_unscaled else sc * (one - sm)
    return dl, logits[torch.arange(n), y] - mx[:, 0] - torch.log(total[:, 0])


@pytest.mark.parametrize("n,k", [(5, 1000), (1, 1), (2, 255), (2, 257), (3, 4097)])
@pytest.mark.parametrize("scale", [1.0, 2.5, 1024.0])
def test_logsoftmax_grad_restatement_emulation_and_defects(n, k, scale):
    logits = _rnd((n, k), 61, 3.0)
    logits[-1] = torch.linspace(-1e4, 1e4, k) if k > 1 else logits[-1]
    y = torch.tensor([0, k - 1, k // 2, 0, k - 1][:n])
    (dl, lp), (bd, bl) = lr.logsoftmax_grad_restate(logits, y, scale)
    ld = logits.double().requires_grad_()
    sel = F.log_softmax(ld, -1)[torch.arange(n), y]
    (scale * sel.sum()).backward()
    torch.testing.assert_close(dl, ld.grad, rtol=1e-10, atol=1e-12 * scale)
    torch.testing.assert_close(lp, sel.detach(), rtol=1e-12, atol=1e-12)
    ge, gl = _logsoftmax_emulated(logits, y, scale)
    r, rl = _ratio(ge, dl, bd), _ratio(gl, lp, bl)
    print(f"logsoftmax_grad n {n} k {k} scale {scale:g}: emulation worst err/bound dl {r:.3f}, logp_sel {rl:.3f}")
    assert r <= 1.0 and rl <= 1.0 and torch.isfinite(ge).all()
    if scale != 1.0 and k > 1:
        rb = _ratio(_logsoftmax_emulated(logits, y, scale, onehot_unscaled=True)[0], dl, bd)
        print(f"logsoftmax_grad: scale on the softmax only {rb:.3g} x the bound")
        assert rb > 1.0


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("b_half", [False, True])
def test_grad_add_restatement_emulation_and_defects(b_half, dtype):
    n, h, w, c = 1, 6, 10, 8
    a = lr.round_t(_rnd((n, h, w, c), 71), dtype)
    b = lr.round_t(_rnd((n, h // 2, w // 2, c) if b_half else (n, h, w, c), 72), dtype)
    ref, bound = lr.grad_add_restate(a, b, b_half, dtype)
    up = F.interpolate(b.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest").permute(0, 2, 3, 1) * 0.25 if b_half else b.double()
    torch.testing.assert_close(ref, a.double() + up, rtol=1e-12, atol=1e-12)
    emu = (a.to(F32) + up.to(F32)).to(dtype)
    assert _ratio(emu, ref, bound) <= 1.0
    if b_half:   # the AvgPool2d backward's 1 / 4 left out
        assert _ratio((a.to(F32) + 4 * up.to(F32)).to(dtype), ref, bound) > 1.0
    assert (_truncate(a.to(F32) + up.to(F32), dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, lr.U[dtype])


# ------------------------------------------------------------------ the KL-f8 encoder's launches
def test_encoder_kinds_are_covered_and_replayed():
    assert lr.SYMBOL_COVERAGE["adm_stem_conv3x3"] == ("stem_conv3x3",) and lr.ENCODER_KINDS == ("stem_conv3x3",)
    assert set(lr.ENCODER_KINDS) <= lr.REPLAYED
    # the big recording does not run the encoder: its kind is no required family there (the encoder replay's own guard asserts it)
    assert not set(lr.ENCODER_KINDS) & set(lr.REQUIRED_FAMILIES) and not set(lr.ENCODER_KINDS) & set(lr.NEW_KINDS)
    assert lr.RESAMPLE_MODES["stride2_odd"] == 5 and lr.VEC_ACT_MODES["gauss_std"] == 3 and lr.VEC_ACT_MODES["gauss_logvar"] == 4
    from autodiffusion_amd import ops
    import inspect
    src = inspect.getsource(ops.resample) + inspect.getsource(ops.vec_act)
    for name, m in list(lr.RESAMPLE_MODES.items()) + list(lr.VEC_ACT_MODES.items()):   # the recorder's tables are ops' own
        assert f'"{name}": {m}' in src, (name, m)


def test_recorder_hooks_the_encoder_launches():
    """The stem's wrapper is replaced, and the recorder takes the odd-pixel pick and the Gaussian modes: each hook records before
    it passes the call on (the call itself fails here: host tensors)."""
    from autodiffusion_amd import ops
    from autodiffusion_amd._lib import AdmError
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        v = torch.zeros(96)
        calls = [lambda: ops.stem_conv3x3(torch.zeros(2, 3, 64, 64), torch.zeros(128, 3, 3, 3), torch.zeros(128), torch.float16),
                 lambda: ops.stem_conv3x3(torch.zeros(1, 3, 8, 16), torch.zeros(32, 3, 3, 3), torch.zeros(32)),
                 lambda: ops.resample(torch.zeros(1, 4, 6, 32, dtype=BF), "stride2_odd"),
                 lambda: ops.resample(torch.zeros(1, 4, 6, 32, dtype=torch.float16), "stride2_odd", (v, v)),
                 lambda: ops.vec_act(v, "gauss_std"), lambda: ops.vec_act(v, "gauss_std", dy=v), lambda: ops.vec_act(v, "gauss_logvar")]
        for call in calls:
            with pytest.raises(AdmError):
                call()
        assert rec.records == {("stem_conv3x3", "f16", 2, 3, 64, 64, 128), ("stem_conv3x3", "bf16", 1, 3, 8, 16, 32),
                               ("resample", "bf16", 1, 4, 6, 32, 5, False), ("resample", "f16", 1, 4, 6, 32, 5, True),
                               ("vec_act", "bf16", 96, 3, False), ("vec_act", "bf16", 96, 3, True), ("vec_act", "bf16", 96, 4, False)}
    assert ops.stem_conv3x3.__module__ == "autodiffusion_amd.ops"   # the patch is undone


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("with_aff", [False, True])
def test_resample_odd_pixels_restatement_emulation_and_defects(with_aff, dtype):
    """Mode 5 is out[y][x] = in[2y + 1][2x + 1]: the restatement against the padded stride-2 pick it stands for, the fp32
    emulation inside the bound (bitwise without the affine), the even pixels and the (2y + 1, 2x) pick outside."""
    n, h, w, c = 2, 6, 4, 16
    x = lr.round_t(_rnd((n, h, w, c), 15), dtype)
    aff = (1 + 0.2 * _rnd((n, c), 16), 0.2 * _rnd((n, c), 17)) if with_aff else None
    xc = x.permute(0, 3, 1, 2).double()
    if with_aff:
        xc = F.silu(aff[0].double()[:, :, None, None] * xc + aff[1].double()[:, :, None, None])
    ref, bound = lr.resample_restate(x, 5, aff, dtype)
    # F.pad(x, (0, 1, 0, 1)) sampled where a pad-0 stride-2 3x3 window has its centre: pixel (2y + 1, 2x + 1)
    torch.testing.assert_close(ref, F.pad(xc, (0, 1, 0, 1))[:, :, 1::2, 1::2][:, :, :h // 2, :w // 2].permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert ref.shape == (n, h // 2, w // 2, c)
    x32 = x.to(F32)
    s32 = F.silu(aff[0][:, None, None, :] * x32 + aff[1][:, None, None, :]) if with_aff else x32
    good, even, mixed = s32[:, 1::2, 1::2], s32[:, ::2, ::2], s32[:, 1::2, ::2]
    if not with_aff:
        assert bound is None and torch.equal(good.to(dtype).double(), ref)
        assert not torch.equal(even.to(dtype).double(), ref) and not torch.equal(mixed.to(dtype).double(), ref)
        return
    err = (good.to(dtype).double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max()
    assert (bound <= 1.01 * 0.5 * lr.ulp_t(ref, dtype) + 2.0 ** -19 * (1 + ref.abs())).all()
    assert err.norm() / ref.norm() <= lr.fro_bound(1, lr.U[dtype])
    for bad in (even, mixed):
        assert ((bad.to(dtype).double() - ref).abs() > bound).any()
    assert (_truncate(good, dtype).double() - ref).norm() / ref.norm() > lr.fro_bound(1, lr.U[dtype])


def test_vec_act_gaussian_modes_restatement_emulation_and_defects():
    """Modes 3 / 4 through vec_act_restate: f32_vae_kernels' restatements; exp(x / 2) without the clamp is outside the bound (at
    the specials beyond the clamp), the clamped log-variance is bitwise."""
    import f32_vae_kernels as V
    x = _rnd((5 * 2048,), 43, 12.0)
    x[:len(lr.GAUSS_SPECIALS)] = torch.tensor(lr.GAUSS_SPECIALS)
    assert lr.GAUSS_SPECIALS is V.GAUSS_SPECIALS and bool((x < -30).any()) and bool((x > 20).any())
    dy = _rnd((5 * 2048,), 44)
    ref, bound = lr.vec_act_restate(x, 3)
    torch.testing.assert_close(ref, torch.exp(0.5 * torch.clamp(x.double(), -30.0, 20.0)), rtol=1e-15, atol=0)
    refb, boundb = lr.vec_act_restate(x, 3, dy)
    torch.testing.assert_close(refb, dy.double() * ref, rtol=1e-15, atol=0)
    emu = torch.exp(0.5 * torch.clamp(x, -30.0, 20.0))
    r, rb = _ratio(emu, ref, bound), _ratio(dy * emu, refb, boundb)
    unclamped = torch.exp(0.5 * x)
    bad, badb = _ratio(unclamped, ref, bound), _ratio(dy * unclamped, refb, boundb)
    print(f"vec_act gauss_std: emulation worst err/bound {r:.3f}, with dy {rb:.3f}; without the clamp {bad:.3g} / {badb:.3g} x the bound")
    assert r <= 1.0 and rb <= 1.0 and bad > 1.0 and badb > 1.0
    # only the elements beyond the clamp tell: without them the defect is invisible, so every replayed operand carries the specials
    inside = (x >= -30.0) & (x <= 20.0)
    assert _ratio(unclamped[inside], ref[inside], bound[inside]) <= 1.0
    lv, none = lr.vec_act_restate(x, 4)
    assert none is None and lv.dtype == torch.float32 and torch.equal(lv, torch.clamp(x, -30.0, 20.0))
    assert torch.equal(torch.signbit(lv), torch.signbit(torch.clamp(x, -30.0, 20.0))) and float(lv.min()) == -30.0 and float(lv.max()) == 20.0
    assert not torch.equal(lv, x)
    with pytest.raises(NotImplementedError):
        lr.vec_act_restate(x, 4, dy)


@pytest.mark.parametrize("dtype", TYPES)
def test_stem_record_restatement_emulation_and_transposed_taps(dtype):
    """A stem_conv3x3 record (kind, n, cin, h, w, cout) restated by f32_kernels.stem_restate at the encoder's channel counts: fp32
    conv2d inside the bound, the same conv with its taps transposed (ky <-> kx) outside."""
    import f32_kernels as fk
    assert lr.stem_restate is fk.stem_restate
    _, _, n, cin, h, w, cout = ("stem_conv3x3", lr.KIND_OF_DTYPE[dtype], 2, 3, 9, 7, 128)
    x, wt, b = fk.stem_inputs(n, cin, h, w, cout, 35)
    ref, bound = lr.stem_restate(x, wt, b, dtype)
    assert ref.shape == (n, h, w, cout)
    torch.testing.assert_close(ref, F.conv2d(x.double(), wt.double(), b.double(), padding=1).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    good = F.conv2d(x, wt, b, padding=1).permute(0, 2, 3, 1).to(dtype)
    assert _ratio(good, ref, bound) <= 1.0
    assert (good.double() - ref).norm() / ref.norm() <= lr.fro_bound(1, lr.U[dtype])
    bad = F.conv2d(x, wt.transpose(2, 3).contiguous(), b, padding=1).permute(0, 2, 3, 1).to(dtype)
    assert _ratio(bad, ref, bound) > 1.0


# ------------------------------------------------------------------ the encoder's head as a composite
HEAD_EPS = 1e-6


def _head_emulated(o, dtype, pad_first=False, fold=None):
    """Encoder._head in fp32 on the operands of lr.head_operands: the GroupNorm affine from float64 statistics as fp32 (a, b),
    SiLU(a h + b) rounded once to T, the pad-1 3x3 conv with round_T weights.  pad_first: the defect -- the map is copied into the
    corner of a zeroed map of the next multiple of 16 BEFORE the activation, so the padding is activated too.  fold: None, or
    "ok" / "no_bq" / "transposed": the head of folded_head (W' = wq Wout and b' = wq b_out + bq in fp32, W' rounded to T), without
    the bq term, or with wq transposed."""
    h, gamma, beta = o["h"], o["gamma"], o["beta"]
    n, side, _, c = h.shape
    _, mean, rstd = lr.gn_affine_restate(h, gamma, beta, HEAD_EPS)
    cpg = c // 32
    a64 = gamma.double() * rstd.repeat_interleave(cpg, 1)
    b64 = beta.double() - mean.repeat_interleave(cpg, 1) * a64
    a, b = a64.to(F32)[:, None, None, :], b64.to(F32)[:, None, None, :]
    x = h.to(F32)
    if pad_first:
        big = -(-side // 16) * 16
        xp = torch.zeros(n, big, big, c)
        xp[:, :side, :side] = x
        x = xp
    act = lr.round_t(F.silu(torch.addcmul(b, a, x)), dtype)
    w, bias = o["w"], o["bias"]
    if fold is not None:
        q = o["wq"].reshape(o["wq"].shape[0], -1)
        q = q.t().contiguous() if fold == "transposed" else q
        w = torch.einsum("om,mcyx->ocyx", q, o["w"])
        bias = q @ o["bias"] + (0.0 if fold == "no_bq" else o["bq"])
    out = F.conv2d(act.permute(0, 3, 1, 2), lr.round_t(w, dtype), bias, padding=1)
    return out[:, :, :side, :side]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("side", [8, 24, 16])
def test_head_restatement_emulation_and_an_activated_padding(side, dtype):
    o = lr.head_operands(2, side, 64, 8, dtype, 9000 + side)
    ref, bound = lr.head_restate(o["h"], o["gamma"], o["beta"], o["w"], o["bias"], HEAD_EPS, dtype)
    assert ref.shape == (2, 8, side, side)
    # the restatement is the reference's norm_out -> SiLU -> conv_out, but for one rounding of the activation to T
    hc = o["h"].double().permute(0, 3, 1, 2)
    plain = F.conv2d(F.silu(F.group_norm(hc, 32, o["gamma"].double(), o["beta"].double(), eps=HEAD_EPS)), lr.round_t(o["w"], dtype).double(),
                     o["bias"].double(), padding=1)
    assert (ref - plain).norm() / plain.norm() <= 2 * lr.U[dtype]
    # the offset does what head_operands says: the GroupNorm shift is about +4, a pixel that is zero before the activation becomes ~ 3.9
    z0 = lr.head_window(torch.zeros_like(o["h"]), o["gamma"], o["beta"], HEAD_EPS)[0]   # all-zero map: z = beta
    _, mean, rstd = lr.gn_affine_restate(o["h"], o["gamma"], o["beta"], HEAD_EPS)
    shift = -(mean * rstd)
    assert z0.abs().max() <= 1.0 and 3.0 <= shift.min() and shift.max() <= 5.5, (shift.min(), shift.max())
    good = _head_emulated(o, dtype)
    r = _ratio(good, ref, bound)
    fro = ((good.double() - ref).norm() / ref.norm()).item()
    assert r <= 1.0 and fro <= lr.fro_bound(1, lr.U[dtype]), (r, fro / lr.U[dtype])
    if side % 16 == 0:
        return
    bad = _head_emulated(o, dtype, pad_first=True)
    ratio = (bad.double() - ref).abs() / bound
    edge = torch.zeros_like(ref, dtype=torch.bool)
    edge[:, :, -1, :] = edge[:, :, :, -1] = True
    print(f"head side {side} {dtype}: emulation worst err/bound {r:.3f}; padding activated: last row / column {ratio[edge].min().item():.3g} .. "
          f"{ratio[edge].max().item():.3g} x the bound (median {ratio[edge].median().item():.3g}), inside {ratio[~edge].max().item():.3f}")
    assert ratio[~edge].max() <= 1.0           # wrong along the two edges only ...
    assert ratio[edge].min() > 1.0 and ratio[edge].median() > 100.0   # ... there on every element, and typically by far more than the bound


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("side", [8, 16])
def test_folded_head_restatement_emulation_and_defects(side, dtype):
    o = lr.head_operands(2, side, 64, 8, dtype, 9000 + side)
    ref, bound = lr.head_restate(o["h"], o["gamma"], o["beta"], o["w"], o["bias"], HEAD_EPS, dtype, o["wq"], o["bq"])
    ref0, bound0 = lr.head_restate(o["h"], o["gamma"], o["beta"], o["w"], o["bias"], HEAD_EPS, dtype)
    # quant_conv(conv_out(act)) from the unfolded weights; the unfolded restatement rounds Wout to T, this one does not
    act = lr.head_activation(o["h"], o["gamma"], o["beta"], HEAD_EPS, dtype)[0].permute(0, 3, 1, 2)
    plain = F.conv2d(F.conv2d(act, o["w"].double(), o["bias"].double(), padding=1), o["wq"].double(), o["bq"].double())
    torch.testing.assert_close(ref, plain, rtol=1e-12, atol=1e-12)
    assert (bound > 0).all() and bound.mean() > bound0.mean()
    good = _head_emulated(o, dtype, fold="ok")
    r = _ratio(good, ref, bound)
    fro = ((good.double() - ref).norm() / ref.norm()).item()
    bad_q, bad_t = _ratio(_head_emulated(o, dtype, fold="no_bq"), ref, bound), _ratio(_head_emulated(o, dtype, fold="transposed"), ref, bound)
    print(f"folded head side {side} {dtype}: emulation worst err/bound {r:.3f}, fro/u {fro / lr.U[dtype]:.3f}; without bq {bad_q:.3g}, "
          f"wq transposed {bad_t:.3g} x the bound")
    assert r <= 1.0 and fro <= lr.fro_bound(1, lr.U[dtype])
    assert bad_q > 1.0 and bad_t > 1.0
