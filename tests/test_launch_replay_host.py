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
    """One record per new kind and library, and the VAE's / CLIP's conv and attention families, shaped as the recorder shapes them."""
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
    recs[("vae_image_out", "bf16")] = ("vae_image_out", "bf16", 1, 512, 512, True, True)
    return recs


def test_coverage_guard_fails_when_a_model_or_a_hook_is_removed():
    """With a stubbed census (every replayed symbol called on both libraries): the full record set passes; without any one new
    hook's records, without the VAE's or without the CLIP encoder's, the guard names what is missing."""
    recs = _fake_records()
    here = {s: cov for s, cov in lr.SYMBOL_COVERAGE.items() if cov[0] != "elsewhere" and set(cov) & set(lr.NEW_KINDS)}
    census = {(s, k) for s in here for k in ("bf16", "f16") if not (s == "adm_vae_image_out" and k == "f16")}
    census |= {("adm_linear_f32", "bf16")}   # held elsewhere: needs no record
    assert lr.coverage_gaps(census, recs.values(), lr.REPLAYED) == []
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
    for kind in lr.NEW_KINDS:
        assert lr.families(recs[(kind, "bf16")]) == {("bf16", kind)}
