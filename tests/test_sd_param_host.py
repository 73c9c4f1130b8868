"""Host: the parameterised latent sampler steps and the SD 2.x plumbing -- tests/sd_param_ref.py's restatements
against the reference solver's composition (dpm_solver.py:297-306 noise_pred_fn in front of the eps-only restatements of
tests/f32_kernels.py / tests/unipc_ref.py), an fp32 emulation of the kernels' operation order against their bounds, planted
defects, the refusals of the new entry points, and the key layout, tokeniser padding, builders and parsers of the OpenCLIP cond
stage.  No GPU: the refusals are answered before any pointer is read."""
import argparse
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import f32_kernels as fk
import sd_param_ref as R
import unipc_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR = (0.81, -0.55, 0.23, -0.07, 0.031)
PRED = (0.64, 0.47, -0.19, 0.052)
DPM = dict(cfg=3.0, sigma_s=0.6, alpha_s=0.8, a=0.75, b0=0.4, b1=-0.12)


def _ratio(got, ref, bound):
    return float(((torch.as_tensor(got).double() - ref).abs() / bound).max())


def _same(a, b, slack=0.0):
    assert float((a - b).abs().max()) <= 1e-12 * (1.0 + float(b.abs().max())) + slack


def _unit_slack(alpha, sigma, x, param):
    """The V data prediction alpha x - sigma o is the composition's (x - sigma (alpha o + sigma x)) / alpha plus exactly
    x (alpha^2 + sigma^2 - 1) / alpha: zero for the schedule's real numbers, a few 1e-8 for their fp32 roundings, which the kernels
    are passed.  The comparison allows that term (coefficients of the states below are < 1 in magnitude, at most 4 of them add)."""
    return 4.0 * abs(1.0 - alpha ** 2 - sigma ** 2) / alpha * float(x.abs().max()) if param == "v" else 0.0


def _cf(cfg, hist, sqrt_at, noise):
    return fk.sd_coefs_dict(fk.sd_coefs_of(cfg, hist, sqrt_at, noise))


# ------------------------------------------------------------------ the fused forms are the reference's composition
@pytest.mark.parametrize("param", ["v", "x0"])
def test_restatements_equal_the_reference_composition(param):
    x, ou, oc, h1, h2, h3, nz, xb = R.latents(500, 3, 8)
    for guided, hist, noise, sqrt_at in itertools.product((True, False), range(4), (True, False), R.SQRT_AT):
        cf = _cf(3.0, hist, sqrt_at, noise)
        hs = [h1, h2, h3][:hist]
        (xp, x0, e), _ = R.sd_step_restate(x, ou if guided else None, oc, hs, nz if noise else None, cf, param)
        o, _ = fk._guided(ou if guided else None, oc, cf["cfg_scale"])
        eps = R.to_eps(o, x, cf["sqrt_at"], cf["sqrt_one_minus_at"], param)
        (wp, w0, we), _ = fk.sd_step_restate(x, None, eps, hs, nz if noise else None, cf)
        _same(e, we), _same(xp, wp)
        # pred_x0: with a history, the eps expression.  Without one (DDIM) the V form sat x - somat o is predict_start_from_z_and_v
        slack = _unit_slack(cf["sqrt_at"], cf["sqrt_one_minus_at"], x, param)
        assert slack < 1e-5
        _same(x0, w0, slack if hist == 0 else 0.0)
        if hist == 0:
            o64, x64 = o.double(), x.double()
            _same(x0, cf["sqrt_at"] * x64 - cf["sqrt_one_minus_at"] * o64 if param == "v" else o64)
    for guided, with_mp in itertools.product((True, False), (True, False)):
        (xn, m), _ = R.dpm_step_restate(x, ou if guided else None, oc, h1 if with_mp else None, param=param, **DPM)
        o, _ = fk._guided(ou if guided else None, oc, fk.f32c(DPM["cfg"]))
        eps = R.to_eps(o, x, fk.f32c(DPM["alpha_s"]), fk.f32c(DPM["sigma_s"]), param)
        (wn, wm), _ = fk.dpm_step_restate(x, None, eps, h1 if with_mp else None, **DPM)
        slack = _unit_slack(fk.f32c(DPM["alpha_s"]), fk.f32c(DPM["sigma_s"]), x, param)
        assert slack < 1e-6
        _same(xn, wn, slack), _same(m, wm, slack)
        for depth, corr, pred in itertools.product(range(4), (CORR, None), (PRED, None)):
            kw = dict(cfg=3.0, sigma=0.929, alpha=0.37, corr=corr, pred=pred)
            got, _ = R.unipc_step_restate(x, ou if guided else None, oc, xb, [h1, h2, h3][:depth], param=param, **kw)
            o, _ = fk._guided(ou if guided else None, oc, fk.f32c(3.0))
            eps = R.to_eps(o, x, fk.f32c(0.37), fk.f32c(0.929), param)
            want, _ = U.sd_step_restate(x, None, eps, xb, [h1, h2, h3][:depth], **kw)
            for a, b in zip(got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    _same(a, b, _unit_slack(fk.f32c(0.37), fk.f32c(0.929), x, param))


def test_eps_restatements_are_the_existing_ones():
    x, ou, oc, h1, nz = R.latents(300, 4, 5)
    cf = _cf(7.5, 1, 0.5, True)
    for a, b in zip(R.sd_step_restate(x, ou, oc, [h1], nz, cf, "eps"), fk.sd_step_restate(x, ou, oc, [h1], nz, cf)):
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    for a, b in zip(R.dpm_step_restate(x, ou, oc, h1, param="eps", **DPM), fk.dpm_step_restate(x, ou, oc, h1, **DPM)):
        assert all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------ fp32 emulation of the header's operation order
def _f(v):
    return np.float32(v)


def _emulate_guided(ou, oc, cfg):
    if ou is None:
        return oc.numpy()
    u, c = ou.numpy(), oc.numpy()
    return u + _f(cfg) * (c - u)


def _emulate_sd(x, ou, oc, hs, nz, cf, param):
    x = x.numpy()
    o = _emulate_guided(ou, oc, cf["cfg_scale"])
    sat, somat = _f(cf["sqrt_at"]), _f(cf["sqrt_one_minus_at"])
    e = sat * o + somat * x if param == "v" else (x - sat * o) / somat
    ep = _f(cf["w"][0]) * e
    for w, h in zip(cf["w"][1:], hs):
        ep = ep + _f(w) * h.numpy()
    x0 = (x - somat * ep) / sat
    xp = _f(cf["sqrt_a_prev"]) * x0 + _f(cf["dir_coef"]) * ep
    if nz is not None:
        xp = xp + _f(cf["sigma"]) * nz.numpy()
    if not hs and cf["w"][0] == 1.0:
        x0 = sat * x - somat * o if param == "v" else o
    return xp, x0, e


@pytest.mark.parametrize("param", ["v", "x0"])
def test_fp32_emulation_is_within_the_bounds_and_planted_defects_are_not(param):
    x, ou, oc, h1, h2, h3, nz = R.latents(4000, 5, 7)
    for guided, hist, noise, sqrt_at in itertools.product((True, False), range(4), (True, False), R.SQRT_AT):
        cf = _cf(3.0, hist, sqrt_at, noise)
        hs = [h1, h2, h3][:hist]
        refs, bounds = R.sd_step_restate(x, ou if guided else None, oc, hs, nz if noise else None, cf, param)
        got = _emulate_sd(x, ou if guided else None, oc, hs, nz if noise else None, cf, param)
        assert all(g.dtype == np.float32 for g in got)
        assert max(_ratio(g, r, b) for g, r, b in zip(got, refs, bounds)) <= 1.0, (guided, hist, noise, sqrt_at)
        if param == "v":     # sqrt_at and sqrt_one_minus_at exchanged in the conversion
            bad, _ = R.sd_step_restate(x, ou if guided else None, oc, hs, nz if noise else None, cf, param, defect="swap")
            assert _ratio(bad[0], refs[0], bounds[0]) > 1.0 and _ratio(bad[2], refs[2], bounds[2]) > 1.0
        if guided:           # the halves converted first and combined with another scale
            bad, _ = R.sd_step_restate(x, ou, oc, hs, nz if noise else None, cf, param, defect="combine_after")
            assert _ratio(bad[0], refs[0], bounds[0]) > 1.0 and _ratio(bad[2], refs[2], bounds[2]) > 1.0
    for guided, with_mp in itertools.product((True, False), (True, False)):
        refs, bounds = R.dpm_step_restate(x, ou if guided else None, oc, h1 if with_mp else None, param=param, **DPM)
        o = _emulate_guided(ou if guided else None, oc, DPM["cfg"])
        m = _f(DPM["alpha_s"]) * x.numpy() - _f(DPM["sigma_s"]) * o if param == "v" else o
        xn = _f(DPM["a"]) * x.numpy() + _f(DPM["b0"]) * m
        if with_mp:
            xn = xn + _f(DPM["b1"]) * h1.numpy()
        assert max(_ratio(xn, refs[0], bounds[0]), _ratio(m, refs[1], bounds[1])) <= 1.0
        if param == "v":
            bad, _ = R.dpm_step_restate(x, ou if guided else None, oc, h1 if with_mp else None, param=param, defect="swap", **DPM)
            assert _ratio(bad[1], refs[1], bounds[1]) > 1.0
            um, ub = R.unipc_step_restate(x, ou if guided else None, oc, h2, [h1], cfg=3.0, sigma=0.6, alpha=0.8, corr=CORR, pred=PRED,
                                          param=param)
            bad, _ = R.unipc_step_restate(x, ou if guided else None, oc, h2, [h1], cfg=3.0, sigma=0.6, alpha=0.8, corr=CORR, pred=PRED,
                                          param=param, defect="swap")
            assert all(_ratio(b, r, bd) > 1.0 for b, r, bd in zip(bad, um, ub))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gelu_restatement_emulation_and_defects(dtype):
    u = R.gelu_inputs(77, 512, dtype, 9)
    ref, bound = R.gelu_restate(u, dtype)
    assert torch.isfinite(ref).all() and (bound > 0).all()
    torch.testing.assert_close(ref[8:].float(), torch.nn.functional.gelu(u.float())[8:], rtol=1e-5, atol=1e-6)
    a = u.float()
    got = (0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752))).to(dtype)      # the kernel's fp32 expression, one rounding
    assert _ratio(got, ref, bound) <= 1.0
    quick = (a * torch.sigmoid(1.702 * a)).to(dtype)                              # the other activation
    tanh = torch.nn.functional.gelu(a, approximate="tanh").to(dtype)              # the tanh approximation
    twice = (0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752))).to(dtype).float().to(dtype)
    assert _ratio(quick, ref, bound) > 1.0 and _ratio(tanh, ref, bound) > 1.0 and _ratio(twice, ref, bound) <= 1.0


# ------------------------------------------------------------------ the entry points
def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks run before any pointer is read: host placeholders stand in for the device buffers, the stream is null."""
    from autodiffusion_amd import _lib
    lib = _lib.load()
    P = 0x1000

    def sd(param, sqrt_one_minus_at=0.6, **over):
        c = fk.sd_coefs_of(3.0, 0, 0.8, False)
        c.sqrt_one_minus_at = sqrt_one_minus_at
        a = dict(x=P, ou=P, oc=P, h1=None, h2=None, h3=None, noise=None, x_prev=P, pred_x0=P, e_out=P, numel=64, c=C.byref(c))
        a.update(over)
        return lib.adm_sd_step_p(*a.values(), None, param)
    for call, word in ((lambda: sd(3), b"param"), (lambda: sd(-1), b"param"), (lambda: sd(1, 0.0), b"x0 parameterisation"),
                       (lambda: sd(2, x=None), b"null"), (lambda: sd(2, oc=None), b"null"), (lambda: sd(1, x_prev=None), b"null"),
                       (lambda: sd(2, c=None), b"null"), (lambda: sd(2, numel=0), b"empty")):
        assert call() == -1 and word in lib.adm_last_error(), word

    def dpm(param, alpha_s=0.8, **over):
        a = dict(x=P, ou=P, oc=P, m_prev=None, x_next=P, m_out=P, numel=64)
        a.update(over)
        return lib.adm_dpm_step_p(*a.values(), 3.0, 0.6, alpha_s, 0.75, 0.4, -0.12, None, param)
    for call, word in ((lambda: dpm(3), b"param"), (lambda: dpm(2, x=None), b"null"), (lambda: dpm(1, oc=None), b"null"),
                       (lambda: dpm(2, x_next=None), b"null"), (lambda: dpm(2, 0.0), b"alpha_s"), (lambda: dpm(1, numel=0), b"empty")):
        assert call() == -1 and word in lib.adm_last_error(), word

    def uni(**over):
        a = _lib.UnipcArgs()
        for k in ("x_eval", "eps_uncond", "eps_cond", "x_base", "h1", "h2", "h3", "m_out", "x_corr", "x_pred"):
            setattr(a, k, P)
        a.numel, a.cfg_scale, a.sigma_s, a.alpha_s = 64, 3.0, 0.929, 0.37
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.adm_unipc_step_p(C.byref(uni()), None, 3) == -1 and b"param" in lib.adm_last_error()
    assert lib.adm_unipc_step_p(None, None, 2) == -1 and b"null" in lib.adm_last_error()
    for over, word in ((dict(x_eval=None), b"null"), (dict(eps_cond=None), b"null"), (dict(m_out=None), b"null"),
                       (dict(x_base=None), b"x_base"), (dict(numel=0), b"numel"), (dict(alpha_s=0.0), b"alpha_s")):
        for param in (1, 2):
            assert lib.adm_unipc_step_p(C.byref(uni(**over)), None, param) == -1 and word in lib.adm_last_error(), over
    # the eps-only symbol keeps refusing a non-zero `flags`
    assert lib.adm_unipc_step(C.byref(uni()), None, 1) == -1 and lib.adm_unipc_step(C.byref(uni()), None, 2) == -1
    for args, word in (((None, P, 4, 8), b"null"), ((P, None, 4, 8), b"null"), ((P, P, 0, 8), b"unsupported"), ((P, P, 4, 12), b"unsupported"),
                       ((P + 2, P, 4, 8), b"unaligned")):
        assert lib.adm_gelu(*args, None, 0) != 0 and word in lib.adm_last_error(), args
    assert lib.adm_gelu(P, P, 4, 8, None, 1) == -1 and b"flags" in lib.adm_last_error()


def test_header_and_binding_table_declare_the_new_symbols():
    from autodiffusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    for name in ("adm_sd_step_p", "adm_dpm_step_p", "adm_unipc_step_p", "adm_gelu"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    for k, v in R.PARAMS.items():
        assert f"#define ADM_PARAM_{k.upper()} {v}" in header and _lib.PARAMS[k] == v


def test_python_steps_and_latent_diffusion_refuse_an_unknown_parameterisation():
    from autodiffusion_amd import sd_sampler as S
    with pytest.raises(ValueError, match="'w'"):
        S.LatentDiffusion(None, device="cpu", parameterization="w")
    for p in ("eps", "x0", "v"):
        assert S.LatentDiffusion(None, device="cpu", parameterization=p).parameterization == p
    assert S.LatentDiffusion(None, device="cpu").parameterization == "eps"
    x = torch.zeros(1, 4, 2, 2)
    for call in (lambda: S.sd_step(x, x, 1, 1.0, (1.0,), (), 0.5, 0.6, 0.0, param="w"),
                 lambda: S.dpm_step(x, x, 1, 1.0, None, 0.6, 0.8, 0.7, 0.4, 0.0, param="w"),
                 lambda: S.unipc_step(x, x, 1, 1.0, None, [], 0.6, 0.8, None, PRED, param="w")):
        with pytest.raises(ValueError, match="'w'"):
            call()

    class Toy:
        pass
    toy = Toy()
    toy.num_timesteps = 10
    assert S.DDIMSampler(toy)._param == "eps"           # the toy models of the existing tests have no such attribute
    toy.parameterization = "v"
    assert S.PLMSSampler(toy)._param == "v"


# ------------------------------------------------------------------ the OpenCLIP cond stage
TINY2 = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=16,
             hidden_act="gelu")


def _openclip_sd(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    c, i = cfg["hidden_size"], cfg["intermediate_size"]
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    sd = {"model.token_embedding.weight": r(cfg["vocab_size"], c), "model.positional_embedding": r(cfg["max_position_embeddings"], c),
          "model.ln_final.weight": r(c), "model.ln_final.bias": r(c)}
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.transformer.resblocks.{l}."
        sd.update({p + "ln_1.weight": r(c), p + "ln_1.bias": r(c), p + "attn.in_proj_weight": r(3 * c, c), p + "attn.in_proj_bias": r(3 * c),
                   p + "attn.out_proj.weight": r(c, c), p + "attn.out_proj.bias": r(c), p + "ln_2.weight": r(c), p + "ln_2.bias": r(c),
                   p + "mlp.c_fc.weight": r(i, c), p + "mlp.c_fc.bias": r(i), p + "mlp.c_proj.weight": r(c, i), p + "mlp.c_proj.bias": r(c)})
    return sd


def test_openclip_state_dict_is_remapped_and_the_unused_keys_are_ignored():
    from autodiffusion_amd.sd_clip import OPENCLIP_VIT_H14_TEXT, FrozenOpenCLIPEmbedder
    assert OPENCLIP_VIT_H14_TEXT == dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24,
                                         num_attention_heads=16, max_position_embeddings=77, hidden_act="gelu")
    sd = _openclip_sd(TINY2)
    emb = FrozenOpenCLIPEmbedder(device="cpu", max_length=16, layer="penultimate", config=TINY2)
    plan = emb.transformer.plan
    assert plan.hidden_act == "gelu" and plan.run_layers == 1 and plan.num_hidden_layers == 2
    extra = {"model.text_projection": torch.zeros(64, 32), "model.logit_scale": torch.zeros(()), "model.attn_mask": torch.zeros(16, 16),
             "model.visual.conv1.weight": torch.zeros(8, 3, 2, 2), "model.visual.transformer.resblocks.0.ln_1.weight": torch.zeros(8)}
    emb.load_state_dict({**sd, **extra}, strict=True)
    got = emb.transformer.state_dict()
    c = TINY2["hidden_size"]
    assert len(got) == len(plan.param_shapes()) == len(sd) + 8       # in_proj weight and bias of two layers become q, k, v each
    assert torch.equal(got["text_model.embeddings.token_embedding.weight"], sd["model.token_embedding.weight"])
    assert torch.equal(got["text_model.embeddings.position_embedding.weight"], sd["model.positional_embedding"])
    assert torch.equal(got["text_model.final_layer_norm.bias"], sd["model.ln_final.bias"])
    for l in range(2):
        p, q = f"model.transformer.resblocks.{l}.", f"text_model.encoder.layers.{l}."
        back = torch.cat([got[q + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        assert torch.equal(back, sd[p + "attn.in_proj_weight"])                                   # the round trip
        assert torch.equal(torch.cat([got[q + f"self_attn.{n}_proj.bias"] for n in "qkv"]), sd[p + "attn.in_proj_bias"])
        assert torch.equal(got[q + "self_attn.v_proj.weight"], sd[p + "attn.in_proj_weight"][2 * c:])
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
                     ("mlp.c_proj", "mlp.fc2")):
            assert torch.equal(got[q + b + ".weight"], sd[p + a + ".weight"]) and torch.equal(got[q + b + ".bias"], sd[p + a + ".bias"])
    with pytest.raises(RuntimeError, match="unexpected"):
        emb.load_state_dict({**sd, "model.unknown": torch.zeros(1)}, strict=True)
    with pytest.raises(RuntimeError, match="unexpected"):
        emb.load_state_dict({**sd, "transformer.text_model.final_layer_norm.bias": torch.zeros(c)}, strict=True)
    emb.load_state_dict({**sd, "model.unknown": torch.zeros(1)}, strict=False)
    with pytest.raises(RuntimeError, match="missing"):
        emb.load_state_dict({k: v for k, v in sd.items() if k != "model.ln_final.bias"})
    last = FrozenOpenCLIPEmbedder(device="cpu", max_length=16, config=TINY2)
    assert last.layer == "last" and last.transformer.plan.run_layers == 0
    with pytest.raises(ValueError):
        FrozenOpenCLIPEmbedder(device="cpu", layer="pooled", config=TINY2)
    with pytest.raises(ValueError):
        FrozenOpenCLIPEmbedder(device="cpu", layer="penultimate", config=dict(TINY2, num_hidden_layers=1))
    # a checkpoint's cond_stage_model.* tensors reach it through LatentDiffusion's router, prefix stripped
    from autodiffusion_amd.sd_sampler import LatentDiffusion

    class _Net:
        def load_state_dict(self, sd, strict=True):
            self.got = dict(sd)
    ld = LatentDiffusion(_Net(), device="cpu", cond_stage=FrozenOpenCLIPEmbedder(device="cpu", max_length=16, config=TINY2),
                         parameterization="v")
    ld.load_state_dict({**{"cond_stage_model." + k: v for k, v in {**sd, **extra}.items()}, "model.diffusion_model.w": torch.zeros(1)})
    assert torch.equal(ld.cond_stage_model.transformer.state_dict()["text_model.final_layer_norm.weight"], sd["model.ln_final.weight"])
    assert list(ld.model.got) == ["w"]


def test_text_transformer_options_are_checked():
    from autodiffusion_amd.sd_clip import CLIPTextTransformer
    base = {k: v for k, v in TINY2.items() if k != "hidden_act"}
    assert CLIPTextTransformer(**base).plan.hidden_act == "quick_gelu" and CLIPTextTransformer(**base).plan.run_layers == 0
    assert CLIPTextTransformer(**base, run_layers=2).plan.run_layers == 2
    for bad in (dict(hidden_act="relu"), dict(run_layers=0), dict(run_layers=3)):
        with pytest.raises(ValueError):
            CLIPTextTransformer(**base, **bad)


class _FakeTokenizer:
    """CLIP's padding: <|endoftext|> up to max_length."""

    def __init__(self, rows):
        self.rows = rows

    def __call__(self, text, max_length, **kw):
        assert kw["padding"] == "max_length" and kw["truncation"]
        return {"input_ids": torch.tensor(self.rows, dtype=torch.int64)[:len(text), :max_length]}


def test_openclip_padding_rule():
    from autodiffusion_amd.sd_clip import FrozenOpenCLIPEmbedder, openclip_pad
    eos, bos = 63, 62
    rows = [[bos, 5, 9, eos, eos, eos, eos, eos], [bos, eos, eos, eos, eos, eos, eos, eos], [bos, 1, 2, 3, 4, 5, 6, eos],
            [bos, 1, 2, 3, 4, 5, 6, 7]]
    want = [[bos, 5, 9, eos, 0, 0, 0, 0], [bos, eos, 0, 0, 0, 0, 0, 0], [bos, 1, 2, 3, 4, 5, 6, eos], [bos, 1, 2, 3, 4, 5, 6, 7]]
    src = torch.tensor(rows)
    assert openclip_pad(src, eos).tolist() == want and src.tolist() == rows     # a copy: the caller's ids are untouched
    emb = FrozenOpenCLIPEmbedder(device="cpu", max_length=8, config=TINY2, tokenizer=_FakeTokenizer(rows))
    seen = []
    emb.transformer.forward = lambda ids: seen.append(ids.clone()) or ids
    emb(["a", "", "b", "c"])
    assert seen[-1].tolist() == want
    emb(src)                                                                     # integer tensors enter unchanged
    assert seen[-1].tolist() == rows
    from autodiffusion_amd.sd_script_util import EmptyPromptTokenizer
    assert EmptyPromptTokenizer(64)([""], 5)["input_ids"].tolist() == [[bos, eos, eos, eos, eos]]
    assert EmptyPromptTokenizer(64, pad=0)(["", ""], 5)["input_ids"].tolist() == 2 * [[bos, eos, 0, 0, 0]]
    assert EmptyPromptTokenizer(64, pad=0)([""], 1)["input_ids"].tolist() == [[bos]]
    with pytest.raises(SystemExit):
        EmptyPromptTokenizer(64, pad=0)(["x"], 5)


# ------------------------------------------------------------------ builders and command lines
class _NoUNet:
    def __init__(self, **kw):
        self.kw = kw

    def set_torso(self, torso):
        return self

    def randomize_(self, seed):
        self.seed = seed

    def to(self, device):
        return self


YAML = """model:
  target: ldm.models.diffusion.ddpm.LatentDiffusion
  params:
    {param_line}
    linear_start: 0.00085
    linear_end: 0.0120
    timesteps: 1000
    scale_factor: 0.18215
    unet_config:
      target: ldm.modules.diffusionmodules.openaimodel.UNetModel
      params:
        use_checkpoint: True
        use_fp16: True
        image_size: 32
        in_channels: 4
        out_channels: 4
        model_channels: 64
        attention_resolutions: [1, 2]
        num_res_blocks: 1
        channel_mult: [1, 2]
        num_head_channels: 64
        use_spatial_transformer: True
        use_linear_in_transformer: True
        transformer_depth: 1
        context_dim: 128
        legacy: False
    first_stage_config:
      target: ldm.models.autoencoder.AutoencoderKL
      params:
        embed_dim: 4
        ddconfig:
          ch: 32
          out_ch: 3
          ch_mult: [1, 2, 4]
          num_res_blocks: 1
          attn_resolutions: []
          dropout: 0.0
          in_channels: 3
          resolution: 32
          z_channels: 4
    cond_stage_config:
      target: {target}
      params:
        {cond_params}
"""


def _build_from_yaml(tmp_path, monkeypatch, **fmt):
    from autodiffusion_amd import logger, sd_script_util
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    path = tmp_path / "model.yaml"
    path.write_text(YAML.format(**fmt))
    loaded = []
    monkeypatch.setattr(sd_script_util, "UNetModel", _NoUNet)
    monkeypatch.setattr(logger, "log", lambda *a: None)
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"state_dict": {"k": 1}})
    monkeypatch.setattr(LatentDiffusion, "load_state_dict", lambda self, sd, strict=True: loaded.append(sd))
    opt = argparse.Namespace(synthetic="", config=str(path), ckpt="none.ckpt", tokenizer_dir="", torso="bf16")
    model = sd_script_util.build_model(opt, torch.device("cpu"), prompt_len=8)
    assert loaded == [{"k": 1}]
    return model


def test_build_model_reads_the_family_from_the_yaml(tmp_path, monkeypatch):
    from autodiffusion_amd.sd_clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder
    m = _build_from_yaml(tmp_path, monkeypatch, param_line='parameterization: "v"',
                         target="ldm.modules.encoders.modules.FrozenOpenCLIPEmbedder",
                         cond_params='freeze: True\n        layer: "penultimate"\n        config: {vocab_size: 512, hidden_size: 128, '
                                     'intermediate_size: 512, num_hidden_layers: 2, num_attention_heads: 2}')
    assert m.parameterization == "v" and type(m.cond_stage_model) is FrozenOpenCLIPEmbedder
    plan = m.cond_stage_model.transformer.plan
    assert plan.hidden_act == "gelu" and plan.run_layers == 1 and m.cond_stage_model.layer == "penultimate"
    assert m.model.kw["use_linear_in_transformer"] is True and m.model.kw["num_head_channels"] == 64
    assert m.cond_stage_model._tokenizer([""], 4)["input_ids"].tolist() == [[510, 511, 0, 0]]
    m = _build_from_yaml(tmp_path, monkeypatch, param_line="conditioning_key: crossattn",
                         target="ldm.modules.encoders.modules.FrozenCLIPEmbedder",
                         cond_params="config: {vocab_size: 512, hidden_size: 128, intermediate_size: 512, num_hidden_layers: 1, "
                                     "num_attention_heads: 2}")
    assert m.parameterization == "eps" and type(m.cond_stage_model) is FrozenCLIPEmbedder
    assert m.cond_stage_model.transformer.plan.hidden_act == "quick_gelu"
    assert m.cond_stage_model._tokenizer([""], 4)["input_ids"].tolist() == [[510, 511, 511, 511]]
    with pytest.raises(SystemExit, match="BERTEmbedder"):
        _build_from_yaml(tmp_path, monkeypatch, param_line="conditioning_key: crossattn",
                         target="ldm.modules.encoders.modules.BERTEmbedder", cond_params="n_embed: 1280")


@pytest.mark.parametrize("synthetic", ["tiny2", "v2"])
def test_synthetic_sd2_families_build_on_the_host(synthetic, monkeypatch):
    from autodiffusion_amd import logger, sd_script_util
    from autodiffusion_amd.sd_arch import SD_V2
    from autodiffusion_amd.sd_clip import FrozenOpenCLIPEmbedder
    monkeypatch.setattr(sd_script_util, "UNetModel", _NoUNet)
    monkeypatch.setattr(logger, "log", lambda *a: None)
    if synthetic == "v2":    # the full-size towers are not allocated on the host: the arguments are what is checked
        made = {}

        class _NoClip(_NoUNet):
            transformer = argparse.Namespace(plan=argparse.Namespace(vocab_size=49408))

            def __init__(self, **kw):
                made.update(kw)
        monkeypatch.setattr(sd_script_util, "FrozenOpenCLIPEmbedder", _NoClip)
        monkeypatch.setattr(sd_script_util, "AutoencoderKL", _NoUNet)
    opt = argparse.Namespace(synthetic=synthetic, config="", ckpt="", tokenizer_dir="", torso="bf16")
    m = sd_script_util.build_model(opt, torch.device("cpu"), prompt_len=8)
    assert m.parameterization == "v" and m.model.seed == 1234
    if synthetic == "v2":
        assert made["config"]["hidden_size"] == 1024 and made["layer"] == "penultimate" and made["max_length"] == 8
        assert {k: m.model.kw[k] for k in SD_V2} == SD_V2
        assert SD_V2 == dict(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=(4, 2, 1), num_res_blocks=2,
                             channel_mult=(1, 2, 4, 4), num_head_channels=64, use_linear_in_transformer=True, transformer_depth=1,
                             context_dim=1024, legacy=False)
        return
    assert type(m.cond_stage_model) is FrozenOpenCLIPEmbedder and m.cond_stage_model.layer == "penultimate"
    plan = m.cond_stage_model.transformer.plan
    assert (plan.hidden_size, plan.num_hidden_layers, plan.run_layers, plan.hidden_act) == (128, 2, 1, "gelu")
    assert m.model.kw["num_head_channels"] == 64 and "num_heads" not in m.model.kw and m.model.kw["use_linear_in_transformer"] is True
    assert m.cond_stage_model._tokenizer([""], 3)["input_ids"].tolist() == [[510, 511, 0]]


def test_linear_transformer_projections_change_only_the_stored_shape():
    from autodiffusion_amd.sd_arch import SDTransformerSpec, sd_unet_plan
    from autodiffusion_amd.sd_script_util import TINY2_UNET, TINY_UNET
    from autodiffusion_amd.sd_unet import UNetModel
    lin, conv = sd_unet_plan(**TINY2_UNET), sd_unet_plan(**dict(TINY2_UNET, use_linear_in_transformer=False))
    a, b = lin.param_shapes(), conv.param_shapes()
    assert list(a) == list(b)
    diff = [k for k in a if a[k] != b[k]]
    assert diff and all(k.endswith(("proj_in.weight", "proj_out.weight")) and b[k] == a[k] + (1, 1) for k in diff)
    specs = [s for s in lin.all_blocks() if isinstance(s, SDTransformerSpec)]
    assert specs and all(s.linear and s.d_head == 64 and s.heads == s.channels // 64 for s in specs)
    assert list(sd_unet_plan(**TINY_UNET).param_shapes()) == list(a)       # the v1-style tiny network has the same tensors by name
    net = UNetModel(image_size=32, use_spatial_transformer=True, **TINY2_UNET)
    sd = net.state_dict()
    assert all(tuple(sd[k].shape) == a[k] for k in a)
    with pytest.raises(Exception):
        net.load_state_dict({k: (v.reshape(v.shape + (1, 1)) if k in diff else v) for k, v in sd.items()})
    net.load_state_dict({k: v.clone() for k, v in sd.items()})


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_synthetic_tiny2_parses_and_nothing_else_moves():
    ea = _script("sd_search_ea").create_argparser()
    base, two = ea.parse_args(["--synthetic", "tiny"]), ea.parse_args(["--synthetic", "tiny2"])
    assert list(vars(base)) == list(vars(two))
    assert {k for k in vars(base) if getattr(base, k) != getattr(two, k)} == {"synthetic"} and two.synthetic == "tiny2"
    assert ea.parse_args(["--synthetic", "v2"]).synthetic == "v2" and ea.parse_args([]).synthetic == ""
    for name, req in (("sd_img2img", ["--init-img", "i.npy"]), ("sd_inpaint", ["--init-img", "i.npy", "--mask", "m.npy"])):
        p = _script(name).create_argparser()
        a, b = p.parse_args(req), p.parse_args(req + ["--synthetic", "tiny2"])
        assert list(vars(a)) == list(vars(b)) and b.synthetic == "tiny2" and a.synthetic == ""
    with pytest.raises(SystemExit):
        ea.parse_args(["--synthetic", "v3"])
