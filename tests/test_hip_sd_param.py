"""GPU: the parameterised latent sampler steps (adm_sd_step_p, adm_dpm_step_p, adm_unipc_step_p) and the exact GELU (adm_gelu)
against the float64 restatements of tests/sd_param_ref.py on guarded operands, and the four latent samplers on a v- / x0-predicting
toy model: DPM-Solver++ against the reference capture (tests/golden/sd_param_dpm.npz), DDIM, PLMS and UniPC update by update
against the restatements on the recorded operands and, end to end, against float64 loops written from the definitions (DESIGN.md
8.7).  Every direct launch writes into carves of tests/guarded.py: margins intact, every element written and within its bound.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import f32_kernels as fk
import guarded
import sd_param_ref as R
from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
CORR = (0.81, -0.55, 0.23, -0.07, 0.031)
PRED = (0.64, 0.47, -0.19, 0.052)
DPM = dict(cfg=3.0, sigma_s=0.6, alpha_s=0.8, a=0.75, b0=0.4, b1=-0.12)
SIZES = [(n, 0) for n in R.NUMELS] + [(4 * 257, 1)]     # (numel, offset in elements): the last one starts 4 bytes off a 16-byte line


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _G:
    """guarded.Guarded whose carves may start `offset` elements (4 bytes each) off the 16-byte line: the margins are then held by
    the same bitwise comparison, without Carve.guard_ok's alignment assertion."""

    def __init__(self, offset=0):
        self.offset, self.carves = offset, []

    def _add(self, what, shape, output, src=None):
        c = guarded.Carve(what, shape, F32, DEV, guarded.GUARD, guarded.GUARD + self.offset, output, guarded.NAN if output else 0.0)
        if src is not None:
            c.view.copy_(src)
        self.carves.append(c)
        return c.view

    def inp(self, what, t):
        return None if t is None else self._add(what, t.shape, False, t)

    def out(self, what, shape):
        return self._add(what, shape, True)

    def check(self):
        for c in self.carves:
            if self.offset == 0:
                c.check()
                continue
            assert c.view.data_ptr() % 16 == 4 * self.offset
            front, back = c._margins()
            for m in (front, back):
                ok = (m.view(torch.int32) == torch.full((1,), guarded.SENTINEL, dtype=F32, device=DEV).view(torch.int32)) if c.output \
                    else torch.isnan(m)
                assert bool(ok.all()), f"{c.what}: a margin was written"
            c.finite_ok()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hold(what, got, ref, bound):
    r = float(((got.cpu().double() - ref).abs() / bound).max())
    assert r <= 1.0, (what, r)
    return r


# ------------------------------------------------------------------ adm_sd_step_p
def _sd_launch(lib, g, t, guided, hist, noise, cs, pid):
    x, ou, oc, h1, h2, h3, nz = t
    d = dict(x=g.inp("x", x), ou=g.inp("ou", ou) if guided else None, oc=g.inp("oc", oc))
    hs = [g.inp(f"h{i + 1}", h) for i, h in enumerate((h1, h2, h3)[:hist])] + [None] * (3 - hist)
    nzd = g.inp("noise", nz) if noise else None
    outs = [g.out(k, x.shape) for k in ("x_prev", "pred_x0", "e_out")]
    args = (_p(d["x"]), _p(d["ou"]), _p(d["oc"]), _p(hs[0]), _p(hs[1]), _p(hs[2]), _p(nzd), *(_p(o) for o in outs), x.numel(), C.byref(cs))
    from autodiffusion_amd import _lib
    if pid is None:
        _lib.check(lib.adm_sd_step(*args, _stream()), "adm_sd_step (guarded)")
    else:
        _lib.check(lib.adm_sd_step_p(*args, _stream(), pid), "adm_sd_step_p (guarded)")
    torch.cuda.synchronize()
    g.check()
    return outs


@pytest.mark.parametrize("numel,offset", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("param", ["eps", "x0", "v"])
def test_sd_step_p_every_operand_subset(param, numel, offset):
    from autodiffusion_amd import _lib
    lib = _lib.load()
    t = R.latents(numel, 40 + numel, 7)
    worst = 0.0
    for j, (guided, hist, noise) in enumerate(itertools.product((True, False), range(4), (True, False))):
        cs = fk.sd_coefs_of(3.0, hist, R.SQRT_AT[j % 3], noise)
        outs = _sd_launch(lib, _G(offset), t, guided, hist, noise, cs, R.PARAMS[param])
        x, ou, oc, h1, h2, h3, nz = t
        refs, bounds = R.sd_step_restate(x, ou if guided else None, oc, [h1, h2, h3][:hist], nz if noise else None, fk.sd_coefs_dict(cs), param)
        for what, got, r, b in zip(("x_prev", "pred_x0", "e_out"), outs, refs, bounds):
            worst = max(worst, _hold((param, what, guided, hist, noise, R.SQRT_AT[j % 3]), got, r, b))
        if param == "eps":       # through the _p symbol: the launch the eps-only symbol makes, bit for bit
            old = _sd_launch(lib, _G(offset), t, guided, hist, noise, cs, None)
            assert all(torch.equal(a, b) for a, b in zip(outs, old))
    print(f"sd_step_p {param} numel {numel} offset {offset}: worst err/bound {worst:.3f}")


def test_sd_step_p_optional_outputs_and_refusals_write_nothing():
    from autodiffusion_amd import _lib
    lib = _lib.load()
    x, o = (v.to(DEV) for v in R.latents(257, 7, 2))
    cs = fk.sd_coefs_of(1.0, 0, 0.5, False)
    g = guarded.Guarded(DEV)
    xp = g.out("x_prev", x.shape, F32)
    _lib.check(lib.adm_sd_step_p(_p(x), None, _p(o), None, None, None, None, _p(xp), None, None, 257, C.byref(cs), _stream(), 2), "adm_sd_step_p")
    torch.cuda.synchronize()
    g.check()
    (ref, _, _), (b, _, _) = R.sd_step_restate(x.cpu(), None, o.cpu(), [], None, fk.sd_coefs_dict(cs), "v")
    _hold("x_prev alone", xp, ref, b)
    bad = fk.sd_coefs_of(1.0, 0, 0.5, False)
    bad.sqrt_one_minus_at = 0.0
    for cs_, pid in ((cs, 3), (cs, -1), (bad, 1)):
        g = guarded.Guarded(DEV)
        outs = [g.out(k, x.shape, F32) for k in ("x_prev", "pred_x0", "e_out")]
        rc = lib.adm_sd_step_p(_p(x), None, _p(o), None, None, None, None, *(_p(t) for t in outs), 257, C.byref(cs_), _stream(), pid)
        torch.cuda.synchronize()
        assert rc == -1 and lib.adm_last_error()
        guarded.untouched(g)


# ------------------------------------------------------------------ adm_dpm_step_p
def _dpm_launch(lib, g, t, guided, with_mp, pid):
    from autodiffusion_amd import _lib
    x, ou, oc, mp = t
    d = [g.inp("x", x), g.inp("ou", ou) if guided else None, g.inp("oc", oc), g.inp("m_prev", mp) if with_mp else None]
    xn, mo = g.out("x_next", x.shape), g.out("m_out", x.shape)
    args = (*(_p(v) for v in d), _p(xn), _p(mo), x.numel(), DPM["cfg"], DPM["sigma_s"], DPM["alpha_s"], DPM["a"], DPM["b0"], DPM["b1"])
    if pid is None:
        _lib.check(lib.adm_dpm_step(*args, _stream()), "adm_dpm_step (guarded)")
    else:
        _lib.check(lib.adm_dpm_step_p(*args, _stream(), pid), "adm_dpm_step_p (guarded)")
    torch.cuda.synchronize()
    g.check()
    return xn, mo


@pytest.mark.parametrize("numel,offset", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("param", ["eps", "x0", "v"])
def test_dpm_step_p_every_operand_subset(param, numel, offset):
    from autodiffusion_amd import _lib
    lib = _lib.load()
    t = R.latents(numel, 50 + numel, 4)
    worst = 0.0
    for guided, with_mp in itertools.product((True, False), (True, False)):
        outs = _dpm_launch(lib, _G(offset), t, guided, with_mp, R.PARAMS[param])
        x, ou, oc, mp = t
        refs, bounds = R.dpm_step_restate(x, ou if guided else None, oc, mp if with_mp else None, param=param, **DPM)
        for what, got, r, b in zip(("x_next", "m_out"), outs, refs, bounds):
            worst = max(worst, _hold((param, what, guided, with_mp), got, r, b))
        if param == "eps":
            old = _dpm_launch(lib, _G(offset), t, guided, with_mp, None)
            assert all(torch.equal(a, b) for a, b in zip(outs, old))
    print(f"dpm_step_p {param} numel {numel} offset {offset}: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------ adm_unipc_step_p
def _uni_launch(lib, g, t, guided, depth, has_corr, has_pred, pid):
    from autodiffusion_amd import _lib
    x, xb, ou, oc, h1, h2, h3 = t
    a = _lib.UnipcArgs()
    a.x_eval, a.eps_cond = _p(g.inp("x_eval", x)), _p(g.inp("oc", oc))
    a.eps_uncond = _p(g.inp("ou", ou)) if guided else None
    a.x_base = _p(g.inp("x_base", xb)) if has_corr else None
    for k, h in list(zip(("h1", "h2", "h3"), (h1, h2, h3)))[:depth]:
        setattr(a, k, _p(g.inp(k, h)))
    m = g.out("m_out", x.shape)
    xc = g.out("x_corr", x.shape) if has_corr else None
    xp = g.out("x_pred", x.shape) if has_pred else None
    a.m_out, a.x_corr, a.x_pred = _p(m), _p(xc), _p(xp)
    a.numel, a.cfg_scale, a.sigma_s, a.alpha_s = x.numel(), 3.0, 0.929, 0.37
    a.ac, a.c0, a.c1, a.c2, a.c3 = CORR
    a.ap, a.p0, a.p1, a.p2 = PRED
    if pid is None:
        _lib.check(lib.adm_unipc_step(C.byref(a), _stream(), 0), "adm_unipc_step (guarded)")
    else:
        _lib.check(lib.adm_unipc_step_p(C.byref(a), _stream(), pid), "adm_unipc_step_p (guarded)")
    torch.cuda.synchronize()
    g.check()
    return m, xc, xp


@pytest.mark.parametrize("numel,offset", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("param", ["eps", "x0", "v"])
def test_unipc_step_p_every_flag_and_depth(param, numel, offset):
    from autodiffusion_amd import _lib
    lib = _lib.load()
    t = R.latents(numel, 60 + numel, 7)
    x, xb, ou, oc, h1, h2, h3 = t
    worst = 0.0
    for guided, depth, has_corr, has_pred in itertools.product((True, False), range(4), (True, False), (True, False)):
        outs = _uni_launch(lib, _G(offset), t, guided, depth, has_corr, has_pred, R.PARAMS[param])
        refs, bounds = R.unipc_step_restate(x, ou if guided else None, oc, xb, [h1, h2, h3][:depth], cfg=3.0, sigma=0.929, alpha=0.37,
                                            corr=CORR if has_corr else None, pred=PRED if has_pred else None, param=param)
        for what, got, r, b in zip(("m", "x_corr", "x_pred"), outs, refs, bounds):
            assert (got is None) == (r is None)
            if got is not None:
                worst = max(worst, _hold((param, what, guided, depth, has_corr, has_pred), got, r, b))
        if param == "eps":
            old = _uni_launch(lib, _G(offset), t, guided, depth, has_corr, has_pred, None)
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(outs, old))
    print(f"unipc_step_p {param} numel {numel} offset {offset}: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------ adm_gelu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,inner", [(1, 8), (3, 40), (77, 512)])
def test_gelu_every_element(rows, inner, dtype):
    from autodiffusion_amd import _lib, ops
    u = R.gelu_inputs(rows, inner, dtype, rows * 1000 + inner)
    ref, bound = R.gelu_restate(u, dtype)
    g = guarded.Guarded(DEV)
    ud = g.inp("u", u.to(DEV))
    out = g.out("out", u.shape, dtype)
    lib = _lib.load("f16" if dtype == torch.float16 else "bf16")
    _lib.check(lib.adm_gelu(_p(ud), _p(out), rows, inner, _stream(), 0), "adm_gelu (guarded)")
    torch.cuda.synchronize()
    g.check()
    err = (out.cpu().double() - ref).abs()
    r = float((err / bound).max())
    ulps = float((err / (2 * fk.half_ulp_t(ref, dtype))).max())
    print(f"gelu {rows}x{inner} {dtype}: worst err/bound {r:.3f}, worst err {ulps:.3f} ulp_T")
    assert r <= 1.0
    via = ops.gelu(u.to(DEV))
    assert via.dtype == dtype and torch.equal(via, out)
    assert lib.adm_gelu(_p(ud), _p(out), rows, inner, _stream(), 1) == -1


# ------------------------------------------------------------------ the samplers on a v- / x0-predicting toy model
class _Toy:
    """tests/test_hip_sd.py's toy latent model with a parameterisation: the toy network's output read as v or x0."""

    def __init__(self, parameterization):
        from autodiffusion_amd.sd_sampler import LatentDiffusion
        base = LatentDiffusion(None, device=DEV, parameterization=parameterization)
        self.num_timesteps, self.device, self.parameterization = base.num_timesteps, base.device, base.parameterization
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = base.betas, base.alphas_cumprod, base.alphas_cumprod_prev
        self.q_sample = base.q_sample
        self.calls = 0

    def apply_model(self, x, t, c):
        from oracle.sd_sampler import toy_model
        self.calls += 1
        return toy_model(x, t, c)


@pytest.fixture(scope="module")
def case():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = golden("sd_param_dpm")
    return g, tuple(torch.from_numpy(g[k]).to(DEV) for k in ("x_T", "c", "uc"))


@pytest.mark.parametrize("param", ["v", "x0"])
def test_dpm_solver_sampler_matches_the_reference_capture(param, case):
    from autodiffusion_amd.sd_sampler import DPMSolverSampler, UniPCSampler
    g, (x_T, c, uc) = case
    cand = [int(v) for v in g["cand"].tolist()]
    for gtag, (scale, u) in {"cfg": (float(g["scale"]), uc), "plain": (1.0, None)}.items():
        m = _Toy(param)
        kw = dict(S=len(cand) - 1, batch_size=2, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T,
                  unconditional_guidance_scale=scale, unconditional_conditioning=u, sampled_timestep=cand)
        got, _ = DPMSolverSampler(m).sample(**kw)
        assert m.calls == len(cand) - 1
        np.testing.assert_allclose(got.cpu().numpy(), g[f"dpm_{param}_{gtag}"], rtol=1e-4, atol=1e-4, err_msg=f"{param} {gtag}")
        # UniPC of order 2, bh2, without its corrector is the same solver
        got, _ = UniPCSampler(m).sample(order=2, variant="bh2", corrector=False, **kw)
        np.testing.assert_allclose(got.cpu().numpy(), g[f"dpm_{param}_{gtag}"], rtol=1e-4, atol=1e-4, err_msg=f"unipc {param} {gtag}")
    eps = _Toy("eps")
    got, _ = DPMSolverSampler(eps).sample(**kw)     # the same network read as eps is another trajectory
    assert float((got.cpu() - torch.from_numpy(g[f"dpm_{param}_plain"])).abs().max()) > 1e-2


def _record_sd_steps(monkeypatch):
    from autodiffusion_amd import sd_sampler as S
    rec, real = [], S.sd_step

    def sd_step(x, eps, batch, cfg_scale, weights, hist, a_t, a_prev, sigma, noise=None, want_e=True, param="eps"):
        out = real(x, eps, batch, cfg_scale, weights, hist, a_t, a_prev, sigma, noise, True, param)
        rec.append(dict(x=x, eps=eps, batch=batch, cfg=cfg_scale, w=tuple(weights), hist=tuple(hist), a_t=a_t, a_prev=a_prev, sigma=sigma,
                        noise=noise, param=param, out=out))
        return out
    monkeypatch.setattr(S, "sd_step", sd_step)
    return rec


def _cf_of(r):
    """The adm_sd_step_coefs sd_sampler.sd_step builds, restated: float32 roots of the float32 table entries."""
    one = np.float32(1.0)
    a_t, a_prev, sigma = np.float32(r["a_t"]), np.float32(r["a_prev"]), np.float32(r["sigma"])
    w = tuple(fk.f32c(v) for v in r["w"]) + (0.0,) * (4 - len(r["w"]))
    return dict(cfg_scale=fk.f32c(r["cfg"]), w=w, sqrt_one_minus_at=float(np.sqrt(one - a_t)), sqrt_at=float(np.sqrt(a_t)),
                sqrt_a_prev=float(np.sqrt(a_prev)), dir_coef=float(np.sqrt(one - a_prev - sigma * sigma)), sigma=float(sigma))


def _hold_records(rec):
    worst = 0.0
    for j, r in enumerate(rec):
        b = r["batch"]
        eps = r["eps"].cpu()
        ou, oc = (eps[:b], eps[b:]) if eps.shape[0] == 2 * b else (None, eps)
        refs, bounds = R.sd_step_restate(r["x"].cpu(), ou, oc, [h.cpu() for h in r["hist"]], None if r["noise"] is None else r["noise"].cpu(),
                                         _cf_of(r), r["param"])
        for what, got, ref, bd in zip(("x_prev", "pred_x0", "e"), r["out"], refs, bounds):
            worst = max(worst, _hold((j, what, r["param"]), got, ref, bd))
    return worst


def _guided64(model64, x, t, c, uc, scale):
    if uc is None or scale == 1.0:
        return model64(x, t, c)
    ou, oc = model64(x, t, uc), model64(x, t, c)
    return ou + scale * (oc - ou)


def _model64(x, t, c):
    from oracle.sd_sampler import toy_model
    return toy_model(x.double(), torch.full((x.shape[0],), int(t), dtype=torch.long), c.double())


def _ddim64(ac, x, c, uc, scale, steps, eta, noises, param):
    """Stability's ddim.py p_sample_ddim for "v" (the guidance on the raw output; e_t = predict_eps_from_z_and_v, pred_x0 =
    predict_start_from_z_and_v), and ddpm.py's "x0" in the same places, in float64 on the float32 table."""
    from oracle.sd_sampler import sampling_parameters
    sig, a, a_prev = (v.double() for v in sampling_parameters(ac, steps, eta))
    x = x.double()
    for i, step in enumerate(reversed(list(steps))):
        k = len(steps) - i - 1
        o = _guided64(_model64, x, step, c, uc, scale)
        sa, s1 = a[k].sqrt(), (1 - a[k]).sqrt()
        e = R.to_eps(o, x, float(sa), float(s1), param)
        x0 = sa * x - s1 * o if param == "v" else o
        x = a_prev[k].sqrt() * x0 + (1 - a_prev[k] - sig[k] ** 2).sqrt() * e + (sig[k] * noises[i].double() if eta else 0.0)
    return x


def _plms64(ac, x, c, uc, scale, steps, param):
    """Stability's plms.py: every model output becomes eps at the point and time it was evaluated at; then the eps-only PLMS."""
    from oracle.sd_sampler import sampling_parameters
    _, a, a_prev = (v.double() for v in sampling_parameters(ac, steps, 0.0))
    acd = ac.double()
    rng = list(reversed(list(steps)))
    x, old = x.double(), []

    def eps_at(x_, t):
        return R.to_eps(_guided64(_model64, x_, t, c, uc, scale), x_, float(acd[t].sqrt()), float((1 - acd[t]).sqrt()), param)

    def update(x_, e, k):
        x0 = (x_ - (1 - a[k]).sqrt() * e) / a[k].sqrt()
        return a_prev[k].sqrt() * x0 + (1 - a_prev[k]).sqrt() * e
    for i, step in enumerate(rng):
        k = len(steps) - i - 1
        e = eps_at(x, step)
        if len(old) == 0:
            ep = (e + eps_at(update(x, e, k), rng[min(i + 1, len(rng) - 1)])) / 2
        elif len(old) == 1:
            ep = (3 * e - old[-1]) / 2
        elif len(old) == 2:
            ep = (23 * e - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            ep = (55 * e - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        x = update(x, ep, k)
        old = (old + [e])[-3:]
    return x


STEPS = [94, 354, 690, 926]     # 4 ascending timesteps


@pytest.mark.parametrize("param", ["v", "x0"])
def test_ddim_and_plms_update_by_update(param, case, monkeypatch):
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler
    g, (x_T, c, uc) = case
    ac = torch.from_numpy(g["alphas_cumprod"])
    scale = float(g["scale"])
    rec = _record_sd_steps(monkeypatch)
    kw = dict(S=4, batch_size=2, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T, unconditional_guidance_scale=scale,
              unconditional_conditioning=uc, sampled_timestep=np.array(STEPS))
    for eta in (0.0, 1.0):
        del rec[:]
        m = _Toy(param)
        torch.manual_seed(3)
        got, inter = DDIMSampler(m).sample(eta=eta, **kw)
        assert m.calls == 4 and len(rec) == 4 and all(r["param"] == param and r["w"] == (1.0,) and not r["hist"] for r in rec)
        assert rec[0]["x"] is not None and all(rec[j + 1]["x"] is rec[j]["out"][0] for j in range(3)) and got is rec[-1]["out"][0]
        assert all((r["noise"] is not None) == (eta > 0) for r in rec)
        worst = _hold_records(rec)
        want = _ddim64(ac, x_T.cpu(), c.cpu(), uc.cpu(), scale, STEPS, eta, [None if r["noise"] is None else r["noise"].cpu() for r in rec], param)
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5, err_msg=f"ddim {param} eta {eta}")
        assert inter["pred_x0"][-1] is rec[-1]["out"][1]
        print(f"DDIM {param} eta {eta}: per-update worst err/bound {worst:.3f}")
    del rec[:]
    m = _Toy(param)
    got, _ = PLMSSampler(m).sample(eta=0.0, **kw)
    # the first step: the update to the predicted point, the second output's eps at (x_mid, t_next), the eps blend; then one launch each
    assert m.calls == 5 and len(rec) == 6
    assert [r["param"] for r in rec] == [param, param, "eps", param, param, param]
    assert rec[1]["x"] is rec[0]["out"][0] and rec[2]["x"] is rec[0]["x"] and rec[2]["eps"] is rec[1]["out"][2]
    assert rec[2]["hist"][0] is rec[0]["out"][2] and rec[2]["w"] == (0.5, 0.5) and rec[2]["cfg"] == 1.0
    assert fk.f32c(rec[1]["a_t"]) == float(ac[STEPS[-2]])
    assert [len(r["hist"]) for r in rec[3:]] == [1, 2, 3] and rec[5]["hist"][0] is rec[4]["out"][2] and rec[5]["hist"][2] is rec[0]["out"][2]
    worst = _hold_records(rec)
    want = _plms64(ac, x_T.cpu(), c.cpu(), uc.cpu(), scale, STEPS, param)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5, err_msg=f"plms {param}")
    print(f"PLMS {param}: per-update worst err/bound {worst:.3f}")


def test_plms_prompt_mask_steps_pass_the_parameterisation_on(case, monkeypatch):
    from autodiffusion_amd.sd_sampler import PLMSSampler
    g, (x_T, c, uc) = case
    rec = _record_sd_steps(monkeypatch)
    m = _Toy("v")
    got, _ = PLMSSampler(m).sample(S=4, batch_size=2, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T, eta=0.0,
                                   unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=uc,
                                   sampled_timestep=np.array(STEPS), prompt_mask=[1, 0, 1, 0])
    assert torch.isfinite(got).all() and [r["param"] for r in rec] == ["v", "v", "eps", "v", "v", "v"]
    assert [r["eps"].shape[0] for r in rec] == [4, 4, 2, 2, 4, 2] and [r["cfg"] for r in rec][3:] == [1.0, float(g["scale"]), 1.0]
    assert _hold_records(rec) <= 1.0


@pytest.mark.parametrize("param", ["v", "x0"])
def test_unipc_update_by_update(param, case):
    from autodiffusion_amd.sd_sampler import UniPCSampler
    g, (x_T, c, uc) = case
    cand = [int(v) for v in g["cand"].tolist()]
    for scale, u in ((float(g["scale"]), uc), (1.0, None)):
        rec, m = [], _Toy(param)
        got, _ = UniPCSampler(m, order=2, variant="bh2", corrector=True).sample(
            S=4, batch_size=2, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T, unconditional_guidance_scale=scale,
            unconditional_conditioning=u, sampled_timestep=cand, record=rec)
        assert m.calls == 4 == len(rec) and got is rec[-1]["x_pred"] and torch.isfinite(got).all()
        worst = 0.0
        for j, r in enumerate(rec):
            assert (r["corr"] is not None) == (j > 0) and (j == 0 or r["x"] is rec[j - 1]["x_pred"])
            eps = r["eps"].cpu()
            ou, oc = (eps[:2], eps[2:]) if u is not None else (None, eps)
            refs, bounds = R.unipc_step_restate(r["x"].cpu(), ou, oc, None if r["x_base"] is None else r["x_base"].cpu(),
                                                [t.cpu() for t in r["hist"]], cfg=scale, sigma=r["sigma"], alpha=r["alpha"], corr=r["corr"],
                                                pred=r["pred"], param=param)
            for what, got_, ref, bd in zip(("m", "x_corr", "x_pred"), (r["m"], r["x_corr"], r["x_pred"]), refs, bounds):
                assert (got_ is None) == (ref is None)
                if got_ is not None:
                    worst = max(worst, _hold((j, what), got_, ref, bd))
        print(f"UniPC {param} scale {scale}: per-update worst err/bound {worst:.3f}")


def test_stochastic_encode_then_decode_under_v(case, monkeypatch):
    from autodiffusion_amd.sd_sampler import DDIMSampler
    g, (x_T, c, uc) = case
    rec = _record_sd_steps(monkeypatch)
    m = _Toy("v")
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False, sampled_timestep=sorted(STEPS))
    noise = torch.randn(x_T.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    z = s.stochastic_encode(x_T, torch.tensor([3, 3]), noise=noise)
    a3 = np.float32(g["alphas_cumprod"][STEPS[3]])
    want = float(np.sqrt(a3)) * x_T.cpu().double() + float(np.sqrt(np.float32(1.0) - a3)) * noise.cpu().double()
    assert float((z.cpu().double() - want).abs().max()) <= 4 * 2.0 ** -24 * (1 + float(want.abs().max()))   # does not depend on v
    out = s.decode(z, c, 3, unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=uc)
    assert torch.isfinite(out).all() and m.calls == 3 and len(rec) == 3 and all(r["param"] == "v" for r in rec)
    assert rec[0]["x"].data_ptr() == z.data_ptr() or torch.equal(rec[0]["x"], z)
    assert _hold_records(rec) <= 1.0 and out is rec[-1]["out"][0]
