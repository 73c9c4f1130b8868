"""GPU: UniPC on the latent (Stable-Diffusion) path -- adm_unipc_step against the float64 restatement of tests/unipc_ref.py,
guarded launches and refusals, UniPCSampler update by update on the toy latent model, its DPM-Solver++(2M) special case against
the reference capture (tests/golden/sd_samplers.npz), bitwise scheduling properties on the tiny latent UNet, and the search
command line under --unipc.

Measured on the MI355X (profiles/unipc/test_hip_unipc.log): step worst err / bound 0.927; per-update loops worst 0.911.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import guarded
import unipc_ref as U
from helpers import golden
from test_hip_sd_search import _cli, _cli_flags, _leading_fid  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CORR = (0.81, -0.55, 0.23, -0.07, 0.031)
PRED = (0.64, 0.47, -0.19, 0.052)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ the fused step
# numel 1: the scalar route, one thread; 140 = 4 * 35: the vector route with a ragged last wave; 768: three blocks
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 4, 5, 7), (3, 4, 8, 8)], ids=lambda s: "numel" + str(int(np.prod(s))))
def test_step_every_element_within_the_restatements_bound(shape):
    from autodiffusion_amd.sd_sampler import unipc_step
    n = shape[0]
    worst = 0.0
    d = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    for j, (guided, depth, has_corr, has_pred) in enumerate(itertools.product((1, 0), (0, 1, 2, 3), (1, 0), (1, 0))):
        g = torch.Generator().manual_seed(100 + j)
        x, xb, eu, ec, h1, h2, h3 = (torch.randn(*shape, generator=g) for _ in range(7))
        hs = [h1, h2, h3][:depth]
        corr, pred = (CORR if has_corr else None), (PRED if has_pred else None)
        eps = torch.cat([eu, ec]) if guided else ec
        m, xc, xp = unipc_step(d(x), d(eps), n, 7.5, d(xb) if has_corr else None, [d(t) for t in hs], 0.929, 0.37, corr, pred)
        (rm, rc, rp), (bm, bc, bp) = U.sd_step_restate(x, eu if guided else None, ec, xb, hs, cfg=7.5, sigma=0.929, alpha=0.37,
                                                       corr=corr, pred=pred)
        assert (xc is None) == (not has_corr) and (xp is None) == (not has_pred)
        for got, ref, b in ((m, rm, bm), (xc, rc, bc), (xp, rp, bp)):
            if got is not None:
                r = float(((got.cpu().double() - ref).abs() / b).max())
                assert r <= 1.0, (shape, guided, depth, has_corr, has_pred, r)
                worst = max(worst, r)
    print(f"latent unipc step {shape}: worst err / bound {worst:.3f}")


def _guarded_args(g, shape, over=None):
    from autodiffusion_amd import _lib
    gen = torch.Generator().manual_seed(5)
    t = lambda: torch.randn(*shape, generator=gen).to(DEV)   # noqa: E731
    a = _lib.UnipcArgs()
    for k in ("x_eval", "eps_uncond", "eps_cond", "x_base", "h1", "h2", "h3"):
        setattr(a, k, g.inp(k, t()).data_ptr())
    outs = {k: g.out(k, shape, guarded.F32) for k in ("m_out", "x_corr", "x_pred")}
    for k, v in outs.items():
        setattr(a, k, v.data_ptr())
    a.numel, a.cfg_scale, a.sigma_s, a.alpha_s = int(np.prod(shape)), 7.5, 0.929, 0.37
    a.ac, a.c0, a.c1, a.c2, a.c3 = CORR
    a.ap, a.p0, a.p1, a.p2 = PRED
    for k, v in (over or {}).items():
        setattr(a, k, v)
    return a, outs


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 4, 5, 7), (3, 4, 8, 8), (2, 4, 64, 64)], ids=str)
def test_guarded_step_writes_exactly_the_requested_outputs_and_refusals_write_nothing(shape):
    from autodiffusion_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for want_corr, want_pred in itertools.product((1, 0), (1, 0)):
        g = guarded.Guarded(DEV)
        a, outs = _guarded_args(g, shape)
        if not want_corr:
            a.x_corr = None
        if not want_pred:
            a.x_pred = None
        _lib.check(lib.adm_unipc_step(C.byref(a), stream, 0), "adm_unipc_step (guarded)")
        torch.cuda.synchronize()
        for name, want in (("x_corr", want_corr), ("x_pred", want_pred)):
            if not want:
                assert torch.isnan(outs[name]).all(), name
                outs[name].zero_()
        g.check()
    for over in (dict(x_eval=None), dict(eps_cond=None), dict(m_out=None), dict(x_base=None), dict(numel=0), dict(numel=-1),
                 dict(alpha_s=0.0)):
        g = guarded.Guarded(DEV)
        a, outs = _guarded_args(g, shape, over)
        rc = lib.adm_unipc_step(C.byref(a), stream, 0)
        torch.cuda.synchronize()
        assert rc != 0 and lib.adm_last_error(), over
        guarded.untouched(g)
    g = guarded.Guarded(DEV)
    a, outs = _guarded_args(g, shape)
    assert lib.adm_unipc_step(C.byref(a), stream, 1) != 0 and lib.adm_unipc_step(None, stream, 0) != 0
    torch.cuda.synchronize()
    guarded.untouched(g)


# ------------------------------------------------------------------ the sampler on the toy latent model
def _toy():
    from test_hip_sd import _ToyLatentModel
    return _ToyLatentModel()


def _cands(g):
    for tag in ("i4", "i6", "f4", "i2"):
        cand = g[f"dpmcand_{tag}"].tolist()
        yield tag, ([int(v) for v in cand] if max(cand) > 1 else cand)


def test_order_two_bh2_without_corrector_matches_the_reference_capture_of_dpm_solver():
    from autodiffusion_amd.sd_sampler import UniPCSampler
    g = golden("sd_samplers")
    x_T, c, uc = (torch.from_numpy(g[k]).to(DEV) for k in ("x_T", "c", "uc"))
    m = _toy()
    for tag, cand in _cands(g):
        for gtag, (scale, u) in {"cfg": (7.5, uc), "plain": (1.0, None)}.items():
            m.calls = 0
            got, _ = UniPCSampler(m).sample(S=len(cand) - 1, batch_size=3, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T,
                                            unconditional_guidance_scale=scale, unconditional_conditioning=u, sampled_timestep=cand,
                                            order=2, variant="bh2", corrector=False)
            assert m.calls == len(cand) - 1
            np.testing.assert_allclose(got.cpu().numpy(), g[f"dpm_{tag}_{gtag}"], rtol=1e-4, atol=1e-4, err_msg=f"{tag} {gtag}")


@pytest.mark.parametrize("order", [1, 2, 3])
def test_every_update_of_the_sampler_is_within_the_restatements_bound(order):
    """Per evaluation of the recorded loop: both states inside the kernel restatement's bound on the recorded operands and within
    1e-5 (1 + max|want|) of the unexpanded float64 update on the recorded history; evaluation j + 1 starts from the tensor
    evaluation j wrote; K network calls for K updates."""
    import adm_dpm_ref as R
    from autodiffusion_amd.sd_sampler import UniPCSampler
    g = golden("sd_samplers")
    x_T, c, uc = (torch.from_numpy(g[k]).to(DEV) for k in ("x_T", "c", "uc"))
    m = _toy()
    ac = m.alphas_cumprod.double().cpu().numpy()
    sc = R.Schedule(1.0 - ac / np.concatenate([[1.0], ac[:-1]]))
    c64 = lambda t: t.cpu().double()   # noqa: E731
    cand = dict(_cands(g))["i6"]
    full = np.linspace(1.0, 1.0 / 1000, 1001, dtype=np.float32)[::-1]
    ts = [float(full[v]) for v in cand]
    K = len(ts) - 1
    orders = R.orders_of(K, order, True)
    for variant, corrector, (scale, u) in itertools.product(("bh1", "bh2"), (True, False), ((7.5, uc), (1.0, None))):
        rec = []
        m.calls = 0
        s = UniPCSampler(m, order=order, variant=variant, corrector=corrector)
        got, _ = s.sample(S=K, batch_size=3, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T, unconditional_guidance_scale=scale,
                          unconditional_conditioning=u, sampled_timestep=cand, record=rec)
        assert m.calls == K == len(rec) and [r["t"] for r in rec] == ts[:K] and got is rec[-1]["x_pred"]
        worst, ms, accepted = 0.0, [], []
        for j, r in enumerate(rec):
            assert r["alpha"] == pytest.approx(sc.alpha(ts[j]), rel=1e-6) and r["sigma"] == pytest.approx(sc.std(ts[j]), rel=1e-6)
            if j:
                assert r["x"] is rec[j - 1]["x_pred"]
            assert (r["corr"] is not None) == (corrector and j > 0)
            eps = r["eps"].cpu()
            eu, ec = (eps[:3], eps[3:]) if u is not None else (None, eps)
            (rm, rc, rp), (bm, bc, bp) = U.sd_step_restate(r["x"].cpu(), eu, ec, None if r["x_base"] is None else r["x_base"].cpu(),
                                                           [t.cpu() for t in r["hist"]], cfg=scale, sigma=r["sigma"], alpha=r["alpha"],
                                                           corr=r["corr"], pred=r["pred"])
            for a_, b_ in zip(r["hist"], ms[::-1]):
                assert a_ is b_
            worst = max(worst, float(((c64(r["m"]) - rm).abs() / bm).max()), float(((c64(r["x_pred"]) - rp).abs() / bp).max()))
            mj, mlist, tlist = c64(r["m"]), [c64(t) for t in ms[-3:]], ts[max(0, j - 3):j]
            if r["corr"] is not None:
                assert r["x_base"] is accepted[-1]
                worst = max(worst, float(((c64(r["x_corr"]) - rc).abs() / bc).max()))
                _, want = U.ref_update(sc, c64(accepted[-1]), mlist, tlist, ts[j], orders[j - 1], variant, True, m_t=mj)
                assert float((rc - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max())), (variant, j, "corrector")
            x_c = r["x_corr"] if r["x_corr"] is not None else r["x"]
            want, _ = U.ref_update(sc, c64(x_c), (mlist + [mj])[-3:], (tlist + [ts[j]])[-3:], ts[j + 1], orders[j], variant, True)
            assert float((rp - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max())), (variant, j, "predictor")
            ms.append(r["m"])
            accepted.append(x_c)
        assert worst <= 1.0, (variant, corrector, scale, worst)
        print(f"latent per-update loop order {order} {variant} corrector {corrector} scale {scale}: worst err / bound {worst:.3f}")


def test_sampler_errors_come_before_any_model_call():
    from autodiffusion_amd.sd_sampler import UniPCSampler
    g = golden("sd_samplers")
    x_T, c = (torch.from_numpy(g[k]).to(DEV) for k in ("x_T", "c"))
    m = _toy()
    kw = dict(batch_size=3, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T)
    with pytest.raises(ValueError):
        UniPCSampler(m, order=3).sample(S=2, sampled_timestep=[0.9, 0.5, 0.1], **kw)
    with pytest.raises(ZeroDivisionError):
        UniPCSampler(m).sample(S=3, sampled_timestep=[0.9, 0.5, 0.5, 0.1], **kw)
    with pytest.raises(NotImplementedError):
        UniPCSampler(m).sample(S=2, sampled_timestep=[0.9, 0.5, 0.1], mask=torch.ones(1), **kw)
    assert m.calls == 0


def test_batch_independence_split_streams_graph_replay_and_two_runs_are_bit_identical():
    from autodiffusion_amd.sd_sampler import LatentDiffusion, UniPCSampler
    from test_hip_sd import _model, sd_case
    g, plan, P = sd_case("sd_unet_tiny")
    unet = _model(plan, P)
    ld = LatentDiffusion(unet, device=DEV)
    x_T, ctx = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["context"]).to(DEV)
    uc = ctx.flip(1).contiguous() * 0.5
    cand = [999, 600, 300, 50, 1]

    def run(x, cx, u, split=True):
        s = UniPCSampler(ld, order=3)
        s.split_guidance = split
        out, _ = s.sample(S=4, batch_size=x.shape[0], shape=[4, 16, 16], conditioning=cx, verbose=False, x_T=x,
                          unconditional_guidance_scale=3.0, unconditional_conditioning=u, sampled_timestep=cand)
        torch.cuda.synchronize()
        return out.clone()
    try:
        want = run(x_T, ctx, uc)
        assert torch.isfinite(want).all() and torch.equal(run(x_T, ctx, uc), want)                      # two runs
        for i in range(x_T.shape[0]):                                                                   # an image alone
            assert torch.equal(run(x_T[i:i + 1].contiguous(), ctx[i:i + 1].contiguous(), uc[i:i + 1].contiguous()), want[i:i + 1])
        assert torch.equal(run(x_T, ctx, uc, split=False), want)                                        # one batch of 2N, one stream
        unet.enable_graph(True)
        for split in (True, False, True):                                                               # capture, then replay
            assert torch.equal(run(x_T, ctx, uc, split=split), want)
    finally:
        unet.enable_graph(False)


# ------------------------------------------------------------------ scripts/sd_search_ea.py --unipc
def test_cli_search_runs_two_epochs_under_unipc(_leading_fid, tmp_path, monkeypatch):  # noqa: F811
    from autodiffusion_amd.sd_sampler import UniPCSampler
    from autodiffusion_amd.sd_search import parse_sd_candidate
    seen = []
    sample = UniPCSampler.sample

    def recording(self, *a, **kw):
        seen.append(([float(v) for v in kw["sampled_timestep"]], kw["S"], self.order, self.variant, self.corrector))
        return sample(self, *a, **kw)
    monkeypatch.setattr(UniPCSampler, "sample", recording)
    s = _cli().main(_cli_flags(tmp_path) + ["--time_step", "2", "--unipc", "--unipc_variant", "bh1"])
    assert type(s.sampler) is UniPCSampler and s.dpm_solver
    lines = (tmp_path / "out" / "log.txt").read_text().splitlines()
    assert "unipc=True" in lines[0] and "unipc_variant='bh1'" in lines[0] and "epoch = 1" in lines
    full = set(s.dpm_params["full_timesteps"])
    cands = [parse_sd_candidate(c) for c in s.vis_dict]
    assert len(cands) >= 4 and all(len(c) == 3 and all(isinstance(v, float) and v in full for v in c) for c in cands)
    assert all(np.isfinite(info["fid"]) for info in s.vis_dict.values())
    assert seen[:2 * len(cands)] == [(c, 2, 2, "bh1", True) for c in cands for _ in range(2)]
    fid = _cli().main(_cli_flags(tmp_path) + ["--time_step", "2", "--unipc", "--unipc_variant", "bh1", "--evaluate", str(cands[0])])
    assert fid == s.vis_dict[str(cands[0])]["fid"]
