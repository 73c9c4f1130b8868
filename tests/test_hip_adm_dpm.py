"""GPU: the pixel-space DPM-Solver -- adm_abs_quantile and adm_pix_dpm_step against torch.quantile and the float64
restatements of tests/adm_dpm_ref.py, guarded launches and refusals, the tiny guided loops step by step and end to end
against the reference capture (tests/golden/adm_dpm.npz), scheduling, and a tiny search run.

Measured on the MI355X (profiles/dpm_solver/test_hip_adm_dpm.log): quantile at most 1 fp32 ulp from torch.quantile (bound 4); step
worst err / bound 0.989 (a single dominating rounding reaches its half ulp somewhere in 12288 x 18 elements); per-step loop worst
err / bound 0.998 (noise prediction: eps - sigma grad, two roundings); end to end against the reference capture rel-Frobenius
3.3e-3 (order 2), 5.4e-3 (order 2, thresholded), 3.7e-3 (order 1), 4.4e-3 (order 3) with _check's bound 2.5e-2 -- the candidate's
largest index is 900, so the bf16 networks' error is amplified by at most 1 / alpha = 6.4; order 1 against the DDIM loop 8.4e-5.
"""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adm_dpm_ref as R
import guarded
from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 0.995


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ quantile
def _rows(kind, n, per, seed):
    """fp32 [n, per] on the CPU.  n > 3: rows are rolled copies of 3 base rows (same multiset, every element at another thread)."""
    g = torch.Generator().manual_seed(seed)
    nb = min(n, 3)
    if kind == "normal":
        b = torch.randn(nb, per, generator=g) * torch.tensor([1.0, 3.0, 0.05])[:nb, None]
    elif kind == "equal":
        b = torch.full((nb, per), -0.3)
    elif kind == "ties":
        b = (3.0 * torch.randn(nb, per, generator=g)).clamp(-1, 1)
    elif kind == "top24":      # bit patterns that differ in their low 8 bits only
        bits = 0x3F8A5500 + torch.randint(0, 256, (nb, per), generator=g, dtype=torch.int32)
        b = bits.view(torch.float32) * (1 - 2 * torch.randint(0, 2, (nb, per), generator=g)).float()
    else:                      # "special": denormals of both signs, +-0, a few ordinary values, one +inf per row
        bits = torch.randint(1, 1 << 23, (nb, per), generator=g, dtype=torch.int32)
        b = bits.view(torch.float32) * (1 - 2 * torch.randint(0, 2, (nb, per), generator=g)).float()
        sel = torch.rand(nb, per, generator=g)
        b = torch.where(sel < 0.2, torch.zeros(()), b)
        b = torch.where((sel >= 0.2) & (sel < 0.3), -torch.zeros(()), b)
        b = torch.where(sel > 0.9, torch.randn(nb, per, generator=g), b)
        if per >= 201:      # above the two order statistics: it must sort last (on one of them torch's lerp itself gives inf - inf)
            b[:, per // 2] = float("inf")
    if n <= 3:
        return b.contiguous(), None
    return torch.stack([torch.roll(b[i % 3], (i * 7919) % per) for i in range(n)]), b


def _ulps(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("per", [3, 12, 192, 201, 12288, 196608])
def test_quantile_matches_torch_quantile_within_4_ulps_and_is_deterministic(per):
    _need_gpu()
    from autodiffusion_amd import ops
    worst = 0
    for n in (1, 3, 300):
        for kind in ("normal", "equal", "ties", "top24", "special"):
            if n == 300 and per == 196608 and kind not in ("normal", "special"):
                continue     # 236 MB per case: two kinds at the largest shape
            v, base = _rows(kind, n, per, 1000 * n + per % 997)
            want = torch.quantile((v if base is None else base).abs(), Q, dim=1)
            if base is not None:
                want = want[torch.arange(n) % 3]
            vd = v.to(DEV)
            got = ops.abs_quantile(vd, Q)
            again = ops.abs_quantile(vd, Q)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (n, per, kind)
            got = got.cpu()
            assert not torch.isnan(got).any(), (n, per, kind)
            u = _ulps(got, want)
            worst = max(worst, u)
            assert u <= 4, (n, per, kind, u, got[:3], want[:3])
    print(f"quantile per={per}: worst distance from torch.quantile {worst} fp32 ulps")


def test_quantile_other_q_and_exact_order_statistics():
    """q at the ends of (0, 1) and in the middle; where the rank is an integer (per = 201, q = 0.995: fp32 rank 199) the result is
    that order statistic bitwise."""
    _need_gpu()
    from autodiffusion_amd import ops
    g = torch.Generator().manual_seed(4)
    for per in (201, 12288, 20000):
        v = torch.randn(5, per, generator=g)
        for q in (1e-6, 0.25, 0.5, 0.75, Q, 0.999999):
            got = ops.abs_quantile(v.to(DEV), q).cpu()
            assert _ulps(got, torch.quantile(v.abs(), q, dim=1)) <= 4, (per, q)
    v = torch.randn(5, 201, generator=g)
    assert torch.equal(ops.abs_quantile(v.to(DEV), Q).cpu(), v.abs().sort(dim=1).values[:, 199])


# ------------------------------------------------------------------ the fused step
MAPS = [(1, 1), (2, 2), (8, 8), (64, 64)]
FLAG_COMBOS = [f for f in itertools.product((1, 2), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1))]
random.Random(0).shuffle(FLAG_COMBOS)
# (model channels / C, grad, history depth, mode 0 eps / 1 x0 / 2 x0 + thresholding, START_X, x_next NULL, u8)
SHAPES = [(n, c, h, w) for (h, w) in MAPS for c in (3, 4) for n in (1, 3)]


def _step_case(ops, n, c, h, w, flags, seed, max_val=1.0, scale0=None):
    mult, has_grad, depth, mode, start_x, next_null, want_u8 = flags
    g = torch.Generator().manual_seed(seed)
    x, xb, h1, h2 = (torch.randn(n, c, h, w, generator=g) for _ in range(4))
    mo = torch.randn(n, c * mult, h, w, generator=g)
    grad = 0.3 * torch.randn(n, c, h, w, generator=g) if has_grad else None
    if scale0 is not None:
        x[0] *= scale0
        mo[0] *= scale0
    kw = dict(alpha=0.37, sigma=0.929, a=0.81, b0=-0.55, b1=0.23, b2=-0.07, start_x=bool(start_x), predict_x0=mode > 0,
              thresholding=mode == 2, max_val=max_val)
    h1, h2 = (h1 if depth >= 1 else None), (h2 if depth >= 2 else None)
    d = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    m, xn, u8, s = ops.pix_dpm_step(d(x), d(mo), d(grad), None if next_null else d(xb), d(h1), d(h2), alpha_s=kw["alpha"],
                                    sigma_s=kw["sigma"], a=kw["a"], b0=kw["b0"], b1=kw["b1"], b2=kw["b2"], start_x=kw["start_x"],
                                    predict_x0=kw["predict_x0"], thresholding=kw["thresholding"], q=Q, max_val=max_val,
                                    want_next=not next_null, want_u8=bool(want_u8), want_s=True)
    (rx, rm, rs), (bx, bm, bs) = R.step_restate(x, mo, grad, xb, h1, h2, want_next=not next_null, **kw)
    worst = float(((m.cpu().double() - rm).abs() / bm).max())
    assert (xn is None) == bool(next_null) and (s is None) == (mode != 2) and (u8 is None) == (not want_u8)
    if xn is not None:
        worst = max(worst, float(((xn.cpu().double() - rx).abs() / bx).max()))
    if s is not None:
        worst = max(worst, float(((s.cpu().double() - rs).abs() / bs).max()))
    if u8 is not None:
        assert torch.equal(u8, ops.pack_u8_nhwc(m if xn is None else xn))
    return worst, s, rs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_every_element_within_the_restatements_bound(shape):
    """The 288 flag combinations, shuffled once and dealt round-robin over the 16 shapes: 18 per shape, every value of every flag at every shape."""
    _need_gpu()
    from autodiffusion_amd import ops
    n, c, h, w = shape
    k = SHAPES.index(shape)
    mine = FLAG_COMBOS[k::len(SHAPES)]
    for name, col in (("model channels", 0), ("grad", 1), ("history", 2), ("mode", 3), ("START_X", 4), ("x_next NULL", 5), ("u8", 6)):
        assert len({f[col] for f in mine}) == len({f[col] for f in FLAG_COMBOS}), (name, shape)   # every value of every flag here
    worst = 0.0
    for j, flags in enumerate(mine):
        r, _, _ = _step_case(ops, n, c, h, w, flags, 100 * k + j)
        assert r <= 1.0, (shape, flags, r)
        worst = max(worst, r)
    print(f"step {shape}: {len(mine)} flag combinations, worst err / bound {worst:.3f}")


def test_step_mixed_batch_has_both_sides_of_max_val():
    _need_gpu()
    from autodiffusion_amd import ops
    for (c, h, w) in ((3, 64, 64), (4, 64, 64), (3, 8, 8)):      # keys in LDS, keys in the work buffer, a small map
        r, s, rs = _step_case(ops, 3, c, h, w, (2, 1, 2, 2, 0, 0, 1), 77, max_val=4.0, scale0=0.05)
        assert r <= 1.0, (c, h, w, r)
        assert float(s[0]) == 4.0 and rs[0] == 4.0 and (s[1:] > 4.0).all(), s


# ------------------------------------------------------------------ guarded launches and refusals
def _guarded_args(g, n, c, h, w, mult, thr, over=None):
    from autodiffusion_amd import _lib
    gen = torch.Generator().manual_seed(5)
    t = lambda *s: torch.randn(*s, generator=gen).to(DEV)   # noqa: E731
    a = _lib.PixDpmArgs()
    ins = dict(x_eval=t(n, c, h, w), model_out=t(n, c * mult, h, w), grad=0.3 * t(n, c, h, w), x_base=t(n, c, h, w),
               h1=t(n, c, h, w), h2=t(n, c, h, w))
    for k_, v in ins.items():
        ins[k_] = g.inp(k_, v)
        setattr(a, k_, ins[k_].data_ptr())
    outs = dict(m_out=g.out("m_out", (n, c, h, w), guarded.F32), x_next=g.out("x_next", (n, c, h, w), guarded.F32),
                u8_nhwc=g.out("u8_nhwc", (n, h, w, c), torch.uint8, fill=0), s_out=g.out("s_out", (n,), guarded.F32))
    lib = _lib.load()
    need = lib.adm_abs_quantile_work_bytes(n, c * h * w)
    nb = need
    pad = torch.zeros(nb // 4, dtype=torch.bool)
    pad[n:(n * 4 + 15) // 16 * 4] = True
    work = g.out("work", (nb // 4,), guarded.F32, exempt=("include/adm_hip.h: the per-image s is padded to 16 bytes", pad))
    for k_, v in outs.items():
        setattr(a, k_, v.data_ptr())
    a.work, a.work_bytes = work.data_ptr(), nb
    a.n, a.c, a.h, a.w, a.model_channels = n, c, h, w, c * mult
    a.start_x, a.predict_x0, a.thresholding = 0, 1, int(thr)
    a.alpha_s, a.sigma_s, a.a, a.b0, a.b1, a.b2, a.q, a.max_val = 0.37, 0.929, 0.81, -0.55, 0.23, -0.07, Q, 1.0
    for k_, v in (over or {}).items():
        setattr(a, k_, v)
    return a, ins, outs, work, need


@pytest.mark.parametrize("shape", [(3, 3, 8, 8, 2), (2, 4, 64, 64, 1), (3, 3, 64, 64, 2), (2, 3, 5, 7, 1)], ids=str)
def test_guarded_step_and_quantile_write_exactly_their_outputs(shape):
    """Every operand behind canaried margins, the work buffer at exactly its queried size."""
    _need_gpu()
    from autodiffusion_amd import _lib
    n, c, h, w, mult = shape
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for thr in (1, 0):
        g = guarded.Guarded(DEV)
        a, ins, outs, work, need = _guarded_args(_NoU8(g), n, c, h, w, mult, thr)
        u8buf = torch.full((4096 + n * h * w * c + 4096,), 0xF9, dtype=torch.uint8, device=DEV)
        a.u8_nhwc = u8buf[4096:].data_ptr()
        _lib.check(lib.adm_pix_dpm_step(C.byref(a), stream, 0), "adm_pix_dpm_step (guarded)")
        torch.cuda.synchronize()
        if not thr:      # without thresholding neither the work buffer nor s_out is written
            assert torch.isnan(work).all() and torch.isnan(outs["s_out"]).all()
            work.zero_()
            outs["s_out"].zero_()
        g.check()
        assert (u8buf[:4096] == 0xF9).all() and (u8buf[4096 + n * h * w * c:] == 0xF9).all()
        from autodiffusion_amd import ops
        assert torch.equal(u8buf[4096:4096 + n * h * w * c].view(n, h, w, c), ops.pack_u8_nhwc(outs["x_next"].contiguous()))
    # the bare quantile
    g = guarded.Guarded(DEV)
    per = c * h * w
    v = g.inp("v", torch.randn(n, per, generator=torch.Generator().manual_seed(1)).to(DEV))
    need = lib.adm_abs_quantile_work_bytes(n, per)
    pad = torch.zeros(need // 4, dtype=torch.bool)
    pad[n:(n * 4 + 15) // 16 * 4] = True
    pad[:n] = True      # the bare quantile does not use the s slots
    work = g.out("work", (need // 4,), guarded.F32, exempt=("include/adm_hip.h: the s slots belong to adm_pix_dpm_step", pad))
    out = g.out("out", (n,), guarded.F32)
    _lib.check(lib.adm_abs_quantile(v.data_ptr(), n, per, Q, work.data_ptr(), need, out.data_ptr(), stream, 0), "adm_abs_quantile (guarded)")
    torch.cuda.synchronize()
    g.check()
    assert _ulps(out.cpu(), torch.quantile(v.cpu().abs(), Q, dim=1)) <= 4


class _NoU8:
    """Guarded front that leaves the uint8 output to the caller (uint8 holds neither NaN nor the float sentinel)."""

    def __init__(self, g):
        self.g = g

    def inp(self, *a, **k):
        return self.g.inp(*a, **k)

    def out(self, what, shape, dtype, **k):
        if dtype == torch.uint8:
            return torch.empty(shape, dtype=dtype, device=DEV)
        return self.g.out(what, shape, dtype, **k)


def test_refusals_write_nothing():
    _need_gpu()
    from autodiffusion_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n, c, h, w = 2, 4, 64, 64           # per = 16384: the keys go to the work buffer
    need = lib.adm_abs_quantile_work_bytes(n, c * h * w)
    assert need == 16 + 4 * n * c * h * w and lib.adm_abs_quantile_work_bytes(3, 12288) == 16
    assert lib.adm_abs_quantile_work_bytes(0, 5) == -1 and lib.adm_abs_quantile_work_bytes(1 << 31, 1 << 31) == -1
    cases = [dict(x_eval=None), dict(model_out=None), dict(m_out=None), dict(x_base=None), dict(predict_x0=0), dict(q=0.0),
             dict(q=1.0), dict(q=float("nan")), dict(work_bytes=need - 4), dict(work=None), dict(max_val=0.0), dict(n=0),
             dict(model_channels=5), dict(h=1 << 20, w=1 << 20), dict(n=1 << 30, h=1 << 15, w=1 << 15)]
    for over in cases:
        g = guarded.Guarded(DEV)
        a, ins, outs, work, _ = _guarded_args(_NoU8(g), n, c, h, w, 2, 1, over)
        u8 = torch.full((n * h * w * c,), 0xF9, dtype=torch.uint8, device=DEV)
        a.u8_nhwc = u8.data_ptr()
        rc = lib.adm_pix_dpm_step(C.byref(a), stream, 0)
        torch.cuda.synchronize()
        assert rc != 0 and lib.adm_last_error(), over
        guarded.untouched(g)
        assert (u8 == 0xF9).all(), over
    assert lib.adm_pix_dpm_step(None, stream, 0) != 0
    per = c * h * w
    for kind in ("v", "work", "out", "q0", "q1", "small", "n0", "overflow"):
        g = guarded.Guarded(DEV)
        v = g.inp("v", torch.randn(n, per).to(DEV))
        work = g.out("work", (need // 4,), guarded.F32)
        out = g.out("out", (n,), guarded.F32)
        args = dict(v=v.data_ptr(), n=n, per=per, q=Q, work=work.data_ptr(), wb=need, out=out.data_ptr())
        args.update({"v": dict(v=None), "work": dict(work=None), "out": dict(out=None), "q0": dict(q=0.0), "q1": dict(q=1.0),
                     "small": dict(wb=need - 1), "n0": dict(n=0), "overflow": dict(n=1 << 40, per=1 << 40)}[kind])
        rc = lib.adm_abs_quantile(args["v"], args["n"], args["per"], args["q"], args["work"], args["wb"], args["out"], stream, 0)
        torch.cuda.synchronize()
        assert rc != 0 and lib.adm_last_error(), kind
        guarded.untouched(g)


# ------------------------------------------------------------------ the tiny guided loops
@pytest.fixture(scope="module")
def m64():
    _need_gpu()
    from test_hip_sampler import _setup_m64
    return _setup_m64()


CAND = [153, 424, 900, 690, 820]


def _evaluator(m64, **kw):
    from autodiffusion_amd.evaluate import CandidateEvaluator
    model, diffusion, clf = m64
    cand = kw.pop("cand", CAND)
    ev = CandidateEvaluator(model, diffusion, kw.pop("classifier", clf), image_size=64, device=DEV, sampler="dpm_solver", **kw)
    return ev.set_candidate(cand)


def _solve(m64, g, order, thr, lower_order_final=True, record=None, px0=True, cand=CAND):
    from autodiffusion_amd.dpm_solver import DPMSolver
    ev = _evaluator(m64)
    solver = DPMSolver(m64[1], predict_x0=px0, thresholding=thr)
    x_T, y = torch.from_numpy(g["t_x_T"]).to(DEV), torch.from_numpy(g["t_y"]).to(DEV)
    sample = solver.sample_candidate(ev._model_fn, tuple(x_T.shape), noise=x_T, cond_fn=ev._cond_fn, model_kwargs={"y": y},
                                     device=torch.device(DEV), indices=cand, order=order, lower_order_final=lower_order_final,
                                     record=record)
    return sample, solver


@pytest.mark.parametrize("tag,order,lof,thr", [("o2", 2, True, False), ("o2_thr", 2, True, True), ("o1", 1, True, False),
                                               ("o3", 3, False, False)])
def test_guided_loops_match_the_reference_capture(m64, tag, order, lof, thr):
    """_check's criteria of tests/test_hip_sampler.py (rel-Frobenius 2.5e-2, the uint8 level histogram) on the final sample; the
    per-step restatement check below isolates the new kernels at fp32 bounds."""
    from autodiffusion_amd import ops
    from test_hip_sampler import _check
    g = golden("adm_dpm")
    assert g["t_cand"].tolist() == CAND
    sample, solver = _solve(m64, g, order, thr, lof)
    _check(sample, solver.last_uint8_nhwc, g, f"t_{tag}")
    assert torch.equal(solver.last_uint8_nhwc, ops.pack_u8_nhwc(sample))
    if thr:
        assert float(sample.abs().max()) <= 1.0 and (solver.last_s >= 1.0).all()


@pytest.mark.parametrize("order,thr,px0", [(1, False, True), (2, True, True), (3, True, True), (3, False, False), (2, False, False)])
def test_every_update_of_the_loop_is_within_the_restatements_bound(m64, order, thr, px0):
    """The loop records each evaluation's (x, model_out, grad, history, coefficients): every launch against the float64
    restatement on those very inputs.  Order 3 with lower_order_final on 4 updates (orders 1, 2, 2, 1) is the case the reference
    cannot run: its second-order update here takes the two newest model values."""
    from autodiffusion_amd import dpm_solver as D
    g = golden("adm_dpm")
    rec = []
    sample, solver = _solve(m64, g, order, thr, True, rec, px0)
    assert len(rec) == len(CAND)
    idx, ts = D.candidate_times(CAND, 1000, order)
    assert [r["t"] for r in rec] == ts
    orders = R.orders_of(len(CAND) - 1, order, True)
    sc = R.Schedule(np.asarray(m64[1].betas))
    worst, hist = 0.0, []
    c = lambda t: None if t is None else t.cpu()   # noqa: E731
    for j, r in enumerate(rec):
        last = j == len(rec) - 1
        assert r["alpha"] == pytest.approx(sc.alpha(ts[j]), rel=1e-12) and r["sigma"] == pytest.approx(sc.std(ts[j]), rel=1e-12)
        if last:
            kw = dict(want_next=False, predict_x0=True)
            h1 = h2 = None
        else:
            a, b, p = r["coefs"]
            assert p == orders[j]
            h1, h2 = (hist[-1] if p >= 2 else None), (hist[-2] if p >= 3 else None)
            assert (r["h1"] is None) == (h1 is None) and (r["h2"] is None) == (h2 is None)
            assert h1 is None or r["h1"] is h1
            assert h2 is None or r["h2"] is h2
            # the float64 coefficients against the unexpanded update on the recorded history
            kw = dict(a=a, b0=b[0], b1=b[1], b2=b[2], predict_x0=px0)
        (rx, rm, rs), (bx, bm, bs) = R.step_restate(c(r["x"]), c(r["model_out"]), c(r["grad"]), c(r["x"]), c(h1), c(h2),
                                                    alpha=r["alpha"], sigma=r["sigma"], thresholding=thr and (px0 or last), **kw)
        worst = max(worst, float(((r["m"].cpu().double() - rm).abs() / bm).max()))
        if not last:
            worst = max(worst, float(((r["x_next"].cpu().double() - rx).abs() / bx).max()))
            want = R.ref_update(sc, r["x"].cpu().double(), [t.cpu().double() for t in (hist + [r["m"]])[-3:]], ts[max(0, j - 2):j + 1],
                                ts[j + 1], p, px0)
            assert float((rx - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max())), (j, p)   # fp32-cast coefficients, fp32 m
        if thr and (px0 or last):
            worst = max(worst, float(((r["s"].cpu().double() - rs).abs() / bs).max()))
        hist.append(r["m"])
    assert torch.equal(sample, rec[-1]["m"])
    assert worst <= 1.0, worst
    print(f"per-step loop order {order} thr {thr} predict_x0 {px0}: worst err / bound {worst:.3f}")


def test_order_one_loop_is_the_ddim_eta_zero_loop(m64):
    from test_hip_sampler import _check
    g = golden("adm_dpm")
    sample, solver = _solve(m64, g, 1, False)
    ev = _evaluator(m64)
    x_T, y = torch.from_numpy(g["t_x_T"]).to(DEV), torch.from_numpy(g["t_y"]).to(DEV)
    d = ev.active_diffusion
    ref = d.ddim_sample_loop(ev._model_fn, tuple(x_T.shape), noise=x_T, clip_denoised=False, model_kwargs={"y": y},
                             cond_fn=ev._cond_fn, device=torch.device(DEV), eta=0.0)
    fake = {"x_sample": ref.cpu().numpy(), "x_uint8": d.last_uint8_nhwc.cpu().numpy()}

    class G(dict):
        files = list(fake)
    _check(sample, solver.last_uint8_nhwc, G(fake), "x")


def test_batch_independence_in_a_merged_pass(m64):
    """An image's result, its threshold included, is bitwise the same alone and inside a merged sample_batches pass."""
    ev = _evaluator(m64, dpm_thresholding=True, dpm_order=3)
    one = [ev.sample_batch(2, seed=s_).clone() for s_ in (21, 22, 23)]
    merged = ev.sample_batches(2, [21, 22, 23])
    for a, b in zip(one, merged):
        assert torch.equal(a, b)
    ev2 = _evaluator(m64, dpm_thresholding=True, dpm_order=3)
    u8, smp = ev2.sample_batch(2, seed=22, return_float=True)
    assert torch.equal(u8, one[1])


def test_two_stream_overlap_and_graph_replay_are_bit_identical(m64):
    model, diffusion, clf = m64
    outs = []
    for overlap in (True, False, True):
        ev = _evaluator(m64, dpm_thresholding=True)
        ev.base_diffusion.overlap_guidance = overlap
        try:
            outs.append(ev.sample_batch(3, seed=11).clone())
        finally:
            del ev.base_diffusion.overlap_guidance      # back to the class attribute
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    try:
        for graph in (True, True):
            ev = _evaluator(m64, dpm_thresholding=True, use_graph=graph)
            assert torch.equal(ev.sample_batch(3, seed=11), outs[0])
        cand = {"timesteps": [94, 217, 574], "skip_layers": [[1], [], [0, 5]]}
        model.enable_graph(False)
        clf.enable_graph(False)
        want = _evaluator(m64, cand=cand).sample_batch(2, seed=6).clone()
        assert torch.equal(_evaluator(m64, cand=cand, use_graph=True).sample_batch(2, seed=6), want)
    finally:
        model.enable_graph(False)
        clf.enable_graph(False)


def test_candidate_errors_and_plain_candidates_still_run_ddim(m64):
    ev = _evaluator(m64, dpm_order=3, cand=[100, 500, 900])
    with pytest.raises(ValueError):
        ev.sample_batch(1, seed=1)
    from autodiffusion_amd.evaluate import CandidateEvaluator
    model, diffusion, clf = m64
    a = CandidateEvaluator(model, diffusion, clf, image_size=64, use_ddim=True, device=DEV).set_candidate(CAND).sample_batch(2, seed=3)
    b = CandidateEvaluator(model, diffusion, clf, image_size=64, use_ddim=True, device=DEV, sampler=None, dpm_order=3,
                           dpm_thresholding=True).set_candidate(CAND).sample_batch(2, seed=3)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ scripts/search_ea.py --dpm_solver True
def test_search_cli_runs_two_epochs_with_dpm_solver(tmp_path):
    _need_gpu()
    from test_search_cli_multi import FLAGS
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, mu=np.zeros(24), sigma=np.eye(24))
    save = str(tmp_path / "dpm")
    flags = [f for f in FLAGS]
    flags[flags.index("--time_step") + 1] = "4"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "search_ea.py")] + flags + [
        "--save_dir", save, "--ref_path", ref, "--dpm_solver", "True", "--dpm_order", "2", "--dpm_thresholding", "True"]
    env = dict(os.environ, OMP_NUM_THREADS="4", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=700, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(os.path.join(save, "log.txt")).read()
    assert "dpm_solver=True" in log and "epoch = 1 : top" in log
    cands = re.findall(r"^cand: (\[.*?\]), fid: ([-0-9.e+]+)", log, flags=re.M)
    assert len(cands) >= 4 and all(np.isfinite(float(f)) for _, f in cands), log[-2000:]
    assert log.count("sampling complete") == len(cands)
