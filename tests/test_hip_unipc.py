"""GPU: UniPC on the pixel path -- adm_pix_unipc_step against the float64 restatement of tests/unipc_ref.py over the product of its
flags, guarded launches and refusals, the tiny guided loops update by update, the special cases against the reference capture of
DPM-Solver (tests/golden/adm_dpm.npz), bitwise scheduling properties, and a tiny search run.

Measured on the MI355X (profiles/unipc/test_hip_unipc.log): step worst err / bound 0.992 over 384 flag combinations x 4 shapes (a single
dominating rounding reaches its half ulp somewhere in 36864 elements); per-update loops worst 0.946 (order 3, bh1, corrector on).
"""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adm_dpm_ref as R
import guarded
import unipc_ref as U
from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 0.995


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ the fused step
# (2, 3, 4, 4): several images in one block; (1, 3, 5, 7): hw is no multiple of the vector width; (3, 3, 64, 64): 12288 elements,
# the largest image whose selection keys stay in LDS; (1, 3, 65, 64): the work-buffer route
SHAPES = [(2, 3, 4, 4), (1, 3, 5, 7), (3, 3, 64, 64), (1, 3, 65, 64)]
# (START_X, mode 0 eps / 1 x0 / 2 x0 + thresholding, grad, history arrays, corrector, predictor, model channels / C)
FLAG_COMBOS = list(itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1, 2, 3), (0, 1), (0, 1), (1, 2)))
CORR = (0.81, -0.55, 0.23, -0.07, 0.031)
PRED = (0.64, 0.47, -0.19, 0.052)


def _step_case(ops, shape, flags, seed):
    n, c, h, w = shape
    start_x, mode, has_grad, depth, has_corr, has_pred, mult = flags
    g = torch.Generator().manual_seed(seed)
    x, xb, h1, h2, h3 = (torch.randn(n, c, h, w, generator=g) for _ in range(5))
    mo = torch.randn(n, c * mult, h, w, generator=g)
    grad = 0.3 * torch.randn(n, c, h, w, generator=g) if has_grad else None
    hs = [t if i < depth else None for i, t in enumerate((h1, h2, h3))]
    corr, pred = (CORR if has_corr else None), (PRED if has_pred else None)
    kw = dict(start_x=bool(start_x), predict_x0=mode > 0, thresholding=mode == 2, max_val=1.0)
    d = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    m, xc, xp, u8, s = ops.pix_unipc_step(d(x), d(mo), d(grad), d(xb) if has_corr else None, *(d(t) for t in hs), alpha_s=0.37,
                                          sigma_s=0.929, corr=corr, pred=pred, q=Q, want_u8=True, want_s=True, **kw)
    (rm, rc, rp, rs), (bm, bc, bp, bs) = U.pix_step_restate(x, mo, grad, xb, *hs, alpha=0.37, sigma=0.929, corr=corr, pred=pred, **kw)
    assert (xc is None) == (not has_corr) and (xp is None) == (not has_pred) and (s is None) == (mode != 2)
    worst = float(((m.cpu().double() - rm).abs() / bm).max())
    if xc is not None:
        worst = max(worst, float(((xc.cpu().double() - rc).abs() / bc).max()))
    if xp is not None:
        worst = max(worst, float(((xp.cpu().double() - rp).abs() / bp).max()))
    if s is not None:
        worst = max(worst, float(((s.cpu().double() - rs).abs() / bs).max()))
    assert torch.equal(u8, ops.pack_u8_nhwc(xp if xp is not None else (xc if xc is not None else m)))
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_every_element_within_the_restatements_bound(shape):
    """The whole product of the flags (384 combinations) at every shape."""
    _need_gpu()
    from autodiffusion_amd import ops
    worst = 0.0
    for j, flags in enumerate(FLAG_COMBOS):
        r = _step_case(ops, shape, flags, 1000 * SHAPES.index(shape) + j)
        assert r <= 1.0, (shape, flags, r)
        worst = max(worst, r)
    print(f"unipc step {shape}: {len(FLAG_COMBOS)} flag combinations, worst err / bound {worst:.3f}")


# ------------------------------------------------------------------ guarded launches and refusals
def _guarded_args(g, n, c, h, w, mult, thr, over=None):
    from autodiffusion_amd import _lib
    gen = torch.Generator().manual_seed(5)
    t = lambda *s: torch.randn(*s, generator=gen).to(DEV)   # noqa: E731
    a = _lib.PixUnipcArgs()
    ins = dict(x_eval=t(n, c, h, w), model_out=t(n, c * mult, h, w), grad=0.3 * t(n, c, h, w), x_base=t(n, c, h, w),
               h1=t(n, c, h, w), h2=t(n, c, h, w), h3=t(n, c, h, w))
    for k_, v in ins.items():
        ins[k_] = g.inp(k_, v)
        setattr(a, k_, ins[k_].data_ptr())
    outs = dict(m_out=g.out("m_out", (n, c, h, w), guarded.F32), x_corr=g.out("x_corr", (n, c, h, w), guarded.F32),
                x_pred=g.out("x_pred", (n, c, h, w), guarded.F32), s_out=g.out("s_out", (n,), guarded.F32))
    need = _lib.load().adm_abs_quantile_work_bytes(n, c * h * w)
    pad = torch.zeros(need // 4, dtype=torch.bool)
    pad[n:(n * 4 + 15) // 16 * 4] = True
    work = g.out("work", (need // 4,), guarded.F32, exempt=("include/adm_hip.h: the per-image s is padded to 16 bytes", pad))
    for k_, v in outs.items():
        setattr(a, k_, v.data_ptr())
    a.work, a.work_bytes = work.data_ptr(), need
    a.n, a.c, a.h, a.w, a.model_channels = n, c, h, w, c * mult
    a.start_x, a.predict_x0, a.thresholding = 0, 1, int(thr)
    a.alpha_s, a.sigma_s, a.q, a.max_val = 0.37, 0.929, Q, 1.0
    a.ac, a.c0, a.c1, a.c2, a.c3 = CORR
    a.ap, a.p0, a.p1, a.p2 = PRED
    for k_, v in (over or {}).items():
        setattr(a, k_, v)
    return a, ins, outs, work, need


@pytest.mark.parametrize("shape", [(3, 3, 8, 8, 2), (3, 3, 64, 64, 2), (1, 3, 65, 64, 1), (2, 3, 5, 7, 1)], ids=str)
def test_guarded_step_writes_exactly_the_requested_outputs(shape):
    """Every operand behind canaried margins, the work buffer at exactly its queried size; every subset of (x_corr, x_pred, u8)."""
    _need_gpu()
    from autodiffusion_amd import _lib, ops
    n, c, h, w, mult = shape
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for thr, want_corr, want_pred, want_u8 in itertools.product((1, 0), (1, 0), (1, 0), (1, 0)):
        g = guarded.Guarded(DEV)
        a, ins, outs, work, need = _guarded_args(g, n, c, h, w, mult, thr)
        u8buf = torch.full((4096 + n * h * w * c + 4096,), 0xF9, dtype=torch.uint8, device=DEV)
        a.u8_nhwc = u8buf[4096:].data_ptr() if want_u8 else None
        if not want_corr:
            a.x_corr = None
        if not want_pred:
            a.x_pred = None
        _lib.check(lib.adm_pix_unipc_step(C.byref(a), stream, 0), "adm_pix_unipc_step (guarded)")
        torch.cuda.synchronize()
        unwritten = ([] if thr else ["work", "s_out"]) + ([] if want_corr else ["x_corr"]) + ([] if want_pred else ["x_pred"])
        for name in unwritten:      # what was not asked for is still NaN everywhere; then it is cleared for the finite check
            buf = work if name == "work" else outs[name]
            assert torch.isnan(buf).all(), (name, thr, want_corr, want_pred)
            buf.zero_()
        g.check()
        inner = u8buf[4096:4096 + n * h * w * c]
        assert (u8buf[:4096] == 0xF9).all() and (u8buf[4096 + n * h * w * c:] == 0xF9).all()
        if want_u8:
            src = outs["x_pred"] if want_pred else (outs["x_corr"] if want_corr else outs["m_out"])
            assert torch.equal(inner.view(n, h, w, c), ops.pack_u8_nhwc(src.contiguous()))
        else:
            assert (inner == 0xF9).all()


def test_refusals_write_nothing():
    _need_gpu()
    from autodiffusion_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n, c, h, w = 2, 4, 64, 64           # per = 16384: the keys go to the work buffer
    need = lib.adm_abs_quantile_work_bytes(n, c * h * w)
    cases = [dict(x_eval=None), dict(model_out=None), dict(m_out=None), dict(x_base=None), dict(predict_x0=0), dict(q=0.0),
             dict(q=1.0), dict(q=float("nan")), dict(work_bytes=need - 4), dict(work=None), dict(max_val=0.0), dict(n=0),
             dict(model_channels=5), dict(h=1 << 20, w=1 << 20), dict(n=1 << 30, h=1 << 15, w=1 << 15)]
    for over in cases:
        g = guarded.Guarded(DEV)
        a, ins, outs, work, _ = _guarded_args(g, n, c, h, w, 2, 1, over)
        u8 = torch.full((n * h * w * c,), 0xF9, dtype=torch.uint8, device=DEV)
        a.u8_nhwc = u8.data_ptr()
        rc = lib.adm_pix_unipc_step(C.byref(a), stream, 0)
        torch.cuda.synchronize()
        assert rc != 0 and lib.adm_last_error(), over
        guarded.untouched(g)
        assert (u8 == 0xF9).all(), over
    assert lib.adm_pix_unipc_step(None, stream, 0) != 0
    g = guarded.Guarded(DEV)
    a, *_ = _guarded_args(g, n, c, h, w, 2, 1)
    assert lib.adm_pix_unipc_step(C.byref(a), stream, 1) != 0
    torch.cuda.synchronize()
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
    ev = CandidateEvaluator(model, diffusion, kw.pop("classifier", clf), image_size=64, device=DEV, sampler="unipc", **kw)
    return ev.set_candidate(cand)


def _solve(m64, g, order, thr, variant="bh2", corrector=True, record=None, px0=True, cand=CAND, calls=None):
    from autodiffusion_amd.unipc import UniPC
    ev = _evaluator(m64)
    solver = UniPC(m64[1], predict_x0=px0, thresholding=thr, variant=variant, corrector=corrector)
    x_T, y = torch.from_numpy(g["t_x_T"]).to(DEV), torch.from_numpy(g["t_y"]).to(DEV)

    def model_fn(x, t, **kw):
        if calls is not None:
            calls.append(int(t[0]))
        return ev._model_fn(x, t, **kw)
    sample = solver.sample_candidate(model_fn, tuple(x_T.shape), noise=x_T, cond_fn=ev._cond_fn, model_kwargs={"y": y},
                                     device=torch.device(DEV), indices=cand, order=order, record=record)
    return sample, solver


@pytest.mark.parametrize("tag,order,thr", [("o2", 2, False), ("o1", 1, False), ("o2_thr", 2, True)])
def test_special_cases_match_the_reference_capture_of_dpm_solver(m64, tag, order, thr):
    """bh2 without the corrector is DPM-Solver++: the reference's own samples, by _check's criteria of tests/test_hip_sampler.py
    (rel-Frobenius 2.5e-2, the uint8 level histogram)."""
    from autodiffusion_amd import ops
    from test_hip_sampler import _check
    g = golden("adm_dpm")
    assert g["t_cand"].tolist() == CAND
    sample, solver = _solve(m64, g, order, thr, "bh2", False)
    _check(sample, solver.last_uint8_nhwc, g, f"t_{tag}")
    assert torch.equal(solver.last_uint8_nhwc, ops.pack_u8_nhwc(sample))
    if thr:
        assert float(sample.abs().max()) <= 1.0 and (solver.last_s >= 1.0).all()


@pytest.mark.parametrize("order,thr", [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)])
def test_every_update_of_the_loop_is_within_the_restatements_bound(m64, order, thr):
    """The loop records each evaluation's operands and coefficients.  Per evaluation: both states inside the kernel restatement's
    bound on those very inputs, and within 1e-5 (1 + max|want|) of the unexpanded float64 update on the recorded history; the x of
    evaluation j + 1 is the tensor evaluation j wrote; K network calls."""
    from autodiffusion_amd import dpm_solver as D
    g = golden("adm_dpm")
    sc = R.Schedule(np.asarray(m64[1].betas))
    idx, ts = D.candidate_times(CAND, 1000, order)
    orders = R.orders_of(len(CAND) - 1, order, True)
    c = lambda t: None if t is None else t.cpu()   # noqa: E731
    c64 = lambda t: t.cpu().double()   # noqa: E731
    for variant, corrector in itertools.product(("bh1", "bh2"), (True, False)):
        rec, calls = [], []
        sample, solver = _solve(m64, g, order, thr, variant, corrector, rec, calls=calls)
        assert calls == idx and len(rec) == len(CAND) and [r["t"] for r in rec] == ts      # K evaluations, at the candidate's integers
        worst, ms, accepted = 0.0, [], []
        for j, r in enumerate(rec):
            last = j == len(rec) - 1
            assert r["alpha"] == pytest.approx(sc.alpha(ts[j]), rel=1e-12) and r["sigma"] == pytest.approx(sc.std(ts[j]), rel=1e-12)
            if j:
                assert r["x"] is rec[j - 1]["x_pred"]
            assert (r["corr"] is not None) == (corrector and 0 < j and not last) and (r["pred"] is not None) == (not last)
            if r["corr"] is not None:
                assert r["x_base"] is accepted[-1]
            hs = [ms[-1 - i] if i < len(ms) else None for i in range(3)]
            for i, name in enumerate(("h1", "h2", "h3")):
                assert r[name] is None or r[name] is hs[i]
            (rm, rc, rp, rs), (bm, bc, bp, bs) = U.pix_step_restate(
                c(r["x"]), c(r["model_out"]), c(r["grad"]), c(r["x_base"]), c(r["h1"]), c(r["h2"]), c(r["h3"]), alpha=r["alpha"],
                sigma=r["sigma"], corr=r["corr"], pred=r["pred"], thresholding=thr, predict_x0=True)
            worst = max(worst, float(((c64(r["m"]) - rm).abs() / bm).max()))
            if thr:
                worst = max(worst, float(((c64(r["s"]) - rs).abs() / bs).max()))
            m64_, mlist, tlist = c64(r["m"]), [c64(t) for t in ms[-3:]], ts[max(0, j - 3):j]
            if r["corr"] is not None:
                worst = max(worst, float(((c64(r["x_corr"]) - rc).abs() / bc).max()))
                assert r["orders"][0] == orders[j - 1]
                _, want = U.ref_update(sc, c64(accepted[-1]), mlist, tlist, ts[j], orders[j - 1], variant, True, m_t=m64_)
                assert float((rc - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max())), (variant, j, "corrector")
            x_c = r["x_corr"] if r["x_corr"] is not None else r["x"]
            if r["pred"] is not None:
                worst = max(worst, float(((c64(r["x_pred"]) - rp).abs() / bp).max()))
                assert r["orders"][1] == orders[j]
                want, _ = U.ref_update(sc, c64(x_c), (mlist + [m64_])[-3:], (tlist + [ts[j]])[-3:], ts[j + 1], orders[j], variant, True)
                assert float((rp - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max())), (variant, j, "predictor")
            ms.append(r["m"])
            accepted.append(x_c)
        assert torch.equal(sample, rec[-1]["m"]) and rec[-1]["x_corr"] is None      # the arrival: its data prediction, uncorrected
        assert worst <= 1.0, (variant, corrector, worst)
        print(f"per-update loop order {order} thr {thr} {variant} corrector {corrector}: worst err / bound {worst:.3f}")


def test_noise_prediction_loop_is_within_the_restatements_bound(m64):
    g = golden("adm_dpm")
    rec = []
    sample, solver = _solve(m64, g, 2, False, "bh1", True, rec, px0=False)
    c = lambda t: None if t is None else t.cpu()   # noqa: E731
    worst = 0.0
    for j, r in enumerate(rec):
        last = j == len(rec) - 1
        (rm, rc, rp, _), (bm, bc, bp, _) = U.pix_step_restate(
            c(r["x"]), c(r["model_out"]), c(r["grad"]), c(r["x_base"]), c(r["h1"]), c(r["h2"]), c(r["h3"]), alpha=r["alpha"],
            sigma=r["sigma"], corr=r["corr"], pred=r["pred"], predict_x0=last)      # the denoise evaluation is a data prediction
        for got, ref, b in ((r["m"], rm, bm), (r["x_corr"], rc, bc), (r["x_pred"], rp, bp)):
            if got is not None:
                worst = max(worst, float(((got.cpu().double() - ref).abs() / b).max()))
    assert worst <= 1.0 and torch.isfinite(sample).all(), worst


def test_corrector_changes_the_sample_and_errors_surface(m64):
    g = golden("adm_dpm")
    on, _ = _solve(m64, g, 2, False, "bh2", True)
    off, _ = _solve(m64, g, 2, False, "bh2", False)
    assert not torch.equal(on, off) and torch.isfinite(on).all()
    assert float((on - off).norm() / off.norm()) < 0.5
    ev = _evaluator(m64, unipc_order=3, cand=[100, 500, 900])
    with pytest.raises(ValueError):
        ev.sample_batch(1, seed=1)


def test_batch_independence_two_runs_streams_and_graph_replay_are_bit_identical(m64):
    model, diffusion, clf = m64
    kw = dict(unipc_thresholding=True, unipc_order=3)
    ev = _evaluator(m64, **kw)
    one = [ev.sample_batch(2, seed=s_).clone() for s_ in (21, 22, 23)]
    merged = ev.sample_batches(2, [21, 22, 23])
    for a, b in zip(one, merged):
        assert torch.equal(a, b)
    assert torch.equal(_evaluator(m64, **kw).sample_batch(2, seed=22), one[1])      # two runs
    outs = []
    for overlap in (True, False):
        ev = _evaluator(m64, **kw)
        ev.base_diffusion.overlap_guidance = overlap
        try:
            outs.append(ev.sample_batch(2, seed=22).clone())
        finally:
            del ev.base_diffusion.overlap_guidance      # back to the class attribute
    assert torch.equal(outs[0], one[1]) and torch.equal(outs[1], one[1])
    try:
        for _ in range(2):      # capture, then replay
            assert torch.equal(_evaluator(m64, use_graph=True, **kw).sample_batch(2, seed=22), one[1])
    finally:
        model.enable_graph(False)
        clf.enable_graph(False)


# ------------------------------------------------------------------ scripts/search_ea.py --unipc True
def test_search_cli_runs_two_epochs_with_unipc(tmp_path):
    _need_gpu()
    from test_search_cli_multi import FLAGS
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, mu=np.zeros(24), sigma=np.eye(24))
    save = str(tmp_path / "unipc")
    flags = [f for f in FLAGS]
    flags[flags.index("--time_step") + 1] = "4"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "search_ea.py")] + flags + [
        "--save_dir", save, "--ref_path", ref, "--unipc", "True", "--unipc_order", "2", "--unipc_thresholding", "True"]
    env = dict(os.environ, OMP_NUM_THREADS="4", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=700, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(os.path.join(save, "log.txt")).read()
    assert "unipc=True" in log and "'sampler': 'unipc'" in log and "epoch = 1 : top" in log
    cands = re.findall(r"^cand: (\[.*?\]), fid: ([-0-9.e+]+)", log, flags=re.M)
    assert len(cands) >= 4 and all(np.isfinite(float(f)) for _, f in cands), log[-2000:]
    assert log.count("sampling complete") == len(cands)
