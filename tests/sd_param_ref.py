"""float64 restatements and per-element first-order fp32 bounds of the parameterised latent sampler steps (adm_sd_step_p,
adm_dpm_step_p, adm_unipc_step_p: include/adm_hip.h) and of the exact GELU (adm_gelu).  Nothing here imports the code
under test.  The GPU tests are in tests/test_hip_sd_param.py, the host tests of this module in tests/test_sd_param_host.py.

Restatement: the operation in float64 on the operands exactly as the kernel sees them (fp32 tensors, every scalar as the fp32 value
the kernel is passed), in the operation order the header states.  Bounds as in tests/f32_kernels.py: first order in e = 2^-24, one
e per fp32 operation relative to its result (a contracted multiply-add rounds once instead of twice, so the bound holds whether
or not the compiler contracts), the error an operand carries propagated absolutely, F32_MIN added at the end.

  o        the guided raw output, f32_kernels._guided: o = ou + cfg (oc - ou), E(o) = e (|cfg| |oc - ou| + |cfg (oc - ou)| + |o|);
           oc alone without ou: exact.
  sd_step  V   t1 = sat o; t2 = somat x; e = t1 + t2:        E(e) = sat E(o) + e (|t1| + |t2| + |e|)
           X0  t1 = sat o; t2 = x - t1; e = t2 / somat:      E(e) = (sat E(o) + e |t1| + e |t2|) / somat + e |e|
           then f32_kernels' sd_step chain from (e, E(e)): e', x0 = (x - somat e') / sat, x_prev.
           pred_x0 without history and with w0 == 1 (DDIM):
           V   s1 = sat x; s2 = somat o; x0 = s1 - s2:       E(x0) = somat E(o) + e (|s1| + |s2| + |x0|)
           X0  x0 = o:                                       E(x0) = E(o)
  dpm_step V   t1 = alpha x; t2 = sigma o; m = t1 - t2:      E(m) = sigma E(o) + e (|t1| + |t2| + |m|)
           X0  m = o:                                        E(m) = E(o)
           then f32_kernels' x_next = a x + b0 m (+ b1 m_prev) from (m, E(m)).
  unipc    m as dpm_step's with x = x_eval; then unipc_ref._states from (m, E(m)).
  gelu     ref = 0.5 u (1 + erf(u / sqrt 2)) of T values u, rounded once to T: ulp_T(|ref|) / 2 + SILU_REL (|ref| + 1).  The second
           term is what launch_replay.geglu_restate holds adm_geglu's gate factor to: there ref = v G with the bound's fp32 part
           SILU_REL (|ref| + |v|) = |v| SILU_REL (|G| + 1).
"""
from __future__ import annotations

import math

import torch

import f32_kernels as fk
import unipc_ref as U
from f32_kernels import E24, F32_MIN, f32c

PARAMS = {"eps": 0, "x0": 1, "v": 2}       # ADM_PARAM_* of include/adm_hip.h
SILU_REL = 2.0 ** -20


def _sd_eps(o, eo, x, sat, somat, param, defect=None):
    """(e, E(e)) of the guided raw output under `param`."""
    if param == "eps":
        return o, eo
    if param == "v":
        if defect == "swap":
            sat, somat = somat, sat
        t1, t2 = sat * o, somat * x
        e = t1 + t2
        return e, sat * eo + E24 * (t1.abs() + t2.abs() + e.abs())
    t1 = sat * o
    t2 = x - t1
    e = t2 / somat
    return e, (sat * eo + E24 * t1.abs() + E24 * t2.abs()) / somat + E24 * e.abs()


def sd_step_restate(x, ou, oc, hist, noise, cf: dict, param: str, defect=None):
    """adm_sd_step_p.  hist: the list of given h1..h3 (newest first); cf: f32_kernels.sd_coefs_dict -> ((x_prev, pred_x0, e),
    (bounds)).  defect: "swap" exchanges sqrt_at / sqrt_one_minus_at in the V conversion; "combine_after" converts both halves
    first and combines the eps values with the scale cfg + 1 (a different function: the host test plants both)."""
    sat, somat = cf["sqrt_at"], cf["sqrt_one_minus_at"]
    x64 = x.double()
    if defect == "combine_after" and ou is not None:
        eu_, _ = _sd_eps(ou.double(), torch.zeros_like(x64), x64, sat, somat, param)
        ec_, _ = _sd_eps(oc.double(), torch.zeros_like(x64), x64, sat, somat, param)
        o, eo = None, None
        e, ee = fk._guided(eu_, ec_, cf["cfg_scale"] + 1.0)
    else:
        o, eo = fk._guided(ou, oc, cf["cfg_scale"])
        e, ee = _sd_eps(o, eo, x64, sat, somat, param, defect)
    w = cf["w"]
    ep = w[0] * e
    eep = abs(w[0]) * ee + E24 * ep.abs()
    for i, h in enumerate(hist):
        t = w[i + 1] * h.double()
        ep = ep + t
        eep = eep + E24 * t.abs() + E24 * ep.abs()
    p = somat * ep
    nm = x64 - p
    x0 = nm / sat
    e0 = (somat * eep + E24 * p.abs() + E24 * nm.abs()) / sat + E24 * x0.abs()
    p1, p2 = cf["sqrt_a_prev"] * x0, cf["dir_coef"] * ep
    xp = p1 + p2
    exp_ = cf["sqrt_a_prev"] * e0 + abs(cf["dir_coef"]) * eep + E24 * (p1.abs() + p2.abs() + xp.abs())
    if noise is not None:
        t = cf["sigma"] * noise.double()
        xp = xp + t
        exp_ = exp_ + E24 * t.abs() + E24 * xp.abs()
    if param != "eps" and not hist and w[0] == 1.0 and o is not None:     # DDIM: the direct pred_x0
        if param == "v":
            s1, s2 = sat * x64, somat * o
            x0 = s1 - s2
            e0 = somat * eo + E24 * (s1.abs() + s2.abs() + x0.abs())
        else:
            x0, e0 = o, eo
    return (xp, x0, e), (exp_ + F32_MIN, e0 + F32_MIN, ee + F32_MIN)


def _dpm_m(o, eo, x64, sigma_s, alpha_s, param, defect=None):
    if param == "eps":
        p = sigma_s * o
        nm = x64 - p
        m = nm / alpha_s
        return m, (abs(sigma_s) * eo + E24 * p.abs() + E24 * nm.abs()) / alpha_s + E24 * m.abs()
    if param == "x0":
        return o, eo
    if defect == "swap":
        sigma_s, alpha_s = alpha_s, sigma_s
    t1, t2 = alpha_s * x64, sigma_s * o
    m = t1 - t2
    return m, abs(sigma_s) * eo + E24 * (t1.abs() + t2.abs() + m.abs())


def dpm_step_restate(x, ou, oc, m_prev, cfg: float, sigma_s: float, alpha_s: float, a: float, b0: float, b1: float, param: str,
                     defect=None):
    """adm_dpm_step_p -> ((x_next, m), (bounds))."""
    cfg, sigma_s, alpha_s, a, b0, b1 = (f32c(v) for v in (cfg, sigma_s, alpha_s, a, b0, b1))
    o, eo = fk._guided(ou, oc, cfg)
    x64 = x.double()
    m, em = _dpm_m(o, eo, x64, sigma_s, alpha_s, param, defect)
    p1, p2 = a * x64, b0 * m
    xn = p1 + p2
    en = abs(b0) * em + E24 * (p1.abs() + p2.abs() + xn.abs())
    if m_prev is not None:
        t = b1 * m_prev.double()
        xn = xn + t
        en = en + E24 * t.abs() + E24 * xn.abs()
    return (xn, m), (en + F32_MIN, em + F32_MIN)


def unipc_step_restate(x, ou, oc, xb, hs, *, cfg, sigma, alpha, corr=None, pred=None, param: str, defect=None):
    """adm_unipc_step_p -> ((m, x_corr | None, x_pred | None), (bounds)).  hs: up to three tensors, newest first."""
    cfg, sigma, alpha = f32c(cfg), f32c(sigma), f32c(alpha)
    o, eo = fk._guided(ou, oc, cfg)
    x64 = x.double()
    m, em = _dpm_m(o, eo, x64, sigma, alpha, param, defect)
    hs = tuple(hs) + (None,) * (3 - len(hs))
    (xc, xp), (bc, bp) = U._states(m, em, x64, xb, hs, corr, pred)
    return (m, xc, xp), (em + F32_MIN, bc, bp)


# ------------------------------------------------------------------ the reference solver's composition (float64, no bounds)
def to_eps(o, x, alpha: float, sigma: float, param: str):
    """dpm_solver.py:297-306 noise_pred_fn: eps of a raw output o at x (alpha = sqrt(abar_t), sigma = sqrt(1 - abar_t))."""
    o, x = o.double(), x.double()
    if param == "v":
        return alpha * o + sigma * x
    if param == "x0":
        return (x - alpha * o) / sigma
    return o


# ------------------------------------------------------------------ the exact GELU
def gelu_restate(u, dtype):
    a = u.double()
    ref = 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    return ref, fk.half_ulp_t(ref, dtype) + SILU_REL * (ref.abs() + 1.0)


def gelu_inputs(rows: int, inner: int, dtype, seed: int):
    """T values spanning +-8 with +-0, the smallest subnormals, the smallest normals and +- the largest finite value planted at the
    front of the first row (inner >= 8)."""
    g = torch.Generator().manual_seed(seed)
    u = ((torch.rand(rows, inner, generator=g) * 2 - 1) * 8.0).to(dtype)
    fi = torch.finfo(dtype)
    sub = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    special = torch.tensor([0.0, -0.0, sub, -sub, fi.tiny, -fi.tiny, fi.max, -fi.max], dtype=torch.float64).to(dtype)
    u.view(-1)[:8] = special
    return u


# ------------------------------------------------------------------ case tables of the GPU test
NUMELS = (1, 3, 257, 4 * 257)     # one thread; a ragged scalar tail; two blocks, ragged; the float4 route over two blocks, ragged
SQRT_AT = (0.9991, 0.5, 0.07)


def latents(numel: int, seed: int, count: int):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(numel, generator=g) for _ in range(count)]
