"""float64 restatements and per-element error bounds of the fp32 launches behind the KL-f8 posterior and the image-to-image
noising, in the convention of tests/f32_kernels.py: adm_vec_act modes 3 / 4 (``ops.vec_act(x, "gauss_std" | "gauss_logvar")``) and
the eps-free use of adm_sd_step (``sd_sampler.axpby_noise``).  The GPU tests are in tests/test_hip_sd_vae_encode.py, the host tests
of this module in tests/test_sd_vae_encode_host.py.

Restatement: the operation in float64 on the operands exactly as the kernel sees them -- fp32 tensors, and every scalar as the
fp32 value the kernel is passed (the adm_sd_step_coefs fields).

Bounds, first order in e = 2^-24 (one fp32 add or multiply, relative to its result); SILU_REL = 2^-20 stands for one library expf;
F32_MIN is added where a result may leave fp32's normal range.

  gauss_logvar  clamp(x, -30, 20): two comparisons, no arithmetic: bitwise (a NaN stays a NaN; -0 stays -0).
  gauss_std     lv = clamp(x, -30, 20) (exact); h = 0.5 lv (a power of two: exact above fp32's subnormals, and below them
                exp(h) = 1 to within e); sd = expf(h): SILU_REL |sd|.  The clamp keeps sd inside [exp(-15), exp(10)], far from
                fp32's limits.  With dy: out = dy sd, one multiply more: (SILU_REL + e) |dy sd| + F32_MIN.
  axpby_noise   adm_sd_step with eu = h1..h3 = NULL, ec = noise = n, w0 = 1, somat = 0, sat = 1, dir = 0, sap = a, sigma = b:
                e' = 1 n = n and x0 = (x - 0 n) / 1 = x are exact for a finite n (0 n = +-0); x_prev = (a x0 + 0 e') + b n: the
                two products round once each and the sum once, the middle add of +-0 is exact (a contracted multiply-add rounds
                less): |got - ref| <= e (|a x| + |b n| + |a x + b n|) + F32_MIN, ref = a x + b n in float64 on the fp32 a, b.
  posterior     z = s mean + s (noise sd): t = noise sd as gauss_std with dy: E(t) = (SILU_REL + e) |t|; then axpby_noise(mean, s,
  sample        t, s): |got - ref| <= |s| E(t) + e (|s mean| + |s t| + |ref|) + F32_MIN, ref = s (mean + sd noise) in float64.
"""
from __future__ import annotations

import torch

from f32_kernels import E24, F32_MIN, SILU_REL, f32c

LOGVAR_MIN, LOGVAR_MAX = -30.0, 20.0


def gauss_logvar_restate(x):
    """fp32 x -> the clamped log-variance, an fp32 tensor to compare bitwise."""
    return torch.clamp(x, LOGVAR_MIN, LOGVAR_MAX)


def gauss_std_restate(x, dy=None):
    """fp32 x (and dy) -> (ref, bound) float64: exp(0.5 clamp(x, -30, 20)) (times dy)."""
    sd = torch.exp(0.5 * torch.clamp(x.double(), LOGVAR_MIN, LOGVAR_MAX))
    if dy is None:
        return sd, SILU_REL * sd
    ref = dy.double() * sd
    return ref, (SILU_REL + E24) * ref.abs() + F32_MIN


def axpby_noise_restate(x, a: float, noise, b: float):
    """fp32 x, noise; a, b as given to sd_sampler.axpby_noise -> (ref, bound) float64 of a x + b noise."""
    ax, bn = f32c(a) * x.double(), f32c(b) * noise.double()
    ref = ax + bn
    return ref, E24 * (ax.abs() + bn.abs() + ref.abs()) + F32_MIN


def posterior_sample_restate(mean, raw_logvar, noise, scale: float = 1.0):
    """The posterior's sample from the kernel's own moments: (ref, bound) float64 of scale (mean + exp(0.5 clamp(logvar)) noise)."""
    s = f32c(scale)
    t, et = gauss_std_restate(raw_logvar, noise)
    sm, st = s * mean.double(), s * t
    ref = sm + st
    return ref, abs(s) * et + E24 * (sm.abs() + st.abs() + ref.abs()) + F32_MIN


# inputs every gauss_std / gauss_logvar check includes: both clamp edges from both sides, far outside, the zeros
GAUSS_SPECIALS = (-40.0, -30.0, 20.0, 25.0, 0.0, -0.0, -30.000002, 19.999998, 1e-40, 88.0, -104.0)
