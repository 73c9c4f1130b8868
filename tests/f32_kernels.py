"""float64 restatements and per-element error bounds of the fp32 kernels outside the 16-bit torso: the embedding path
(adm_linear_f32, adm_timestep_embedding), the sampler steps (adm_ddim_step, adm_ddpm_step, adm_sd_step, adm_dpm_step), the
uint8 pack and the direct stem conv.  tests/launch_replay.py imports the first two for its record kinds; the GPU tests are in
tests/test_hip_f32_kernels.py and tests/test_hip_launch_replay.py, the host tests of this module in tests/test_f32_kernels_host.py.

Restatement: the operation in float64 on the operands exactly as the kernel sees them -- fp32 tensors, and every scalar as the
fp32 value the kernel is passed (the adm_step_coefs / adm_sd_step_coefs fields, the float arguments).

Bounds, first order in e = 2^-24 (one fp32 add, multiply, division or sqrtf, relative to its result; a sum's rounding is
counted at the magnitude of the sum, a cancelling difference's operand errors are carried absolutely).  SILU_REL = 2^-20 stands
for one library expf / logf / cosf / sinf or one adm_silu; F32_MIN is added where a result may leave fp32's normal range.

  linear     s_k = silu_in ? adm_silu(x_k) : x_k;  ref = Σ_k w_k s_k + bias + table[idx]:
               |got - ref| <= g(k + 2) Σ_k |w_k s_k| + Σ_k |w_k| E_s(x_k) + e (c_b |bias| + |table|),   g(m) = m e / (1 - m e)
             E_s(x) = SILU_REL (1 + |x|) |s| is launch_replay.silu_terms without the affine in front.  A product and the adds
             that follow it are at most k roundings in each of the three kernels: the tile kernel adds sequentially; the matrix
             pipe adds four products per instruction, k / 4 instructions in sequence; the GEMV kernel chains 4 ceil(k / 256)
             multiply-adds in a lane and adds the lanes in ceil(log2(min(64, k / 4))) butterfly steps that are not exact, and
             4 ceil(k / 256) + log2(k / 4) <= k from k = 4 on.  The two epilogue adds round at |acc + bias| and |acc + bias +
             table|: the + 2 on the products, once on the table, and c_b = 2 on the bias when a table follows it (the bias
             passes through both adds), c_b = 1 otherwise.
  timestep   nn.py:103-121 on the fp32 t: z_k = -log(P) k / half, freq = exp(z), a = t freq, out = cos a | sin a | 0.
             The kernel's z is -logf(P) (host: SILU_REL), times (float)k (exact below 2^24), one multiply, one division:
             rel(z) = 2 e + SILU_REL -- two fp32 operations, not three: the negation and the conversions of k and half are exact.
             rel(freq) = |z| rel(z) + SILU_REL (expf); rel(a) = rel(freq) + e; |out - ref| <= |a| rel(a) + SILU_REL (cosf / sinf
             are 1-Lipschitz).  Columns >= 2 (dim / 2) are +0 bitwise.
  ddim/ddpm  gaussian_diffusion.py:258-326 (p_mean_variance), :365-393 (condition_mean / condition_score), :430-439 (p_sample),
             :565-584 (ddim_sample), in float64 on the fp32 adm_step_coefs.  The kernel compiles with fp contract(off): every
             operation below rounds once.  E(v) is the absolute error carried by v.
             host scalars (fp32): somac = sqrtf(1 - ac): 2 e; sap = sqrtf(ac_prev): e; sigma = eta sqrtf((1 - ap) / (1 - ac))
               sqrtf(1 - ac / ap): the first root 2.5 e (two subtractions and a division under it, halved, and its own), the
               second 0.5 (e q / (1 - q) + e) + e with q = ac / ap (the subtraction cancels), two multiplies: rel(sigma) =
               (6 + 0.5 q / (1 - q)) e.  d = (1 - ap) - sigma^2 cancels: E(d) = e (1 - ap) + (2 rel(sigma) + e) sigma^2 + e d,
               and dir = sqrtf(d) carries E(d) / (sqrt(d) + sqrt(max(d - E(d), 0))) + e dir.
             x0 = A x - Bm eps: E = e (|A x| + |Bm eps| + |x0|); predict_xstart: 0.  The clamp is 1-Lipschitz.
             condition_score: e1 = (A x - x0) / Bm: E = (e |A x| + E(x0) + e |A x - x0|) / Bm + e |e1|; e2 = e1 - somac g:
               E(e1) + 3 e |somac g| + e |e2|; x0' = A x - Bm e2: e |A x| + Bm E(e2) + e |Bm e2| + e |x0'|.
             eps = (A x - x0) / Bm as e1.  sample = x0 sap + dir eps (+ sigma noise): sap E(x0) + 2 e |x0 sap| + |dir| E(eps) +
               E(dir) |eps| + e |dir eps| + e |sum| (+ (rel(sigma) + e) |sigma noise| + e |sample|).
             ddpm: frac = (v + 1) / 2: e |frac|; logvar = frac hi + (1 - frac) lo: |hi| E(frac) + e |frac hi| + |lo| (E(frac) +
               e |1 - frac|) + e |(1 - frac) lo| + e |logvar|; var = expf(logvar): relative E(logvar) + SILU_REL; fixed
               variance: both are the struct's values, exact.  mean = c1 x0 + c2 x: |c1| E(x0) + e (|c1 x0| + |c2 x| + |mean|);
               + var g: (rel(var) + e) |var g| + e |mean'|; + expf(0.5 logvar) noise: (0.5 E(logvar) + SILU_REL + e) |sd noise| +
               e |sample|.
  pack       trunc(clamp((x + 1) 127.5, 0, 255)): two IEEE fp32 operations and a truncation, restated in numpy fp32: bitwise.
  sd_step    include/adm_hip.h: e = eu + cfg (ec - eu) (ec alone without eu: exact); e' = w0 e + Σ_i w_i h_i;
             x0 = (x - somat e') / sat; x_prev = sap x0 + dir e' (+ sigma noise).  One e per operation (a contracted
             multiply-add rounds less): E(e) = |cfg| e |ec - eu| + e |cfg (ec - eu)| + e |e|; E(e') = |w0| E(e) + e |w0 e| +
             Σ_i e (|w_i h_i| + |partial sum_i|); E(x0) = (somat E(e') + e |somat e'| + e |x - somat e'|) / sat + e |x0|; E(x_prev) = sap E(x0) +
             |dir| E(e') + e (|sap x0| + |dir e'| + |sum|) (+ e |sigma noise| + e |x_prev|).  The division by sat carries the
             cancellation of x - somat e' at 1 / sat: at sat = 0.07 that is 14 times the operands' rounding.
  dpm_step   e as above; m = (x - sigma_s e) / alpha_s: E(m) = (sigma_s E(e) + e |sigma_s e| + e |x - sigma_s e|) / alpha_s + e |m|;
             x_next = a x + b0 m (+ b1 m_prev): |b0| E(m) + e (|a x| + |b0 m| + |sum|) (+ e |b1 m_prev| + e |x_next|).
  stem       conv3x3 pad 1 of the fp32 image, rounded once to T: ulp_T(|ref|) / 2 + (9 cin + 1) e (Σ |w v| + |bias|): the
             accumulator starts at the bias and takes 9 cin multiply-adds.
"""
from __future__ import annotations

import math

import numpy as np
import torch

SILU_REL = 2.0 ** -20   # one library expf / logf / cosf / sinf or one adm_silu: a few fp32 ulps
F32_MIN = 2.0 ** -126
E24 = 2.0 ** -24
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def f32c(x: float) -> float:
    """The fp32 value a C `float` argument receives."""
    return float(torch.tensor(x, dtype=torch.float32))


def half_ulp_t(v: torch.Tensor, dtype) -> torch.Tensor:
    """Half a unit in the last place of T at |v| (float64); fp16's subnormal spacing 2^-24 below 2^-14."""
    v = v.abs().double()
    _, e = torch.frexp(v)
    ul = torch.ldexp(torch.full_like(v, 2.0 * U[dtype]), (e - 1).to(torch.int32))
    floor = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    return 0.5 * torch.where(v == 0, torch.full_like(v, floor), ul.clamp_min(floor))


# ------------------------------------------------------------------ embedding path
def silu_err(x):
    """float64 s = SiLU(x) and the error of the kernels' adm_silu(x): launch_replay.silu_terms without the affine."""
    z = x.double()
    s = z * torch.sigmoid(z)
    return s, SILU_REL * (1 + z.abs()) * s.abs()


def gamma(m: int) -> float:
    return m * E24 / (1 - m * E24)


def linear_path(k: int, aligned: bool = True) -> str:
    """Which of adm_linear_f32's kernels runs (csrc/adm_embed.hip): chosen by k and the operands' alignment alone."""
    if aligned and k % 16 == 0:
        return "mfma"
    if aligned and k % 4 == 0 and 16 * k * 4 <= 128 * 1024:
        return "gemv"
    return "tile"


def linear_restate(x, w, bias, table, idx, silu_in: bool):
    """x [n, k], w [o, k], bias [o] | None, table [rows, o] and idx [n] | None -> (ref, bound) [n, o]."""
    k = x.shape[1]
    if silu_in:
        s, es = silu_err(x)
    else:
        s, es = x.double(), None
    wd = w.double()
    ref = s @ wd.T
    bound = gamma(k + 2) * (s.abs() @ wd.abs().T)
    if es is not None:
        bound = bound + es @ wd.abs().T
    if bias is not None:
        ref = ref + bias.double()
        bound = bound + (2 if table is not None else 1) * E24 * bias.double().abs()
    if table is not None:
        tr = table.double()[idx]
        ref = ref + tr
        bound = bound + E24 * tr.abs()
    return ref, bound + F32_MIN


def timestep_restate(t, dim: int, max_period: float):
    """t fp32 [n] -> (ref, bound) [n, dim]; the columns >= 2 (dim // 2) are zero with a zero bound (compared bitwise)."""
    half = dim // 2
    n = t.shape[0]
    lp = math.log(f32c(max_period))
    z = -lp * torch.arange(half, dtype=torch.float64, device=t.device) / half
    rel_f = z.abs() * (2 * E24 + SILU_REL) + SILU_REL
    a = t.double()[:, None] * torch.exp(z)[None]
    ea = a.abs() * (rel_f + E24)[None] + SILU_REL
    ref = torch.zeros((n, dim), dtype=torch.float64, device=t.device)
    bound = torch.zeros_like(ref)
    ref[:, :half], ref[:, half:2 * half] = torch.cos(a), torch.sin(a)
    bound[:, :half], bound[:, half:2 * half] = ea, ea
    return ref, bound


# ------------------------------------------------------------------ sampler steps
STEP_FIELDS = ("sqrt_recip_ac", "sqrt_recipm1_ac", "ac", "ac_prev", "coef1", "coef2", "log_var_lo", "log_var_hi", "fixed_var",
               "eta", "nonzero", "learned_range", "predict_xstart", "clip_denoised")


def coefs_dict(c) -> dict:
    """The fields of an adm_step_coefs (ctypes: already fp32) as Python numbers."""
    return {f: getattr(c, f) for f in STEP_FIELDS}


def ddim_scalars(cf: dict) -> dict:
    """float64 values of the scalars launch_step derives in fp32, and the absolute error each carries."""
    ac, ap, eta = cf["ac"], cf["ac_prev"], cf["eta"]
    somac = math.sqrt(1 - ac)
    sap = math.sqrt(ap)
    u, q = 1 - ap, ac / ap
    sigma = eta * math.sqrt(u / (1 - ac)) * math.sqrt(1 - q)
    rel_sigma = (6 + 0.5 * q / (1 - q)) * E24 if sigma != 0 else 0.0
    d = u - sigma * sigma
    e_d = E24 * u + (2 * rel_sigma + E24) * sigma * sigma + E24 * abs(d)
    dirc = math.sqrt(max(d, 0.0))
    den = dirc + math.sqrt(max(d - e_d, 0.0))
    e_dir = (e_d / den if den > 0 else math.sqrt(e_d)) + E24 * dirc
    return {"somac": somac, "rel_somac": 2 * E24, "sap": sap, "rel_sap": E24, "sigma": sigma, "rel_sigma": rel_sigma,
            "dir": dirc, "e_dir": e_dir}


def _x0(x, eps, cf):
    """pred_xstart of p_mean_variance and its error."""
    if cf["predict_xstart"]:
        x0, e0 = eps, torch.zeros_like(eps)
    else:
        ax, be = cf["sqrt_recip_ac"] * x, cf["sqrt_recipm1_ac"] * eps
        x0 = ax - be
        e0 = E24 * (ax.abs() + be.abs() + x0.abs())
    if cf["clip_denoised"]:
        x0 = x0.clamp(-1.0, 1.0)
    return x0, e0


def _eps_of(x, x0, e0, cf):
    ax = cf["sqrt_recip_ac"] * x
    bm = cf["sqrt_recipm1_ac"]
    nm = ax - x0
    eps = nm / bm
    return eps, (E24 * ax.abs() + e0 + E24 * nm.abs()) / bm + E24 * eps.abs()


def ddim_restate(x, mo, grad, noise, cf: dict):
    """x [n, c, h, w], mo [n, c | 2c, h, w], grad / noise | None -> ((x_prev, pred_xstart), (bound, bound))."""
    c = x.shape[1]
    k = ddim_scalars(cf)
    x, eps = x.double(), mo[:, :c].double()
    x0, e0 = _x0(x, eps, cf)
    if grad is not None:
        e1, ee1 = _eps_of(x, x0, e0, cf)
        p = k["somac"] * grad.double()
        e2 = e1 - p
        ee2 = ee1 + (k["rel_somac"] + E24) * p.abs() + E24 * e2.abs()
        ax, m = cf["sqrt_recip_ac"] * x, cf["sqrt_recipm1_ac"] * e2
        x0 = ax - m
        e0 = E24 * ax.abs() + cf["sqrt_recipm1_ac"] * ee2 + E24 * m.abs() + E24 * x0.abs()
    eps, ee = _eps_of(x, x0, e0, cf)
    p1, p2 = x0 * k["sap"], k["dir"] * eps
    s = p1 + p2
    es = k["sap"] * e0 + (k["rel_sap"] + E24) * p1.abs() + k["dir"] * ee + k["e_dir"] * eps.abs() + E24 * p2.abs() + E24 * s.abs()
    if cf["nonzero"] and k["sigma"] != 0:
        p3 = k["sigma"] * noise.double()
        s = s + p3
        es = es + (k["rel_sigma"] + E24) * p3.abs() + E24 * s.abs()
    return (s, x0), (es + F32_MIN, e0 + F32_MIN)


def ddpm_restate(x, mo, grad, noise, cf: dict):
    """As ddim_restate for adm_ddpm_step; the variance half mo[:, c:2c] is read when cf['learned_range']."""
    c = x.shape[1]
    x, eps = x.double(), mo[:, :c].double()
    x0, e0 = _x0(x, eps, cf)
    if cf["learned_range"]:
        lo, hi = cf["log_var_lo"], cf["log_var_hi"]
        frac = (mo[:, c:2 * c].double() + 1) / 2
        ef = E24 * frac.abs()
        om = 1 - frac
        p1, p2 = frac * hi, om * lo
        logvar = p1 + p2
        el = abs(hi) * ef + E24 * p1.abs() + abs(lo) * (ef + E24 * om.abs()) + E24 * p2.abs() + E24 * logvar.abs()
        var = torch.exp(logvar)
    else:
        logvar, el = torch.full_like(x, cf["log_var_lo"]), torch.zeros_like(x)
        var = torch.full_like(x, cf["fixed_var"])
    rel_var = (el + SILU_REL) if cf["learned_range"] else torch.zeros_like(x)
    p1, p2 = cf["coef1"] * x0, cf["coef2"] * x
    s = p1 + p2
    es = abs(cf["coef1"]) * e0 + E24 * (p1.abs() + p2.abs() + s.abs())
    if grad is not None:
        qv = var * grad.double()
        s = s + qv
        es = es + (rel_var + E24) * qv.abs() + E24 * s.abs()
    if cf["nonzero"]:
        t = torch.exp(0.5 * logvar) * noise.double()
        s = s + t
        es = es + (0.5 * el + SILU_REL + E24) * t.abs() + E24 * s.abs()
    return (s, x0), (es + F32_MIN, e0 + F32_MIN)


def pack_u8_restate(x):
    """fp32 NCHW (any device) -> uint8 NHWC numpy: trunc(clamp((x + 1) * 127.5, 0, 255)) in IEEE fp32."""
    v = x.detach().cpu().numpy().astype(np.float32, copy=False)
    with np.errstate(over="ignore"):
        q = (v + np.float32(1.0)) * np.float32(127.5)
    q = np.minimum(np.maximum(q, np.float32(0.0)), np.float32(255.0))
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))


def pack_seeds() -> list:
    """The values every pack tensor is seeded with: the ends of the range, -0, the fp32 extremes, the neighbours of +-1, and for
    k in (1, 2, 127, 128, 254, 255) the fp32 value nearest k / 127.5 - 1 with its two fp32 neighbours."""
    vals = [-1.0, 1.0, -0.0, 3e38, -3e38, 1.0000001, -1.0000001]
    for k in (1, 2, 127, 128, 254, 255):
        v = np.float32(k / 127.5 - 1.0)
        vals += [float(np.nextafter(v, np.float32(-2.0))), float(v), float(np.nextafter(v, np.float32(2.0)))]
    return vals


SD_FIELDS = ("cfg_scale", "sqrt_one_minus_at", "sqrt_at", "sqrt_a_prev", "dir_coef", "sigma")


def sd_coefs_dict(c) -> dict:
    d = {f: getattr(c, f) for f in SD_FIELDS}
    d["w"] = tuple(c.w[i] for i in range(4))
    return d


def _guided(eu, ec, cfg: float):
    """e = eu + cfg (ec - eu), or ec without eu, and its error."""
    ec = ec.double()
    if eu is None:
        return ec, torch.zeros_like(ec)
    u = eu.double()
    d = ec - u
    p = cfg * d
    e = u + p
    return e, abs(cfg) * E24 * d.abs() + E24 * p.abs() + E24 * e.abs()


def sd_step_restate(x, eu, ec, hist, noise, cf: dict):
    """hist: the list of given h1..h3 (newest first) -> ((x_prev, pred_x0, e), (bounds))."""
    e, ee = _guided(eu, ec, cf["cfg_scale"])
    w = cf["w"]
    ep = w[0] * e
    eep = abs(w[0]) * ee + E24 * ep.abs()
    for i, h in enumerate(hist):
        t = w[i + 1] * h.double()
        ep = ep + t
        eep = eep + E24 * t.abs() + E24 * ep.abs()
    x = x.double()
    p = cf["sqrt_one_minus_at"] * ep
    nm = x - p
    x0 = nm / cf["sqrt_at"]
    e0 = (cf["sqrt_one_minus_at"] * eep + E24 * p.abs() + E24 * nm.abs()) / cf["sqrt_at"] + E24 * x0.abs()
    p1, p2 = cf["sqrt_a_prev"] * x0, cf["dir_coef"] * ep
    xp = p1 + p2
    exp_ = cf["sqrt_a_prev"] * e0 + abs(cf["dir_coef"]) * eep + E24 * (p1.abs() + p2.abs() + xp.abs())
    if noise is not None:
        t = cf["sigma"] * noise.double()
        xp = xp + t
        exp_ = exp_ + E24 * t.abs() + E24 * xp.abs()
    return (xp, x0, e), (exp_ + F32_MIN, e0 + F32_MIN, ee + F32_MIN)


def dpm_step_restate(x, eu, ec, m_prev, cfg: float, sigma_s: float, alpha_s: float, a: float, b0: float, b1: float):
    """The float arguments as the fp32 values the kernel is passed -> ((x_next, m), (bounds))."""
    cfg, sigma_s, alpha_s, a, b0, b1 = (f32c(v) for v in (cfg, sigma_s, alpha_s, a, b0, b1))
    e, ee = _guided(eu, ec, cfg)
    x = x.double()
    p = sigma_s * e
    nm = x - p
    m = nm / alpha_s
    em = (abs(sigma_s) * ee + E24 * p.abs() + E24 * nm.abs()) / alpha_s + E24 * m.abs()
    p1, p2 = a * x, b0 * m
    xn = p1 + p2
    en = abs(b0) * em + E24 * (p1.abs() + p2.abs() + xn.abs())
    if m_prev is not None:
        t = b1 * m_prev.double()
        xn = xn + t
        en = en + E24 * t.abs() + E24 * xn.abs()
    return (xn, m), (en + F32_MIN, em + F32_MIN)


# ------------------------------------------------------------------ stem
def stem_restate(x, w, bias, dtype):
    """x fp32 [n, cin, h, w], w [cout, cin, 3, 3], bias [cout] -> (ref, bound) NHWC [n, h, w, cout] for the output type T."""
    import torch.nn.functional as F
    n, cin, h, wd_ = x.shape
    cout = w.shape[0]
    cols = F.unfold(x.double(), 3, padding=1)                      # [n, cin * 9, h * w], zeros outside the image
    wm, bd = w.double().reshape(cout, cin * 9), bias.double()
    ref = (wm @ cols + bd[:, None]).reshape(n, cout, h, wd_).permute(0, 2, 3, 1)
    mag = (wm.abs() @ cols.abs() + bd.abs()[:, None]).reshape(n, cout, h, wd_).permute(0, 2, 3, 1)
    return ref, half_ulp_t(ref, dtype) + (9 * cin + 1) * E24 * mag


# ------------------------------------------------------------------ cases shared by the host and the GPU tests
SCHEDULES = {"cosine": (0, 153, 926, 999), "linear": (10, 500, 990)}   # a 1000-step schedule reset to a searched candidate


def step_tables(name: str):
    from oracle import schedule
    return schedule.OracleDiffusion(steps=1000, noise_schedule=name).reset(list(SCHEDULES[name])).tables


def step_coefs_of(tables, i: int, var: str, predict_xstart: bool, clip: bool, eta: float = 0.0):
    """var: 'learned' | 'small' | 'large' -> the ctypes adm_step_coefs of step i, as the sampler packs it."""
    from autodiffusion_amd.sampler import step_coefs
    return step_coefs(tables, i, learned_range=(var == "learned"), fixed=("small" if var == "small" else "large"),
                      predict_xstart=predict_xstart, clip_denoised=clip, eta=eta)


def step_inputs(shape, learned: bool, seed: int) -> dict:
    """CPU fp32 operands of one step: x, model_out (the variance half uniform in [-1.5, 1.5]), grad, noise."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    mo = torch.randn(n, c, h, w, generator=g)
    if learned:
        mo = torch.cat([mo, torch.rand(n, c, h, w, generator=g) * 3 - 1.5], 1)
    return {"x": torch.randn(shape, generator=g), "mo": mo.contiguous(), "grad": 0.3 * torch.randn(shape, generator=g),
            "noise": torch.randn(shape, generator=g)}


def step_flag_product(ddim: bool):
    """The full product of the issue's flags: (var, predict_xstart, clip, with_grad, eta) per step index."""
    out = []
    for var in (("learned", "large") if ddim else ("learned", "small", "large")):
        for px in (False, True):
            for clip in (False, True):
                for with_grad in (False, True):
                    for eta in ((0.0, 0.7, 1.0) if ddim else (0.0,)):
                        out.append((var, px, clip, with_grad, eta))
    return out


PLMS_W = {0: (1.0, 0.0, 0.0, 0.0), 1: (1.5, -0.5, 0.0, 0.0), 2: (23 / 12, -16 / 12, 5 / 12, 0.0),
          3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
SD_SQRT_AT = (0.9991, 0.5, 0.07)


def sd_coefs_of(cfg: float, hist: int, sqrt_at: float, with_noise: bool):
    """A ctypes adm_sd_step_coefs: PLMS weights of the given history depth, alpha_prev a step ahead of alpha_t, eta = 1's sigma
    when noise is asked (dir_coef = sqrt(1 - a_prev - sigma^2) evaluated in float64 and rounded once)."""
    from autodiffusion_amd._lib import SdStepCoefs
    at = sqrt_at * sqrt_at
    ap = min(0.9999, at + 0.3 * (1 - at))
    sigma = math.sqrt((1 - ap) / (1 - at)) * math.sqrt(1 - at / ap) if with_noise else 0.0
    c = SdStepCoefs()
    c.cfg_scale = cfg
    for i in range(4):
        c.w[i] = PLMS_W[hist][i]
    c.sqrt_one_minus_at, c.sqrt_at, c.sqrt_a_prev = math.sqrt(1 - at), sqrt_at, math.sqrt(ap)
    c.sigma = sigma
    c.dir_coef = math.sqrt(max(1 - ap - sigma * sigma, 0.0))
    return c


def sd_subsets():
    """Every subset of {eps_uncond, h1, h1+h2, h1+h2+h3, noise, pred_x0, e_out} the header allows: the history is nested."""
    return [(eu, hist, nz, px0, eo) for eu in (False, True) for hist in range(4) for nz in (False, True) for px0 in (False, True)
            for eo in (False, True)]


LINEAR_SHAPES = [("mfma", 1, 16, 1), ("mfma", 64, 16, 33), ("mfma", 65, 16, 33), ("mfma", 63, 48, 129), ("mfma", 257, 32, 31),
                 ("mfma", 2, 768, 96), ("gemv", 1, 4, 1), ("gemv", 16, 20, 8), ("gemv", 17, 20, 9), ("gemv", 3, 260, 33),
                 ("gemv", 5, 1000, 40), ("gemv", 2, 2044, 5), ("tile", 7, 30, 50), ("tile", 65, 7, 65), ("tile", 4, 1, 4),
                 ("tile", 3, 2052, 10)]
TABLE_ROWS = 10


def linear_inputs(n: int, k: int, o: int, seed: int) -> dict:
    """CPU fp32 operands; idx hits row 0, the table's last row and a repeat (as far as n allows)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, TABLE_ROWS, (n,), generator=g)
    for j, v in enumerate((0, TABLE_ROWS - 1, TABLE_ROWS - 1)[:n]):
        idx[n - 1 - j] = v
    return {"x": torch.randn(n, k, generator=g), "w": torch.randn(o, k, generator=g) * k ** -0.5,
            "bias": 0.1 * torch.randn(o, generator=g), "table": torch.randn(TABLE_ROWS, o, generator=g), "idx": idx}


TIMESTEPS = (0.0, 1.0, 250.0, 999.0, 999.75, 0.5)
TIMESTEP_DIMS = (2, 3, 32, 33, 320, 1280)
STEM_SHAPES = [(1, 1, 1, 1, 8), (2, 3, 5, 7, 24), (1, 8, 4, 4, 224), (3, 3, 64, 64, 512)]


def stem_inputs(n, cin, h, w, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, cin, h, w, generator=g), 0.2 * torch.randn(cout, cin, 3, 3, generator=g), 0.1 * torch.randn(cout, generator=g))


# ------------------------------------------------------------------ k-NN cases on the exact lattice of tests/test_hip_evaluator.py
def _centers(d: int):
    return np.random.default_rng(4).integers(-3, 4, size=(16, d))


def smallest_case(nq: int, nx: int, d: int, kk: int):
    """(q, x, ref [nq, kk]): lattice rows (exact in fp16, every distance exact in fp32); with nx >= 3 three rows of x are copies of
    one query row, so that equal distances meet in the lists."""
    from test_evaluator_host import ref_distances
    from test_hip_evaluator import lattice
    c = _centers(d)
    q, x = lattice(nq, d, 40 + nq, c[:12]), lattice(nx, d, 41 + nx, c[4:])
    if nx >= 3:
        x[[0, nx // 2, nx - 1]] = q[nq // 2]
    return q, x, np.sort(ref_distances(q, x), axis=1)[:, :kk]


def cover_case(na: int, nb: int, d: int, K: int):
    """(a, ra, b, rb): lattice rows and their own k-NN radii from ref_radii (neighbourhood sizes 0 .. K - 1, 3 for K = 1, capped at
    the set's size): the radii are distances of the lattice, so the cover's `<=` meets ties."""
    from test_evaluator_host import ref_radii
    from test_hip_evaluator import lattice
    c = _centers(d)
    fa, fb = lattice(na, d, 50 + na, c[:12]), lattice(nb, d, 51 + nb, c[4:])

    def radii(f):
        sizes = tuple(min(j, len(f) - 1) for j in (range(K) if K > 1 else (3,)))
        return ref_radii(f, sizes).astype(np.float32)
    return fa, radii(fa), fb, radii(fb)


def cover_membership(fa, ra, fb, rb):
    """ref_pr's two membership tables before it averages them: a_in [na, K], b_in [nb, K]."""
    from test_evaluator_host import ref_distances
    d = ref_distances(fa, fb)[..., None]
    return (d <= np.asarray(rb, np.float64)[None]).any(1), (d <= np.asarray(ra, np.float64)[:, None]).any(0)
