"""CPU checks of tests/f32_kernels.py: every restatement equals a plain torch float64 composition, an fp32 emulation of the
kernel's operation order stays inside the derived bound, and each named defect lands outside it -- at the shapes the GPU tests
(tests/test_hip_f32_kernels.py) run.  A wrong reference or a bound that a wrong kernel fits would otherwise pass unnoticed."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_kernels as fk

F32 = torch.float32
BF, FP16 = torch.bfloat16, torch.float16


def _ratio(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(got.double()) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    return r.max().item()


def _silu32(z):
    return z * (1.0 / (1.0 + torch.exp2(z * torch.tensor(-1.4426950408889634, dtype=F32))))


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, the sum rounds to fp32."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------ linear
def _linear_emulated(path, x, w, bias, table, idx, silu_in, *, silu_twice=False, no_bias_from=None, idx0=False, k_limit=None):
    """adm_linear_f32 in fp32, in the summation order of the kernel `path` names (csrc/adm_embed.hip).  Defects: SiLU applied
    twice, the bias skipped from column no_bias_from on, the table row of idx[0] for every row, the k >= k_limit dropped."""
    n, k = x.shape
    s = _silu32(x) if silu_in else x
    if silu_twice:
        s = _silu32(s)
    if k_limit is not None:
        s, w, k = s[:, :k_limit], w[:, :k_limit], k_limit
    if path == "tile":      # sequential over k, one multiply and one add each
        acc = torch.zeros(n, w.shape[0])
        for j in range(k):
            acc = acc + s[:, j, None] * w[None, :, j]
    elif path == "mfma":    # per 16-deep step four instructions; instruction e adds the products k = 16 step + 4 lq + e, lq = 0..3
        acc = torch.zeros(n, w.shape[0])
        for st in range(k // 16):
            for e in range(4):
                inner = torch.zeros_like(acc)
                for lq in range(4):
                    j = 16 * st + 4 * lq + e
                    inner = inner + s[:, j, None] * w[None, :, j]
                acc = acc + inner
    else:                   # GEMV: lane l chains multiply-adds over k = 256 pass + 4 l + (0..3), six butterfly steps add the lanes
        passes = (k + 255) // 256
        sp, wp = F.pad(s, (0, passes * 256 - k)), F.pad(w, (0, passes * 256 - k))
        sp, wp = sp.reshape(n, 1, passes, 64, 4), wp.reshape(1, -1, passes, 64, 4)
        acc = torch.zeros(n, w.shape[0], 64)
        for p in range(passes):
            for j in range(4):
                acc = _fma(wp[:, :, p, :, j], sp[:, :, p, :, j], acc)
        while acc.shape[-1] > 1:
            half = acc.shape[-1] // 2
            acc = acc[..., :half] + acc[..., half:]
        acc = acc[..., 0]
    if bias is not None:
        b = bias.clone()
        if no_bias_from is not None:
            b[no_bias_from:] = 0.0
        acc = acc + b
    if table is not None:
        acc = acc + table[idx[:1].expand_as(idx) if idx0 else idx]
    return acc


LINEAR_FLAGS = [(s, b, t) for s in (False, True) for b, t in ((False, False), (True, False), (True, True))]


@pytest.mark.parametrize("path,n,k,o", fk.LINEAR_SHAPES)
def test_linear_restatement_matches_torch_and_the_emulations_stay_inside(path, n, k, o):
    assert fk.linear_path(k) == path
    d = fk.linear_inputs(n, k, o, 11)
    assert n < 3 or {0, fk.TABLE_ROWS - 1} <= set(d["idx"].tolist()) and len(set(d["idx"].tolist())) < n
    worst = 0.0
    for silu_in, with_bias, with_table in LINEAR_FLAGS:
        bias = d["bias"] if with_bias else None
        table, idx = (d["table"], d["idx"]) if with_table else (None, None)
        ref, bound = fk.linear_restate(d["x"], d["w"], bias, table, idx, silu_in)
        xd = d["x"].double()
        plain = F.linear(F.silu(xd) if silu_in else xd, d["w"].double(), None if bias is None else bias.double())
        if with_table:
            plain = plain + table.double()[idx]
        torch.testing.assert_close(ref, plain, rtol=1e-12, atol=1e-12)
        orders = {"tile"} | ({"gemv"} if k % 4 == 0 else set()) | ({"mfma"} if k % 16 == 0 else set())   # every order this k admits
        for order in sorted(orders):
            r = _ratio(_linear_emulated(order, d["x"], d["w"], bias, table, idx, silu_in), ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (order, silu_in, with_bias, with_table, r)
    print(f"linear {path} {(n, k, o)}: worst emulated err/bound {worst:.3f}")


def test_linear_defects_land_outside_the_bound():
    d = fk.linear_inputs(64, 16, 33, 12)
    ref, bound = fk.linear_restate(d["x"], d["w"], d["bias"], d["table"], d["idx"], True)
    assert _ratio(_linear_emulated("mfma", d["x"], d["w"], d["bias"], d["table"], d["idx"], True), ref, bound) <= 1.0
    # the bias skipped on the last partial column tile (columns 32 of 33)
    assert _ratio(_linear_emulated("mfma", d["x"], d["w"], d["bias"], d["table"], d["idx"], True, no_bias_from=32), ref, bound) > 1.0
    # the table row taken from idx[0]
    assert _ratio(_linear_emulated("mfma", d["x"], d["w"], d["bias"], d["table"], d["idx"], True, idx0=True), ref, bound) > 1.0
    # SiLU applied twice
    assert _ratio(_linear_emulated("mfma", d["x"], d["w"], d["bias"], d["table"], d["idx"], True, silu_twice=True), ref, bound) > 1.0
    # the GEMV's second lane pass dropped at k = 260
    d = fk.linear_inputs(3, 260, 33, 13)
    ref, bound = fk.linear_restate(d["x"], d["w"], d["bias"], None, None, False)
    assert _ratio(_linear_emulated("gemv", d["x"], d["w"], d["bias"], None, None, False), ref, bound) <= 1.0
    assert _ratio(_linear_emulated("gemv", d["x"], d["w"], d["bias"], None, None, False, k_limit=256), ref, bound) > 1.0


def test_linear_path_follows_the_library():
    assert [fk.linear_path(k) for k in (16, 768, 4, 20, 1000, 2044, 2052, 30, 7, 1)] == ["mfma", "mfma"] + ["gemv"] * 4 + ["tile"] * 4
    assert fk.linear_path(32, aligned=False) == "tile"


# ------------------------------------------------------------------ timestep embedding
def _timestep_emulated(t, dim, max_period, *, swap=False, half_minus_one=False, odd_garbage=False):
    half = dim // 2
    nlp = -torch.log(torch.tensor(max_period, dtype=F32))
    k = torch.arange(half, dtype=F32)
    freq = torch.exp(nlp * k / torch.tensor(float(half - 1 if half_minus_one else half), dtype=F32))
    a = t[:, None] * freq[None]
    out = torch.zeros(t.shape[0], dim) if not odd_garbage else torch.ones(t.shape[0], dim)
    c, s = (torch.sin(a), torch.cos(a)) if swap else (torch.cos(a), torch.sin(a))
    out[:, :half], out[:, half:2 * half] = c, s
    return out


@pytest.mark.parametrize("max_period", [10000.0, 100.0])
@pytest.mark.parametrize("dim", fk.TIMESTEP_DIMS)
def test_timestep_restatement_emulation_and_defects(dim, max_period):
    t = torch.tensor(fk.TIMESTEPS, dtype=F32)
    ref, bound = fk.timestep_restate(t, dim, max_period)
    half = dim // 2   # nn.py:103-121
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    plain = torch.cat([torch.cos(args), torch.sin(args)], -1)
    if dim % 2:
        plain = torch.cat([plain, torch.zeros_like(plain[:, :1])], -1)
    torch.testing.assert_close(ref, plain, rtol=1e-13, atol=1e-13)
    got = _timestep_emulated(t, dim, max_period)
    inside = 2 * half
    assert _ratio(got[:, :inside], ref[:, :inside], bound[:, :inside]) <= 1.0
    assert not bool(bound[:, inside:].any()) and not bool(ref[:, inside:].any())
    assert _ratio(_timestep_emulated(t, dim, max_period, swap=True)[:, :inside], ref[:, :inside], bound[:, :inside]) > 1.0
    if half > 2:   # k / (half - 1) is k / half at k = 0 alone
        assert _ratio(_timestep_emulated(t, dim, max_period, half_minus_one=True)[:, :inside], ref[:, :inside], bound[:, :inside]) > 1.0
    if dim % 2:
        assert bool(_timestep_emulated(t, dim, max_period, odd_garbage=True)[:, inside:].view(torch.int32).any())
        assert not bool(got[:, inside:].view(torch.int32).any())


# ------------------------------------------------------------------ ddim / ddpm
def _host_scalars(cf):
    """launch_step's fp32 scalar arithmetic (csrc/adm_sampler.hip), in numpy float32."""
    f, one = np.float32, np.float32(1.0)
    ac, ap, eta = f(cf["ac"]), f(cf["ac_prev"]), f(cf["eta"])
    sigma = eta * np.sqrt((one - ap) / (one - ac)) * np.sqrt(one - ac / ap)
    return {"somac": float(np.sqrt(one - ac)), "sap": float(np.sqrt(ap)), "sigma": float(sigma),
            "dir": float(np.sqrt(one - ap - sigma * sigma))}


def _step_emulated(ddim, x, mo, grad, noise, cf, *, reclamp=False, noise_at_zero=False, swap_lo_hi=False, var_offset=None,
                   skip_tail=0):
    """step_kernel in fp32, one rounding per operation.  Defects: x0 clamped again after condition_score; the noise term added
    although nonzero == 0; lo / hi swapped; the variance half read var_offset channels in; the last skip_tail pixels unwritten."""
    c = x.shape[1]
    k = _host_scalars(cf)
    A, Bm = cf["sqrt_recip_ac"], cf["sqrt_recipm1_ac"]
    ev = mo[:, :c]
    x0 = ev if cf["predict_xstart"] else A * x - Bm * ev
    if cf["clip_denoised"]:
        x0 = x0.clamp(-1.0, 1.0)
    if ddim:
        if grad is not None:
            e = (A * x - x0) / Bm
            e = e - k["somac"] * grad
            x0 = A * x - Bm * e
            if reclamp and cf["clip_denoised"]:
                x0 = x0.clamp(-1.0, 1.0)
        e = (A * x - x0) / Bm
        s = x0 * k["sap"] + k["dir"] * e
        sigma_nz = k["sigma"] if (cf["nonzero"] or noise_at_zero) else 0.0
        if noise is not None and (sigma_nz != 0.0 or noise_at_zero):
            s = s + sigma_nz * noise
    else:
        if cf["learned_range"]:
            lo, hi = (cf["log_var_hi"], cf["log_var_lo"]) if swap_lo_hi else (cf["log_var_lo"], cf["log_var_hi"])
            off = c if var_offset is None else var_offset
            frac = (mo[:, off:off + c] + 1.0) / 2.0
            logvar = frac * hi + (1.0 - frac) * lo
            var = torch.exp(logvar)
        else:
            logvar, var = torch.full_like(x, cf["log_var_lo"]), torch.full_like(x, cf["fixed_var"])
        s = cf["coef1"] * x0 + cf["coef2"] * x
        if grad is not None:
            s = s + var * grad
        if noise is not None and (cf["nonzero"] or noise_at_zero):
            s = s + (1.0 if cf["nonzero"] else 0.0) * torch.exp(0.5 * logvar) * noise
    if skip_tail:
        s = s.clone()
        s.flatten(2)[:, :, -skip_tail:] = float("nan")
    return s, x0


def _u8_emulated(s, c_index=None):
    """The kernel's uint8 NHWC store, flat; c_index: the channel count the index is computed with."""
    n, c, h, w = s.shape
    ci = c if c_index is None else c_index
    out = np.zeros(n * h * w * max(c, ci), np.uint8)
    q = ((s + 1.0) * 127.5).clamp(0.0, 255.0).to(torch.uint8).numpy()
    for img in range(n):
        for ch in range(c):
            for p in range(h * w):
                out[(img * h * w + p) * ci + ch] = q[img, ch].reshape(-1)[p]
    return out


def _plain_step(ddim, x, mo, grad, noise, cf):
    """gaussian_diffusion.py's p_mean_variance, condition_score / condition_mean and ddim_sample / p_sample, written out in
    float64 on the struct's fields."""
    c = x.shape[1]
    x, eps = x.double(), mo[:, :c].double()
    A, Bm = cf["sqrt_recip_ac"], cf["sqrt_recipm1_ac"]
    pred = eps if cf["predict_xstart"] else A * x - Bm * eps
    if cf["clip_denoised"]:
        pred = pred.clamp(-1, 1)
    nonzero = 1.0 if cf["nonzero"] else 0.0
    nz = torch.zeros_like(x) if noise is None else torch.nan_to_num(noise.double())
    if ddim:
        if grad is not None:
            eps2 = (A * x - pred) / Bm - math.sqrt(1 - cf["ac"]) * grad.double()
            pred = A * x - Bm * eps2
        eps3 = (A * x - pred) / Bm
        ab, abp = cf["ac"], cf["ac_prev"]
        sigma = cf["eta"] * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
        mean_pred = pred * math.sqrt(abp) + math.sqrt(max(1 - abp - sigma ** 2, 0.0)) * eps3
        return mean_pred + nonzero * sigma * nz, pred
    if cf["learned_range"]:
        frac = (mo[:, c:].double() + 1) / 2
        logv = frac * cf["log_var_hi"] + (1 - frac) * cf["log_var_lo"]
        var = torch.exp(logv)
    else:
        logv, var = torch.full_like(x, cf["log_var_lo"]), torch.full_like(x, cf["fixed_var"])
    mean = cf["coef1"] * pred + cf["coef2"] * x
    if grad is not None:
        mean = mean + var * grad.double()
    return mean + nonzero * torch.exp(0.5 * logv) * nz, pred


@pytest.mark.parametrize("schedule", sorted(fk.SCHEDULES))
@pytest.mark.parametrize("ddim", [True, False])
def test_step_restatement_matches_the_plain_composition_and_the_emulation_stays_inside(ddim, schedule):
    tables = fk.step_tables(schedule)
    last = len(fk.SCHEDULES[schedule]) - 1
    restate = fk.ddim_restate if ddim else fk.ddpm_restate
    worst = 0.0
    for var, px, clip, with_grad, eta in fk.step_flag_product(ddim):
        d = fk.step_inputs((2, 3, 8, 8), var == "learned", 21)
        for i in (0, 1, last):
            cf = fk.coefs_dict(fk.step_coefs_of(tables, i, var, px, clip, eta))
            grad = d["grad"] if with_grad else None
            unused = (i == 0) or (ddim and eta == 0.0)
            noise = torch.full_like(d["noise"], float("nan")) if unused else d["noise"]
            (rs, r0), (bs, b0) = restate(d["x"], d["mo"], grad, noise, cf)
            ps, p0 = _plain_step(ddim, d["x"], d["mo"], grad, noise, cf)
            torch.testing.assert_close(rs, ps, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(r0, p0, rtol=1e-12, atol=1e-12)
            gs, g0 = _step_emulated(ddim, d["x"], d["mo"], grad, None if unused else noise, cf)
            r = max(_ratio(gs, rs, bs), _ratio(g0, r0, b0))
            worst = max(worst, r)
            assert r <= 1.0, (var, px, clip, with_grad, eta, i, r)
    print(f"{'ddim' if ddim else 'ddpm'} {schedule}: worst emulated err/bound {worst:.3f}")


def test_step_restatement_matches_the_oracle_sampler():
    """The oracle's own statement of the two steps (oracle/sampler.py, fp32 coefficients) on float64 tensors."""
    from oracle import sampler as osm, schedule
    for learn in (True, False):
        d = schedule.OracleDiffusion(steps=1000, noise_schedule="cosine", learn_sigma=learn).reset(list(fk.SCHEDULES["cosine"]))
        t = fk.step_inputs((2, 3, 8, 8), learn, 22)
        x, mo, g, nz = (t[k].double() for k in ("x", "mo", "grad", "noise"))
        for i in (0, 1, 3):
            cf = fk.coefs_dict(fk.step_coefs_of(d.tables, i, "learned" if learn else "large", False, True, 0.7))
            (rs, r0), _ = fk.ddim_restate(t["x"], t["mo"], t["grad"], t["noise"], cf)
            ref = osm.ddim_step(d, mo, x, i, g, nz, 0.7)
            scale = 1e-5 * (1 + cf["sqrt_recip_ac"])
            assert (rs - ref["sample"]).abs().max() <= scale and (r0 - ref["pred_xstart"]).abs().max() <= scale
            (rs, r0), _ = fk.ddpm_restate(t["x"], t["mo"], t["grad"], t["noise"], cf)
            ref = osm.ddpm_step(d, mo, x, i, g, nz)
            assert (rs - ref["sample"]).abs().max() <= scale and (r0 - ref["pred_xstart"]).abs().max() <= scale


def test_step_defects_land_outside_the_bound():
    tables = fk.step_tables("cosine")
    # ddim: x0 clamped again after condition_score
    d = fk.step_inputs((2, 3, 8, 8), False, 23)
    cf = fk.coefs_dict(fk.step_coefs_of(tables, 1, "large", False, True, 0.0))
    (rs, r0), (bs, b0) = fk.ddim_restate(d["x"], d["mo"], d["grad"], None, cf)
    gs, g0 = _step_emulated(True, d["x"], d["mo"], d["grad"], None, cf)
    assert max(_ratio(gs, rs, bs), _ratio(g0, r0, b0)) <= 1.0
    gs, g0 = _step_emulated(True, d["x"], d["mo"], d["grad"], None, cf, reclamp=True)
    assert _ratio(g0, r0, b0) > 1.0 and _ratio(gs, rs, bs) > 1.0
    # ddim and ddpm: the noise added at i == 0 -- the tests hand a NaN-filled noise there
    nan = torch.full_like(d["noise"], float("nan"))
    for ddim in (True, False):
        cf = fk.coefs_dict(fk.step_coefs_of(tables, 0, "large", False, True, 1.0))
        (rs, _), (bs, _) = (fk.ddim_restate if ddim else fk.ddpm_restate)(d["x"], d["mo"], None, nan, cf)
        assert bool(torch.isfinite(rs).all())
        assert _ratio(_step_emulated(ddim, d["x"], d["mo"], None, nan, cf)[0], rs, bs) <= 1.0
        assert _ratio(_step_emulated(ddim, d["x"], d["mo"], None, nan, cf, noise_at_zero=True)[0], rs, bs) == float("inf")
    # ddpm: lo / hi swapped in the interpolation
    d = fk.step_inputs((2, 3, 8, 8), True, 24)
    cf = fk.coefs_dict(fk.step_coefs_of(tables, 1, "learned", False, True))
    (rs, _), (bs, _) = fk.ddpm_restate(d["x"], d["mo"], d["grad"], d["noise"], cf)
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf)[0], rs, bs) <= 1.0
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf, swap_lo_hi=True)[0], rs, bs) > 1.0
    # ddpm: fixed_var of "small" where "large" was asked
    d = fk.step_inputs((2, 3, 8, 8), False, 25)
    large = fk.coefs_dict(fk.step_coefs_of(tables, 1, "large", False, True))
    small = fk.coefs_dict(fk.step_coefs_of(tables, 1, "small", False, True))
    (rs, _), (bs, _) = fk.ddpm_restate(d["x"], d["mo"], d["grad"], d["noise"], large)
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], large)[0], rs, bs) <= 1.0
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], small)[0], rs, bs) > 1.0
    # ddpm: the variance half read at mo + 3 hw with c = 4
    d = fk.step_inputs((1, 4, 4, 4), True, 26)
    cf = fk.coefs_dict(fk.step_coefs_of(tables, 1, "learned", False, True))
    (rs, _), (bs, _) = fk.ddpm_restate(d["x"], d["mo"], d["grad"], d["noise"], cf)
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf)[0], rs, bs) <= 1.0
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf, var_offset=3)[0], rs, bs) > 1.0
    # the last hw % 4 pixels of an image left unwritten (hw = 35)
    d = fk.step_inputs((1, 3, 5, 7), True, 27)
    (rs, _), (bs, _) = fk.ddpm_restate(d["x"], d["mo"], d["grad"], d["noise"], cf)
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf)[0], rs, bs) <= 1.0
    assert _ratio(_step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf, skip_tail=35 % 4)[0], rs, bs) == float("inf")
    # the u8 image indexed as if c == 3 with c = 1
    d = fk.step_inputs((2, 1, 6, 6), True, 28)
    gs, _ = _step_emulated(False, d["x"], d["mo"], d["grad"], d["noise"], cf)
    want = fk.pack_u8_restate(gs).reshape(-1)
    assert np.array_equal(_u8_emulated(gs)[:want.size], want)
    assert not np.array_equal(_u8_emulated(gs, c_index=3)[:want.size], want)


def test_pack_restatement_matches_torch_on_the_seeds():
    vals = fk.pack_seeds()
    assert len(vals) == 7 + 18
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(29)) * 1.2
    x.view(-1)[:len(vals)] = torch.tensor(vals, dtype=F32)
    plain = ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert np.array_equal(fk.pack_u8_restate(x), plain)
    got = fk.pack_u8_restate(torch.tensor(vals, dtype=F32).reshape(1, 1, 1, -1)).reshape(-1)
    assert list(got[:7]) == [0, 255, 127, 255, 0, 255, 0]
    # around k / 127.5 - 1 the byte steps from k - 1 to k within the three neighbours
    for j, k in enumerate((1, 2, 127, 128, 254, 255)):
        three = got[7 + 3 * j:10 + 3 * j]
        assert set(three) <= {k - 1, k, min(k + 1, 255)} and three[0] <= three[1] <= three[2]


# ------------------------------------------------------------------ latent steps
def _sd_emulated(x, eu, ec, hist, noise, cf, *, w2_on_h3=False, x0_from_e=False):
    e = ec if eu is None else eu + cf["cfg_scale"] * (ec - eu)
    w = cf["w"]
    ep = w[0] * e
    for i, h in enumerate(hist):
        ep = ep + (w[2] if (w2_on_h3 and i == 2) else w[i + 1]) * h
    x0 = (x - cf["sqrt_one_minus_at"] * (e if x0_from_e else ep)) / cf["sqrt_at"]
    xp = cf["sqrt_a_prev"] * ((x - cf["sqrt_one_minus_at"] * ep) / cf["sqrt_at"]) + cf["dir_coef"] * ep
    if noise is not None:
        xp = xp + cf["sigma"] * noise
    return xp, x0, e


def _latents(numel, seed, count=8):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(numel, generator=g) for _ in range(count)]


def test_sd_step_restatement_emulation_and_defects():
    x, eu, ec, h1, h2, h3, nz, _ = _latents(1000, 31)
    worst = 0.0
    for j, (with_eu, hist, with_nz, _, _) in enumerate(fk.sd_subsets()):
        for cfg in (1.0, 7.5):
            cf = fk.sd_coefs_dict(fk.sd_coefs_of(cfg, hist, fk.SD_SQRT_AT[j % 3], with_nz))
            hs = [h1, h2, h3][:hist]
            args = (x, eu if with_eu else None, ec, hs, nz if with_nz else None, cf)
            refs, bounds = fk.sd_step_restate(*args)
            # the header's formulas, written out
            e = ec.double() if not with_eu else eu.double() + cf["cfg_scale"] * (ec.double() - eu.double())
            ep = cf["w"][0] * e + sum(cf["w"][i + 1] * h.double() for i, h in enumerate(hs))
            x0 = (x.double() - cf["sqrt_one_minus_at"] * ep) / cf["sqrt_at"]
            xp = cf["sqrt_a_prev"] * x0 + cf["dir_coef"] * ep + (cf["sigma"] * nz.double() if with_nz else 0.0)
            for r, p in zip(refs, (xp, x0, e)):
                torch.testing.assert_close(r, p, rtol=1e-12, atol=1e-12)
            r = max(_ratio(g, r_, b) for g, r_, b in zip(_sd_emulated(*args), refs, bounds))
            worst = max(worst, r)
            assert r <= 1.0, (with_eu, hist, with_nz, cfg, r)
    print(f"sd_step: worst emulated err/bound {worst:.3f}")
    cf = fk.sd_coefs_dict(fk.sd_coefs_of(7.5, 3, 0.5, True))
    args = (x, eu, ec, [h1, h2, h3], nz, cf)
    refs, bounds = fk.sd_step_restate(*args)
    bad = _sd_emulated(*args, w2_on_h3=True)
    assert _ratio(bad[0], refs[0], bounds[0]) > 1.0 and _ratio(bad[1], refs[1], bounds[1]) > 1.0
    bad = _sd_emulated(*args, x0_from_e=True)
    assert _ratio(bad[0], refs[0], bounds[0]) <= 1.0 and _ratio(bad[1], refs[1], bounds[1]) > 1.0
    # dir_coef is the header's sqrt(1 - a_prev - sigma^2)
    raw = fk.sd_coefs_of(1.0, 0, 0.5, True)
    assert abs(raw.dir_coef ** 2 + raw.sigma ** 2 + raw.sqrt_a_prev ** 2 - 1) < 1e-6


DPM = dict(cfg=7.5, sigma_s=0.6, alpha_s=0.8, a=0.75, b0=0.4, b1=-0.12)


def _dpm_emulated(x, eu, ec, m_prev, p, *, m_after_blend=False):
    p = {k: fk.f32c(v) for k, v in p.items()}
    e = ec if eu is None else eu + p["cfg"] * (ec - eu)
    m = (x - p["sigma_s"] * e) / p["alpha_s"]
    xn = p["a"] * x + p["b0"] * m
    m_out = m
    if m_prev is not None:
        xn = xn + p["b1"] * m_prev
        if m_after_blend:
            m_out = p["b0"] * m + p["b1"] * m_prev
    return xn, m_out


def test_dpm_step_restatement_emulation_and_defects():
    x, eu, ec, mp = _latents(1000, 32, 4)
    for with_eu in (False, True):
        for with_mp in (False, True):
            args = (x, eu if with_eu else None, ec, mp if with_mp else None)
            refs, bounds = fk.dpm_step_restate(*args, **DPM)
            p = {k: fk.f32c(v) for k, v in DPM.items()}
            e = ec.double() if not with_eu else eu.double() + p["cfg"] * (ec.double() - eu.double())
            m = (x.double() - p["sigma_s"] * e) / p["alpha_s"]
            xn = p["a"] * x.double() + p["b0"] * m + (p["b1"] * mp.double() if with_mp else 0.0)
            torch.testing.assert_close(refs[0], xn, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(refs[1], m, rtol=1e-12, atol=1e-12)
            assert max(_ratio(g, r, b) for g, r, b in zip(_dpm_emulated(*args, DPM), refs, bounds)) <= 1.0
    args = (x, eu, ec, mp)
    refs, bounds = fk.dpm_step_restate(*args, **DPM)
    bad = _dpm_emulated(*args, DPM, m_after_blend=True)
    assert _ratio(bad[0], refs[0], bounds[0]) <= 1.0 and _ratio(bad[1], refs[1], bounds[1]) > 1.0


# ------------------------------------------------------------------ stem
def _stem_emulated(x, w, b, dtype, wrapped=False):
    """stem_kernel in fp32: the accumulator starts at the bias and takes the taps in (ci, ky, kx) order.  wrapped: a tap left of
    the image reads the flat index before it (the previous row's last pixel) instead of being skipped."""
    n, cin, h, wd = x.shape
    acc = b[None, None, None, :].expand(n, h, wd, -1).clone()
    flat = F.pad(x.reshape(n, cin, h * wd), (1, 1))
    for ci in range(cin):
        for ky in range(3):
            for kx in range(3):
                if wrapped:
                    idx = (torch.arange(h)[:, None] + ky - 1) * wd + torch.arange(wd)[None] + kx - 1
                    ok = ((idx >= 0) & (idx < h * wd))
                    v = flat[:, ci][:, (idx.clamp(-1, h * wd) + 1).reshape(-1)].reshape(n, h, wd) * ok
                else:
                    v = F.pad(x[:, ci], (1, 1, 1, 1))[:, ky:ky + h, kx:kx + wd]
                acc = acc + v[..., None] * w[None, None, None, :, ci, ky, kx]
    return acc.to(dtype)


@pytest.mark.parametrize("dtype", [BF, FP16])
@pytest.mark.parametrize("shape", fk.STEM_SHAPES[:3])
def test_stem_restatement_emulation_and_defects(shape, dtype):
    x, w, b = fk.stem_inputs(*shape, 33)
    ref, bound = fk.stem_restate(x, w, b, dtype)
    plain = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    torch.testing.assert_close(ref, plain, rtol=1e-12, atol=1e-12)
    assert _ratio(_stem_emulated(x, w, b, dtype), ref, bound) <= 1.0
    if shape[3] > 1:
        assert _ratio(_stem_emulated(x, w, b, dtype, wrapped=True), ref, bound) > 1.0


# ------------------------------------------------------------------ k-NN on the lattice
def test_cover_with_a_strict_comparison_differs_on_the_lattice():
    """The radii of ref_radii are distances of the lattice themselves, so `<=` meets ties: a cover kernel comparing with `<`
    is told apart at the shapes the GPU test runs."""
    from test_evaluator_host import ref_distances, ref_pr, ref_radii
    for na, nb, d in ((127, 129, 64), (260, 5, 192)):
        fa, ra, fb, rb = fk.cover_case(na, nb, d, 8)
        a_in, b_in = fk.cover_membership(fa, ra, fb, rb)
        prec, rec = ref_pr(fa, ra, fb, rb)
        assert np.array_equal(b_in.mean(0), prec) and np.array_equal(a_in.mean(0), rec)
        dist = ref_distances(fa, fb)[..., None]
        strict_a, strict_b = (dist < rb[None]).any(1), (dist < ra[:, None]).any(0)
        assert not (np.array_equal(strict_a, a_in) and np.array_equal(strict_b, b_in))
        assert (ref_radii(fa, tuple(range(8))) == ra).all()
