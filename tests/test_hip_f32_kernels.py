"""The fp32 kernels outside the 16-bit torso on the MI355X against the float64 restatements of tests/f32_kernels.py: the embedding
path (adm_linear_f32's three kernels, adm_timestep_embedding), the sampler steps (adm_ddim_step, adm_ddpm_step, adm_sd_step,
adm_dpm_step), adm_pack_u8_nhwc, adm_stem_conv3x3 in both libraries, and the k-NN kernels at narrow feature widths on the exact
lattice.  Every launch goes through the library symbol onto test-owned buffers: NaN-filled outputs (every element must be
written) with a sentinel guard behind them, and every element is held to worst_ratio(got, ref, bound) <= 1 with the bounds
derived in f32_kernels' docstring (tested on the host by tests/test_f32_kernels_host.py); bytes, zeros and the lattice's exact
distances are compared bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import f32_kernels as fk
from launch_replay import worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
SENTINEL = -7.0
BYTE_FILL, BYTE_SENTINEL = 0x5A, 0xC3
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _owned(shape, dtype=F32, offset=0, fill=None):
    """A test-owned output: `shape` elements of NaN (bytes: BYTE_FILL, or `fill`) that must all be written, `offset` elements
    into a buffer with GUARD sentinel elements behind them."""
    numel = int(np.prod(shape))
    byte = dtype == torch.uint8
    buf = torch.full((offset + numel + GUARD,), (BYTE_FILL if fill is None else fill) if byte else float("nan"), dtype=dtype, device=DEV)
    buf[offset + numel:] = BYTE_SENTINEL if byte else SENTINEL
    return buf, buf[offset:offset + numel].view(shape)


def _guard_ok(buf, what):
    s = BYTE_SENTINEL if buf.dtype == torch.uint8 else SENTINEL
    assert bool((buf[-GUARD:] == s).all()), f"{what}: the guard behind the output was written"


def _call(kind, name, *args):
    from autodiffusion_amd import _lib
    _lib.check(getattr(_lib.load(kind), name)(*args, torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, offset=0):
    """A device copy of t; offset: as a contiguous view `offset` elements into its buffer."""
    if t is None:
        return None
    buf = torch.empty(offset + t.numel(), dtype=t.dtype, device=DEV)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def _hold(what, got, ref, bound):
    w, _, _, rep = worst_ratio(got, ref, bound)
    assert w <= 1.0, (what, w, rep)
    return w


# ------------------------------------------------------------------ adm_linear_f32
LINEAR_FLAGS = [(s, b, t) for s in (False, True) for b, t in ((False, False), (True, False), (True, True))]
LINEAR_CASES = [(p, n, k, o, 0) for p, n, k, o in fk.LINEAR_SHAPES] + [("tile", 8, 32, 16, 1)]


def _check_linear(kind, n, k, o, silu_in, with_bias, with_table, offset=0, seed=11):
    d = fk.linear_inputs(n, k, o, seed)
    x, w = _dev(d["x"], offset), _dev(d["w"], offset)
    bias = _dev(d["bias"]) if with_bias else None
    table, idx = (_dev(d["table"]), _dev(d["idx"])) if with_table else (None, None)
    buf, out = _owned((n, o))
    _call(kind, "adm_linear_f32", _p(x), _p(w), _p(bias), _p(table), _p(idx), _p(out), n, k, o, int(silu_in))
    _guard_ok(buf, "adm_linear_f32")
    ref, bound = fk.linear_restate(x, w, bias, table, idx, silu_in)
    return worst_ratio(out, ref, bound)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("path,n,k,o,offset", LINEAR_CASES)
def test_linear_f32_at_edges(path, n, k, o, offset, kind):
    assert fk.linear_path(k, aligned=not offset) == path
    worst = 0.0
    for silu_in, with_bias, with_table in LINEAR_FLAGS:
        w, _, _, rep = _check_linear(kind, n, k, o, silu_in, with_bias, with_table, offset)
        assert w <= 1.0, (silu_in, with_bias, with_table, w, rep)
        worst = max(worst, w)
    print(f"linear_f32 {path} {(n, k, o)}{' misaligned' if offset else ''} [{kind}]: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------ adm_timestep_embedding
def _check_timestep(t, dim, max_period):
    t = t.to(DEV)
    n = t.shape[0]
    buf, out = _owned((n, dim))
    _call("bf16", "adm_timestep_embedding", _p(t), _p(out), n, dim, max_period)
    _guard_ok(buf, "adm_timestep_embedding")
    ref, bound = fk.timestep_restate(t, dim, max_period)
    inside = 2 * (dim // 2)
    if bool(out[:, inside:].contiguous().view(torch.int32).any()):
        return float("inf"), 0.0, 0.0, "the odd column is not +0"
    return worst_ratio(out[:, :inside], ref[:, :inside], bound[:, :inside])


@pytest.mark.parametrize("max_period", [10000.0, 100.0])
@pytest.mark.parametrize("dim", fk.TIMESTEP_DIMS)
def test_timestep_embedding_at_edges(dim, max_period):
    w, _, _, rep = _check_timestep(torch.tensor(fk.TIMESTEPS, dtype=F32), dim, max_period)
    print(f"timestep_embedding dim {dim} period {max_period:g}: worst err/bound {w:.3f}")
    assert w <= 1.0, (w, rep)


def test_timestep_embedding_past_the_block_cap():
    w, _, _, rep = _check_timestep((torch.arange(1025) % 1000).to(F32), 256, 10000.0)   # 1025 blocks of work on 1024
    print(f"timestep_embedding n 1025 dim 256: worst err/bound {w:.3f}")
    assert w <= 1.0, (w, rep)


# ------------------------------------------------------------------ adm_ddim_step / adm_ddpm_step
def _check_step(ddim, d, cs, *, with_grad, noise, want_x0=True, want_u8=True, offset=0):
    """One launch; noise: 'given' | 'nan' (must not be read) | None.  -> worst err / bound over x_prev and pred_xstart."""
    name = "adm_ddim_step" if ddim else "adm_ddpm_step"
    n, c, h, w = d["x"].shape
    x, mo = _dev(d["x"], offset), _dev(d["mo"], offset)
    grad = _dev(d["grad"], offset) if with_grad else None
    nz = None if noise is None else _dev(d["noise"] if noise == "given" else torch.full_like(d["noise"], float("nan")), offset)
    bp, xp = _owned((n, c, h, w), offset=offset)
    b0, x0 = _owned((n, c, h, w), offset=offset) if want_x0 else (None, None)
    bu, u8 = _owned((n, h, w, c), torch.uint8) if want_u8 else (None, None)
    _call("bf16", name, _p(x), _p(mo), _p(grad), _p(nz), _p(xp), _p(x0), _p(u8), n, c, h, w, C.byref(cs))
    for b in (bp, b0, bu):
        if b is not None:
            _guard_ok(b, name)
    (rs, r0), (bs, bb0) = (fk.ddim_restate if ddim else fk.ddpm_restate)(x, mo, grad, nz, fk.coefs_dict(cs))
    worst, _, _, rep = worst_ratio(xp, rs, bs)
    assert worst <= 1.0, (name, "x_prev", worst, rep)
    if want_x0:
        w0, _, _, rep = worst_ratio(x0, r0, bb0)
        assert w0 <= 1.0, (name, "pred_xstart", w0, rep)
        worst = max(worst, w0)
    if want_u8:   # two IEEE operations and a truncation on the kernel's own x_prev
        assert np.array_equal(u8.cpu().numpy(), fk.pack_u8_restate(xp)), (name, "the uint8 image differs from the fp32 restatement")
    return worst


@pytest.mark.parametrize("schedule", sorted(fk.SCHEDULES))
@pytest.mark.parametrize("ddim", [True, False], ids=["ddim", "ddpm"])
def test_sampler_step_flag_product(ddim, schedule):
    tables = fk.step_tables(schedule)
    last = len(fk.SCHEDULES[schedule]) - 1
    worst, at = 0.0, None
    for var, px, clip, with_grad, eta in fk.step_flag_product(ddim):
        d = fk.step_inputs((2, 3, 8, 8), var == "learned", 21)
        for i in (0, 1, last):
            cs = fk.step_coefs_of(tables, i, var, px, clip, eta)
            unused = i == 0 or (ddim and eta == 0.0)
            noise = "given" if not unused else (None if i == 0 and with_grad else "nan")
            try:
                w = _check_step(ddim, d, cs, with_grad=with_grad, noise=noise)
            except AssertionError as e:
                raise AssertionError((var, px, clip, with_grad, eta, i, noise)) from e
            if w > worst:
                worst, at = w, (var, px, clip, with_grad, eta, i)
    print(f"{'ddim' if ddim else 'ddpm'}_step {schedule} (2, 3, 8, 8): worst err/bound {worst:.3f} at {at}")


STEP_SHAPES = [((1, 3, 5, 7), 0, True, "hw 35: the scalar instantiation"), ((2, 1, 6, 6), 0, True, "c 1"), ((1, 4, 4, 4), 0, True, "c 4"),
               ((2, 3, 8, 8), 1, True, "misaligned operands"), ((5, 1, 1024, 1024), 0, True, "past the block cap"),
               ((2, 3, 8, 8), 0, False, "x0 and u8 NULL")]


@pytest.mark.parametrize("ddim", [True, False], ids=["ddim", "ddpm"])
@pytest.mark.parametrize("shape,offset,outputs,why", STEP_SHAPES, ids=[s[3] for s in STEP_SHAPES])
def test_sampler_step_shapes(shape, offset, outputs, why, ddim):
    cs = fk.step_coefs_of(fk.step_tables("cosine"), 1, "learned", False, True, 0.7)
    d = fk.step_inputs(shape, True, 27)
    w = _check_step(ddim, d, cs, with_grad=True, noise="given", want_x0=outputs, want_u8=outputs, offset=offset)
    print(f"{'ddim' if ddim else 'ddpm'}_step {shape} ({why}): worst err/bound {w:.3f}")


# ------------------------------------------------------------------ adm_pack_u8_nhwc
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 3, 5, 7), (3, 1, 64, 64), (5, 1, 1024, 1024)])
def test_pack_u8_bitwise(shape):
    vals = torch.tensor(fk.pack_seeds(), dtype=F32)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(29)) * 1.2
    x.view(-1)[:len(vals)] = vals
    x.view(-1)[-len(vals):] = vals      # and in the last pixels of the last image
    n, c, h, w = shape
    xd = _dev(x)
    buf, out = _owned((n, h, w, c), torch.uint8)
    _call("bf16", "adm_pack_u8_nhwc", _p(xd), _p(out), n, c, h, w)
    _guard_ok(buf, "adm_pack_u8_nhwc")
    ref = fk.pack_u8_restate(x)
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} bytes differ"


# ------------------------------------------------------------------ adm_sd_step / adm_dpm_step
def _latents(numel, seed, count):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(numel, generator=g).to(DEV) for _ in range(count)]


def _check_sd_step(t, with_eu, hist, with_nz, with_x0, with_eo, cfg, sqrt_at):
    x, eu, ec, h1, h2, h3, nz = t
    numel = x.numel()
    cs = fk.sd_coefs_of(cfg, hist, sqrt_at, with_nz)
    hs = [h1, h2, h3][:hist] + [None] * (3 - hist)
    bp, xp = _owned((numel,))
    b0, x0 = _owned((numel,)) if with_x0 else (None, None)
    be, eo = _owned((numel,)) if with_eo else (None, None)
    _call("bf16", "adm_sd_step", _p(x), _p(eu) if with_eu else None, _p(ec), _p(hs[0]), _p(hs[1]), _p(hs[2]),
          _p(nz) if with_nz else None, _p(xp), _p(x0), _p(eo), numel, C.byref(cs))
    for b in (bp, b0, be):
        if b is not None:
            _guard_ok(b, "adm_sd_step")
    refs, bounds = fk.sd_step_restate(x, eu if with_eu else None, ec, hs[:hist], nz if with_nz else None, fk.sd_coefs_dict(cs))
    worst = 0.0
    for what, got, r, b in zip(("x_prev", "pred_x0", "e_out"), (xp, x0, eo), refs, bounds):
        if got is not None:
            worst = max(worst, _hold(("adm_sd_step", what, with_eu, hist, with_nz, cfg, sqrt_at), got, r, b))
    return worst


def test_sd_step_every_operand_subset():
    t = _latents(1000, 31, 7)
    worst, at = 0.0, None
    for j, (with_eu, hist, with_nz, with_x0, with_eo) in enumerate(fk.sd_subsets()):
        for cfg in (1.0, 7.5):
            w = _check_sd_step(t, with_eu, hist, with_nz, with_x0, with_eo, cfg, fk.SD_SQRT_AT[j % 3])
            if w > worst:
                worst, at = w, (with_eu, hist, with_nz, with_x0, with_eo, cfg, fk.SD_SQRT_AT[j % 3])
    print(f"sd_step numel 1000: worst err/bound {worst:.3f} at {at}")


BIG_NUMEL = 8192 * 256 + 259   # past the 8192-block cap, and not a multiple of 256


def test_sd_step_past_the_block_cap():
    w = _check_sd_step(_latents(BIG_NUMEL, 32, 7), True, 3, True, True, True, 7.5, 0.07)
    print(f"sd_step numel {BIG_NUMEL}: worst err/bound {w:.3f}")


@pytest.mark.parametrize("numel", [1000, BIG_NUMEL])
def test_dpm_step_every_operand_subset(numel):
    x, eu, ec, mp = _latents(numel, 33, 4)
    p = dict(cfg=7.5, sigma_s=0.6, alpha_s=0.8, a=0.75, b0=0.4, b1=-0.12)
    worst = 0.0
    for with_eu in (False, True):
        for with_mp in (False, True):
            for with_mo in (False, True):
                bn, xn = _owned((numel,))
                bm, mo = _owned((numel,)) if with_mo else (None, None)
                _call("bf16", "adm_dpm_step", _p(x), _p(eu) if with_eu else None, _p(ec), _p(mp) if with_mp else None, _p(xn), _p(mo),
                      numel, p["cfg"], p["sigma_s"], p["alpha_s"], p["a"], p["b0"], p["b1"])
                _guard_ok(bn, "adm_dpm_step")
                refs, bounds = fk.dpm_step_restate(x, eu if with_eu else None, ec, mp if with_mp else None, **p)
                worst = max(worst, _hold(("adm_dpm_step x_next", with_eu, with_mp), xn, refs[0], bounds[0]))
                if with_mo:
                    _guard_ok(bm, "adm_dpm_step m_out")
                    worst = max(worst, _hold(("adm_dpm_step m_out", with_eu, with_mp), mo, refs[1], bounds[1]))
    print(f"dpm_step numel {numel}: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------ adm_stem_conv3x3
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", fk.STEM_SHAPES)
def test_stem_conv_at_edges(shape, dtype):
    n, cin, h, w, cout = shape
    x, wt, b = (_dev(t) for t in fk.stem_inputs(*shape, 33))
    buf, out = _owned((n, h, w, cout), dtype)
    _call("f16" if dtype == torch.float16 else "bf16", "adm_stem_conv3x3", _p(x), _p(wt), _p(b), _p(out), n, cin, h, w, cout)
    _guard_ok(buf, "adm_stem_conv3x3")
    ref, bound = fk.stem_restate(x, wt, b, dtype)
    wr = _hold(("adm_stem_conv3x3", shape, dtype), out, ref, bound)
    print(f"stem_conv3x3 {shape} {dtype}: worst err/bound {wr:.3f}")


# ------------------------------------------------------------------ k-NN at narrow widths, on the exact lattice
def _half_rows(f):
    x16 = torch.from_numpy(f).to(DEV).to(torch.float16).contiguous()
    return x16, x16.float().pow(2).sum(1).contiguous()


def _smallest(q16, qn, x16, xn, kk, splits):
    nq, nx, d = q16.shape[0], x16.shape[0], q16.shape[1]
    buf, out = _owned((nq, kk))
    bw, ws = _owned((splits, nq, kk)) if splits > 1 else (None, None)
    _call("bf16", "adm_knn_smallest", _p(q16), nq, _p(qn), _p(x16), nx, _p(xn), d, kk, _p(out), _p(ws), splits)
    _guard_ok(buf, "adm_knn_smallest")
    if bw is not None:
        _guard_ok(bw, "adm_knn_smallest workspace")
    return out


@pytest.mark.parametrize("d", [64, 128, 192])
@pytest.mark.parametrize("nq,nx", [(1, None), (129, 130), (300, 257)], ids=["nx == kk", "129x130", "300x257"])
def test_knn_smallest_at_narrow_widths(nq, nx, d):
    for kk in range(1, 9):
        q, x, ref = fk.smallest_case(nq, nx or kk, d, kk)
        (q16, qn), (x16, xn) = _half_rows(q), _half_rows(x)
        rtiles = (x.shape[0] + 127) // 128
        one = _smallest(q16, qn, x16, xn, kk, 1)
        assert np.array_equal(one.cpu().numpy(), ref.astype(np.float32)), (kk, "splits 1 differs from the restatement")
        if rtiles > 1:
            assert torch.equal(_smallest(q16, qn, x16, xn, kk, rtiles), one), (kk, "the outputs depend on splits")


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("na,nb", [(1, 1), (127, 129), (129, 127), (260, 5)])
def test_knn_cover_at_narrow_widths(na, nb, K, d):
    fa, ra, fb, rb = fk.cover_case(na, nb, d, K)
    (a16, an), (b16, bn) = _half_rows(fa), _half_rows(fb)
    rad, rbd = torch.from_numpy(ra).to(DEV).contiguous(), torch.from_numpy(rb).to(DEV).contiguous()
    ba, a_in = _owned((na, K), torch.uint8, fill=0)     # the kernel stores only the ones: the flags start at zero
    bb, b_in = _owned((nb, K), torch.uint8, fill=0)
    _call("bf16", "adm_knn_cover", _p(a16), na, _p(an), _p(rad), _p(b16), nb, _p(bn), _p(rbd), d, K, _p(a_in), _p(b_in))
    _guard_ok(ba, "adm_knn_cover a_in")
    _guard_ok(bb, "adm_knn_cover b_in")
    ra_in, rb_in = fk.cover_membership(fa, ra, fb, rb)
    assert np.array_equal(a_in.cpu().numpy().astype(bool), ra_in) and np.array_equal(b_in.cpu().numpy().astype(bool), rb_in)
    assert set(np.unique(a_in.cpu().numpy())) | set(np.unique(b_in.cpu().numpy())) <= {0, 1}
