"""Every (kernel, shape, flags) launch the shipped models make, replayed against float64 in both torsos.

The models (built as tests/test_hip_fullsize.py, tests/test_hip_sd_vae.py and tests/test_hip_clip.py build them; the weights'
values do not matter, only the launch list does) run eagerly at the batches bench.py uses and at batch 1-2, in the bf16 and the
fp16 torso, under tests/launch_replay.Recorder: ADM-64 / 128 / 256, the classifiers (the shipped attention-pool ones, and the
adaptive / spatial / spatial_v2 heads at width 64), the SD latent UNet, the KL-f8 VAE decoder
(with the image exit that follows it) and the CLIP text encoder; the KL-f8 VAE encoder is recorded and replayed by
tests/test_hip_vae_encoder_replay.py, on this file's replay functions.  The fp32 embedding path rides along: every adm_linear_f32 and
adm_timestep_embedding launch of those evaluations is a record too (tests/f32_kernels.py states and bounds them).  Each distinct record is then launched again through the same
entry point with fresh seeded operands and compared element by element with the float64 restatement of tests/launch_replay.py,
within the per-element bounds derived there (and tested on the host by tests/test_launch_replay_host.py).  Large conv maps are
compared at the corners of every 16x16 (8x8) output tile of every image plus seeded random pixels, all channels.  A coverage
guard fails if a family of launches the models are known to reach is missing, if a launch symbol the models called has no entry
in launch_replay.SYMBOL_COVERAGE, or if a symbol mapped to a record kind left no record of that kind.

Also here: GroupNorm statistics and LayerNorm at a large |mean| / std, the causal attention at the tile edges of its schedule,
and the classifier heads' kernels, the loss gradient and adm_grad_add at the smallest shapes that can still go wrong, each launched
through the library symbol on NaN-filled outputs with a guard block behind them.
"""
import ctypes as C
import time

import pytest
import torch

import guarded as gd
import launch_replay as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import ops as _ops
    return _ops


def _inputs(size, n, classes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, size, size, generator=g).to(DEV)
    t = torch.randint(0, 1000, (n,), generator=g).to(DEV)
    y = torch.randint(0, 1000, (n,), generator=g).to(DEV) if classes else None
    return x, t, y


def _run_models(torso):
    """Every shipped model at bench.py's batch and at batch 1-2, in one torso."""
    from test_hip_fullsize import adm64, clf, load_filled
    from bench import adm128_flags, adm256_flags
    from autodiffusion_amd.script_util import create_model_and_diffusion
    with torch.no_grad():
        m, _ = adm64()
        m.set_torso(torso)
        for n in (256, 2):
            m(*_inputs(64, n, True, 1))
        del m
    c = clf(64, 4).set_torso(torso)
    for n in (256, 2):
        c.log_prob_grad(*_inputs(64, n, True, 2), 1.0)
    del c
    with torch.no_grad():
        m, _ = create_model_and_diffusion(**adm128_flags())
        load_filled(m).set_torso(torso)
        for n in (32, 2):
            m(*_inputs(128, n, True, 3))
        del m
    c = clf(128, 2).set_torso(torso)
    for n in (32, 2):
        c.log_prob_grad(*_inputs(128, n, True, 4), 1.0)
    del c
    with torch.no_grad():
        for cc in (True, False):
            flags = adm256_flags()
            flags["class_cond"] = cc     # class-conditional ADM-256 (BASELINE configs[4] as written) and LSUN-256
            m, _ = create_model_and_diffusion(**flags)
            load_filled(m).set_torso(torso)
            skip = list(range(1, m.layer_num, 3))
            for n in (64, 1):
                x, t, y = _inputs(256, n, cc, 5)
                for sk in ([], skip):
                    m(x, t, y, skip_layer=sk)
            del m
            torch.cuda.empty_cache()
        from autodiffusion_amd.sd_arch import SD_V1, sd_unet_plan
        from oracle.fill import fill_state_dict
        from test_hip_sd import _model
        plan = sd_unet_plan(**SD_V1)
        m = _model(plan, {k: torch.from_numpy(v) for k, v in fill_state_dict(plan.param_shapes()).items()})
        m.set_torso(torso)
        for splitk in (False, True):
            m.enable_splitk(splitk)
            for n in (6, 1):
                g = torch.Generator().manual_seed(6)
                m(torch.randn(n, 4, 64, 64, generator=g).to(DEV), torch.randint(0, 1000, (n,), generator=g).to(DEV),
                  torch.randn(n, 77, 768, generator=g).to(DEV))
        del m
    torch.cuda.empty_cache()
    _run_vae_and_clip(torso)


def _run_pool_head_classifiers(torso):
    """The adaptive, spatial and spatial_v2 heads (csrc/adm_clfhead.hip) at the smallest plan of tests/test_variants.py: width 64,
    a 64x64 input, batch 2."""
    from helpers import filled
    from test_variants import clf_plan_of
    from autodiffusion_amd.classifier import EncoderUNetModel
    for tag in ("adaptive_noss_convres", "spatial", "spatialv2_noss"):
        plan = clf_plan_of(tag)
        c = EncoderUNetModel(plan)
        c.load_state_dict({k: torch.from_numpy(v) for k, v in filled(plan).items()})
        c.to(DEV).eval().set_torso(torso)
        c.log_prob_grad(*_inputs(64, 2, True, 8), 1.0)
        del c
    torch.cuda.empty_cache()


_FILLS = {}   # host fills of the VAE / CLIP state dicts, shared by the two torsos and dropped by the fixture
TINY_CLIP_256 = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                     max_position_embeddings=256)


def _fill(key, prefix, shapes):
    from oracle.fill import fill_array
    if key not in _FILLS:
        _FILLS[key] = {k: torch.from_numpy(fill_array(prefix + k, tuple(shape))) for k, shape in shapes.items()}
    return _FILLS[key]


def _run_vae_and_clip(torso):
    """The KL-f8 decoder at the shipped 64x64 latent map (batch 1: the 512x512 launches) and at 8x8 (batch 2), each followed by
    the image exit as sd_evaluate calls it; the CLIP text encoder at 77 tokens (8x16 map, 51 dead rows), 20 tokens (8x8 map) and
    a one-layer 256-position config at 200 tokens (16x16 map, the causal attention's LDS above 64 KB)."""
    from autodiffusion_amd import ops as hip_ops
    from autodiffusion_amd.sd_clip import CLIP_VIT_L14_TEXT, CLIPTextPlan, FrozenCLIPEmbedder
    from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL
    g = torch.Generator().manual_seed(7)
    vae = AutoencoderKL(**SD_V1_VAE)
    vae.load_state_dict(_fill("vae", "first_stage_model.", {k: v.shape for k, v in vae.state_dict().items()}))
    vae.set_torso(torso).to(DEV)
    for shape in ((1, 4, 64, 64), (2, 4, 8, 8)):
        x = vae.decode(torch.randn(shape, generator=g).to(DEV))
        hip_ops.vae_image_out(x, want_unit=True, want_u8=True)
    del vae, x
    torch.cuda.empty_cache()
    for name, cfg, prompts in (("vitl14", CLIP_VIT_L14_TEXT, ((3, 77), (1, 20))), ("tiny256", TINY_CLIP_256, ((2, 200),))):
        emb = FrozenCLIPEmbedder(device="cpu", max_length=cfg["max_position_embeddings"], config=cfg)
        fill = _fill(name, "cond_stage_model.transformer.", CLIPTextPlan(**cfg).param_shapes())
        emb.load_state_dict({"transformer." + k: v for k, v in fill.items()})
        emb.set_torso(torso).to(DEV)
        for n, t in prompts:
            emb(torch.randint(0, cfg["vocab_size"], (n, t), generator=g).to(DEV))
        del emb
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def recorded(ops):
    t0 = time.time()
    heads_s = 0.0
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        for torso in ("bf16", "fp16"):
            _run_models(torso)
            torch.cuda.synchronize()
            t1 = time.time()
            _run_pool_head_classifiers(torso)
            torch.cuda.synchronize()
            heads_s += time.time() - t1
    _FILLS.clear()
    torch.cuda.synchronize()
    print(f"\nrecorded {sum(rec.counts.values())} calls ({rec.counts}), {len(rec.records)} distinct, in {time.time() - t0:.0f} s "
          f"({heads_s:.1f} s of it the adaptive / spatial / spatial_v2 classifiers)")
    return rec


# ------------------------------------------------------------------ coverage guard
def test_recorded_launches_cover_every_known_family(recorded):
    fams = set()
    for r in recorded.records:
        fams |= lr.families(r)
    for kind in ("bf16", "f16"):
        have = sorted(f for k, f in fams if k == kind)
        print(f"{kind}: {len([r for r in recorded.records if r[1] == kind])} distinct launches; families {have}")
        print(f"{kind}: launch symbols called: {sorted(s for s, k in recorded.census if k == kind)}")
        print(f"{kind}: distinct launches per new kind: "
              f"{ {op: sum(1 for r in recorded.records if r[0] == op and r[1] == kind) for op in lr.NEW_KINDS + lr.EMBED_KINDS} }")
    missing = lr.missing_families(recorded.records)
    assert not missing, f"the models no longer reach (or the recorder missed) {missing}"
    # every kind of record is replayed below: a new kind must get a restatement, not be dropped
    assert {r[0] for r in recorded.records} <= REPLAYED, {r[0] for r in recorded.records} - REPLAYED
    # the census: every launch symbol the models called is accounted for, and one that is replayed here left a record
    assert {s for s, _ in recorded.census} <= set(lr.SYMBOL_COVERAGE), {s for s, _ in recorded.census} - set(lr.SYMBOL_COVERAGE)
    gaps = lr.coverage_gaps(recorded.census, recorded.records, REPLAYED)
    assert not gaps, gaps
    here = sorted({s for s, _ in recorded.census if lr.SYMBOL_COVERAGE[s][0] != "elsewhere"})
    print(f"census: {len({s for s, _ in recorded.census})} launch symbols called, {len(here)} replayed here: {here}")


REPLAYED = lr.REPLAYED


# ------------------------------------------------------------------ conv replay
def _conv_operands(ops, d, T, seed, g=None):
    return gd.conv_operands(ops, d, T, seed, DEV, g)


def _launch_conv(lib, orig, d, t, packed, w32p, out, g=None):
    return gd.launch_conv(lib, orig, d, t, packed, w32p, out, g or gd.Guarded(DEV, guard_inputs=False))


def _replay_conv(ops, orig, rec, seed):
    """One recorded launch again: the output, the fused statistics and the split-K workspace are guarded carves (NaN inside,
    sentinels around); the full-size inputs stay plain tensors."""
    from autodiffusion_amd import _lib
    d = lr.record_dict(rec)
    T = lr.KIND_DTYPE[rec[1]]
    lib = _lib.load(rec[1])
    g = gd.Guarded(DEV, guard_inputs=False)
    t, packed, w32p, out = _conv_operands(ops, d, T, seed, g)
    stats = _launch_conv(lib, orig, d, t, packed, w32p, out, g)
    g.check()
    return gd.compare_conv(d, T, t, out, stats, seed, rec)


def _label(rec):
    d = lr.record_dict(rec)
    flags = [f for f in ("in1", "res", "aff_a", "fold0", "out_stats", "w_packed32") if d["has_" + f]]
    return (f"{rec[1]} v{d['variant']} n{d['n']} {d['h']}x{d['w']} {d['c0']}+{d['c1']}->{d['cout']} taps{d['taps']} pro{d['prologue']} "
            f"om{d['out_mode']} sc{d['out_scale']:g} ks{d['ksplit']} up{d['up_phase']} iu{d['in_up']} ru{d['res_up']} gg{d['geglu']} "
            + ",".join(flags))


def test_conv_launches_match_float64(ops, recorded):
    t0 = time.time()
    convs = sorted(r for r in recorded.records if r[0] == "conv")
    assert convs, "the recorder captured no adm_conv launch"
    fam_worst, fails = {}, []
    for i, rec in enumerate(convs):
        worst, fro = _replay_conv(ops, recorded.orig[rec[1]], rec, 1000 + i)
        u = lr.U[lr.KIND_DTYPE[rec[1]]]
        ok = worst <= 1.0 and fro <= lr.fro_bound(lr.conv_roundings(lr.record_dict(rec)), u)
        print(f"conv {_label(rec)}: worst err/bound {worst:.3f}, fro/u {fro / u:.3f}{'' if ok else '  FAIL'}")
        for f in lr.families(rec):
            fam_worst[f] = max(fam_worst.get(f, 0.0), worst)
        if not ok:
            fails.append((_label(rec), worst, fro / u))
    for k in ("bf16", "f16"):
        print(f"{k}: {sum(1 for r in convs if r[1] == k)} distinct conv launches replayed")
    for f in sorted(fam_worst):
        print(f"worst err/bound {f}: {fam_worst[f]:.3f}")
    print(f"conv replay: {time.time() - t0:.0f} s")
    assert not fails, fails


# ------------------------------------------------------------------ attention replay
def test_attention_launches_match_float64(ops, recorded):
    t0 = time.time()
    recs = sorted(r for r in recorded.records if r[0] in ("attention", "attention_cross"))
    assert recs
    hip = gd.Hip(ops)
    fam_worst, fails = {}, []
    for i, rec in enumerate(recs):
        kind = rec[1]
        T = lr.KIND_DTYPE[kind]
        torch.manual_seed(2000 + i)
        g = gd.Guarded(DEV, guard_inputs=False)   # out and lse: NaN inside, sentinels around; the full-size inputs stay plain
        if rec[0] == "attention":
            _, _, n, t, c3, heads, new_order, want_lse = rec
            qkv = torch.randn(n, t, c3, device=DEV).to(T)
            d, scale = c3 // 3 // heads, (c3 // 3 // heads) ** -0.5
            out = g.out("out", (n, t, c3 // 3), T, gd.margin_rows(c3 // 3))
            lse = g.out("lse", (n, heads, t), torch.float32) if want_lse else None
            if heads == 1 and d == 512:   # ops.attention's rule: the VAE decoder's single 512-wide head
                hip.attention_1h512(qkv, out)
            else:
                hip.attention_lse(qkv, out, lse, heads, d, new_order)
        else:
            _, _, n, tq, qs, rows, kvs, tk, heads, d, scale = rec
            hd = heads * d
            if qs == kvs and rows == tq:    # self-attention over a fused [q | k | v] projection: kv aliases q's storage
                buf = torch.randn(n, tq, qs, device=DEV).to(T)
                q, kv = buf, buf[:, :, hd:]
            else:
                q, kv = torch.randn(n, tq, qs, device=DEV).to(T), torch.randn(n, rows, kvs, device=DEV).to(T)
            out = g.out("out", (n, tq, hd), T, gd.margin_rows(hd))
            hip.attention_cross(q, q.stride(1), kv, kv.stride(1), kv.shape[1], out, n, tq, tk, heads, d, scale)
        torch.cuda.synchronize()
        g.check()
        sel = sorted({0, n - 1, int(torch.randint(0, n, (1,)).item())})
        worst, num, den = 0.0, 0.0, 0.0
        for j in sel:
            if rec[0] == "attention":
                qh, kh, vh = lr.split_qkv(qkv[j:j + 1], heads, new_order)
            else:
                qh = q[j, :, :hd].reshape(tq, heads, d).permute(1, 0, 2)
                kh = kv[j, :tk, :hd].reshape(tk, heads, d).permute(1, 0, 2)
                vh = kv[j, :tk, hd:2 * hd].reshape(tk, heads, d).permute(1, 0, 2)
            ref, bound = lr.attention_restate(qh, kh, vh, scale, T)
            if rec[0] == "attention" and want_lse:   # the log-sum-exp the backward reads
                lref, lb = lr.lse_restate(qh, kh, scale, T)
                worst = max(worst, ((lse[j].double() - lref).abs() / lb).max().item())
            got = out[j].reshape(-1, heads, d).permute(1, 0, 2)
            assert torch.isfinite(got).all(), rec
            err = (got.double() - ref).abs()
            worst = max(worst, (err / bound).max().item())
            num += (err ** 2).sum().item()
            den += (ref ** 2).sum().item()
        fro = (num / den) ** 0.5
        u = lr.U[T]
        ok = worst <= 1.0 and fro <= lr.fro_bound(2, u)
        print(f"{rec}: worst err/bound {worst:.3f}, fro/u {fro / u:.3f}{'' if ok else '  FAIL'}")
        for f in lr.families(rec):
            fam_worst[f] = max(fam_worst.get(f, 0.0), worst)
        if not ok:
            fails.append((rec, worst, fro / u))
    for f in sorted(fam_worst):
        print(f"worst err/bound {f}: {fam_worst[f]:.3f}")
    print(f"attention replay: {len(recs)} launches, {time.time() - t0:.0f} s")
    assert not fails, fails


# ------------------------------------------------------------------ classifier backward and GroupNorm replay
def _report(name, recs, results, fam_worst=None):
    fails = [(r, w) for r, w in zip(recs, results) if not w <= 1.0]
    for r, w in zip(recs, results):
        print(f"{r}: worst err/bound {w:.3f}{'' if w <= 1.0 else '  FAIL'}")
    for k in ("bf16", "f16"):
        ws = [w for r, w in zip(recs, results) if r[1] == k]
        print(f"worst err/bound ('{k}', '{name}'): {max(ws) if ws else float('nan'):.3f} over {len(ws)} launches")
    assert not fails, fails


def test_attention_backward_launches_match_float64(ops, recorded):
    recs = sorted(r for r in recorded.records if r[0] == "attention_bwd")
    assert recs
    hip = gd.Hip(ops)
    results = []
    for i, rec in enumerate(recs):
        _, kind, n, t, c3, heads, new_order = rec
        T = lr.KIND_DTYPE[kind]
        d = c3 // 3 // heads
        scale = d ** -0.5
        torch.manual_seed(3000 + i)
        qkv = torch.randn(n, t, c3, device=DEV).to(T)
        g = gd.Guarded(DEV, guard_inputs=False)
        out = g.out("out", (n, t, c3 // 3), T, gd.margin_rows(c3 // 3))
        lse = g.out("lse", (n, heads, t), torch.float32)
        hip.attention_lse(qkv, out, lse, heads, d, new_order)
        dout = torch.randn(n, t, c3 // 3, device=DEV).to(T)
        delta = g.out("delta_ws", (n, heads, t), torch.float32)
        dqkv = g.out("dqkv", (n, t, c3), T, gd.margin_rows(c3))
        hip.attention_bwd(qkv, out, dout, lse, delta, dqkv, heads, d, new_order)
        torch.cuda.synchronize()
        g.check()
        worst = 0.0
        for j in sorted({0, n - 1, int(torch.randint(0, n, (1,)).item())}):
            qh, kh, vh = lr.split_qkv(qkv[j:j + 1], heads, new_order)
            oh = out[j].reshape(t, heads, d).permute(1, 0, 2)
            doh = dout[j].reshape(t, heads, d).permute(1, 0, 2)
            refs, bounds = lr.attention_bwd_restate(qh, kh, vh, oh, doh, scale, T)
            gots = lr.split_qkv(dqkv[j:j + 1], heads, new_order)
            for g, r, b in zip(gots, refs, bounds):
                assert torch.isfinite(g).all(), rec
                worst = max(worst, ((g.double() - r).abs() / b).max().item())
        results.append(worst)
    _report("attention_bwd", recs, results)


def test_groupnorm_backward_launches_match_float64(ops, recorded):
    recs = sorted(r for r in recorded.records if r[0] == "gn_bwd")
    assert recs
    hip = gd.Hip(ops)
    results = []
    for i, rec in enumerate(recs):
        _, kind, n, h, w, c, silu, dy_half, has_add, add_half, has_partial, has_norm_add = rec
        T = lr.KIND_DTYPE[kind]
        torch.manual_seed(4000 + i)
        x = torch.randn(n, h, w, c, device=DEV).to(T)
        e = 0.3 * torch.randn(n, c, device=DEV) if has_norm_add else None
        _, mean, rstd = lr.gn_affine_restate(x, torch.ones(c, device=DEV), torch.zeros(c, device=DEV), 1e-5, add=e)
        stats = torch.stack([mean, rstd], -1).float()
        a, b = 1 + 0.2 * torch.randn(n, c, device=DEV), 0.2 * torch.randn(n, c, device=DEV)
        hs, ws_ = (h // 2, w // 2)
        dy = torch.randn(n, hs if dy_half else h, ws_ if dy_half else w, c, device=DEV).to(T)
        add = torch.randn(n, hs if add_half else h, ws_ if add_half else w, c, device=DEV).to(T) if has_add else None
        partial = None
        if has_partial:   # dy is the producing conv's dz, with its (sum dz, sum dz x) slab sums: one slab, summed in float64
            dzd = dy.double()
            partial = torch.stack([dzd.sum((1, 2)), (dzd * x.double()).sum((1, 2))], -1)[:, None].float().contiguous()
        g = gd.Guarded(DEV, guard_inputs=False)   # partial, k1 / k0 and dx: NaN inside, sentinels around
        slabs = 1 if has_partial else max(1, h * w // ops.GN_BWD_SLAB_PIXELS)
        if not has_partial:
            partial = g.out("partial", (n, slabs, c, 2), torch.float32)
        k1, k0 = g.out("k1", (n, c), torch.float32), g.out("k0", (n, c), torch.float32)
        got = g.out("dx", (n, h, w, c), T, gd.margin_rows(c))
        # with the producing conv's sums (has_partial) dy is its dz: no partial pass, the SiLU derivative is already inside
        hip.gn_backward(x, dy, a, b, stats, e, add, partial, k1, k0, got, silu and not has_partial, dy_half, add_half, slabs,
                        partial_given=has_partial)
        torch.cuda.synchronize()
        g.check()
        ref, bound = lr.gn_bwd_restate(x, dy, a, b, stats, silu and not has_partial, dy_half, add, add_half, e, T)
        assert torch.isfinite(got).all(), rec
        results.append(((got.double() - ref).abs() / bound).max().item())
    _report("gn_bwd", recs, results)


def _gn_affine_guarded(hip, g, ops, x0, gamma, beta, x1, film, film_stride, want_stats, eps, add):
    """ops.gn_affine's three paths on the library symbols, with every output carved from g -> (a, b[, stats])."""
    n, h, w, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[3]
    c, hw, T, f32 = c0 + c1, h * w, x0.dtype, torch.float32
    a, b = g.out("aff_a", (n, c), f32), g.out("aff_b", (n, c), f32)
    stats = g.out("stats", (n, 32, 2), f32) if want_stats else None
    fused0 = getattr(x0, "_adm_stats", None)
    fused1 = getattr(x1, "_adm_stats", None) if x1 is not None else None
    p = gd._p

    def partial_of(src1):
        slabs = ops.gn_slabs(hw)
        part = g.out("partial", (n, slabs, c, 2), f32)
        hip.call(T, "adm_gn_partial", p(x0), c0, p(src1), 0 if src1 is None else c1, p(part), n, hw, slabs)
        return part, slabs
    if add is not None:
        part, slabs = fused0 if fused0 is not None else partial_of(None)
        hip.call(T, "adm_gn_finalize_add", p(part), p(gamma), p(beta), p(add), add.stride(0), p(a), p(b), p(stats), n, c, hw, slabs, eps)
    elif fused0 is not None and (x1 is None or fused1 is not None):
        p1, s1 = fused1 if fused1 is not None else (None, 0)
        hip.call(T, "adm_gn_finalize2", p(fused0[0]), c0, fused0[1], p(p1), c1, s1, p(gamma), p(beta), p(film), film_stride, p(a), p(b),
                 p(stats), n, hw, eps)
    else:
        part, slabs = partial_of(x1)
        hip.call(T, "adm_gn_finalize", p(part), p(gamma), p(beta), p(film), film_stride, p(a), p(b), p(stats), n, c, hw, slabs, eps)
    return (a, b, stats) if want_stats else (a, b)


def test_groupnorm_affine_launches_match_float64(ops, recorded):
    recs = sorted(r for r in recorded.records if r[0] == "gn_affine")
    assert recs
    hip = gd.Hip(ops)
    results = []
    for i, rec in enumerate(recs):
        _, kind, n, h, w, c0, c1, has_film, has_add, fused, want_stats, eps = rec
        T = lr.KIND_DTYPE[kind]
        c = c0 + c1
        torch.manual_seed(5000 + i)

        def src(ch):
            if fused:   # a tensor that carries its producing conv's fused statistics (1x1 or 3x3: whichever offers them here)
                xin = torch.randn(n, h, w, 32, device=DEV).to(T)
                for taps in (1, 9):
                    wt = torch.randn(ch, 32, *((3, 3) if taps == 9 else ()), device=DEV) * (32 * taps) ** -0.5
                    y = ops.conv(xin, ops.pack_conv_weight(wt, T), 0.3 * torch.randn(ch, device=DEV), ch, taps, want_stats=True)
                    if getattr(y, "_adm_stats", None) is not None:
                        return y
                raise AssertionError(f"no conv offers fused statistics for {rec}")
            return (0.3 + torch.randn(n, h, w, ch, device=DEV)).to(T)
        x0 = src(c0)
        x1 = src(c1) if c1 else None
        gamma, beta = 1 + 0.2 * torch.randn(c, device=DEV), 0.2 * torch.randn(c, device=DEV)
        film = 0.3 * torch.randn(n, 2 * c, device=DEV) if has_film else None
        add = 0.3 * torch.randn(n, c, device=DEV) if has_add else None
        g = gd.Guarded(DEV, guard_inputs=False)   # partial, a / b and the kept statistics: NaN inside, sentinels around
        res = _gn_affine_guarded(hip, g, ops, x0, gamma, beta, x1, film, 2 * c if has_film else 0, want_stats, eps, add)
        torch.cuda.synchronize()
        g.check()
        x = x0 if x1 is None else torch.cat([x0, x1], 3)
        y, mean, rstd = lr.gn_affine_restate(x, gamma, beta, eps, film=film, add=add)
        got = res[0].double()[:, None, None, :] * x.double() + res[1].double()[:, None, None, :]
        worst = ((got - y).abs() / (lr.U[T] / 8 * (1 + y.abs()))).max().item()
        if want_stats:   # (mean, rstd) kept for the backward: fp32 values of the float64 statistics
            st = res[2].double()
            worst = max(worst, ((st[..., 0] - mean).abs() / (2.0 ** -20 * (mean.abs() + 1 / rstd))).max().item(),
                        ((st[..., 1] - rstd).abs() / (2.0 ** -20 * rstd)).max().item())
        results.append(worst)
    _report("gn_affine", recs, results)


# ------------------------------------------------------------------ token, resample, layout, VAE entry / exit, stride-2 conv
SEEDS = {k: 6000 + 1000 * i for i, k in enumerate(lr.NEW_KINDS + lr.EMBED_KINDS + lr.ENCODER_KINDS)}


def _replay_kind(name, recorded, replay, roundings=1):
    """replay(rec, T, seed) -> (worst err / bound, relative Frobenius error | None, report); bitwise kinds return 0 or inf."""
    t0 = time.time()
    recs = sorted(r for r in recorded.records if r[0] == name)
    assert recs, f"the recorder captured no {name} launch"
    results, fails = [], []
    for i, rec in enumerate(recs):
        T = lr.KIND_DTYPE[rec[1]]
        torch.manual_seed(SEEDS[name] + i)
        worst, fro, report = replay(rec, T, SEEDS[name] + i)
        torch.cuda.synchronize()
        u = lr.U[T]
        ok = worst <= 1.0 and (fro is None or fro <= lr.fro_bound(roundings, u))
        print(f"{rec}: worst err/bound {worst:.3f}" + ("" if fro is None else f", fro/u {fro / u:.3f}") + ("" if ok else f"  FAIL {report}"))
        results.append(worst)
        if not ok:
            fails.append((rec, worst, None if fro is None else fro / u, report))
    for k in ("bf16", "f16"):
        ws = [w for r, w in zip(recs, results) if r[1] == k]
        print(f"worst err/bound ('{k}', '{name}'): {max(ws) if ws else float('nan'):.3f} over {len(ws)} distinct launches")
    print(f"{name} replay: {len(results)} launches, {time.time() - t0:.0f} s")
    assert len(results) == len(recs)
    assert not fails, fails


def _bitwise(got, ref, what):
    """0.0 where got and ref hold the same bit patterns, else inf with the count and the first mismatch."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[got.element_size()]
    bad = got.contiguous().view(view) != ref.contiguous().view(view)
    if not bool(bad.any()):
        return 0.0, ""
    j = int(bad.flatten().nonzero()[0])
    return float("inf"), f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at flat index {j}: got {got.flatten()[j].item()!r} ref {ref.flatten()[j].item()!r}"


def _rows_limit(rec, numel):
    if numel > lr.BIG:
        raise NotImplementedError(f"the row-wise comparison does not subsample: {rec} has {numel} elements")


def _gamma_beta(c):
    return 1 + 0.2 * torch.randn(c, device=DEV), 0.1 * torch.randn(c, device=DEV)


def test_layernorm_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):
        _, _, rows, c, eps = rec
        _rows_limit(rec, rows * c)
        x = (torch.randn(rows, c, device=DEV) * 2 + 0.5).to(T)
        gamma, beta = _gamma_beta(c)
        got = ops.layernorm(x, gamma, beta, eps)
        ref, bound = lr.layernorm_restate(x, gamma, beta, eps, T)
        w, e2, r2, rep = lr.worst_ratio(got, ref, bound)
        return w, (e2 / r2) ** 0.5, rep
    _replay_kind("layernorm", recorded, replay)


def test_layernorm_f32out_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):
        _, _, n, t, pitch, c, eps = rec
        _rows_limit(rec, n * t * c)
        x = (torch.randn(n, pitch, c, device=DEV) * 3 + 0.5).to(T)
        x[:, t:] = float("nan")   # the pad rows are never read
        gamma, beta = _gamma_beta(c)
        got = ops.layernorm_f32out(x, t, gamma, beta, eps)
        assert got.shape == (n, t, c) and got.dtype == torch.float32
        ref, bound = lr.layernorm_restate(x[:, :t], gamma, beta, eps, T, f32out=True)
        w, _, _, rep = lr.worst_ratio(got, ref, bound)
        return w, None, rep
    _replay_kind("layernorm_f32out", recorded, replay)


def test_geglu_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):
        _, _, rows, inner = rec
        _rows_limit(rec, rows * inner)
        u = (torch.randn(rows, 2 * inner, device=DEV) * 1.5).to(T)
        got = ops.geglu(u)
        ref, bound = lr.geglu_restate(u, T)
        w, e2, r2, rep = lr.worst_ratio(got, ref, bound)
        return w, (e2 / r2) ** 0.5, rep
    _replay_kind("geglu", recorded, replay)


def test_quick_gelu_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):
        _, _, rows, inner = rec
        _rows_limit(rec, rows * inner)
        u = torch.randn(rows, inner, device=DEV) * 4.0    # the fc1 outputs reach about +-12
        u.view(-1)[:8] = torch.tensor(lr.QUICK_GELU_SPECIALS, device=DEV)
        u = u.to(T)
        got = ops.quick_gelu(u)
        ref, bound = lr.quick_gelu_restate(u, T)
        w, e2, r2, rep = lr.worst_ratio(got, ref, bound)
        return w, (e2 / r2) ** 0.5, rep
    _replay_kind("quick_gelu", recorded, replay)


SENTINEL = gd.SENTINEL


def _causal_launch(qkv, heads, t, guard=4096):
    """adm_attention_causal on a sentinel-filled `out` with a sentinel-filled guard behind it -> out [n, pitch, C]; the rows >= t
    and the guard must keep the sentinel."""
    from autodiffusion_amd import _lib
    n, pitch, c3 = qkv.shape
    c = c3 // 3
    lib = _lib.load(lr.kind_of(qkv))
    buf = torch.full((n * pitch * c + guard,), SENTINEL, dtype=qkv.dtype, device=qkv.device)
    _lib.check(lib.adm_attention_causal(qkv.data_ptr(), buf.data_ptr(), n, t, pitch, heads, 64, torch.cuda.current_stream().cuda_stream),
               "adm_attention_causal (replay)")
    torch.cuda.synchronize()
    out = buf[:n * pitch * c].view(n, pitch, c)
    assert bool((buf[n * pitch * c:] == SENTINEL).all()), "the guard behind out was written"
    assert bool((out[:, t:] == SENTINEL).all()), "out rows >= t were written"
    return out


def _causal_compare(qkv, out, heads, t, T, images):
    worst, num, den, report = 0.0, 0.0, 0.0, ""
    c = heads * 64
    for j in images:
        q, k, v = (qkv[j, :t, i * c:(i + 1) * c].reshape(t, heads, 64).permute(1, 0, 2) for i in range(3))
        ref, bound = lr.attention_restate(q, k, v, 0.125, T, causal=True)
        got = out[j, :t].reshape(t, heads, 64).permute(1, 0, 2)
        w, e2, r2, rep = lr.worst_ratio(got, ref, bound)
        if w > worst:
            worst, report = w, f"prompt {j} (head, row, channel) {rep}"
        num, den = num + e2, den + r2
    return worst, (num / den) ** 0.5, report


def _causal_qkv(n, t, pitch, heads, T):
    qkv = torch.full((n, pitch, 3 * heads * 64), float("nan"), device=DEV)   # rows >= t are never read
    qkv[:, :t] = torch.randn(n, t, 3 * heads * 64, device=DEV)
    return qkv.to(T)


def test_attention_causal_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):
        _, _, n, t, pitch, heads = rec
        qkv = _causal_qkv(n, t, pitch, heads, T)
        out = _causal_launch(qkv, heads, t)
        return _causal_compare(qkv, out, heads, t, T, sorted({0, n - 1, int(torch.randint(0, n, (1,)).item())}))
    _replay_kind("attention_causal", recorded, replay, roundings=2)


def test_clip_embed_launches_are_bit_exact(ops, recorded):
    def replay(rec, T, seed):
        _, _, n, t, pitch, c, vocab, positions = rec
        tok, pos = torch.randn(vocab, c, device=DEV), 0.3 * torch.randn(positions, c, device=DEV)
        ids = torch.randint(0, vocab, (n, t), device=DEV)
        ids[0, 0], ids[-1, -1] = 0, vocab - 1
        got = ops.clip_embed(ids, tok, pos, pitch, T)
        w, rep = _bitwise(got, lr.clip_embed_restate(ids, tok, pos, pitch, T), "clip_embed")
        return w, None, rep
    _replay_kind("clip_embed", recorded, replay)


def test_resample_launches_match_float64(ops, recorded):
    names = {v: k for k, v in lr.RESAMPLE_MODES.items()}

    def replay(rec, T, seed):
        _, _, n, h, w, c, mode, has_aff = rec
        x = torch.randn(n, h, w, c, device=DEV).to(T)
        aff = (1 + 0.2 * torch.randn(n, c, device=DEV), 0.2 * torch.randn(n, c, device=DEV)) if has_aff else None
        got = ops.resample(x, names[mode], aff)
        torch.cuda.synchronize()
        worst, num, den, report = 0.0, 0.0, 0.0, ""
        for j in lr.compared_images(n, max(x.numel(), got.numel()), seed):
            ref, bound = lr.resample_restate(x[j:j + 1], mode, None if aff is None else (aff[0][j:j + 1], aff[1][j:j + 1]), T)
            if bound is None:   # a copy: bitwise
                wj, rep = _bitwise(got[j:j + 1], ref.to(T), f"image {j}")
            else:
                wj, e2, r2, rep = lr.worst_ratio(got[j:j + 1], ref, bound)
                num, den = num + e2, den + r2
            if wj > worst:
                worst, report = wj, f"image {j} {rep}"
        return worst, ((num / den) ** 0.5 if den else None), report
    _replay_kind("resample", recorded, replay)


def test_nchw_to_nhwc_pad_launches_are_bit_exact(ops, recorded):
    def replay(rec, T, seed):
        _, _, n, c, h, w, cpad = rec
        x = torch.randn(n, c, h, w, device=DEV) * 1.5
        got = ops.nchw_to_nhwc_pad(x, cpad, T)
        worst, report = 0.0, ""
        for j in lr.compared_images(n, got.numel(), seed):
            wj, rep = _bitwise(got[j:j + 1], lr.nchw_to_nhwc_pad_restate(x[j:j + 1], cpad, T), f"image {j}")
            if wj > worst:
                worst, report = wj, rep
        return worst, None, report
    _replay_kind("nchw_to_nhwc_pad", recorded, replay)


def test_vae_latent_in_launches_match_float64(ops, recorded):
    import numpy as np
    inv = float(np.float32(1.0 / 0.18215))   # LatentDiffusion's 1 / scale_factor, as the kernel receives it

    def replay(rec, T, seed):
        _, _, n, zc, e, h, w = rec
        z = torch.randn(n, e, h, w, device=DEV) * 4 * 0.18215
        wt, b = torch.randn(zc, e, 1, 1, device=DEV) * 0.5, torch.randn(zc, device=DEV) * 0.1
        got = ops.vae_latent_in(z, wt, b, inv, T)
        assert got.shape == (n, h, w, 32)
        if bool((got[..., zc:] != 0).any()):
            return float("inf"), None, "a pad channel is not zero"
        ref, bound = lr.vae_latent_in_restate(z, wt, b, inv, T)
        wst, e2, r2, rep = lr.worst_ratio(got[..., :zc], ref, bound)
        return wst, (e2 / r2) ** 0.5, rep
    _replay_kind("vae_latent_in", recorded, replay)


def test_vae_image_out_launches_are_bit_exact(ops, recorded):
    def replay(rec, T, seed):
        _, _, n, h, w, want_unit, want_u8 = rec
        x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed)) * 1.2
        x.view(-1)[:len(lr.IMAGE_OUT_SPECIALS)] = torch.tensor(lr.IMAGE_OUT_SPECIALS)
        x.view(-1)[-len(lr.IMAGE_OUT_SPECIALS):] = torch.tensor(lr.IMAGE_OUT_SPECIALS)
        unit_ref, u8_ref = lr.vae_image_out_restate(x)   # on the host, as tests/test_hip_sd_vae.py::test_image_out_is_bit_exact
        unit, u8 = ops.vae_image_out(x.to(DEV), want_unit=want_unit, want_u8=want_u8)
        if (unit is None) != (not want_unit) or (u8 is None) != (not want_u8):
            return float("inf"), None, "the outputs asked for were not returned"
        worst, report = 0.0, ""
        for got, ref, what in ((unit, unit_ref, "unit"), (u8, u8_ref, "u8")):
            if got is not None:
                wj, rep = _bitwise(got.cpu(), ref.contiguous(), what)
                if wj > worst:
                    worst, report = wj, rep
        return worst, None, report
    _replay_kind("vae_image_out", recorded, replay)


def test_stride2_conv2d_launches_match_float64(ops, recorded):
    """The UNets' stride-2 convs on adm_conv2d, at shapes the Inception replay never sees: inception_replay's own restatement,
    bound and comparison."""
    import inception_replay as ir

    def replay(rec, T, seed):
        worst, fro, report = ir.replay_conv(ops, rec, seed, DEV)
        print(f"  conv2d {ir.conv_label(rec)}")
        return worst, fro, report
    _replay_kind("conv2d", recorded, replay)


# ------------------------------------------------------------------ fp16 range
@pytest.mark.parametrize("case", ["one pass 3x3", "split-K 3x3", "resident 1x1", "fp32 NCHW head"])
def test_fp16_conv_outputs_beyond_the_range_become_signed_inf(ops, case):
    """Weights scaled so that some outputs pass 65504: an element whose float64 reference (minus its bound) is beyond 65520 (where
    round-to-nearest overflows) must be +-inf with the reference's sign; one whose reference (plus its bound) is below 65504 must be
    finite and within its bound; none may be NaN (the reference's fp16-torso behaviour).  The fp32 NCHW head has no 16-bit output:
    every element must be finite and within its bound."""
    T = torch.float16
    n, hw, cin, cout, taps, ks, om = {"one pass 3x3": (2, 16, 128, 192, 9, 1, 0), "split-K 3x3": (2, 16, 256, 128, 9, 2, 0),
                                      "resident 1x1": (2, 16, 256, 384, 1, 1, 0), "fp32 NCHW head": (2, 32, 128, 6, 9, 1, 1)}[case]
    torch.manual_seed(11)
    k = 3 if taps == 9 else 1
    x = torch.randn(n, hw, hw, cin, device=DEV).to(T)
    w32 = torch.randn(cout, cin, k, k, device=DEV) * (cin * taps) ** -0.5 * 40000.0
    bias = 0.1 * torch.randn(cout, device=DEV)
    out = ops.conv(x, ops.pack_conv_weight(w32, T), bias, cout, taps, out_f32_nchw=bool(om), ksplit=ks, variant=10 if taps == 1 else 0)
    torch.cuda.synchronize()
    d = dict(taps=taps, prologue=0, out_mode=om, ksplit=ks, up_phase=0, in_up=0, res_up=0, geglu=0, out_scale=0.0, has_fold0=False,
             has_res=False)
    img, oy, ox = lr.sample_pixels(n, hw, hw, 3)
    ref, bound = lr.conv_restate(d, T, {"x0": x, "x1": None, "w": lr.round_t(w32, T), "bias": bias}, img, oy, ox)
    got = (out.permute(0, 2, 3, 1) if om else out)[img.to(DEV), oy.to(DEV), ox.to(DEV)].double()
    assert not torch.isnan(got).any()
    over = (ref.abs() - bound) > 65520.0
    inside = (ref.abs() + bound) < 65504.0
    n_over = int(over.sum())
    print(f"fp16 range {case}: {n_over} of {ref.numel()} sampled outputs beyond the range, max |ref| {ref.abs().max().item():.4g}")
    if om:
        assert torch.isfinite(got).all() and ((got - ref).abs() <= bound).all()
        assert ref.abs().max().item() > 65504.0
        return
    assert n_over > 0
    assert torch.isinf(got[over]).all() and torch.equal(torch.sign(got[over]), torch.sign(ref[over]))
    assert torch.isfinite(got[inside]).all() and ((got[inside] - ref[inside]).abs() <= bound[inside]).all()


# ------------------------------------------------------------------ GroupNorm at a large mean
RATIOS = (0, 4, 16, 64, 256)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_groupnorm_statistics_at_a_large_mean(ops, dtype):
    """gn_affine against a float64 GroupNorm of the same 16-bit tensor at |mean| / std in RATIOS, from conv-fused statistics (plain and
    `add` = x + embedding) and from adm_gn_partial.  Bound on the normalised output y = (x - mean) rstd: u / 8 (1 + |y|) -- well below
    the rounding to T that the consuming conv's prologue applies next.  Must hold up to a ratio of 16; the largest passing ratio is
    printed."""
    n, hw, cin, c = 2, 32, 64, 128
    u = lr.U[dtype]
    torch.manual_seed(7)
    x_in = torch.randn(n, hw, hw, cin, device=DEV).to(dtype)
    wp = ops.pack_conv_weight(torch.randn(c, cin, device=DEV) * cin ** -0.5, dtype)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    passing = {}
    for form in ("fused", "fused_add", "partial"):
        best = None
        for r in RATIOS:
            if form == "fused_add":
                x = ops.conv(x_in, wp, torch.zeros(c, device=DEV), c, 1, want_stats=True)
                e = r + 0.1 * torch.randn(n, c, device=DEV)
                a, b = ops.gn_affine(x, gamma, beta, add=e)
                xe = x.double() + e.double()[:, None, None, :]
            else:
                x = ops.conv(x_in, wp, torch.full((c,), float(r), device=DEV), c, 1, want_stats=True)
                if form == "partial":
                    x = x.clone()           # no fused statistics: the adm_gn_partial pass
                assert (getattr(x, "_adm_stats", None) is not None) == (form == "fused")
                a, b = ops.gn_affine(x, gamma, beta)
                xe = x.double()
            g = xe.reshape(n, hw * hw, 32, c // 32)
            mean = g.mean((1, 3), keepdim=True)
            var = ((g - mean) ** 2).mean((1, 3), keepdim=True)
            y = ((g - mean) / torch.sqrt(var + 1e-5)).reshape(n, hw, hw, c)
            got = a.double()[:, None, None, :] * x.double() + b.double()[:, None, None, :]
            ratio = (((got - y).abs()) / (u / 8 * (1 + y.abs()))).max().item()
            print(f"GroupNorm {dtype} {form} |mean|/std {r}: worst err/bound {ratio:.3f}")
            if ratio <= 1.0 and (best is None or best == RATIOS[RATIOS.index(r) - 1]):
                best = r
        passing[form] = best
    print(f"GroupNorm {dtype}: largest |mean|/std within the bound: {passing}")
    assert all(v is not None and v >= 16 for v in passing.values()), passing


# ------------------------------------------------------------------ LayerNorm at a large mean
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layernorm_at_a_large_mean(ops, dtype):
    """adm_layernorm and adm_layernorm_f32out against the float64 LayerNorm of the same 16-bit rows at |mean| / std in RATIOS, within
    launch_replay's LayerNorm bound: c = 320 and 768, 64 rows.  Must hold up to a ratio of 16, what GroupNorm is held to above; the
    largest passing ratio is printed."""
    rows = 64
    passing = {}
    torch.manual_seed(9)
    for c in (320, 768):
        gamma, beta = _gamma_beta(c)
        for form in ("layernorm", "layernorm_f32out"):
            best = None
            for r in RATIOS:
                x = (torch.randn(rows, c, device=DEV) + r).to(dtype)
                if form == "layernorm":
                    got = ops.layernorm(x, gamma, beta, 1e-5)
                else:
                    got = ops.layernorm_f32out(x.view(2, rows // 2, c), rows // 2, gamma, beta, 1e-5).view(rows, c)
                ref, bound = lr.layernorm_restate(x, gamma, beta, 1e-5, dtype, f32out=form != "layernorm")
                ratio, _, _, rep = lr.worst_ratio(got, ref, bound)
                print(f"LayerNorm {dtype} {form} c {c} |mean|/std {r}: worst err/bound {ratio:.3f}" + ("" if ratio <= 1.0 else f"  ({rep})"))
                if ratio <= 1.0 and (best is None or best == RATIOS[RATIOS.index(r) - 1]):
                    best = r
            passing[(form, c)] = best
    print(f"LayerNorm {dtype}: largest |mean|/std within the bound: {passing}")
    assert all(v is not None and v >= 16 for v in passing.values()), passing


# ------------------------------------------------------------------ causal attention at the tile edges of its schedule
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t", [1, 16, 17, 32, 33, 77, 192, 193, 256])
def test_attention_causal_at_tile_edges(ops, t, dtype):
    """The 16-query and 32-key tile boundaries and the LDS size switch above T = 192: 2 heads, 2 prompts, every element against the
    causal restatement; nothing beyond row t - 1 is written."""
    n, heads = 2, 2
    torch.manual_seed(100 + t)
    qkv = _causal_qkv(n, t, t, heads, dtype)
    out = _causal_launch(qkv, heads, t)
    worst, fro, report = _causal_compare(qkv, out, heads, t, dtype, range(n))
    u = lr.U[dtype]
    print(f"attention_causal T {t} {dtype}: worst err/bound {worst:.3f}, fro/u {fro / u:.3f}")
    assert worst <= 1.0 and fro <= lr.fro_bound(2, u), (worst, fro / u, report)


# ------------------------------------------------------------------ classifier heads, loss gradient, gradient add
GUARD = gd.GUARD
_owned, _guard_ok = gd.owned, gd.guard_ok   # (carve, view): the carve answers data_ptr() with the view's


def _call(kind, name, *args):
    from autodiffusion_amd import _lib
    _lib.check(getattr(_lib.load(kind), name)(*args, torch.cuda.current_stream().cuda_stream), name + " (replay)")
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


def _fro(e2, r2):
    return (e2 / r2) ** 0.5 if r2 > 0 else None


def _affine(n, c):
    return 1 + 0.2 * torch.randn(n, c, device=DEV), 0.2 * torch.randn(n, c, device=DEV)


def _check_pool_prep(n, hw, c, tpad, T):
    h = torch.randn(n, hw, c, device=DEV).to(T)
    a, b = _affine(n, c)
    t = hw + 1
    pos = torch.randn(c, t, device=DEV) * c ** -0.5 + 0.01 * torch.arange(c * t, device=DEV).reshape(c, t) / (c * t)   # distinct
    buf, tok = _owned((n, tpad, c), T)
    _call(lr.KIND_OF_DTYPE[T], "adm_pool_prep", _p(h), _p(a), _p(b), _p(pos), _p(buf), n, hw, c, tpad)
    _guard_ok(buf, "adm_pool_prep")
    ref, bound = lr.pool_prep_restate(h, a, b, pos, tpad, T)
    w, e2, r2, rep = lr.worst_ratio(tok[:, :t], ref, bound)
    if bool(tok[:, t:].contiguous().view(torch.int16).any()):
        return float("inf"), None, "a pad row of tok is not zero"
    return w, _fro(e2, r2), rep


def _pool_qkv(n, t, tpad, heads, d, T, qk=1.0):
    qkv = torch.full((n, tpad, 3 * heads * d), float("nan"), device=DEV)   # the rows >= t are never read
    qkv[:, :t] = torch.randn(n, t, 3 * heads * d, device=DEV)
    qkv[:, :t, :2 * heads * d] *= qk
    return qkv.to(T)


def _launch_pool_fwd(qkv, t, heads):
    n, tpad, c3 = qkv.shape
    c = c3 // 3
    ba, a0 = _owned((n, c), torch.float32)
    bw, wts = _owned((n, heads, tpad), torch.float32)
    _call(lr.kind_of(qkv), "adm_pool_attn_fwd", _p(qkv), _p(ba), _p(bw), n, t, tpad, heads, c // heads)
    _guard_ok(ba, "adm_pool_attn_fwd a0")
    _guard_ok(bw, "adm_pool_attn_fwd wts")
    return a0, wts


def _check_pool_attn_fwd(n, t, tpad, heads, d, T, qk=1.0):
    qkv = _pool_qkv(n, t, tpad, heads, d, T, qk)
    a0, wts = _launch_pool_fwd(qkv, t, heads)
    (w, a), (bw, ba) = lr.pool_attn_fwd_restate(qkv, t, heads)
    r1, _, _, rep1 = lr.worst_ratio(wts[..., :t], w, bw)
    r2, _, _, rep2 = lr.worst_ratio(a0, a, ba)
    if bool(wts[..., t:].contiguous().view(torch.int32).any()):
        return float("inf"), None, "wts[t:tpad] is not zero"
    one = ((wts[..., :t].double().sum(-1) - 1).abs() / bw.sum(-1)).max().item()     # the weights sum to 1 within their bounds
    q, k, _ = lr.pool_split(qkv, t, heads)
    s = torch.einsum("nhd,nhtd->nht", q, k) * d ** -0.5
    print(f"  pool_attn_fwd logits {s.min().item():.1f} .. {s.max().item():.1f}: weights {r1:.3f}, a0 {r2:.3f}, |sum - 1| {one:.3f} of the bound")
    return max(r1, r2, one), None, f"weights {rep1}; a0 {rep2}"


def _check_pool_attn_bwd(n, t, tpad, heads, d, T, mag):
    qkv = _pool_qkv(n, t, tpad, heads, d, T)
    _, wts = _launch_pool_fwd(qkv, t, heads)
    c = heads * d
    da0 = torch.randn(n, c, device=DEV) * mag
    buf, dqkv = _owned((n, tpad, 3 * c), T)
    _call(lr.kind_of(qkv), "adm_pool_attn_bwd", _p(qkv), _p(wts), _p(da0), _p(buf), n, t, tpad, heads, d)
    _guard_ok(buf, "adm_pool_attn_bwd")
    ref, bound = lr.pool_attn_bwd_restate(qkv, wts, da0, t, heads, T)
    w, _, _, rep = lr.worst_ratio(dqkv[:, :t], ref, bound)
    if not lr.pool_zero_rows_ok(dqkv, t):
        return float("inf"), None, "a pad row or a dQ row above token 0 is not zero"
    under = float(((dqkv[:, :t, c:2 * c] == 0) & (ref[:, :, c:2 * c] != 0)).float().mean())
    print(f"  pool_attn_bwd {T} |da0| {mag:g}: dK elements flushed to zero {under:.2%}")
    if t == 1 and not bool((dqkv[:, 0, :2 * c] == 0).all()):
        return float("inf"), None, "a single key: dQ and dK must be zero"
    return w, None, rep


def _check_pool_prep_bwd(n, hw, c, tpad, T):
    dtok = torch.full((n, tpad, c), float("nan"), device=DEV)               # the rows above hw are never read
    dtok[:, :hw + 1] = torch.randn(n, hw + 1, c, device=DEV)
    dtok = dtok.to(T)
    buf, dact = _owned((n, hw, c), T)
    _call(lr.KIND_OF_DTYPE[T], "adm_pool_prep_bwd", _p(dtok), _p(buf), n, hw, c, tpad)
    _guard_ok(buf, "adm_pool_prep_bwd")
    ref, bound = lr.pool_prep_bwd_restate(dtok, hw, T)
    w, e2, r2, rep = lr.worst_ratio(dact, ref, bound)
    return w, _fro(e2, r2), rep


def _check_channel_mean(n, hw, c, affine, col, cols, T):
    h = torch.randn(n, hw, c, device=DEV).to(T)
    aff = _affine(n, c) if affine else None
    buf, out = _owned((n, cols), torch.float32, SENTINEL)
    out[:, col:col + c] = float("nan")
    _call(lr.KIND_OF_DTYPE[T], "adm_channel_mean", _p(h), _p(aff[0]) if affine else None, _p(aff[1]) if affine else None,
          buf.data_ptr() + 4 * col, cols, n, hw, c)
    _guard_ok(buf, "adm_channel_mean")
    if not (bool((out[:, :col] == SENTINEL).all()) and bool((out[:, col + c:] == SENTINEL).all())):
        return float("inf"), None, "a column outside the window was written"
    ref, bound = lr.channel_mean_restate(h, aff)
    w, _, _, rep = lr.worst_ratio(out[:, col:col + c], ref, bound)
    return w, None, rep


def _check_bcast_add(n, hw, c, with_add, col, vcols, T):
    v = torch.randn(n, vcols, device=DEV)
    scale = 1.0 / hw
    add = torch.randn(n, hw, c, device=DEV).to(T) if with_add else None
    buf, out = _owned((n, hw, c), T)
    _call(lr.KIND_OF_DTYPE[T], "adm_bcast_add", v.data_ptr() + 4 * col, vcols, scale, _p(add), _p(buf), n, hw, c)
    _guard_ok(buf, "adm_bcast_add")
    ref, bound = lr.bcast_add_restate(v[:, col:col + c], scale, add, hw, T)
    if bound is None:
        w, rep = _bitwise(out, ref, "bcast_add without add")
        return w, None, rep
    w, e2, r2, rep = lr.worst_ratio(out, ref, bound)
    return w, _fro(e2, r2), rep


VEC_SPECIALS = (0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e-3, -1.2784645)


def _check_vec_act(items, mode, backward):
    if mode in (3, 4):   # the KL-f8 posterior's log-variance: both clamp edges from both sides, far outside, the zeros
        x, specials = torch.randn(items, device=DEV) * 12, lr.GAUSS_SPECIALS
    else:
        x, specials = torch.randn(items, device=DEV) * 3, VEC_SPECIALS
    k = min(items, len(specials))
    x[:k] = torch.tensor(specials[:k], device=DEV)
    dy = torch.randn(items, device=DEV) if backward else None
    buf, out = _owned((items,), torch.float32)
    _call("bf16", "adm_vec_act", _p(x), _p(dy), _p(buf), items, mode)
    _guard_ok(buf, "adm_vec_act")
    if bool(torch.isnan(out).any()):
        return float("inf"), None, "NaN in the output"
    ref, bound = lr.vec_act_restate(x, mode, dy)
    if mode == 4:       # the clamped log-variance: bitwise, -0 stays -0
        w, rep = _bitwise(out, ref, "gauss_logvar")
        return w, None, rep
    if bound is None:   # ReLU: equal as values, ReLU'(0) = 0
        bad = out.double() != ref
        return (float("inf"), None, f"{int(bad.sum())} elements differ") if bool(bad.any()) else (0.0, None, "")
    w, _, _, rep = lr.worst_ratio(out, ref, bound)
    return w, None, rep


def _vec_rows(n, c, offset=0.0, std=1.0):
    return torch.randn(n, c, device=DEV) * std + offset, 1 + 0.2 * torch.randn(c, device=DEV), 0.1 * torch.randn(c, device=DEV)


def _launch_vec_gn(x, gamma, beta, eps):
    n, c = x.shape
    by, y = _owned((n, c), torch.float32)
    bs, st = _owned((n, 32, 2), torch.float32)
    _call("bf16", "adm_vec_gn", _p(x), _p(gamma), _p(beta), _p(by), _p(bs), n, c, eps)
    _guard_ok(by, "adm_vec_gn y")
    _guard_ok(bs, "adm_vec_gn stats")
    return y, st


def _check_vec_gn(n, c, eps, offset=0.0, std=1.0):
    x, gamma, beta = _vec_rows(n, c, offset, std)
    y, st = _launch_vec_gn(x, gamma, beta, eps)
    (ry, rm, rr), (by, bm, br) = lr.vec_gn_restate(x, gamma, beta, eps)
    res = [lr.worst_ratio(g, r, b) for g, r, b in ((y, ry, by), (st[..., 0], rm, bm), (st[..., 1], rr, br))]
    if c == 32 and not torch.equal(y, beta[None].expand(n, -1)):
        return float("inf"), None, "one value per group: y must be beta exactly"
    return max(r[0] for r in res), None, "; ".join(r[3] for r in res)


def _check_vec_gn_bwd(n, c, offset=0.0, std=1.0):
    x, gamma, beta = _vec_rows(n, c, offset, std)
    _, st = _launch_vec_gn(x, gamma, beta, 1e-5)
    dz = torch.randn(n, c, device=DEV)
    buf, dx = _owned((n, c), torch.float32)
    _call("bf16", "adm_vec_gn_bwd", _p(x), _p(gamma), _p(st), _p(dz), _p(buf), n, c)
    _guard_ok(buf, "adm_vec_gn_bwd")
    ref, bound = lr.vec_gn_bwd_restate(x, gamma, st, dz)
    if c == 32 and not bool((dx == 0).all()):
        return float("inf"), None, "one value per group: dx must be zero exactly"
    w, _, _, rep = lr.worst_ratio(dx, ref, bound)
    return w, None, rep


def _check_logsoftmax_grad(n, k, scale, spread=False):
    logits = torch.randn(n, k, device=DEV) * 3
    if spread and k > 1:
        logits[-1] = torch.linspace(-1e4, 1e4, k, device=DEV)[torch.randperm(k, device=DEV)]
    y = torch.randint(0, k, (n,), device=DEV)
    y[0], y[-1] = 0, k - 1
    bd, dl = _owned((n, k), torch.float32)
    bl, lp = _owned((n,), torch.float32)
    _call("bf16", "adm_logsoftmax_grad", _p(logits), _p(y), _p(bd), _p(bl), n, k, scale)
    _guard_ok(bd, "adm_logsoftmax_grad dlogits")
    _guard_ok(bl, "adm_logsoftmax_grad logp_sel")
    (rd, rl), (bnd, bnl) = lr.logsoftmax_grad_restate(logits, y, scale)
    torch.testing.assert_close(rl, torch.log_softmax(logits.double(), -1)[torch.arange(n, device=DEV), y], rtol=1e-12, atol=1e-12)
    w1, _, _, rep1 = lr.worst_ratio(dl, rd, bnd)
    w2, _, _, rep2 = lr.worst_ratio(lp, rl, bnl)
    return max(w1, w2), None, f"dlogits {rep1}; logp_sel {rep2}"


def _replay_head(name, recorded, check, roundings=1):
    def replay(rec, T, seed):
        return check(*rec[2:], T) if name in ("pool_prep", "pool_attn_fwd", "pool_prep_bwd", "channel_mean", "bcast_add") else check(*rec[2:])
    _replay_kind(name, recorded, replay, roundings)


def test_pool_prep_launches_match_float64(ops, recorded):
    _replay_head("pool_prep", recorded, _check_pool_prep)


def test_pool_attn_fwd_launches_match_float64(ops, recorded):
    _replay_head("pool_attn_fwd", recorded, _check_pool_attn_fwd)


def test_pool_attn_bwd_launches_match_float64(ops, recorded):
    def replay(rec, T, seed):   # d a0 of the unscaled bf16 network is ~ 1e-3; the fp16 classifier carries it times 2^10
        return _check_pool_attn_bwd(*rec[2:], T, 1e-3 * (1024 if T == torch.float16 else 1))
    _replay_kind("pool_attn_bwd", recorded, replay)


def test_pool_prep_bwd_launches_match_float64(ops, recorded):
    _replay_head("pool_prep_bwd", recorded, _check_pool_prep_bwd)


def test_channel_mean_launches_match_float64(ops, recorded):
    _replay_head("channel_mean", recorded, _check_channel_mean)


def test_bcast_add_launches_match_float64(ops, recorded):
    _replay_head("bcast_add", recorded, _check_bcast_add)


def test_vec_act_launches_match_float64(ops, recorded):
    _replay_head("vec_act", recorded, _check_vec_act)


def test_vec_gn_launches_match_float64(ops, recorded):
    _replay_head("vec_gn", recorded, _check_vec_gn)


def test_vec_gn_bwd_launches_match_float64(ops, recorded):
    _replay_head("vec_gn_bwd", recorded, _check_vec_gn_bwd)


def test_logsoftmax_grad_launches_match_float64(ops, recorded):
    _replay_head("logsoftmax_grad", recorded, _check_logsoftmax_grad)


# ------------------------------------------------------------------ the fp32 embedding path
LABEL_ROWS = 1000


def _check_linear_f32(n, k, o, silu_in, has_bias, has_table, aligned):
    off = 0 if aligned else 1      # as recorded: operands one float into their buffers take the tile kernel
    xb, wb = torch.randn(off + n * k, device=DEV), torch.randn(off + o * k, device=DEV) * k ** -0.5
    x, w = xb[off:].view(n, k), wb[off:].view(o, k)
    bias = 0.1 * torch.randn(o, device=DEV) if has_bias else None
    table = idx = None
    if has_table:
        table = torch.randn(LABEL_ROWS, o, device=DEV)
        idx = torch.randint(0, LABEL_ROWS, (n,), device=DEV)
        idx[0], idx[-1] = 0, LABEL_ROWS - 1
        if n > 2:
            idx[1] = idx[2] = 7          # a repeated row
    buf, out = _owned((n, o), torch.float32)
    _call("bf16", "adm_linear_f32", _p(x), _p(w), _p(bias), _p(table), _p(idx), _p(buf), n, k, o, int(silu_in))
    _guard_ok(buf, "adm_linear_f32")
    ref, bound = lr.linear_restate(x, w, bias, table, idx, silu_in)
    wr, _, _, rep = lr.worst_ratio(out, ref, bound)
    return wr, None, rep


def _check_timestep_embedding(n, dim, max_period):
    t = torch.randint(0, 1000, (n,), device=DEV).float()
    t[0], t[-1] = 0.0, 999.0
    buf, out = _owned((n, dim), torch.float32)
    _call("bf16", "adm_timestep_embedding", _p(t), _p(buf), n, dim, max_period)
    _guard_ok(buf, "adm_timestep_embedding")
    ref, bound = lr.timestep_restate(t, dim, max_period)
    inside = 2 * (dim // 2)
    if bool(out[:, inside:].contiguous().view(torch.int32).any()):
        return float("inf"), None, "the odd column is not +0"
    wr, _, _, rep = lr.worst_ratio(out[:, :inside], ref[:, :inside], bound[:, :inside])
    return wr, None, rep


def test_linear_f32_launches_match_float64(ops, recorded):
    _replay_head("linear_f32", recorded, _check_linear_f32)
    ks = {r[3] for r in recorded.records if r[0] == "linear_f32"}
    assert any(k % 16 == 0 for k in ks) and any(k % 4 == 0 and k % 16 for k in ks), sorted(ks)


def test_timestep_embedding_launches_match_float64(ops, recorded):
    _replay_head("timestep_embedding", recorded, _check_timestep_embedding)


# ------------------------------------------------------------------ the same kernels at the smallest shapes that can still go wrong
TORSOS = [torch.bfloat16, torch.float16]


def _edge(what, res, T=None, roundings=1):
    worst, fro, report = res
    u = lr.U[T] if T is not None else None
    print(f"{what}: worst err/bound {worst:.3f}" + ("" if fro is None or u is None else f", fro/u {fro / u:.3f}"))
    assert worst <= 1.0, (what, worst, report)
    if fro is not None and u is not None:
        assert fro <= lr.fro_bound(roundings, u), (what, fro / u)


POOL_PREP_SHAPES = [(2, 64, 256, 128), (1, 64, 512, 128), (3, 1, 8, 2), (2, 9, 72, 16), (1, 16, 264, 17)]


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("n,hw,c,tpad", POOL_PREP_SHAPES)
def test_pool_prep_at_edges(ops, n, hw, c, tpad, dtype):
    """The channel loop's second trip (c > 256), one pixel, an odd map, no pad row; pos distinct per (channel, token)."""
    torch.manual_seed(200 + hw + c)
    _edge(f"pool_prep {(n, hw, c, tpad)} {dtype}", _check_pool_prep(n, hw, c, tpad, dtype), dtype)


POOL_ATTN_SHAPES = [(2, 4, 64, 65, 128), (1, 8, 64, 65, 128), (3, 1, 32, 1, 64), (2, 2, 64, 64, 64), (1, 3, 32, 130, 192), (2, 1, 8, 17, 24)]


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("n,heads,d,t,tpad", POOL_ATTN_SHAPES)
def test_pool_attn_fwd_at_edges(ops, n, heads, d, t, tpad, dtype):
    """A single key, no pad row, three trips of the 64-lane key loop (the last with two lanes), the smallest d."""
    torch.manual_seed(300 + t + d)
    _edge(f"pool_attn_fwd {(n, heads, d, t, tpad)} {dtype}", _check_pool_attn_fwd(n, t, tpad, heads, d, dtype))


@pytest.mark.parametrize("dtype", TORSOS)
def test_pool_attn_fwd_at_logits_of_sixty(ops, dtype):
    """q and k scaled so that the logits span about +-60: the weights stay finite, within their bound, and sum to 1 within it."""
    torch.manual_seed(360)
    _edge(f"pool_attn_fwd logits +-60 {dtype}", _check_pool_attn_fwd(2, 65, 128, 4, 64, dtype, qk=4.3))


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("mag", [1e-3, 1.024])
@pytest.mark.parametrize("n,heads,d,t,tpad", POOL_ATTN_SHAPES)
def test_pool_attn_bwd_at_edges(ops, n, heads, d, t, tpad, mag, dtype):
    """d a0 at the magnitude of the unscaled bf16 network (1e-3) and times 1024: the bound carries fp16's subnormal spacing, so it
    holds for both; the share of fp16's dK that underflows in the first is printed."""
    torch.manual_seed(400 + t + d)
    _edge(f"pool_attn_bwd {(n, heads, d, t, tpad)} |da0| {mag:g} {dtype}", _check_pool_attn_bwd(n, t, tpad, heads, d, dtype, mag))


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("n,hw,c,tpad", POOL_PREP_SHAPES + [(33, 64, 512, 128)])
def test_pool_prep_bwd_at_edges(ops, n, hw, c, tpad, dtype):
    """The shapes of pool_prep, and 1 081 344 items: past the 4096 x 256 grid."""
    torch.manual_seed(500 + hw + c)
    _edge(f"pool_prep_bwd {(n, hw, c, tpad)} {dtype}", _check_pool_prep_bwd(n, hw, c, tpad, dtype), dtype)


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("n,hw,c", [(3, 64, 96), (2, 1, 8), (2, 9, 40), (2, 63, 200), (1, 4096, 64)])
def test_channel_mean_at_edges(ops, n, hw, c, affine, dtype):
    """Channel counts off the 64-channel block, pixel counts off the four lanes, a 64x64 map; written into a column window."""
    torch.manual_seed(600 + hw + c)
    _edge(f"channel_mean {(n, hw, c)} affine {affine} {dtype}", _check_channel_mean(n, hw, c, affine, 24, c + 56, dtype))


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n,hw,c", [(3, 64, 96), (1, 1, 8), (2, 4100, 1024)])
def test_bcast_add_at_edges(ops, n, hw, c, with_add, dtype):
    """1 049 600 items enter the grid-stride loop; col > 0; without `add` the result is round_T(v scale), bitwise."""
    torch.manual_seed(700 + hw + c)
    _edge(f"bcast_add {(n, hw, c)} add {with_add} {dtype}", _check_bcast_add(n, hw, c, with_add, 16, c + 40, dtype), dtype)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("items", [1, 255, 5 * 2048, 4096 * 256 + 3])
def test_vec_act_at_edges(ops, items, mode, backward):
    """+-0, +-88 and +-104 among the inputs: no NaN, ReLU'(0) = 0; one item, a partial block, past the 4096 x 256 grid."""
    torch.manual_seed(800 + items % 1000)
    _edge(f"vec_act items {items} mode {mode} backward {backward}", _check_vec_act(items, mode, backward))


VEC_GN_SHAPES = [(5, 2048, 0.3, 1.0), (1, 32, 0.3, 1.0), (3, 96, 0.0, 1.0), (2, 288, 0.0, 2.0), (4, 2048, 100.0, 0.1)]


@pytest.mark.parametrize("n,c,offset,std", VEC_GN_SHAPES)
def test_vec_gn_at_edges(ops, n, c, offset, std):
    """One value per group (y = beta exactly), a lane's second trip (c = 288), rows of mean 100 and standard deviation 0.1."""
    torch.manual_seed(900 + c)
    _edge(f"vec_gn {(n, c)} mean {offset} std {std}", _check_vec_gn(n, c, 1e-5, offset, std))


@pytest.mark.parametrize("n,c,offset,std", VEC_GN_SHAPES)
def test_vec_gn_bwd_at_edges(ops, n, c, offset, std):
    torch.manual_seed(950 + c)
    _edge(f"vec_gn_bwd {(n, c)} mean {offset} std {std}", _check_vec_gn_bwd(n, c, offset, std))


@pytest.mark.parametrize("scale", [1.0, 2.5, 1024.0])
@pytest.mark.parametrize("n,k", [(5, 1000), (1, 1), (2, 255), (2, 256), (2, 257), (3, 4097)])
def test_logsoftmax_grad_at_edges(ops, n, k, scale):
    """k around the 256 threads of the block, one class, y at 0 and at k - 1, a row of logits spread over +-1e4, the fp16
    classifier's scale; logp_sel against float64 log_softmax."""
    torch.manual_seed(1000 + k)
    _edge(f"logsoftmax_grad {(n, k)} scale {scale:g}", _check_logsoftmax_grad(n, k, scale, spread=True))


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("n,h,w,c,b_half", [(2, 8, 8, 64, 0), (2, 8, 8, 64, 1), (1, 2, 2, 8, 1), (1, 6, 10, 72, 1), (3, 128, 128, 256, 0)])
def test_grad_add_at_edges(ops, n, h, w, c, b_half, dtype):
    """adm_grad_add has no caller in the package: round_T(a + s b) with one fp32 add, at same and half resolution, a non-square
    map, and 1 572 864 items: past the 4096 x 256 grid."""
    torch.manual_seed(1100 + h + c)
    a = torch.randn(n, h, w, c, device=DEV).to(dtype)
    b = torch.randn(n, h // 2 if b_half else h, w // 2 if b_half else w, c, device=DEV).to(dtype)
    buf, out = _owned((n, h, w, c), dtype)
    _call(lr.KIND_OF_DTYPE[dtype], "adm_grad_add", _p(a), _p(b), _p(buf), n, h, w, c, b_half)
    _guard_ok(buf, "adm_grad_add")
    ref, bound = lr.grad_add_restate(a, b, bool(b_half), dtype)
    wst, e2, r2, rep = lr.worst_ratio(out, ref, bound)
    _edge(f"grad_add {(n, h, w, c, b_half)} {dtype}", (wst, _fro(e2, r2), rep), dtype)
    if n == 2:
        assert torch.equal(ops.grad_add(a, b, bool(b_half)), out)      # the ops wrapper reaches the same kernel


@pytest.mark.parametrize("dtype", TORSOS)
@pytest.mark.parametrize("h,w", [(5, 8), (8, 7)])
def test_grad_add_refuses_an_odd_size_at_half_resolution(ops, h, w, dtype):
    """Row h / 2 of an h / 2-row operand lies past its end: refused before the launch."""
    from autodiffusion_amd._lib import AdmError
    a = torch.zeros(1, h, w, 8, device=DEV, dtype=dtype)
    b = torch.zeros(1, (h + 1) // 2, (w + 1) // 2, 8, device=DEV, dtype=dtype)
    with pytest.raises(AdmError, match="odd size"):
        ops.grad_add(a, b, b_half=True)
    assert ops.grad_add(a, a).shape == a.shape
