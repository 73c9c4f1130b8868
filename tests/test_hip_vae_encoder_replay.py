"""Every (kernel, shape, flags) launch of the KL-f8 VAE encoder, replayed against float64 in both torsos, and the encoder's head
as a composite on both of its routes.

Recording.  AutoencoderKL(**SD_V1_VAE, with_encoder=True), filled from oracle/fill.py as tests/test_hip_launch_replay.py fills the
decoder, runs ``encode(x)`` and ``posterior.sample(noise=...)`` under tests/launch_replay.Recorder in each torso on
  (1, 3, 512, 512)   the shipped shape: the 512^2 / 256^2 / 128^2 conv records, attention at t = 4096, the head's direct route
  (2, 3, 64, 64)     an 8 x 8 mid map: the head's padded route (16 x 16), attention at t = 64
  (1, 3, 192, 192)   a 24 x 24 mid map.  The first run of this file found that no conv kernel tiles such a map (adm_conv: 8 x 8, or
                     a multiple of 16 pixels a side), so ``encode`` failed inside mid.block_1 after half the network had run:
                     Encoder.check_images now refuses the size before the first launch, which the fixture asserts (by the census).
                     What the case was for is recorded all the same: the head (Encoder._head, which does take the map) on a seeded
                     (1, 24, 24, 512) mid map -- padded to 32 x 32, so the padding crosses a 16-pixel tile boundary, not only a map edge.
Each distinct record is then launched again through the same library entry point on fresh seeded operands, with the outputs on
guarded carves (tests/guarded.py), and compared with the float64 restatement of tests/launch_replay.py under the bounds derived
there and fro_bound -- by the replay functions of tests/test_hip_launch_replay.py themselves, handed this file's records; conv
maps above the full-comparison size are sampled by launch_replay.sample_pixels (tile corners of every image plus seeded pixels).
The direct stem (adm_stem_conv3x3, the encoder's conv_in) is the one kind that file does not replay: f32_kernels.stem_restate,
every element.  A coverage guard holds the census against launch_replay.SYMBOL_COVERAGE and asserts the records that make the
encoder's launches its own (the stem, the odd-pixel pick, the Downsample convs, both head routes, the posterior's vector kernels).

The head (Encoder._head) as a composite, on a small Encoder (64 -> 8 channels) and seeded 16-bit mid maps of sides 8, 24 (the
padded route) and 16, 32 (the direct route), every element against launch_replay.head_restate: float64 GroupNorm + SiLU of the
stored map rounded once to T, then the pad-1 3x3 conv of the UNPADDED map -- the same restatement for both routes, so a padded
route that activated its padding, or rounded differently from the conv's prologue, fails along the map's last row and column.
The maps have a mean of launch_replay.HEAD_OFFSET = -4 standard deviations (head_operands says why).  The same again for
``folded_head(wq, bq)`` against quant_conv(conv_out(act)) in float64 from the unfolded fp32 weights, with the fold's terms in the
bound.  The premise of the bound's rounding window -- the kernels' own GroupNorm affine lies within head_window's dz of the
float64 one -- is asserted on the affine ops.gn_affine returns.
"""
import time

import pytest
import torch

import f32_kernels as fk
import guarded as gd
import launch_replay as lr
import test_hip_launch_replay as big

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = ((1, 3, 512, 512), (2, 3, 64, 64))
REFUSED = (1, 3, 192, 192)      # a 24 x 24 mid map: refused by Encoder.check_images
HEAD_ALONE = (1, 24, 24, 512)   # ... whose head is recorded on a seeded mid map
LIBS = ("bf16", "f16")
DOWNSAMPLE_CONVS = ((512, 128), (256, 256), (128, 512))   # (map side, channels) of the three Downsample convs


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import ops as _ops
    return _ops


class _Records:
    """What the replay functions of tests/test_hip_launch_replay.py read of a Recorder: the records (of one library, or of all)
    and the unpatched adm_conv of each library."""

    def __init__(self, rec, kind=None):
        self.records = {r for r in rec.records if kind is None or r[1] == kind}
        self.orig, self.census = rec.orig, rec.census


@pytest.fixture(scope="module")
def recorded(ops):
    from autodiffusion_amd._lib import AdmError
    from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL
    t0 = time.time()
    with pytest.MonkeyPatch.context() as mp:
        rec = lr.Recorder(mp)
        vae = AutoencoderKL(**SD_V1_VAE, with_encoder=True)
        vae.load_state_dict(big._fill("vae_enc", "first_stage_model.", {k: v.shape for k, v in vae.state_dict().items()}))
        for torso in ("bf16", "fp16"):
            vae.set_torso(torso).to(DEV)
            g = torch.Generator().manual_seed(7)
            for shape in INPUTS:
                x = torch.randn(shape, generator=g).clamp_(-1.0, 1.0).to(DEV)
                post = vae.encode(x)
                z = post.sample(noise=torch.randn(post.mean.shape, generator=g).to(DEV))
                assert z.shape == (shape[0], 4, shape[2] // 8, shape[3] // 8) and bool(torch.isfinite(z).all()), (torso, shape)
            before = (set(rec.census), dict(rec.counts))
            with pytest.raises(AdmError, match="24 x 24 mid map does not tile"):
                vae.encode(torch.randn(REFUSED, generator=g).to(DEV))
            assert (rec.census, rec.counts) == before, "a refused image must not reach a launch"
            h = (torch.randn(HEAD_ALONE, generator=g) + lr.HEAD_OFFSET).to(vae.compute_dtype).to(DEV)
            with torch.no_grad():
                mom = vae.encoder._head(vae._enc_head, h)
            assert mom.shape == (1, 8, 24, 24) and bool(torch.isfinite(mom).all()), torso
            torch.cuda.synchronize()
        del vae
    big._FILLS.clear()
    torch.cuda.empty_cache()
    rec_s = time.time() - t0
    print(f"\nencoder: recorded {sum(rec.counts.values())} calls ({rec.counts}), {len(rec.records)} distinct, in {rec_s:.1f} s")
    yield rec
    print(f"\nencoder replay: recording {rec_s:.1f} s, total wall time of the file {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ coverage guard
def test_encoder_launches_are_recorded_and_covered(recorded):
    recs = recorded.records
    kinds = sorted({r[0] for r in recs})
    for lib in LIBS:
        print(f"{lib}: distinct encoder launches per kind: { {k: sum(1 for r in recs if r[0] == k and r[1] == lib) for k in kinds} }")
        print(f"{lib}: launch symbols called: {sorted(s for s, k in recorded.census if k == lib)}")
    called = {s for s, _ in recorded.census}
    assert called <= set(lr.SYMBOL_COVERAGE), called - set(lr.SYMBOL_COVERAGE)
    assert {r[0] for r in recs} <= lr.REPLAYED, {r[0] for r in recs} - lr.REPLAYED
    gaps = lr.coverage_gaps(recorded.census, recs, lr.REPLAYED)
    assert not gaps, gaps
    here = sorted(s for s in called if lr.SYMBOL_COVERAGE[s][0] != "elsewhere")
    print(f"census: {len(called)} launch symbols called, {len(here)} replayed here: {here}")
    assert {"adm_stem_conv3x3", "adm_resample", "adm_vec_act", "adm_conv", "adm_attention_1h512"} <= set(here), here
    # what makes the encoder's launch list its own: a later change that stops reaching one of these must fail here
    convs = {lib: [lr.record_dict(r) for r in recs if r[0] == "conv" and r[1] == lib] for lib in LIBS}
    for lib in LIBS:
        for n, _, side, _ in INPUTS:
            assert ("stem_conv3x3", lib, n, 3, side, side, 128) in recs, (lib, side)
        assert any(r[0] == "resample" and r[1] == lib and r[6] == lr.RESAMPLE_MODES["stride2_odd"] and not r[7] for r in recs), lib
        for side, ch in DOWNSAMPLE_CONVS:
            assert any(d["taps"] == 9 and d["prologue"] == 0 and d["out_mode"] == 0 and (d["h"], d["w"], d["c0"], d["c1"], d["cout"])
                       == (side, side, ch, 0, ch) and not d["has_res"] for d in convs[lib]), (lib, "Downsample conv", side, ch)
        for side in (16, 32):   # the padded head route: no prologue, the 8 x 8 (24 x 24) map in the corner of a 16 x 16 (32 x 32) one
            assert any(d["out_mode"] == 1 and d["prologue"] == 0 and (d["h"], d["w"], d["cout"]) == (side, side, 8)
                       for d in convs[lib]), (lib, "padded head route", side)
        assert any(d["out_mode"] == 1 and d["prologue"] == 2 and (d["h"], d["w"], d["cout"]) == (64, 64, 8) for d in convs[lib]), lib
        # the channel-widening ResnetBlocks' 1x1 nin_shortcut
        for side, cin, cout in ((256, 128, 256), (128, 256, 512)):
            assert any(d["taps"] == 1 and (d["h"], d["c0"], d["cout"]) == (side, cin, cout) for d in convs[lib]), (lib, "nin_shortcut", side)
        assert {r[3] for r in recs if r[0] == "attention" and r[1] == lib} == {4096, 64}, lib
        assert any(r[0] == "gn_affine" and r[1] == lib and r[2:6] == HEAD_ALONE for r in recs), (lib, "norm_out on the 24 x 24 map")
    # the posterior's vector kernels are fp32, launched from the bf16 library whatever the torso
    modes = {(r[3], r[4]) for r in recs if r[0] == "vec_act"}
    assert {(3, False), (3, True), (4, False)} <= modes, modes


# ------------------------------------------------------------------ the replay, on the functions of tests/test_hip_launch_replay.py
@pytest.mark.parametrize("lib", LIBS)
def test_encoder_conv_launches_match_float64(ops, recorded, lib):
    big.test_conv_launches_match_float64(ops, _Records(recorded, lib))


@pytest.mark.parametrize("lib", LIBS)
def test_encoder_attention_launches_match_float64(ops, recorded, lib):
    big.test_attention_launches_match_float64(ops, _Records(recorded, lib))


@pytest.mark.parametrize("lib", LIBS)
def test_encoder_groupnorm_affine_launches_match_float64(ops, recorded, lib):
    big.test_groupnorm_affine_launches_match_float64(ops, _Records(recorded, lib))


def test_encoder_resample_launches_match_float64(ops, recorded):
    big.test_resample_launches_match_float64(ops, _Records(recorded))


def test_encoder_vec_act_launches_match_float64(ops, recorded):
    big.test_vec_act_launches_match_float64(ops, _Records(recorded))


def test_encoder_stem_launches_match_float64(ops, recorded):
    hip = gd.Hip(ops)

    def replay(rec, T, seed):
        _, _, n, cin, h, w, cout = rec
        x, wt, b = (t.to(DEV) for t in fk.stem_inputs(n, cin, h, w, cout, seed))
        g = gd.Guarded(DEV, guard_inputs=False)   # the output: NaN inside, sentinels around
        out = g.out("out", (n, h, w, cout), T, gd.margin_rows(cout))
        hip.call(T, "adm_stem_conv3x3", gd._p(x), gd._p(wt), gd._p(b), gd._p(out), n, cin, h, w, cout)
        g.check()
        ref, bound = lr.stem_restate(x, wt, b, T)
        wr, e2, r2, rep = lr.worst_ratio(out, ref, bound)
        return wr, (e2 / r2) ** 0.5, rep
    big._replay_kind("stem_conv3x3", _Records(recorded), replay)


def test_every_encoder_record_kind_is_replayed_above(recorded):
    """The kinds the encoder records are exactly those the tests above replay: a new kind in the encoder's launch list needs a
    replay here, not only an entry in launch_replay.REPLAYED."""
    assert {r[0] for r in recorded.records} == {"conv", "attention", "gn_affine", "resample", "vec_act", "stem_conv3x3"}


# ------------------------------------------------------------------ the head as a composite
HEAD_ENCODER = dict(ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), in_channels=3, resolution=64, z_channels=4)
HEAD_N, HEAD_C, HEAD_COUT = 2, 64, 8
TORSO_OF = {torch.bfloat16: "bf16", torch.float16: "fp16"}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("side", [8, 24, 16, 32])   # 8, 24: padded to 16, 32; 16, 32: blocks.head with the prologue inside the conv
def test_head_routes_match_float64(ops, side, folded, dtype):
    from autodiffusion_amd.sd_vae import Encoder
    o = lr.head_operands(HEAD_N, side, HEAD_C, HEAD_COUT, dtype, 9000 + side)
    enc = Encoder(**HEAD_ENCODER)
    sd = enc.state_dict()
    assert sd["conv_out.weight"].shape == (HEAD_COUT, HEAD_C, 3, 3) and sd["norm_out.weight"].shape == (HEAD_C,)
    sd.update({"norm_out.weight": o["gamma"], "norm_out.bias": o["beta"], "conv_out.weight": o["w"], "conv_out.bias": o["bias"]})
    enc.load_state_dict(sd)
    enc.set_torso(TORSO_OF[dtype]).to(DEV)
    pr = enc._prepare()
    d = {k: v.to(DEV) for k, v in o.items()}
    hd = enc.folded_head(d["wq"], d["bq"]) if folded else pr.head
    with torch.no_grad():
        got = enc._head(hd, d["h"])
        a, b = ops.gn_affine(d["h"], hd["g"], hd["b"], eps=enc.GN_EPS)
    torch.cuda.synchronize()
    assert got.shape == (HEAD_N, HEAD_COUT, side, side) and got.dtype == torch.float32
    # the premise of the rounding window: the kernels' affine within dz of the float64 GroupNorm
    z, dz = lr.head_window(d["h"], d["gamma"], d["beta"], enc.GN_EPS)
    zk = a.double()[:, None, None, :] * d["h"].double() + b.double()[:, None, None, :]
    premise = ((zk - z).abs() / dz).max().item()
    ref, bound = lr.head_restate(d["h"], d["gamma"], d["beta"], d["w"], d["bias"], enc.GN_EPS, dtype,
                                 d["wq"] if folded else None, d["bq"] if folded else None)
    worst, e2, r2, rep = lr.worst_ratio(got, ref, bound)
    edge = torch.zeros_like(ref, dtype=torch.bool)
    edge[:, :, -1, :] = edge[:, :, :, -1] = True
    err = (got.double() - ref).abs() / bound
    u = lr.U[dtype]
    fro = (e2 / r2) ** 0.5
    print(f"head {'folded ' if folded else ''}{dtype} side {side} ({'padded' if side % 16 else 'direct'} route): worst err/bound {worst:.3f} "
          f"(last row / column {err[edge].max().item():.3f}, inside {err[~edge].max().item():.3f}), fro/u {fro / u:.3f}, "
          f"affine |z_kernel - z| / dz {premise:.3f}")
    assert premise <= 1.0, premise
    assert worst <= 1.0 and fro <= lr.fro_bound(1, u), (worst, fro / u, rep)
