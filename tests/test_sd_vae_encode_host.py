"""Host-side checks of the Stable-Diffusion first stage's encode half (sd_vae.Encoder, AutoencoderKL(with_encoder=True)), of the
two float64 identities it is built on, of the restatements in tests/f32_vae_kernels.py and of the new modes' argument handling
(no GPU)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_vae_kernels as V
from autodiffusion_amd import _lib, ops
from autodiffusion_amd._lib import AdmError
from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL, Encoder
from oracle.fill import fill_array

from helpers import GOLDEN

TINY = dict(double_z=True, ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3,
            resolution=32, z_channels=4)


# ------------------------------------------------------------------ key table
def test_v1_encoder_parameter_table_matches_the_reference_state_dict():
    enc = json.load(open(os.path.join(GOLDEN, "sd_vae_encoder_keys.json")))
    dec = json.load(open(os.path.join(GOLDEN, "sd_vae_keys.json")))
    assert len(enc) == 106 + 2 and len(dec) == 140
    # autoencoder.py:298-303 registers encoder, decoder, (loss,) quant_conv, post_quant_conv
    want = [(k, s) for k, s in enc.items() if k.startswith("encoder.")] + [(k, s) for k, s in dec.items() if k.startswith("decoder.")] \
        + [(k, s) for k, s in enc.items() if k.startswith("quant_conv.")] + [(k, s) for k, s in dec.items() if k.startswith("post_quant_conv.")]
    assert len(want) == 248
    vae = AutoencoderKL(**SD_V1_VAE, with_encoder=True)
    mine = [(k, list(v.shape)) for k, v in vae.state_dict().items()]
    assert mine == want   # names, shapes and the reference's registration order
    assert sum(int(np.prod(s)) for k, s in enc.items() if k.startswith("encoder.")) == 34_163_592
    assert sum(v.numel() for v in vae.encoder.parameters()) == 34_163_592
    assert enc["quant_conv.weight"] == [8, 8, 1, 1]
    # the default object is what it was
    plain = AutoencoderKL(**SD_V1_VAE)
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == dec and list(plain.state_dict()) == list(dec)
    assert plain.encoder is None
    # FLOPs of one 512 x 512 image from the plan: executed = algorithmic + 3 x the three Downsample convs
    # at their output maps, - the 8 -> 8 quant_conv the fold removes
    p = vae.encoder.plan
    alg, exe = p.flops(512, 512, embed_dim=4), p.flops(512, 512, executed=True, embed_dim=4)
    down = sum(2.0 * (512 >> (i + 1)) ** 2 * c * c * 9 for i, c in enumerate((128, 256, 512)))
    assert exe - alg == pytest.approx(3 * down - 2.0 * 64 * 64 * 8 * 8, rel=1e-12)
    assert alg == pytest.approx(1.11666e12, rel=1e-4) and exe == pytest.approx(1.29060e12, rel=1e-4)


def _filled(vae):
    return {k: torch.from_numpy(fill_array("first_stage_model." + k, tuple(v.shape))) for k, v in vae.state_dict().items()}


def test_autoencoder_state_dict_routing_with_the_encoder():
    vae = AutoencoderKL(TINY, 4, with_encoder=True)
    sd = _filled(vae)
    full = dict(sd)
    full["loss.logvar"] = torch.zeros(())
    full["loss.discriminator.main.0.weight"] = torch.zeros(3)
    vae.load_state_dict(full)   # the training half is still ignored
    got = vae.state_dict()
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    for key in ("encoder.down.1.block.0.nin_shortcut.weight", "encoder.down.0.downsample.conv.bias", "quant_conv.weight"):
        missing = dict(sd)
        del missing[key]
        with pytest.raises(RuntimeError, match=key):
            vae.load_state_dict(missing)
    for key, shape in (("encoder.conv_out.weight", (8, 128, 1, 1)), ("quant_conv.weight", (4, 8, 1, 1))):
        bad = dict(sd)
        bad[key] = torch.zeros(shape)
        with pytest.raises(RuntimeError, match="size mismatch"):
            vae.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="encoder.nope"):
        vae.load_state_dict(dict(sd, **{"encoder.nope": torch.zeros(1)}))
    # the default object ignores the same tensors, of any shape
    plain = AutoencoderKL(TINY, 4)
    plain.load_state_dict(dict({k: v for k, v in sd.items() if k.startswith(("decoder.", "post_quant_conv."))},
                               **{"encoder.conv_in.weight": torch.zeros(3), "quant_conv.weight": torch.zeros(2)}))


# ------------------------------------------------------------------ the two identities, float64 on the CPU
def test_downsample_is_the_pad1_conv_at_the_odd_pixels():
    """model.py:60-79: pad (0, 1, 0, 1), then conv3x3 stride 2 pad 0 == conv3x3 stride 1 pad 1 sampled at [1::2, 1::2]: output (y, x)
    of the first reads rows 2y .. 2y + 2, which are the second's rows around its centre 2y + 1; the centre's lower / right
    neighbour beyond the edge is the zero both paddings supply."""
    g = torch.Generator().manual_seed(1)
    for h, w in ((2, 2), (6, 10), (16, 16)):
        x = torch.randn(2, 5, h, w, generator=g, dtype=torch.float64)
        wt, b = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64), torch.randn(7, generator=g, dtype=torch.float64)
        ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
        got = F.conv2d(x, wt, b, padding=1)[:, :, 1::2, 1::2]
        assert got.shape == ref.shape == (2, 7, h // 2, w // 2)
        assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
        even = F.conv2d(x, wt, b, padding=1)[:, :, ::2, ::2]   # mode 3's pick is another conv
        assert float((even - ref).abs().max()) > 1e-3


def test_quant_conv_folds_into_conv_out():
    g = torch.Generator().manual_seed(2)
    h = torch.randn(2, 32, 8, 8, generator=g, dtype=torch.float64)
    wo, bo = torch.randn(8, 32, 3, 3, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    wq, bq = torch.randn(8, 8, 1, 1, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.conv2d(h, wo, bo, padding=1), wq, bq)
    w2 = torch.einsum("om,mcyx->ocyx", wq[:, :, 0, 0], wo)
    b2 = wq[:, :, 0, 0] @ bo + bq
    got = F.conv2d(h, w2, b2, padding=1)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ------------------------------------------------------------------ restatements: a plain fp32 emulation inside, defects outside
def _worst(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


def _gauss_inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1000, generator=g) * 12
    x[:len(V.GAUSS_SPECIALS)] = torch.tensor(V.GAUSS_SPECIALS)
    return x, torch.randn(1000, generator=g)


def test_gauss_std_restatement_holds_fp32_and_rejects_defects():
    x, dy = _gauss_inputs()
    lv = torch.clamp(x, -30.0, 20.0)
    assert torch.equal(V.gauss_logvar_restate(x), lv)
    assert bool((x < -30).any()) and bool((x > 20).any()) and bool((x == -30).any()) and bool((x == 20).any())
    for d in (None, dy):
        ref, bound = V.gauss_std_restate(x, d)
        mul = 1.0 if d is None else d
        assert _worst(torch.exp(0.5 * lv) * mul, ref, bound) <= 1.0                        # plain fp32
        assert _worst(torch.exp(0.5 * x.clamp(-80, 80)) * mul, ref, bound) > 1e3           # clamp missing
        assert _worst(torch.exp(0.5 * torch.clamp(x, -30.0, 30.0)) * mul, ref, bound) > 1e3   # wrong upper edge
        assert _worst(torch.exp(lv) * mul, ref, bound) > 1e3                               # the 0.5 missing
        assert _worst(torch.exp(0.5 * lv) * mul * (1 + 2.0 ** -17), ref, bound) > 1.0       # 8 times the allowed relative error
    ref, bound = V.gauss_std_restate(x)
    assert float(ref.min()) == pytest.approx(np.exp(-15.0)) and float(ref.max()) == pytest.approx(np.exp(10.0))


def test_axpby_noise_restatement_holds_fp32_and_rejects_defects():
    g = torch.Generator().manual_seed(4)
    x, n = torch.randn(2, 4, 8, 8, generator=g) * 3, torch.randn(2, 4, 8, 8, generator=g)
    for a, b in ((0.9991, 0.0424), (0.0683, 0.9977), (0.18215, 0.18215), (0.18215, 0.0), (1.0, 1.0)):
        a32, b32 = float(np.float32(a)), float(np.float32(b))
        ref, bound = V.axpby_noise_restate(x, a, n, b)
        assert _worst(torch.tensor(a32) * x + torch.tensor(b32) * n, ref, bound) <= 1.0     # plain fp32
        if a != b:
            assert _worst(torch.tensor(b32) * x + torch.tensor(a32) * n, ref, bound) > 1e3   # coefficients swapped
        assert _worst(torch.tensor(a32) * x - torch.tensor(b32) * n, ref, bound) > 1e3 or b == 0.0
    mean, lv = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g) * 2
    for s in (1.0, 0.18215):
        ref, bound = V.posterior_sample_restate(mean, lv, n, s)
        s32 = torch.tensor(float(np.float32(s)))
        assert _worst(s32 * mean + s32 * (n * torch.exp(0.5 * lv)), ref, bound) <= 1.0
        assert _worst(s32 * (mean + n * torch.exp(0.5 * lv)), ref, bound) <= 1.0               # the reference's association, too
        assert _worst(s32 * mean + s32 * (n * torch.exp(lv)), ref, bound) > 1e3


# ------------------------------------------------------------------ refusals
def test_unsupported_encoder_arguments_raise_at_construction():
    for kw in (dict(double_z=False), dict(attn_type="linear"), dict(use_linear_attn=True)):
        with pytest.raises(NotImplementedError):
            Encoder(**dict(TINY, **kw))
    with pytest.raises(NotImplementedError):   # 48 channels: not a multiple of 32
        Encoder(**dict(TINY, ch=48))
    with pytest.raises(NotImplementedError):   # a single head of 288 channels: no kernel of that width
        Encoder(**dict(TINY, ch=96, ch_mult=(1, 3)))
    with pytest.raises(NotImplementedError):   # 2 embed_dim > 16 moment channels
        AutoencoderKL(TINY, 9, with_encoder=True)
    AutoencoderKL(TINY, 9)                       # ... which the decode half alone takes, as before
    with pytest.raises(NotImplementedError):
        AutoencoderKL(TINY, 4).encode(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        AutoencoderKL(dict(TINY, double_z=False), 4, with_encoder=True)


def test_encode_refuses_bad_images_and_cpu_tensors():
    from autodiffusion_amd.sd_sampler import DDIMSampler, LatentDiffusion, axpby_noise
    vae = AutoencoderKL(TINY, 4, with_encoder=True)
    assert vae.encoder.side_multiple == 32
    for shape in ((1, 3, 48, 48), (1, 3, 16, 16), (1, 3, 40, 40)):
        with pytest.raises(AdmError, match="multiple of 32"):
            vae.encode(torch.zeros(shape))
    with pytest.raises(AdmError, match="square"):
        vae.encode(torch.zeros(1, 3, 32, 64))
    # a mid map that the conv kernels cannot tile (12 x 12, 20 x 20: no multiple of 16 and not 8 x 8) is refused by name, before
    # any launch; 8 x 8 and the multiples of 16 pass the shape check (and stop at the host tensor)
    for side in (96, 160):
        with pytest.raises(AdmError, match="mid map does not tile"):
            vae.encode(torch.zeros(1, 3, side, side))
    for side in (32, 64, 128, 192):
        with pytest.raises(AdmError, match="device tensor"):
            vae.encode(torch.zeros(1, 3, side, side))
    v1 = AutoencoderKL(**SD_V1_VAE, with_encoder=True).encoder
    assert v1.side_multiple == 64
    for side, ok in ((64, True), (128, True), (192, False), (256, True), (320, False), (512, True)):
        with pytest.raises(AdmError, match="device tensor" if ok else "24 x 24 mid map|40 x 40 mid map"):
            v1.check_images(torch.zeros(1, 3, side, side))
    with pytest.raises(AdmError, match=r"\[N, 3, H, W\]"):
        vae.encode(torch.zeros(1, 4, 32, 32))
    for fn in (vae.encode, vae.encode_moments, vae.encoder):
        with pytest.raises(AdmError, match="device tensor"):
            fn(torch.zeros(1, 3, 32, 32))
    with pytest.raises(AdmError):
        ops.resample(torch.zeros(1, 2, 2, 32, dtype=torch.bfloat16), "stride2_odd")
    with pytest.raises(AdmError):
        ops.vec_act(torch.zeros(8), "gauss_std")
    with pytest.raises(AdmError):
        axpby_noise(torch.zeros(8), 1.0, torch.zeros(8), 1.0)
    with pytest.raises(AdmError):
        axpby_noise(torch.zeros(8), 1.0, torch.zeros(9), 1.0)
    ld = LatentDiffusion(vae.encoder, first_stage=AutoencoderKL(TINY, 4))
    with pytest.raises(AdmError, match="with_encoder"):
        ld.encode_first_stage(torch.zeros(1, 3, 32, 32))
    s = DDIMSampler(ld)
    s.make_schedule(4, verbose=False)
    with pytest.raises(NotImplementedError):
        s.stochastic_encode(torch.zeros(1, 4, 8, 8), torch.tensor([1]), use_original_steps=True)
    with pytest.raises(NotImplementedError):
        s.decode(torch.zeros(1, 4, 8, 8), None, 2, use_original_steps=True)
    with pytest.raises(IndexError):            # the table has entries 0 .. 3, as the reference's
        s.stochastic_encode(torch.zeros(1, 4, 8, 8), torch.tensor([4]))
    with pytest.raises(NotImplementedError):   # one launch, one pair of coefficients
        s.stochastic_encode(torch.zeros(2, 4, 8, 8), torch.tensor([1, 2]))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_new_modes_refuse_null_pointers(kind):
    lib = _lib.load(kind)
    p = 0x1000   # argument checks run before any pointer is read: host placeholders stand in for device buffers
    calls = {
        "adm_resample": [lambda: lib.adm_resample(None, None, None, p, 1, 2, 2, 32, 5, None),
                         lambda: lib.adm_resample(p, None, None, None, 1, 2, 2, 32, 5, None)],
        "adm_vec_act": [lambda: lib.adm_vec_act(None, None, p, 8, 3, None), lambda: lib.adm_vec_act(p, None, None, 8, 3, None),
                        lambda: lib.adm_vec_act(None, p, p, 8, 3, None), lambda: lib.adm_vec_act(p, None, None, 8, 4, None)],
    }
    for name, fns in calls.items():
        for fn in fns:
            lib.adm_conv(None, None)   # leaves another entry point's text behind
            assert fn() == -1, name    # ADM_E_ARG
            msg = lib.adm_last_error()
            assert name.encode() in msg and b"null" in msg, msg
    assert lib.adm_resample(p, p, None, p, 1, 2, 2, 32, 5, None) == -1     # aff_a / aff_b go together
    assert lib.adm_resample(p, None, None, p, 1, 2, 2, 32, 6, None) == -1  # no mode 6
    assert lib.adm_resample(p, None, None, p, 1, 3, 2, 32, 5, None) == -2  # ADM_E_SHAPE: odd height
    assert lib.adm_vec_act(p, p, p, 8, 4, None) == -1                      # the clamped log-variance takes no dy
    assert lib.adm_vec_act(p, None, p, 8, 5, None) == -1 and lib.adm_vec_act(p, None, p, 0, 3, None) == -1
    assert lib.adm_abi_version() == 10 and _lib.ABI_VERSION == 10
