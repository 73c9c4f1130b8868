"""Host-side checks of the Stable-Diffusion first stage (sd_vae), its C entry points' argument handling, the checkpoint
routing and the SD candidate evaluator's batch / seed plan (no GPU: stub sampler, decoder, extractor and statistics sink)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from autodiffusion_amd import _lib
from autodiffusion_amd._lib import AdmError
from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL, Decoder
from oracle.fill import fill_array

from helpers import GOLDEN

TINY = dict(ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3,
            resolution=32, z_channels=4)


def test_v1_decoder_parameter_table_matches_the_reference_state_dict():
    keys = json.load(open(os.path.join(GOLDEN, "sd_vae_keys.json")))
    assert len(keys) == 138 + 2
    vae = AutoencoderKL(**SD_V1_VAE)
    mine = {k: list(v.shape) for k, v in vae.state_dict().items()}
    assert mine == keys
    assert list(mine) == list(keys)   # the reference's registration order, too
    assert sum(int(np.prod(s)) for k, s in keys.items() if k.startswith("decoder.")) == 49_490_179
    # algorithmic FLOPs of one 64 x 64 latent, from the plan
    assert vae.decoder.plan.flops(64, 64) == pytest.approx(2.5145e12, rel=1e-4)


def test_unsupported_decoder_arguments_raise_at_construction():
    for kw in (dict(attn_type="linear"), dict(use_linear_attn=True), dict(tanh_out=True), dict(give_pre_end=True),
               dict(use_conv_shortcut=True)):
        with pytest.raises(NotImplementedError):
            Decoder(**TINY, **kw)
    with pytest.raises(NotImplementedError):   # a single head of 288 channels: no kernel of that width
        Decoder(**dict(TINY, ch=96, ch_mult=(1, 3)))
    with pytest.raises(NotImplementedError):
        AutoencoderKL(dict(TINY, double_z=True), 4).encode(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_new_entry_points_refuse_null_pointers(kind):
    lib = _lib.load(kind)
    p = 0x1000   # argument checks run before any pointer is read: host placeholders stand in for device buffers
    calls = {
        "adm_attention_1h512": [lambda: lib.adm_attention_1h512(None, p, 1, 64, None), lambda: lib.adm_attention_1h512(p, None, 1, 64, None)],
        "adm_vae_latent_in": [lambda: lib.adm_vae_latent_in(None, p, p, 1.0, p, 1, 4, 4, 8, 8, None),
                              lambda: lib.adm_vae_latent_in(p, None, p, 1.0, p, 1, 4, 4, 8, 8, None),
                              lambda: lib.adm_vae_latent_in(p, p, None, 1.0, p, 1, 4, 4, 8, 8, None),
                              lambda: lib.adm_vae_latent_in(p, p, p, 1.0, None, 1, 4, 4, 8, 8, None)],
        "adm_vae_image_out": [lambda: lib.adm_vae_image_out(None, p, p, 1, 8, 8, None),
                              lambda: lib.adm_vae_image_out(p, None, None, 1, 8, 8, None)],   # at least one output
    }
    for name, fns in calls.items():
        for fn in fns:
            lib.adm_conv(None, None)   # leaves another entry point's text behind
            assert fn() == -1, name    # ADM_E_ARG
            msg = lib.adm_last_error()
            assert name.encode() in msg and b"null" in msg, msg
    with pytest.raises(AdmError):
        _lib.check(-1, "adm_vae_image_out")
    assert lib.adm_attention_1h512(p, p, 0, 64, None) == -1 and lib.adm_attention_1h512(p, p, 1, 0, None) == -1
    assert lib.adm_vae_latent_in(p, p, p, 1.0, p, 1, 33, 4, 8, 8, None) == -2   # ADM_E_SHAPE: more than 32 channels
    assert lib.adm_abi_version() == 10


def _filled_vae_sd(vae, prefix=""):
    return {prefix + k: torch.from_numpy(fill_array("first_stage_model." + k, tuple(v.shape))) for k, v in vae.state_dict().items()}


def test_autoencoder_state_dict_routing():
    vae = AutoencoderKL(TINY, 4)
    sd = _filled_vae_sd(vae)
    full = dict(sd)
    full.update({"encoder.conv_in.weight": torch.zeros(3), "quant_conv.weight": torch.zeros(2), "loss.logvar": torch.zeros(())})
    vae.load_state_dict(full)   # the training half of a first-stage checkpoint is ignored
    got = vae.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    missing = dict(sd)
    del missing["decoder.mid.attn_1.q.weight"]
    with pytest.raises(RuntimeError, match="decoder.mid.attn_1.q.weight"):
        vae.load_state_dict(missing)
    bad = dict(sd)
    bad["decoder.conv_out.weight"] = torch.zeros(3, 32, 1, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):
        vae.load_state_dict(bad)
    nopq = {k: v for k, v in sd.items() if not k.startswith("post_quant_conv.")}
    with pytest.raises(RuntimeError, match="post_quant_conv"):
        vae.load_state_dict(nopq)


def test_decode_refuses_cpu_tensors():
    vae = AutoencoderKL(TINY, 4)
    with pytest.raises(AdmError):
        vae.decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(AdmError):
        vae.decoder(torch.zeros(1, 4, 8, 8))
    from autodiffusion_amd import ops
    with pytest.raises(AdmError):
        ops.vae_image_out(torch.zeros(1, 3, 8, 8))
    with pytest.raises(AdmError):
        ops.vae_latent_in(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 1, 1), torch.zeros(4))


def test_latent_diffusion_routes_checkpoint_prefixes(capsys):
    from autodiffusion_amd.sd_sampler import LatentDiffusion

    class Sink:
        device = torch.device("cpu")

        def load_state_dict(self, sd, strict=True):
            self.got = dict(sd)

    unet, vae = Sink(), Sink()
    ld = LatentDiffusion(unet, first_stage=vae, scale_factor=0.5)
    sd = {"model.diffusion_model.out.2.bias": torch.zeros(4), "model.diffusion_model.time_embed.0.weight": torch.zeros(2),
          "first_stage_model.decoder.conv_in.bias": torch.ones(3), "first_stage_model.encoder.conv_in.bias": torch.ones(3),
          "cond_stage_model.transformer.x": torch.zeros(1), "model_ema.decay": torch.zeros(()), "betas": torch.zeros(5),
          "alphas_cumprod": torch.zeros(5)}
    res = ld.load_state_dict(sd)
    assert sorted(unet.got) == ["out.2.bias", "time_embed.0.weight"]
    assert sorted(vae.got) == ["decoder.conv_in.bias", "encoder.conv_in.bias"]
    assert res["model"] == 2 and res["first_stage_model"] == 2
    assert res["ignored"] == {"cond_stage_model": 1, "model_ema": 1, "betas": 1, "alphas_cumprod": 1}
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "load_state_dict" in ln]
    assert len(lines) == 1 and "cond_stage_model (1)" in lines[0] and "model_ema (1)" in lines[0]
    # the defaults keep the latents-only model: no first stage, the v1 scale factor
    plain = LatentDiffusion(Sink())
    assert plain.first_stage_model is None and plain.scale_factor == 0.18215
    with pytest.raises(AdmError):
        plain.decode_first_stage(torch.zeros(1, 4, 8, 8))


# ------------------------------------------------------------------ SDCandidateEvaluator: batch and seed plan on stubs
class _HostStats:
    """Statistics sink with ActivationAccumulator's surface, on the host."""

    def __init__(self):
        self.rows = []

    def add(self, acts):
        self.rows.append(acts.detach().clone().double().numpy())

    def statistics(self, group=None, local=False):
        from autodiffusion_amd.fid import compute_statistics
        return compute_statistics(np.concatenate(self.rows, 0))


class _StubSampler:
    def __init__(self):
        self.calls = []

    def sample(self, **kw):
        self.calls.append(kw)
        x = kw["x_T"]
        return x + 1e-4 * float(np.sum(kw["sampled_timestep"])) + kw["conditioning"].mean(), None


def _stub_evaluator(n_batches, num_samples, n_samples, seed=3):
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    W = torch.from_numpy(np.random.RandomState(0).randn(3 * 8 * 8, 12)).float()
    feats = []

    def features(images):
        assert images.dtype == torch.float32 and images.shape[1:] == (3, 8, 8) and 0 <= float(images.min()) and float(images.max()) <= 1
        feats.append(images.clone())
        return images.reshape(images.shape[0], -1) @ W

    def image_out(x, out):
        out.copy_(torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0))

    model = types.SimpleNamespace(device=torch.device("cpu"), decode_first_stage=lambda z: torch.tanh(z[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.7) * 1.3)
    cond = [(torch.full((n_samples, 2, 4), 0.1 * i), torch.zeros(n_samples, 2, 4)) for i in range(n_batches)]
    sampler = _StubSampler()
    rs = np.random.RandomState(1)
    a = rs.randn(40, 12)
    ev = SDCandidateEvaluator(model, sampler, cond, a.mean(0), np.cov(a, rowvar=False), num_samples, features=features, seed=seed,
                              image_out=image_out, accumulator=_HostStats, device="cpu")
    return ev, sampler, feats, W


def _opt(n_samples, fixed_code=False, scale=7.5):
    return types.SimpleNamespace(n_samples=n_samples, C=4, H=32, W=32, f=8, scale=scale, ddim_eta=0.0, time_step=3, fixed_code=fixed_code)


def test_evaluator_stops_on_strictly_more_samples_and_scores_all_of_them():
    from autodiffusion_amd.fid import calculate_frechet_distance
    from autodiffusion_amd.sd_evaluate import batch_seed, candidate_seed
    cand = [100, 500, 900]
    ev, sampler, feats, W = _stub_evaluator(n_batches=6, num_samples=4, n_samples=2)
    fid = ev.get_cand_fid(cand, _opt(2))
    # 2, 4 (not > 4), 6 -> three batches, all six samples scored
    assert len(sampler.calls) == 3 and ev.last_times["images"] == 6 and sum(f.shape[0] for f in feats) == 6
    seed0 = candidate_seed(3, cand)
    assert ev.last_plan == [(i, batch_seed(seed0, i)) for i in range(3)]
    for i, kw in enumerate(sampler.calls):
        want = torch.randn([2, 4, 4, 4], generator=torch.Generator().manual_seed(batch_seed(seed0, i)))
        assert torch.equal(kw["x_T"], want)
        assert kw["S"] == 3 and kw["batch_size"] == 2 and kw["shape"] == [4, 4, 4] and kw["eta"] == 0.0
        assert kw["unconditional_guidance_scale"] == 7.5 and kw["unconditional_conditioning"] is not None
        assert isinstance(kw["sampled_timestep"], np.ndarray) and kw["sampled_timestep"].tolist() == cand
    assert not torch.equal(sampler.calls[0]["x_T"], sampler.calls[1]["x_T"])
    acts = (torch.cat(feats).reshape(6, -1) @ W).double().numpy()
    want = calculate_frechet_distance(acts.mean(0), np.cov(acts, rowvar=False), ev.ref_stats.mu, ev.ref_stats.sigma)
    assert fid == pytest.approx(want, rel=1e-9)
    assert ev.get_cand_fid(cand, _opt(2)) == fid                 # a candidate's score does not depend on what ran before
    assert ev.get_cand_fid([100, 500, 901], _opt(2)) != fid
    ev2, sampler2, _, _ = _stub_evaluator(n_batches=6, num_samples=3, n_samples=2)
    ev2.get_cand_fid(cand, _opt(2))
    assert len(sampler2.calls) == 2                               # 4 > 3
    ev3, sampler3, _, _ = _stub_evaluator(n_batches=2, num_samples=100, n_samples=2)
    ev3.get_cand_fid(cand, _opt(2, scale=1.0))                    # the conditioning runs out first: what was collected is scored
    assert len(sampler3.calls) == 2 and sampler3.calls[0]["unconditional_conditioning"] is None


def test_evaluator_fixed_code_reuses_one_start_code_per_call():
    from autodiffusion_amd.sd_evaluate import batch_seed, candidate_seed
    ev, sampler, _, _ = _stub_evaluator(n_batches=4, num_samples=4, n_samples=2)
    ev.get_cand_fid([5, 6, 7], _opt(2, fixed_code=True))
    xs = [kw["x_T"] for kw in sampler.calls]
    assert len(xs) == 3 and all(x is xs[0] for x in xs)
    assert torch.equal(xs[0], torch.randn([2, 4, 4, 4], generator=torch.Generator().manual_seed(batch_seed(candidate_seed(3, [5, 6, 7]), 0))))
    assert candidate_seed(3, [5, 6, 7]) == candidate_seed(3, np.array([5, 6, 7])) != candidate_seed(4, [5, 6, 7])


def test_evaluator_feeds_the_extractor_320_images_at_a_time():
    ev, sampler, feats, _ = _stub_evaluator(n_batches=5, num_samples=500, n_samples=200)
    ev.get_cand_fid([1, 2, 3], _opt(200))
    assert len(sampler.calls) == 3 and [f.shape[0] for f in feats] == [320, 280]


def test_default_extractor_refuses_random_inception_weights():
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    net = types.SimpleNamespace(weights_loaded=False)
    args = (types.SimpleNamespace(device=torch.device("cpu")), None, [], np.zeros(4), np.eye(4), 10)
    with pytest.raises(ValueError, match="random weights"):
        SDCandidateEvaluator(*args, inception=net)
    ev = SDCandidateEvaluator(*args, inception=net, allow_random_inception=True)
    assert "RANDOM" in ev.fid_note
    with pytest.raises(ValueError):
        SDCandidateEvaluator(*args)
