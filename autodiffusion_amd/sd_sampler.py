"""Latent-diffusion samplers with a searched timestep list on the HIP path.

Host-side mirror of the reference's ``DDIMSampler`` / ``PLMSSampler`` ("Stable Diffusion"/ldm/models/diffusion/ddim.py:60-203,
plms.py:63-258) as AutoDiffusion drives them (scripts/search_ea.py:528-538): ``sampler.sample(S, batch_size, shape,
conditioning, ..., unconditional_guidance_scale, unconditional_conditioning, eta, x_T, sampled_timestep=cand)`` returning
``(samples, intermediates)``, attribute ``ddpm_num_timesteps``.  ``model`` is anything with the attributes the reference
samplers read from ``LatentDiffusion`` -- ``num_timesteps, betas, alphas_cumprod, alphas_cumprod_prev, device,
apply_model(x, t, c)`` -- e.g. ``LatentDiffusion`` below around the HIP latent UNet (``sd_unet.UNetModel``).

Every update (classifier-free-guidance combine, PLMS multistep blend, pred_x0, x_prev) is ONE ``adm_sd_step`` launch; the
per-step scalars are computed on the host in float32 exactly as the reference's float32 tables hold them.

A model whose output is not eps (``model.parameterization`` "v" -- Stable Diffusion 2.x -- or "x0"; a model without the attribute
predicts eps) goes through the ``_p`` twins of the three fused steps: the guidance combine is applied to the raw
output and the conversion to eps / to the data prediction happens inside the same launch.
"""
from __future__ import annotations

import ctypes as C
import itertools

import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import AdmError, SdStepCoefs, check


_CALL_IDS = itertools.count()  # one id per sample() call in this process: the context key handed to the model


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """The four named beta schedules of ldm/modules/diffusionmodules/util.py:21-43, float64 numpy."""
    grid = lambda lo, hi: np.linspace(lo, hi, n_timestep, dtype=np.float64)  # noqa: E731
    if schedule == "linear":        # linear in sqrt(beta): the latent-diffusion default
        return grid(linear_start ** 0.5, linear_end ** 0.5) ** 2
    if schedule == "sqrt_linear":
        return grid(linear_start, linear_end)
    if schedule == "sqrt":
        return grid(linear_start, linear_end) ** 0.5
    if schedule == "cosine":
        t = np.arange(n_timestep + 1, dtype=np.float64) / n_timestep + cosine_s
        abar = np.cos(t / (1 + cosine_s) * np.pi / 2) ** 2
        abar /= abar[0]
        return np.clip(1 - abar[1:] / abar[:-1], 0, 0.999)
    raise ValueError(f"schedule '{schedule}' unknown.")


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    """util.py:46-63: the fallback grid when no searched list is given.  The reference ROUNDS the stride (it does not
    floor it) and shifts every step by one."""
    if ddim_discr_method == "uniform":
        stride = round(num_ddpm_timesteps / num_ddim_timesteps)
        steps = np.arange(0, num_ddpm_timesteps, stride)
    elif ddim_discr_method == "quad":
        steps = (np.linspace(0, np.sqrt(num_ddpm_timesteps * .8), num_ddim_timesteps) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    return steps + 1


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    """util.py:66-78 on float32 values: (sigmas, alphas, alphas_prev), numpy float32."""
    ac = np.asarray(alphacums, dtype=np.float32)
    steps = [int(t) for t in ddim_timesteps]
    alphas = ac[steps]
    alphas_prev = np.concatenate([ac[:1], ac[steps[:-1]]]).astype(np.float32)
    one = np.float32(1.0)
    sigmas = np.float32(eta) * np.sqrt((one - alphas_prev) / (one - alphas) * (one - alphas / alphas_prev))
    return sigmas.astype(np.float32), alphas, alphas_prev


class LatentDiffusion:
    """The slice of ``ldm.models.diffusion.ddpm.LatentDiffusion`` the samplers use (register_schedule ddpm.py:117-137,
    apply_model with ``conditioning_key: crossattn``): float32 schedule tables and the UNet call."""

    parameterization = "eps"

    def __init__(self, unet, timesteps=1000, beta_schedule="linear", linear_start=0.00085, linear_end=0.0120,
                 cosine_s=8e-3, device=None, first_stage=None, scale_factor=0.18215, cond_stage=None, parameterization="eps"):
        if parameterization not in _lib.PARAMS:
            raise ValueError(f"LatentDiffusion: parameterization {parameterization!r} (one of {sorted(_lib.PARAMS)})")
        self.parameterization = parameterization   # what the UNet's output is: ddpm.py's "eps" / "x0", SD 2.x's "v"
        betas = make_beta_schedule(beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end,
                                   cosine_s=cosine_s)
        ac = np.cumprod(1.0 - betas, axis=0)
        self.num_timesteps = int(timesteps)
        self.device = torch.device(device) if device is not None else getattr(unet, "device", torch.device("cpu"))
        self.betas = torch.tensor(betas, dtype=torch.float32, device=self.device)
        self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32, device=self.device)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32, device=self.device)
        self.model = unet
        self.first_stage_model = first_stage       # sd_vae.AutoencoderKL (None: latents only, as before)
        self.scale_factor = float(scale_factor)
        self.cond_stage_model = cond_stage         # sd_clip.FrozenCLIPEmbedder (None: the caller brings embeddings, as before)

    def get_learned_conditioning(self, c):
        """ddpm.py:551-562, the ``encode`` branch: prompts (list of strings, or an integer tensor of token ids) -> fp32
        [N, T, context_dim] device embeddings."""
        if self.cond_stage_model is None:
            raise AdmError("LatentDiffusion.get_learned_conditioning: constructed without cond_stage= (sd_clip.FrozenCLIPEmbedder)")
        return self.cond_stage_model.encode(c)

    DECODE_CHUNK_64 = 8   # latents per decoder pass at 64 x 64 (peak: two 512 x 512 x 128 16-bit maps + the fp32 image per latent)

    def decode_first_stage(self, z, chunk=None):
        """ddpm.py:706-713 + autoencoder.py:329-332: first_stage_model.decode(z / scale_factor) -> fp32 NCHW images in about
        [-1, 1].  The batch goes through the decoder ``chunk`` latents at a time (default 8 at 64 x 64, scaled by the latent's
        area) so that peak activation memory does not grow with the batch; every kernel's arithmetic per latent is independent
        of the batch it rides in, so the result is bitwise independent of ``chunk``."""
        if self.first_stage_model is None:
            raise AdmError("LatentDiffusion.decode_first_stage: constructed without first_stage= (sd_vae.AutoencoderKL)")
        if not torch.is_tensor(z) or z.dim() != 4:
            raise AdmError("decode_first_stage: expected [N, C, H, W] latents")
        n, _, h, w = z.shape
        if chunk is None:
            chunk = max(1, self.DECODE_CHUNK_64 * 64 * 64 // max(1, h * w))
        chunk = max(1, int(chunk))
        inv_scale = float(np.float32(1.0 / self.scale_factor))
        z = z.to(torch.float32).contiguous()
        if n <= chunk:
            return self.first_stage_model.decode(z, inv_scale)
        out = None
        for i in range(0, n, chunk):
            x = self.first_stage_model.decode(z[i:i + chunk], inv_scale)
            if out is None:
                out = torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            out[i:i + chunk].copy_(x)
        return out

    ENCODE_CHUNK_512 = 8   # images per encoder pass at 512 x 512 (peak: two 512 x 512 x 128 16-bit maps per image, as the decoder's)

    def encode_first_stage(self, x, chunk=None):
        """ddpm.py:826: first_stage_model.encode(x) -> the posterior (sd_vae.DiagonalGaussianPosterior) of fp32 NCHW device images
        in [-1, 1].  The batch goes through the encoder ``chunk`` images at a time (default 8 at 512 x 512, scaled by the image's
        area); every kernel's arithmetic per image is independent of the batch, so the moments are bitwise independent of ``chunk``."""
        from .sd_vae import DiagonalGaussianPosterior
        vae = self.first_stage_model
        if vae is None or getattr(vae, "encoder", None) is None:
            raise AdmError("LatentDiffusion.encode_first_stage: needs first_stage=sd_vae.AutoencoderKL(..., with_encoder=True)")
        if not torch.is_tensor(x) or x.dim() != 4:
            raise AdmError("encode_first_stage: expected [N, C, H, W] images")
        n, _, h, w = x.shape
        if chunk is None:
            chunk = max(1, self.ENCODE_CHUNK_512 * 512 * 512 // max(1, h * w))
        chunk = max(1, int(chunk))
        if n <= chunk:
            return vae.encode(x)
        x = x.to(torch.float32).contiguous()
        out = None
        for i in range(0, n, chunk):
            m = vae.encode_moments(x[i:i + chunk])
            if out is None:
                out = torch.empty((n,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device)
            out[i:i + chunk].copy_(m)
        return DiagonalGaussianPosterior(out)

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """ddpm.py:542-549: scale_factor * z, z the posterior's sample (``noise``: the normal draw to use) or the tensor itself."""
        if hasattr(encoder_posterior, "sample") and hasattr(encoder_posterior, "mode"):
            return encoder_posterior.sample(noise=noise, scale=self.scale_factor)
        if torch.is_tensor(encoder_posterior):
            z = encoder_posterior.to(torch.float32).contiguous()
            return axpby_noise(z, self.scale_factor, z, 0.0)
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:274-277: sqrt(abar_t) x_start + sqrt(1 - abar_t) noise, from the float32 tables; t: one timestep (an int, or a
        tensor whose entries all agree -- one launch has one pair of coefficients)."""
        t = _one_index(t, self.num_timesteps, "q_sample")
        ac = self.alphas_cumprod[t].cpu().numpy().astype(np.float32)
        if noise is None:
            noise = torch.randn_like(x_start)
        return axpby_noise(x_start, np.sqrt(ac), noise, np.sqrt(np.float32(1.0) - ac))

    _ROUTES = (("model.diffusion_model.", "model"), ("first_stage_model.", "first_stage_model"))

    def load_state_dict(self, sd, strict=True):
        """A full latent-diffusion checkpoint's state dict: ``model.diffusion_model.*`` goes to the UNet, ``first_stage_model.*``
        to the first stage and ``cond_stage_model.*`` to the cond stage (each when one was given); everything else
        (``model_ema.*``, the schedule buffers, the stages not given) is not used on this path and is reported in one log line.
        Returns {route: number of tensors}; ``cond_stage_model`` is among the routes only when a cond stage was given."""
        from . import logger
        routes = self._ROUTES + ((("cond_stage_model.", "cond_stage_model"),) if self.cond_stage_model is not None else ())
        parts = {attr: {} for _, attr in routes}
        other = {}
        for k, v in sd.items():
            for prefix, attr in routes:
                if k.startswith(prefix):
                    parts[attr][k[len(prefix):]] = v
                    break
            else:
                head = k.split(".", 1)[0]
                other[head] = other.get(head, 0) + 1
        self.model.load_state_dict(parts["model"], strict=strict)
        if self.first_stage_model is not None:
            self.first_stage_model.load_state_dict(parts["first_stage_model"], strict=strict)
        elif parts["first_stage_model"]:
            other["first_stage_model"] = len(parts["first_stage_model"])
        cond = ""
        if self.cond_stage_model is not None:
            self.cond_stage_model.load_state_dict(parts["cond_stage_model"], strict=strict)
            cond = ", %d cond-stage tensors" % len(parts["cond_stage_model"])
        logger.log("LatentDiffusion.load_state_dict: %d UNet tensors, %d first-stage tensors%s; not used on this path: %s"
                   % (len(parts["model"]), len(parts["first_stage_model"]) if self.first_stage_model is not None else 0, cond,
                      ", ".join(f"{k} ({v})" for k, v in sorted(other.items())) or "none"))
        out = {"model": len(parts["model"]), "first_stage_model": len(parts["first_stage_model"]), "ignored": other}
        if self.cond_stage_model is not None:
            out["cond_stage_model"] = len(parts["cond_stage_model"])
        return out

    def apply_model(self, x_noisy, t, cond, context_key=None, skip_layer=()):
        """skip_layer: the layer ids this evaluation bypasses (sd_unet.UNetModel.forward); forwarded only when there are any, so
        that a UNet without the keyword keeps working."""
        kw = {}
        if context_key is not None and getattr(self.model, "accepts_context_key", False):
            kw["context_key"] = context_key
        if skip_layer is not None and len(skip_layer):
            kw["skip_layer"] = skip_layer
        return self.model(x_noisy, t, context=cond, **kw)

    accepts_context_key = True


def _f32ptr(t, name):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise AdmError(f"{name}: expected a contiguous float32 device tensor (the HIP path has no CPU fallback)")
    return t.data_ptr()


def _param_id(param, who):
    if param not in _lib.PARAMS:
        raise ValueError(f"{who}: param {param!r} (one of {sorted(_lib.PARAMS)})")
    return _lib.PARAMS[param]


def sd_step(x, eps, batch, cfg_scale, weights, hist, a_t, a_prev, sigma, noise=None, want_e=True, param="eps"):
    """One fused update.  eps: model output, [2*batch, ...] (unconditional half first) under guidance, else [batch, ...].
    weights/hist: multistep blend e' = w[0]*e + sum w[k]*hist[k-1].  a_t, a_prev, sigma: float32 scalars.
    param: what the model output is ("eps", "x0", "v"); anything but "eps" goes through adm_sd_step_p, e is eps in every case.
    Returns (x_prev, pred_x0, e)."""
    pid = _param_id(param, "sd_step")
    guided = eps.shape[0] == 2 * batch
    if not guided and eps.shape[0] != batch:
        raise AdmError(f"sd_step: model output batch {eps.shape[0]} is neither {batch} nor {2 * batch}")
    eps = eps.contiguous()
    eu, ec = (eps[:batch], eps[batch:]) if guided else (None, eps)
    x_prev, pred = torch.empty_like(x), torch.empty_like(x)
    e_out = torch.empty_like(x) if want_e else None
    one = np.float32(1.0)
    a_t, a_prev, sigma = np.float32(a_t), np.float32(a_prev), np.float32(sigma)
    co = SdStepCoefs()
    co.cfg_scale = float(cfg_scale)
    w = list(weights) + [0.0] * (4 - len(weights))
    co.w = (C.c_float * 4)(*[float(v) for v in w])
    co.sqrt_one_minus_at = float(np.sqrt(one - a_t))
    co.sqrt_at = float(np.sqrt(a_t))
    co.sqrt_a_prev = float(np.sqrt(a_prev))
    co.dir_coef = float(np.sqrt(one - a_prev - sigma * sigma))
    co.sigma = float(sigma)
    h = list(hist) + [None] * (3 - len(hist))
    args = (_f32ptr(x, "x"), _f32ptr(eu, "eps"), _f32ptr(ec, "eps"), _f32ptr(h[0], "old_eps"), _f32ptr(h[1], "old_eps"),
            _f32ptr(h[2], "old_eps"), _f32ptr(noise, "noise"), x_prev.data_ptr(), pred.data_ptr(),
            None if e_out is None else e_out.data_ptr(), x.numel(), C.byref(co))
    stream = torch.cuda.current_stream().cuda_stream
    if pid == 0:
        check(_lib.load().adm_sd_step(*args, stream), "adm_sd_step")
    else:
        check(_lib.load().adm_sd_step_p(*args, stream, pid), "adm_sd_step_p")
    return x_prev, pred, e_out


def axpby_noise(x, a, noise, b):
    """a * x + b * noise on fp32 device tensors, as one ``adm_sd_step`` launch with its eps terms switched off: sqrt_at = 1,
    sqrt_one_minus_at = 0 and dir_coef = 0 make pred_x0 = x exactly for a finite eps operand (the noise itself stands in), so the
    update is sqrt_a_prev * x + sigma * noise with sqrt_a_prev = a, sigma = b.  q_sample, DDIMSampler.stochastic_encode and the
    posterior's sample (sd_vae.DiagonalGaussianPosterior) are this."""
    if tuple(x.shape) != tuple(noise.shape):
        raise AdmError(f"axpby_noise: x {tuple(x.shape)} vs noise {tuple(noise.shape)}")
    out = torch.empty_like(x)
    co = SdStepCoefs()
    co.cfg_scale = 1.0
    co.w = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    co.sqrt_one_minus_at, co.sqrt_at, co.dir_coef = 0.0, 1.0, 0.0
    co.sqrt_a_prev, co.sigma = float(np.float32(a)), float(np.float32(b))
    npt = _f32ptr(noise, "noise")
    check(_lib.load().adm_sd_step(_f32ptr(x, "x"), None, npt, None, None, None, npt, out.data_ptr(), None, None, x.numel(),
                                  C.byref(co), torch.cuda.current_stream().cuda_stream), "adm_sd_step")
    return out


def masked_blend(img, orig, keep, drop):
    """ddim.py:160 / plms.py:162 ``img_orig * mask + (1. - mask) * img`` for a 0/1 mask, from launches the library has: ``keep`` is
    the mask expanded to the latent's shape, ``drop`` = 1 - keep.  ``vec_act(m, "relu", dy=t)`` is t * [m > 0] (t itself, or a zero)
    and ``axpby_noise(a, 1, b, 1)`` adds the two disjoint halves, so every element is ``orig`` or ``img`` to the bit: a select
    in three launches (four per step with ``q_sample``'s).  Adding the other half's zero turns a selected -0.0 into +0.0, as the
    reference's expression does; every other value, denormals included, keeps its bits."""
    return axpby_noise(ops.vec_act(keep, "relu", dy=orig), 1.0, ops.vec_act(drop, "relu", dy=img), 1.0)


def _one_index(t, size, who):
    """The single index a batch of equal indices (tensor, sequence or int) stands for; it must lie in [0, size)."""
    vals = {int(v) for v in torch.as_tensor(t).reshape(-1).tolist()}
    if len(vals) != 1:
        raise NotImplementedError(f"{who}: per-sample timesteps {sorted(vals)} (one launch has one pair of coefficients)")
    i = vals.pop()
    if not 0 <= i < size:
        raise IndexError(f"{who}: index {i} outside [0, {size})")
    return i


_SIDE_STREAMS = {}  # device -> second HIP stream for the unconditional half of a guided evaluation


class _LatentSampler:
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True, sampled_timestep=None):
        if sampled_timestep is None:
            self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps, verbose)
        else:
            self.ddim_timesteps = sampled_timestep
        ac = self.model.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.alphas_cumprod_host = ac.detach().to(torch.float32).cpu().numpy()
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = make_ddim_sampling_parameters(
            self.alphas_cumprod_host, self.ddim_timesteps, ddim_eta, verbose)
        self.ddim_sqrt_one_minus_alphas = np.sqrt(np.float32(1.0) - self.ddim_alphas)

    @property
    def _param(self):
        """What the model's output is; a model without the attribute (the reference's toy and v1 models) predicts eps."""
        return getattr(self.model, "parameterization", "eps")

    def _unsupported(self, **kw):
        bad = [k for k, v in kw.items() if v]
        if bad:
            raise NotImplementedError(f"{type(self).__name__}: {bad} are not built on the HIP path (unused by search_ea.py)")

    # Classifier-free guidance evaluates the UNet on [uncond | cond] (ddim.py:177-181 concatenates them into one batch of
    # 2N).  At the search's n_samples (6 latents) most launches of that batch under-fill 256 CUs, so the two halves run as
    # two evaluations of N on two HIP streams instead (each stream replays its own captured graph: sd_unet.py keys graphs
    # and conditioning projections by the launching stream) and fill each other's tails.  Bit-identical: every kernel's
    # arithmetic per latent is independent of the batch it rides in.  ADM_SD_SPLIT_GUIDANCE=0 restores the single batch.
    split_guidance = os.environ.get("ADM_SD_SPLIT_GUIDANCE", "1") != "0"

    def _begin(self, c, uc, scale):
        """Per sample() call: the guidance batch [uncond | cond] of the conditioning is built once, and models that
        take a ``context_key`` (LatentDiffusion over the HIP UNet) are told that it stays fixed for the call's steps."""
        self._guided = not (uc is None or scale == 1.)
        self._split = bool(self._guided and self.split_guidance and c.is_cuda and getattr(self.model, "accepts_context_key", False))
        self._c, self._uc = c, uc
        self._c_in = torch.cat([uc, c]) if (self._guided and not self._split) else c
        self._key = ("sample", next(_CALL_IDS)) if getattr(self.model, "accepts_context_key", False) else None

    def _eps(self, x, t, uncond_only=False, skip=None):
        """skip: the layer-skip list of the timestep this evaluation is at -- every UNet call made here carries it (both halves
        of the guidance, split or batched, and the unguided call of a prompt_mask step); handed on only when it holds ids."""
        kw = {"skip_layer": skip} if skip is not None and len(skip) else {}
        if uncond_only:
            # plms.py:164-171: one evaluation of N on the unconditional conditioning, on the CURRENT stream.  sd_unet.py keeps one
            # set of conditioning projections and one graph per shape PER LAUNCHING STREAM, so this call never touches what the
            # side stream holds under the same key (split guidance); it replaces the current stream's projections (the guided
            # step that follows recomputes them) and replays the current stream's own graph, in stream order.
            if self._key is not None:
                return self.model.apply_model(x, t, self._uc, context_key=(self._key, "u"), **kw)
            return self.model.apply_model(x, t, self._uc, **kw)
        if self._guided and self._split:
            cur = torch.cuda.current_stream(x.device)
            side = _SIDE_STREAMS.get(x.device)
            if side is None:
                side = _SIDE_STREAMS[x.device] = torch.cuda.Stream(device=x.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                eu = self.model.apply_model(x, t, self._uc, context_key=(self._key, "u"), **kw)
            ec = self.model.apply_model(x, t, self._c, context_key=(self._key, "c"), **kw)
            cur.wait_stream(side)
            eu.record_stream(cur)
            return torch.cat([eu, ec])
        if self._guided:
            x, t = torch.cat([x] * 2), torch.cat([t] * 2)
        if self._key is not None:
            return self.model.apply_model(x, t, self._c_in, context_key=self._key, **kw)
        return self.model.apply_model(x, t, self._c_in, **kw)

    # ---- per-step layer-skip lists
    _skips = None   # during a sample() call of DDIM / PLMS: one list per entry of ddim_timesteps

    @staticmethod
    def _check_skip_layers(skip_layers, count, who, what):
        """-> None, or `count` lists of ints.  A wrong length raises here, before anything is launched; the UNet checks the ids."""
        if skip_layers is None:
            return None
        lists = [[int(v) for v in sk] for sk in skip_layers]
        if len(lists) != count:
            raise ValueError(f"{who}: skip_layers holds {len(lists)} lists for {count} {what}")
        return lists

    def _skip_at(self, index):
        return None if self._skips is None else self._skips[index]

    def _start(self, shape, x_T):
        device = self.model.betas.device
        if device.type != "cuda":
            raise AdmError("latent samplers: the model's tables are on the CPU (the HIP path has no CPU fallback)")
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        return device, img.contiguous()

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, sampled_timestep=None, prompt_mask=None, skip_layers=None, **kwargs):
        """skip_layers: one list of layer ids per timestep, ``skip_layers[i]`` belonging to ``sampled_timestep[i]`` as passed (it
        travels with its timestep through the sampler's ordering); every UNet evaluation at a timestep bypasses that timestep's
        layers.  None: nothing changes."""
        self._unsupported(quantize_x0=quantize_x0, noise_dropout=noise_dropout > 0., score_corrector=score_corrector is not None)
        if conditioning is not None and not isinstance(conditioning, dict) and conditioning.shape[0] != batch_size:
            print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        C_, H, W = shape
        self._check_mask(mask, x0, (batch_size, C_, H, W))
        if skip_layers is not None and sampled_timestep is not None:
            skip_layers = self._check_skip_layers(skip_layers, len(sampled_timestep), type(self).__name__, "timesteps")
            sampled_timestep, skip_layers = self._order(sampled_timestep, skip_layers)
        else:
            sampled_timestep = self._order(sampled_timestep)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose, sampled_timestep=sampled_timestep)
        self._skips = self._check_skip_layers(skip_layers, len(self.ddim_timesteps), type(self).__name__, "timesteps")
        self._prompt_mask = self._check_prompt_mask(prompt_mask, len(self.ddim_timesteps), unconditional_conditioning)
        self._mask = self._begin_mask(mask, x0, (batch_size, C_, H, W))
        try:
            return self._loop(conditioning, (batch_size, C_, H, W), x_T=x_T, callback=callback, img_callback=img_callback,
                              log_every_t=log_every_t, temperature=temperature,
                              unconditional_guidance_scale=unconditional_guidance_scale,
                              unconditional_conditioning=unconditional_conditioning)
        finally:
            self._mask = self._prompt_mask = self._skips = None

    # ---- masked sampling (ddim.py:157-160, plms.py:159-162): mask 1 keeps x0, 0 is generated
    _mask = None          # (keep, drop, x0) during a masked sample() call
    _prompt_mask = None   # PLMS only: per loop position, 0 = that step runs unguided on the unconditional conditioning

    def _check_mask(self, mask, x0, shape):
        """The host-side checks, before any launch: the layout first, then x0 (the reference asserts it, ddim.py:158)."""
        if mask is None:
            return
        n, c, h, w = shape
        if not (torch.is_tensor(mask) and mask.dim() == 4 and mask.shape[0] in (1, n) and mask.shape[1] in (1, c)
                and tuple(mask.shape[2:]) == (h, w)):
            got = tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__
            raise NotImplementedError(f"{type(self).__name__}: mask {got} is not built on the HIP path; accepted layouts are "
                                      f"[N or 1, C or 1, H, W] for latents {shape}")
        if not torch.is_tensor(x0) or tuple(x0.shape) != tuple(shape):
            got = None if x0 is None else (tuple(x0.shape) if torch.is_tensor(x0) else type(x0).__name__)
            raise AdmError(f"{type(self).__name__}: mask= needs x0= of the latents' shape {shape}, got {got}")

    def _check_prompt_mask(self, prompt_mask, steps, uc):
        return None   # PLMS only (plms.py:85); the reference's other samplers swallow the keyword unread, and so do these

    def _begin_mask(self, mask, x0, shape):
        """Per call: the values are checked on the device (one sync), the mask is expanded to contiguous fp32 ``keep`` and
        ``drop`` = 1 - keep is formed by one launch."""
        if mask is None:
            return None
        device = self.model.betas.device
        if device.type != "cuda":
            raise AdmError("latent samplers: the model's tables are on the CPU (the HIP path has no CPU fallback)")
        m = mask.to(device=device, dtype=torch.float32)
        if not bool(((m == 0) | (m == 1)).all()):
            raise NotImplementedError(f"{type(self).__name__}: soft masks are not built on the HIP path (no fp32 launch multiplies two "
                                      "tensors; the blend is a select): every mask value must be exactly 0 or 1")
        keep = m.expand(shape).contiguous()
        drop = axpby_noise(keep, -1.0, torch.ones_like(keep), 1.0)
        return keep, drop, x0.to(device=device, dtype=torch.float32).contiguous()

    def _blend(self, img, ts):
        """Before the step's model call(s), exactly where the reference blends: the kept region becomes a freshly noised x0."""
        if self._mask is None:
            return img
        keep, drop, x0 = self._mask
        return masked_blend(img, self.model.q_sample(x0, ts), keep, drop)


class DDIMSampler(_LatentSampler):
    def _order(self, sampled_timestep, skip_layers=None):
        """ddim.py:93-94 sorts the list; with skip_layers -> (timesteps, lists), each list moving with its timestep."""
        if skip_layers is None:
            return None if sampled_timestep is None else sorted(int(t) for t in sampled_timestep)
        order = sorted(range(len(sampled_timestep)), key=lambda i: int(sampled_timestep[i]))   # stable, as sorted() on the values
        return [int(sampled_timestep[i]) for i in order], [skip_layers[i] for i in order]

    def _loop(self, cond, shape, x_T, callback, img_callback, log_every_t, temperature, unconditional_guidance_scale,
              unconditional_conditioning):
        device, img = self._start(shape, x_T)
        self._begin(cond, unconditional_conditioning, unconditional_guidance_scale)
        b = shape[0]
        timesteps = np.asarray(self.ddim_timesteps)
        total = timesteps.shape[0]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        for i, step in enumerate(np.flip(timesteps)):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            # ddim.py:157-160.  The reference does not blend again after the last update: the kept region of the RESULT is the
            # model's last update of it, not x0; and x_inter below stays the post-step latent.
            img = self._blend(img, ts)
            eps = self._eps(img, ts, skip=self._skip_at(index))
            sigma = self.ddim_sigmas[index]
            noise = torch.randn(shape, device=device) * temperature if sigma != 0 else None  # ddim.py:198 noise_like
            img, pred_x0, _ = sd_step(img, eps, b, unconditional_guidance_scale, (1.0,), (), self.ddim_alphas[index],
                                      self.ddim_alphas_prev[index], sigma, noise, want_e=False, param=self._param)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates


    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:219-233: sqrt(ddim_alphas[t]) x0 + ddim_sqrt_one_minus_alphas[t] noise -- ``t`` INDEXES the table make_schedule
        built (uniform or ``sampled_timestep``), it is not a timestep."""
        self._unsupported(use_original_steps=use_original_steps)
        t = _one_index(t, len(self.ddim_alphas), "DDIMSampler.stochastic_encode")
        x0 = x0.to(torch.float32).contiguous()
        if noise is None:
            noise = torch.randn_like(x0)
        return axpby_noise(x0, np.sqrt(self.ddim_alphas[t]), noise, self.ddim_sqrt_one_minus_alphas[t])

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, skip_layers=None):
        """ddim.py:235-254: the DDIM updates of ``ddim_timesteps[:t_start]``, downwards, from x_latent.  With the reference's
        conventions a latent from ``stochastic_encode(x0, t)`` carries the noise level of table entry t and is decoded with
        ``t_start = t``, whose first update is entry t - 1's: the off-by-one is the reference's and is kept.
        skip_layers: one list of layer ids per entry of ``ddim_timesteps`` (the table make_schedule built), in the table's order;
        the update of entry i bypasses list i's layers."""
        self._unsupported(use_original_steps=use_original_steps)
        skips = self._check_skip_layers(skip_layers, len(self.ddim_timesteps), "DDIMSampler.decode", "timesteps of the schedule")
        device, img = self._start(tuple(x_latent.shape), x_latent)
        self._begin(cond, unconditional_conditioning, unconditional_guidance_scale)
        b = img.shape[0]
        timesteps = np.asarray(self.ddim_timesteps)[:int(t_start)]
        total = timesteps.shape[0]
        for i, step in enumerate(np.flip(timesteps)):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            eps = self._eps(img, ts, skip=None if skips is None else skips[index])
            sigma = self.ddim_sigmas[index]
            noise = torch.randn(img.shape, device=device) if sigma != 0 else None
            img, _, _ = sd_step(img, eps, b, unconditional_guidance_scale, (1.0,), (), self.ddim_alphas[index],
                                self.ddim_alphas_prev[index], sigma, noise, want_e=False, param=self._param)
        return img


class PLMSSampler(_LatentSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True, sampled_timestep=None):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose, sampled_timestep)

    def _order(self, sampled_timestep, skip_layers=None):
        # plms.py takes the list as given; search_ea.py sorts its candidates (:480)
        return sampled_timestep if skip_layers is None else (sampled_timestep, skip_layers)

    def _check_prompt_mask(self, prompt_mask, steps, uc):
        """plms.py:85,131,164: one entry per loop position i (entry 0 is the first, noisiest step)."""
        if prompt_mask is None:
            return None
        pm = [int(v) for v in prompt_mask]
        if len(pm) != steps:
            raise AdmError(f"PLMSSampler: prompt_mask holds {len(pm)} entries for {steps} steps")
        if uc is None and 0 in pm:
            raise AdmError("PLMSSampler: a prompt_mask entry of 0 needs unconditional_conditioning")
        return pm

    def _plms_second(self, img, x_mid, out2, b, scale, e_t, a_t, a_prev, sigma, t_next, param):
        """The second half of the first step: e' = (e_t + e_next) / 2 applied to img.  Under "v" / "x0" SD 2's plms.py converts the
        second output at the point and time it was evaluated at (x_mid, t_next), not at (img, t): one adm_sd_step_p launch for
        that eps (its x_prev is not used), then the eps blend, already guided, as an unguided adm_sd_step."""
        if param == "eps":
            return sd_step(img, out2, b, scale, (0.5, 0.5), (e_t,), a_t, a_prev, sigma, want_e=False)
        a_next = self.alphas_cumprod_host[t_next]
        _, _, e_next = sd_step(x_mid, out2, b, scale, (1.0,), (), a_next, a_next, 0.0, param=param)
        return sd_step(img, e_next, b, 1.0, (0.5, 0.5), (e_t,), a_t, a_prev, sigma, want_e=False)

    def _loop(self, cond, shape, x_T, callback, img_callback, log_every_t, temperature, unconditional_guidance_scale,
              unconditional_conditioning):
        device, img = self._start(shape, x_T)
        b = shape[0]
        timesteps = np.asarray(self.ddim_timesteps)
        total = timesteps.shape[0]
        time_range = np.flip(timesteps)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        self._begin(cond, uc, scale)
        old_eps, param = [], self._param
        for i, step in enumerate(time_range):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=device, dtype=torch.long)
            a_t, a_prev, sigma = self.ddim_alphas[index], self.ddim_alphas_prev[index], self.ddim_sigmas[index]
            # plms.py:159-162: one blend per loop iteration, before BOTH model calls of the first step (the second one sees the
            # predicted point, unblended).  Not repeated after the last update; x_inter below stays the post-step latent.
            img = self._blend(img, ts)
            # plms.py:164-171: on a prompt_mask entry of 0 every model call of the step is one unguided evaluation on the
            # unconditional conditioning (scale 1), and that eps is what the multistep history keeps
            un = self._prompt_mask is not None and self._prompt_mask[i] == 0
            scale = 1.0 if un else unconditional_guidance_scale
            eps = self._eps(img, ts, un, skip=self._skip_at(index))
            if len(old_eps) == 0:    # pseudo improved Euler (2nd order): a second model call at the predicted point
                x_mid, _, e_t = sd_step(img, eps, b, scale, (1.0,), (), a_t, a_prev, sigma, param=param)
                eps2 = self._eps(x_mid, ts_next, un, skip=self._skip_at(max(index - 1, 0)))   # t_next's own list
                img, pred_x0, _ = self._plms_second(img, x_mid, eps2, b, scale, e_t, a_t, a_prev, sigma, int(ts_next[0]), param)
            else:                    # Adams-Bashforth of order 2 / 3 / 4 over the kept eps history (newest first)
                w = {1: (3 / 2, -1 / 2), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[len(old_eps)]
                img, pred_x0, e_t = sd_step(img, eps, b, scale, w, tuple(reversed(old_eps)), a_t, a_prev, sigma, param=param)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates


# ------------------------------------------------------------------ DPM-Solver++(2M)
class NoiseScheduleVP:
    """The 'discrete' VP schedule of dpm_solver.py:99-156: log(alpha_t) is the piecewise-linear interpolant of
    0.5*log(alphas_cumprod) over t = 1/N .. 1 (linear extrapolation outside, as interpolate_fn :1144-1188)."""

    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None):
        if schedule != "discrete":
            raise NotImplementedError("only the discrete schedule is used by DPMSolverSampler (sampler.py:60)")
        ac = np.asarray(torch.as_tensor(alphas_cumprod).detach().cpu(), dtype=np.float64) if alphas_cumprod is not None \
            else np.cumprod(1.0 - np.asarray(torch.as_tensor(betas).detach().cpu(), dtype=np.float64))
        self.schedule, self.total_N, self.T = schedule, len(ac), 1.0
        self.log_alpha_array = 0.5 * np.log(ac)
        self.t_array = np.linspace(0.0, 1.0, self.total_N + 1)[1:]

    def marginal_log_mean_coeff(self, t: float) -> float:
        k = min(max(int(np.searchsorted(self.t_array, t)), 1), self.total_N - 1)
        x0, x1 = self.t_array[k - 1], self.t_array[k]
        y0, y1 = self.log_alpha_array[k - 1], self.log_alpha_array[k]
        return float(y0 + (t - x0) * (y1 - y0) / (x1 - x0))

    def marginal_alpha(self, t):
        return float(np.exp(self.marginal_log_mean_coeff(t)))

    def marginal_std(self, t):
        return float(np.sqrt(1.0 - np.exp(2.0 * self.marginal_log_mean_coeff(t))))

    def marginal_lambda(self, t):
        lm = self.marginal_log_mean_coeff(t)
        return lm - 0.5 * float(np.log(1.0 - np.exp(2.0 * lm)))


def dpm_step(x, eps, batch, cfg_scale, m_prev, sigma_s, alpha_s, a, b0, b1, param="eps"):
    """One fused multistep update; returns (x_next, m) with m the data prediction at the current point.  param: what the model
    output is ("eps", "x0", "v"); anything but "eps" goes through adm_dpm_step_p."""
    pid = _param_id(param, "dpm_step")
    guided = eps.shape[0] == 2 * batch
    if not guided and eps.shape[0] != batch:
        raise AdmError(f"dpm_step: model output batch {eps.shape[0]} is neither {batch} nor {2 * batch}")
    eps = eps.contiguous()
    eu, ec = (eps[:batch], eps[batch:]) if guided else (None, eps)
    x_next, m = torch.empty_like(x), torch.empty_like(x)
    args = (_f32ptr(x, "x"), _f32ptr(eu, "eps"), _f32ptr(ec, "eps"), _f32ptr(m_prev, "model_prev"), x_next.data_ptr(), m.data_ptr(),
            x.numel(), float(cfg_scale), float(sigma_s), float(alpha_s), float(a), float(b0), float(b1))
    stream = torch.cuda.current_stream().cuda_stream
    if pid == 0:
        check(_lib.load().adm_dpm_step(*args, stream), "adm_dpm_step")
    else:
        check(_lib.load().adm_dpm_step_p(*args, stream, pid), "adm_dpm_step_p")
    return x_next, m


class DPMSolverSampler(_LatentSampler):
    """dpm_solver/sampler.py:5-83: multistep DPM-Solver++ of order 2 in data-prediction form, ``lower_order_final``,
    classifier-free guidance, over K+1 searched time points (``sampled_timestep``: integers index the ascending
    1000-point uniform time grid in the given order; floats are continuous times, sorted descending --
    dpm_solver.py:1079-1091) or the uniform grid when none are given."""

    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        self.alphas_cumprod = model.alphas_cumprod.detach().to(torch.float32)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, sampled_timestep=None, skip_layers=None, **kwargs):
        """skip_layers: one list of layer ids per model evaluation, in the order evaluated: K lists for K + 1 times."""
        if conditioning is not None and not isinstance(conditioning, dict) and conditioning.shape[0] != batch_size:
            print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        C_, H, W = shape
        steps, order = int(S), 2
        assert steps >= order
        skips = self._check_skip_layers(skip_layers, steps, "DPMSolverSampler", "model evaluations")
        device, x = self._start((batch_size, C_, H, W), x_T)
        ns = NoiseScheduleVP('discrete', alphas_cumprod=self.alphas_cumprod)
        if sampled_timestep is None:
            ts = [float(v) for v in np.linspace(ns.T, 1.0 / ns.total_N, steps + 1, dtype=np.float32)]
        else:
            ea = [v.item() if hasattr(v, "item") else v for v in sampled_timestep]
            if max(ea) > 1:
                full = np.linspace(ns.T, 1.0 / ns.total_N, 1000 + 1, dtype=np.float32)[::-1]
                ts = [float(full[int(e)]) for e in ea]
            else:
                ts = [float(np.float32(t)) for t in sorted(ea, reverse=True)]
        assert len(ts) - 1 == steps
        uc, scale = unconditional_conditioning, unconditional_guidance_scale

        self._begin(conditioning, uc, scale)

        def eps_at(x_, t, skip):  # model_wrapper: discrete-time input (t - 1/N) * 1000, guidance batch = [uncond | cond]
            t_in = torch.full((batch_size,), (t - 1.0 / ns.total_N) * 1000.0, device=device, dtype=torch.float32)
            return self._eps(x_, t_in, skip=skip)

        m_prev, lam_prev = None, None
        for step in range(1, steps + 1):
            s, t = ts[step - 1], ts[step]
            if step == 1:
                step_order = 1
            else:
                step_order = min(order, steps + 1 - step) if steps < 15 else order  # lower_order_final
            lam_s, lam_t = ns.marginal_lambda(s), ns.marginal_lambda(t)
            h = lam_t - lam_s
            phi = ns.marginal_alpha(t) * (np.exp(-h) - 1.0)
            a = ns.marginal_std(t) / ns.marginal_std(s)
            if step_order == 2:
                r0 = (lam_s - lam_prev) / h
                b0, b1 = -phi * (1.0 + 0.5 / r0), 0.5 * phi / r0
            else:
                b0, b1 = -phi, 0.0
            x, m = dpm_step(x, eps_at(x, s, None if skips is None else skips[step - 1]), batch_size, scale, m_prev if step_order == 2 else None,
                            ns.marginal_std(s), ns.marginal_alpha(s), a, b0, b1, param=self._param)
            m_prev, lam_prev = m, lam_s
        return x, None


# ------------------------------------------------------------------ UniPC
def unipc_step(x_eval, eps, batch, cfg_scale, x_base, hist, sigma_s, alpha_s, corr=None, pred=None, param="eps"):
    """One model evaluation of UniPC on the latents (adm_unipc_step): m = the guided data prediction at x_eval; corr = (ac, c0, c1,
    c2, c3) asks for x_corr = ac x_base + c0 m + c1 h1 + c2 h2 + c3 h3, pred = (ap, p0, p1, p2) for x_pred = ap x_c + p0 m + p1 h1 +
    p2 h2 with x_c = x_corr (x_eval without corr).  hist: up to three earlier model values, newest first.  param: what the model
    output is ("eps", "x0", "v"); anything but "eps" goes through adm_unipc_step_p.
    -> (m, x_corr | None, x_pred | None)"""
    from ._lib import UnipcArgs
    pid = _param_id(param, "unipc_step")
    guided = eps.shape[0] == 2 * batch
    if not guided and eps.shape[0] != batch:
        raise AdmError(f"unipc_step: model output batch {eps.shape[0]} is neither {batch} nor {2 * batch}")
    eps = eps.contiguous()
    eu, ec = (eps[:batch], eps[batch:]) if guided else (None, eps)
    for name, t in [("x_base", x_base)] + [("history", h) for h in hist]:
        if t is not None and tuple(t.shape) != tuple(x_eval.shape):
            raise AdmError(f"unipc_step: {name} shape {tuple(t.shape)} != {tuple(x_eval.shape)}")
    h = list(hist) + [None] * (3 - len(hist))
    a = UnipcArgs()
    a.x_eval, a.eps_uncond, a.eps_cond = _f32ptr(x_eval, "x"), _f32ptr(eu, "eps"), _f32ptr(ec, "eps")
    a.x_base = _f32ptr(x_base, "x_base") if corr is not None else None
    a.h1, a.h2, a.h3 = (_f32ptr(t, "history") for t in h[:3])
    m = torch.empty_like(x_eval)
    x_corr = torch.empty_like(x_eval) if corr is not None else None
    x_pred = torch.empty_like(x_eval) if pred is not None else None
    a.m_out = m.data_ptr()
    a.x_corr = None if x_corr is None else x_corr.data_ptr()
    a.x_pred = None if x_pred is None else x_pred.data_ptr()
    a.numel, a.cfg_scale, a.sigma_s, a.alpha_s = x_eval.numel(), float(cfg_scale), float(sigma_s), float(alpha_s)
    if corr is not None:
        a.ac, a.c0, a.c1, a.c2, a.c3 = (float(v) for v in corr)
    if pred is not None:
        a.ap, a.p0, a.p1, a.p2 = (float(v) for v in pred)
    if pid == 0:
        check(_lib.load().adm_unipc_step(C.byref(a), torch.cuda.current_stream().cuda_stream, 0), "adm_unipc_step")
    else:
        check(_lib.load().adm_unipc_step_p(C.byref(a), torch.cuda.current_stream().cuda_stream, pid), "adm_unipc_step_p")
    return m, x_corr, x_pred


class UniPCSampler(_LatentSampler):
    """Multistep UniPC (Zhao et al. 2023; unipc.py) in data-prediction form with ``lower_order_final``, over
    ``DPMSolverSampler``'s time points and model input: K + 1 searched times (``sampled_timestep``) or the uniform grid, K
    evaluations, classifier-free guidance.  Evaluation j yields, in one launch, the corrected point at its own time and the
    predicted point at the next; the arrival point is not corrected.  ``order=2, variant="bh2", corrector=False`` is
    DPM-Solver++(2M)."""

    def __init__(self, model, order=2, variant="bh2", corrector=True, **kwargs):
        super().__init__(model, **kwargs)
        self.alphas_cumprod = model.alphas_cumprod.detach().to(torch.float32)
        self.order, self.variant, self.corrector = int(order), variant, bool(corrector)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, sampled_timestep=None, order=None, variant=None, corrector=None, record=None,
               skip_layers=None, **kwargs):
        """skip_layers: one list of layer ids per model evaluation, in the order evaluated: K lists for K + 1 times."""
        from .unipc import plan_evaluations
        skips = self._check_skip_layers(skip_layers, int(S), "UniPCSampler", "model evaluations")
        order = self.order if order is None else int(order)
        variant = self.variant if variant is None else variant
        corrector = self.corrector if corrector is None else bool(corrector)
        if mask is not None or x0 is not None:
            raise NotImplementedError("UniPCSampler: masked sampling is not built (DDIM / PLMS have it)")
        if conditioning is not None and not isinstance(conditioning, dict) and conditioning.shape[0] != batch_size:
            print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        C_, H, W = shape
        device, x = self._start((batch_size, C_, H, W), x_T)
        ns = NoiseScheduleVP('discrete', alphas_cumprod=self.alphas_cumprod)
        steps = int(S)
        if sampled_timestep is None:
            ts = [float(v) for v in np.linspace(ns.T, 1.0 / ns.total_N, steps + 1, dtype=np.float32)]
        else:
            ea = [v.item() if hasattr(v, "item") else v for v in sampled_timestep]
            if max(ea) > 1:
                full = np.linspace(ns.T, 1.0 / ns.total_N, 1000 + 1, dtype=np.float32)[::-1]
                ts = [float(full[int(e)]) for e in ea]
            else:
                ts = [float(np.float32(t)) for t in sorted(ea, reverse=True)]
        assert len(ts) - 1 == steps
        plan = plan_evaluations(ns, ts, order, True, variant, True, corrector)   # float64, raises before anything is launched
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        self._begin(conditioning, uc, scale)
        hist, x_base = [], None      # model values, newest first; the accepted state at the previous time
        for j, e in enumerate(plan):
            t_in = torch.full((batch_size,), (ts[j] - 1.0 / ns.total_N) * 1000.0, device=device, dtype=torch.float32)
            eps = self._eps(x, t_in, skip=None if skips is None else skips[j])
            depth = max(e["corr"][2] if e["corr"] else 0, e["pred"][2] - 1)
            corr = None if e["corr"] is None else (e["corr"][0], *e["corr"][1])
            pred = (e["pred"][0], *e["pred"][1])
            m, x_corr, x_pred = unipc_step(x, eps, batch_size, scale, x_base if corr else None, hist[:depth],
                                           ns.marginal_std(ts[j]), ns.marginal_alpha(ts[j]), corr, pred, param=self._param)
            if record is not None:
                record.append(dict(j=j, t=ts[j], x=x, eps=eps, x_base=x_base if corr else None, hist=list(hist[:depth]), corr=corr,
                                   pred=pred, sigma=ns.marginal_std(ts[j]), alpha=ns.marginal_alpha(ts[j]), m=m, x_corr=x_corr,
                                   x_pred=x_pred))
            hist = ([m] + hist)[:3]
            x_base = x_corr if x_corr is not None else x
            x = x_pred
        return x, None
