#!/usr/bin/env python3
"""Time the full-size Stable-Diffusion v1 latent UNet (859.5 M parameters, 64x64 latents, 77 x 768 context) on the HIP
path: ms per UNet evaluation, latents/s and model TFLOP/s (803.3 GFLOP per latent per evaluation).
GRAPH=1 replays a captured hipGraph.  BATCH (default 12 = the reference's n_samples 6 with classifier-free guidance), REPS, BREAKDOWN=1 for per-shape conv time.
SAMPLER=ddim|plms|dpm additionally times BASELINE config 4's candidate evaluation: K searched steps (K, default 6),
classifier-free guidance 7.5, N_SAMPLES latents per batch (default 6) -> finished latents/s.
--decode times the first stage instead: `decode_first_stage` of 6 latents of 64 x 64 through the v1 KL-f8 decoder per torso (ms per
latent, model TFLOP/s from the plan's algorithmic FLOPs) and `adm_attention_1h512` alone at n = 6, T = 4096 next to a
torch-composed 16-bit bmm-softmax-bmm, alternating, median of 5.
--encode times the cond stage: `FrozenCLIPEmbedder.encode` of 6 and 12 prompts of 77 tokens through the ViT-L/14 text transformer
per torso (ms per call, launches per call, model TFLOP/s from the plan's algorithmic FLOPs) next to the same transformer composed
from torch's own 16-bit ops on the same weights, alternating, median of 5 windows of 20 calls.
--vae-encode times the first stage's other half: `encode_first_stage` of 1 and 8 images of 512 x 512 through the v1 KL-f8 encoder per
torso (ms per pass and per image, median of 5 passes after 2 warm-ups; TFLOP/s and the fraction of the 2.5 PFLOP/s dense 16-bit MFMA
peak on the plan's algorithmic FLOPs and on the executed ones, which run the three Downsample convs at stride 1).
--clip-image times the CLIP ViT-L/14 image tower (`FrozenClipImageEmbedder`, random weights) on 6 and 320 images of 512 x 512 in
[-1, 1] per torso: ms per call, images/s and model TFLOP/s from the plan's algorithmic FLOPs, median of 5 windows; and the bicubic
resize entry alone.
--prompt-mask "[1,1,1,0,0,0]" times the K-step PLMS loop at the search's 6-latent call with that `prompt_mask` against all ones, and
--masked the K-step DDIM loop with `mask=, x0=` against the unmasked one and the per-step blend alone: both on a captured hipGraph
(GRAPH=0: eager), alternating windows of REPS (default 3) batches in one process, median of 5.
--skip_layers "[ids]" (may be given several times; `transformers` and `level0` name the 16 transformers and the layers of the
first, 64 x 64, level) times one UNet evaluation of BATCH latents with each layer-skip set beside the full network: alternating
windows of REPS (default 5) evaluations between device events, median of 5, on a captured hipGraph (GRAPH=0: eager), one line per
set with its launches per evaluation.  --synthetic {v1,tiny} picks the network (default v1)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autodiffusion_amd import ops  # noqa: E402
from autodiffusion_amd.sd_arch import SD_V1  # noqa: E402
from autodiffusion_amd.sd_unet import UNetModel  # noqa: E402

DEV = "cuda:0"
GFLOP_PER_LATENT = 803.27


def main():
    b = int(os.environ.get("BATCH", "12"))
    reps = int(os.environ.get("REPS", "5"))
    m = UNetModel(image_size=32, use_spatial_transformer=True, **SD_V1).to(DEV)
    m.randomize_(1234)
    if os.environ.get("GRAPH") == "1":
        m.enable_graph()
    x = torch.randn(b, 4, 64, 64, device=DEV)
    t = torch.full((b,), 500, device=DEV, dtype=torch.int64)
    ctx = torch.randn(b, 77, 768, device=DEV)
    for _ in range(2):
        out = m(x, t, ctx)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    if os.environ.get("BREAKDOWN") == "1":
        ops.CONV_PROFILE = []
    t0 = time.perf_counter()
    for _ in range(reps):
        m(x, t, ctx)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"SD v1 UNet batch {b}: {dt * 1e3:.1f} ms / evaluation, {b / dt:.1f} latents/s, "
          f"{b / dt * GFLOP_PER_LATENT / 1e3:.1f} model TFLOP/s")
    if os.environ.get("SAMPLER"):
        sampler_bench(m)
    if ops.CONV_PROFILE:
        prof, ops.CONV_PROFILE = ops.CONV_PROFILE, None
        agg = {}
        for e0, e1, f, key, shape in prof:
            a = agg.setdefault((key, shape), [0.0, 0.0, 0])
            a[0] += e0.elapsed_time(e1); a[1] += f; a[2] += 1
        tot = sum(v[0] for v in agg.values()) / reps
        print(f"conv launches: {tot:.1f} ms of {dt * 1e3:.1f} ms")
        for (key, shape), (ms_, fl_, cnt) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:25]:
            print(f"  conv {key} nhwc_in={shape[:4]} cout={shape[4]} x{cnt // reps}: {ms_ / reps:8.2f} ms {fl_ / ms_ / 1e9:7.1f} TFLOP/s")


def _timed(fn, reps=1):
    """ms of `reps` calls between two device events (a launch returns before the kernel finishes)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def decode_bench():
    import statistics
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL
    n, hw = int(os.environ.get("N_SAMPLES", "6")), 64
    z = torch.randn(n, 4, hw, hw, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)) * 0.9
    for torso in ("bf16", "fp16"):
        vae = AutoencoderKL(**SD_V1_VAE).set_torso(torso).to(DEV).randomize_(4321)
        ld = LatentDiffusion(vae.decoder, device=DEV, first_stage=vae)   # the schedule tables are not used here
        gflop = vae.decoder.plan.flops(hw, hw) / 1e9
        for _ in range(2):
            out = ld.decode_first_stage(z)
        torch.cuda.synchronize()
        assert out.shape == (n, 3, 8 * hw, 8 * hw) and torch.isfinite(out).all()
        ms = statistics.median(_timed(lambda: ld.decode_first_stage(z)) for _ in range(5))
        exit_ms = statistics.median(_timed(lambda: ops.vae_image_out(out), 5) for _ in range(5))
        print(f"SD v1 VAE decode [{torso}] {n} latents of {hw}x{hw}: {ms:.1f} ms / pass, {ms / n:.2f} ms / latent, "
              f"{n * gflop / ms:.1f} model TFLOP/s ({gflop:.1f} GFLOP per latent, from the plan); adm_vae_image_out {exit_ms:.3f} ms")
        # the 512-wide attention alone: n = 6, T = 4096, against torch's composed 16-bit bmm - softmax - bmm, alternating
        dt = vae.compute_dtype
        qkv = (torch.randn(n, hw * hw, 1536, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))).to(dt)
        q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=-1))

        def composed():
            return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (512 ** -0.5), dim=-1), v)
        for _ in range(3):
            a, b = ops.attention(qkv, 1, True), composed()
        torch.cuda.synchronize()
        err = float((a.float() - b.float()).norm() / b.float().norm())
        ta, tb = [], []
        for _ in range(5):
            ta.append(_timed(lambda: ops.attention(qkv, 1, True), 10))
            tb.append(_timed(composed, 10))
        fl = 4.0 * n * (hw * hw) ** 2 * 512
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"attention 1 x 512 [{torso}] n={n} T={hw * hw}: adm_attention_1h512 {ma:.3f} ms ({fl / ma / 1e9:.1f} TFLOP/s), "
              f"torch bmm-softmax-bmm {mb:.3f} ms ({fl / mb / 1e9:.1f} TFLOP/s); rel diff of the two {err:.2g}")
        del vae, ld


PEAK_16BIT_TFLOPS = 2500.0   # MI355X dense bf16 / fp16 MFMA peak


def vae_encode_bench():
    import statistics
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    from autodiffusion_amd.sd_vae import SD_V1_VAE, AutoencoderKL
    hw = int(os.environ.get("HW", "512"))
    for torso in ("bf16", "fp16"):
        vae = AutoencoderKL(**SD_V1_VAE, with_encoder=True).set_torso(torso).to(DEV).randomize_(4321)
        ld = LatentDiffusion(vae.encoder, device=DEV, first_stage=vae)   # the schedule tables are not used here
        alg, exe = (vae.encoder.plan.flops(hw, hw, executed=e, embed_dim=vae.embed_dim) / 1e9 for e in (False, True))
        for n in (1, 8):
            x = torch.tanh(torch.randn(n, 3, hw, hw, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)))
            for _ in range(2):
                out = ld.encode_first_stage(x).parameters
            torch.cuda.synchronize()
            assert out.shape == (n, 2 * vae.embed_dim, hw // 8, hw // 8) and torch.isfinite(out).all()
            ts = [_timed(lambda: ld.encode_first_stage(x)) for _ in range(5)]
            ms = statistics.median(ts)
            print(f"SD v1 VAE encode [{torso}] {n} images of {hw}x{hw}: {ms:.1f} ms / pass ({min(ts):.1f} .. {max(ts):.1f}), {ms / n:.2f} ms / image; "
                  f"algorithmic {alg:.1f} GFLOP / image: {n * alg / ms:.1f} TFLOP/s = {100 * n * alg / ms / PEAK_16BIT_TFLOPS:.1f} % of peak; "
                  f"executed {exe:.1f} GFLOP / image: {n * exe / ms:.1f} TFLOP/s = {100 * n * exe / ms / PEAK_16BIT_TFLOPS:.1f} % of peak")
        del vae, ld


def _torch_clip(P, plan, dt):
    """The text transformer composed from torch's 16-bit ops on the same parameters: ids -> fp32 [N, T, C]."""
    import torch.nn.functional as F
    W = {k[len("text_model."):]: v.to(dt) for k, v in P.items()}
    c, heads, eps = plan.hidden_size, plan.num_attention_heads, plan.layer_norm_eps

    def run(ids):
        n, t = ids.shape
        x = (P["text_model.embeddings.token_embedding.weight"][ids] + P["text_model.embeddings.position_embedding.weight"][:t]).to(dt)
        mask = torch.full((t, t), float("-inf"), device=ids.device, dtype=dt).triu(1)
        for l in range(plan.num_hidden_layers):
            p = f"encoder.layers.{l}"
            h = F.layer_norm(x, (c,), W[f"{p}.layer_norm1.weight"], W[f"{p}.layer_norm1.bias"], eps)
            q, k, v = (F.linear(h, W[f"{p}.self_attn.{a}_proj.weight"], W[f"{p}.self_attn.{a}_proj.bias"])
                       .view(n, t, heads, 64).transpose(1, 2) for a in "qkv")
            w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * 0.125 + mask, dim=-1)
            a = torch.matmul(w, v).transpose(1, 2).reshape(n, t, c)
            x = x + F.linear(a, W[f"{p}.self_attn.out_proj.weight"], W[f"{p}.self_attn.out_proj.bias"])
            h = F.layer_norm(x, (c,), W[f"{p}.layer_norm2.weight"], W[f"{p}.layer_norm2.bias"], eps)
            u = F.linear(h, W[f"{p}.mlp.fc1.weight"], W[f"{p}.mlp.fc1.bias"])
            x = x + F.linear(u * torch.sigmoid(1.702 * u), W[f"{p}.mlp.fc2.weight"], W[f"{p}.mlp.fc2.bias"])
        return F.layer_norm(x.float(), (c,), P["text_model.final_layer_norm.weight"], P["text_model.final_layer_norm.bias"], eps)
    return run


def encode_bench():
    import statistics
    from autodiffusion_amd.sd_clip import FrozenCLIPEmbedder
    t, reps = 77, int(os.environ.get("REPS", "20"))
    for torso in ("bf16", "fp16"):
        emb = FrozenCLIPEmbedder(device="cpu").set_torso(torso).randomize_(2468).to(DEV)
        plan = emb.transformer.plan
        composed = _torch_clip(emb.transformer.state_dict(), plan, emb.compute_dtype)
        for n in (6, 12):
            ids = torch.randint(0, plan.vocab_size, (n, t), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
            for _ in range(3):
                a, b = emb.encode(ids), composed(ids)
            torch.cuda.synchronize()
            assert a.shape == (n, t, plan.hidden_size) and torch.isfinite(a).all()
            err = float((a - b).norm() / b.norm())
            launches = []   # one entry per libadm_hip.so launch of a call
            names = ("clip_embed", "layernorm", "conv", "attention_causal", "quick_gelu", "layernorm_f32out")
            saved = {k: getattr(ops, k) for k in names}
            for k, fn in saved.items():
                setattr(ops, k, (lambda fn, k: lambda *a_, **kw: launches.append(k) or fn(*a_, **kw))(fn, k))
            try:
                emb.encode(ids)
            finally:
                for k, fn in saved.items():
                    setattr(ops, k, fn)
            ta, tb = [], []
            for _ in range(5):
                ta.append(_timed(lambda: emb.encode(ids), reps))
                tb.append(_timed(lambda: composed(ids), reps))
            ma, mb = statistics.median(ta), statistics.median(tb)
            fl = n * plan.flops(t)
            print(f"CLIP ViT-L/14 text encode [{torso}] {n} prompts x {t} tokens: HIP path {ma:.3f} ms / call ({len(launches)} launches, "
                  f"{fl / ma / 1e9:.1f} model TFLOP/s; windows {min(ta):.3f} .. {max(ta):.3f}), torch-composed 16-bit {mb:.3f} ms / call "
                  f"({fl / mb / 1e9:.1f} TFLOP/s; windows {min(tb):.3f} .. {max(tb):.3f}); rel diff of the two {err:.2g}")
        del emb, composed


def clip_image_bench():
    import statistics
    from autodiffusion_amd.sd_clip import FrozenClipImageEmbedder
    for torso in ("bf16", "fp16"):
        emb = FrozenClipImageEmbedder("ViT-L/14", device="cpu").set_torso(torso).randomize_(1357).to(DEV)
        plan = emb.model.plan
        for n, reps in ((6, 10), (320, 2)):
            x = torch.rand(n, 3, 512, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 2 - 1
            for _ in range(2):
                out = emb(x)
            torch.cuda.synchronize()
            assert out.shape == (n, plan.projection_dim) and torch.isfinite(out).all()
            ta = [_timed(lambda: emb(x), reps) for _ in range(5)]
            tr = [_timed(lambda: emb.preprocess(x), reps) for _ in range(5)]
            ma, fl = statistics.median(ta), n * plan.flops()
            print(f"CLIP ViT-L/14 image tower [{torso}] {n} images 512x512: {ma:.2f} ms / call, {n / ma * 1e3:.1f} images/s, "
                  f"{fl / ma / 1e9:.1f} model TFLOP/s (windows {min(ta):.2f} .. {max(ta):.2f}); bicubic entry alone "
                  f"{statistics.median(tr):.3f} ms; {plan.tokens} tokens in {plan.pitch} rows ({1 - plan.tokens / plan.pitch:.1%} dead)")
        del emb


def sampler_bench(m):
    from autodiffusion_amd.sd_sampler import DDIMSampler, DPMSolverSampler, LatentDiffusion, PLMSSampler
    kind = os.environ["SAMPLER"]
    k, n = int(os.environ.get("K", "6")), int(os.environ.get("N_SAMPLES", "6"))
    reps = int(os.environ.get("REPS", "5"))
    ld = LatentDiffusion(m, device=DEV)
    cand = sorted([94, 834, 217, 944, 574, 354, 153, 690, 424, 926][:k])
    if kind == "dpm":
        cand = sorted(cand + [3], reverse=True)  # K+1 time points
    sampler = {"ddim": DDIMSampler, "plms": PLMSSampler, "dpm": DPMSolverSampler}[kind](ld)
    c, uc = torch.randn(n, 77, 768, device=DEV), torch.randn(n, 77, 768, device=DEV)

    def run(seed):
        x_T = torch.randn(n, 4, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        return sampler.sample(S=k, batch_size=n, shape=[4, 64, 64], conditioning=c, verbose=False, eta=0.0, x_T=x_T,
                              unconditional_guidance_scale=7.5, unconditional_conditioning=uc, sampled_timestep=cand)[0]
    for w in range(2):
        out = run(-1 - w)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    t0 = time.perf_counter()
    for r in range(reps):
        run(r)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    evals = k + (1 if kind == "plms" else 0)
    print(f"SD v1 {kind} K={k} cfg 7.5, {n} latents/batch: {dt * 1e3:.1f} ms / batch, {n / dt:.2f} finished latents/s, "
          f"{2 * n * evals / dt * GFLOP_PER_LATENT / 1e3:.1f} model TFLOP/s ({evals} guided UNet evaluations)")


def _alternate(title, variants, n, windows=5):
    """Times ``variants`` (name -> fn(seed), each one finished batch of n latents) in alternating windows of ``reps`` batches (host
    clock around a device synchronise), after two warm-up batches each; prints the median window per variant and its ratio to the first."""
    import statistics
    reps = int(os.environ.get("REPS", "3"))
    for fn in variants.values():
        for w in range(2):
            out = fn(-1 - w)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
    ms = {k: [] for k in variants}
    for w in range(windows):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r in range(reps):
                fn(w * reps + r)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / reps * 1e3)
    base = None
    for k, v in ms.items():
        med = statistics.median(v)
        base = med if base is None else base
        print(f"{title} {k}: {med:.1f} ms / batch ({min(v):.1f} .. {max(v):.1f} over {windows} windows of {reps}), "
              f"{n / med * 1e3:.2f} finished latents/s, {med / base:.4f} x the first")
    return ms


def _sd_v1_sampling():
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    m = UNetModel(image_size=32, use_spatial_transformer=True, **SD_V1).to(DEV)
    m.randomize_(1234)
    if os.environ.get("GRAPH", "1") == "1":
        m.enable_graph()
    k, n = int(os.environ.get("K", "6")), int(os.environ.get("N_SAMPLES", "6"))
    cand = sorted([94, 834, 217, 944, 574, 354, 153, 690, 424, 926][:k])
    c, uc = torch.randn(n, 77, 768, device=DEV), torch.randn(n, 77, 768, device=DEV)

    def x_T(seed):
        return torch.randn(n, 4, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return LatentDiffusion(m, device=DEV), k, n, cand, c, uc, x_T


def prompt_mask_bench(prompt_mask):
    """--prompt-mask "[1,1,1,0,0,0]": the PLMS loop at the search's call (K steps, 6 latents, cfg 7.5, hipGraph replay unless GRAPH=0)
    with the mask against all ones, alternating in one process."""
    from autodiffusion_amd.sd_sampler import PLMSSampler
    ld, k, n, cand, c, uc, x_T = _sd_v1_sampling()
    if len(prompt_mask) != k:
        raise SystemExit(f"sd_bench.py: --prompt-mask holds {len(prompt_mask)} entries; K is {k}")
    sampler = PLMSSampler(ld)

    def run(pm):
        return lambda seed: sampler.sample(S=k, batch_size=n, shape=[4, 64, 64], conditioning=c, verbose=False, eta=0.0, x_T=x_T(seed),
                                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, sampled_timestep=cand,
                                           prompt_mask=pm)[0]
    points = [prompt_mask[0]] + list(prompt_mask)     # the first step evaluates twice
    print(f"prompt_mask {prompt_mask}: {sum(2 if p else 1 for p in points)} UNet evaluations of {n} latents against {2 * len(points)}")
    _alternate(f"SD v1 plms K={k} cfg 7.5, {n} latents/batch, prompt_mask", {"all ones": run([1] * k), str(prompt_mask): run(list(prompt_mask))}, n)


def masked_bench():
    """--masked: K-step DDIM at the search's call, unmasked against masked (half-plane mask; four more launches per step: q_sample,
    two selects, their sum), alternating in one process; then the four launches alone."""
    import statistics
    from autodiffusion_amd.sd_sampler import DDIMSampler, axpby_noise, masked_blend
    ld, k, n, cand, c, uc, x_T = _sd_v1_sampling()
    sampler = DDIMSampler(ld)
    x0 = torch.randn(n, 4, 64, 64, device=DEV) * 0.8
    mask = torch.zeros(1, 1, 64, 64, device=DEV)
    mask[..., :32] = 1.0

    def run(masked):
        kw = dict(mask=mask, x0=x0) if masked else {}
        return lambda seed: sampler.sample(S=k, batch_size=n, shape=[4, 64, 64], conditioning=c, verbose=False, eta=0.0, x_T=x_T(seed),
                                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, sampled_timestep=cand, **kw)[0]
    _alternate(f"SD v1 ddim K={k} cfg 7.5, {n} latents/batch,", {"unmasked": run(False), "masked": run(True)}, n)
    keep = mask.expand(n, 4, 64, 64).contiguous()
    drop = axpby_noise(keep, -1.0, torch.ones_like(keep), 1.0)
    img = x_T(0)
    one = lambda: masked_blend(img, ld.q_sample(x0, 500), keep, drop)   # noqa: E731
    for _ in range(3):
        one()
    us = statistics.median(_timed(one, 200) for _ in range(5)) * 1e3
    print(f"the blend alone ({n} latents of 64x64: q_sample + 2 x adm_vec_act + adm_sd_step, with torch.randn_like): {us:.1f} us per step, "
          f"{us / 4:.1f} us per launch")


def named_skip_set(plan, text):
    """--skip_layers' value -> sorted layer ids: a list literal, `transformers`, or `level0` (every layer at the input resolution)."""
    import ast
    from autodiffusion_amd.sd_arch import SDDownSpec, SDTransformerSpec, SDUpSpec
    if text == "transformers":
        return sorted(b.layer_id for b in plan.all_blocks() if isinstance(b, SDTransformerSpec))
    if text == "level0":
        ids, depth = [], 0
        for seq in plan.input_blocks + [plan.middle_block] + plan.output_blocks:
            for b in seq:
                if getattr(b, "layer_id", -1) >= 0 and depth == 0:
                    ids.append(b.layer_id)
                depth += isinstance(b, SDDownSpec) - isinstance(b, SDUpSpec)
        return sorted(ids)
    ids = ast.literal_eval(text)
    if not isinstance(ids, (list, tuple)) or not all(isinstance(i, int) and not isinstance(i, bool) for i in ids):
        raise SystemExit(f"sd_bench.py: --skip_layers: a list of layer ids, `transformers` or `level0`, got {text!r}")
    return sorted(ids)


def skip_bench(texts, synthetic="v1"):
    import statistics
    from autodiffusion_amd.sd_script_util import TINY_UNET
    cfg, hw, s_ctx = (SD_V1, 64, 77) if synthetic == "v1" else (TINY_UNET, 16, 77)
    b, reps = int(os.environ.get("BATCH", "12")), int(os.environ.get("REPS", "5"))
    m = UNetModel(image_size=32, use_spatial_transformer=True, **cfg).to(DEV)
    m.randomize_(1234)
    graph = os.environ.get("GRAPH", "1") == "1"
    m.enable_graph(graph)
    sets = [("none", ())] + [(t, tuple(named_skip_set(m.plan, t))) for t in texts]
    m.plan_graphs(len({s_ for _, s_ in sets if s_}))
    x = torch.randn(b, 4, hw, hw, device=DEV)
    t = torch.full((b,), 500, device=DEV, dtype=torch.int64)
    ctx = torch.randn(b, s_ctx, m.plan.context_dim, device=DEV)
    launches = {}
    names = ("conv", "conv2d", "gn_affine", "layernorm", "attention_cross", "geglu", "resample", "linear_f32", "timestep_embedding",
             "nchw_to_nhwc_pad")
    for name, ids in sets:     # launches per evaluation: counted on an eager pass through the ops entry points
        count = [0]
        saved = {k: getattr(ops, k) for k in names}
        for k, fn in saved.items():
            setattr(ops, k, (lambda fn: lambda *a_, **kw: count.__setitem__(0, count[0] + 1) or fn(*a_, **kw))(fn))
        try:
            m.enable_graph(False)(x, t, ctx, skip_layer=ids)
        finally:
            for k, fn in saved.items():
                setattr(ops, k, fn)
            m.enable_graph(graph)
        launches[name] = count[0]
        for _ in range(2):
            out = m(x, t, ctx, context_key="bench", skip_layer=ids)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
    ms = {name: [] for name, _ in sets}
    for _ in range(5):
        for name, ids in sets:
            ms[name].append(_timed(lambda: m(x, t, ctx, context_key="bench", skip_layer=ids), reps))
    base = statistics.median(ms["none"])
    for name, ids in sets:
        med = statistics.median(ms[name])
        print(f"SD {synthetic} UNet batch {b} ({'hipGraph' if graph else 'eager'}), skip_layers {name} ({len(ids)} of {m.layer_num} layers, "
              f"{launches[name]} op calls): {med:.2f} ms / evaluation ({min(ms[name]):.2f} .. {max(ms[name]):.2f} over 5 windows of {reps}), "
              f"{med / base:.3f} x the full network")


if __name__ == "__main__":
    if "--skip_layers" in sys.argv[1:]:
        argv = sys.argv[1:]
        skip_bench([argv[i + 1] for i, a in enumerate(argv) if a == "--skip_layers"],
                   argv[argv.index("--synthetic") + 1] if "--synthetic" in argv else "v1")
    elif "--prompt-mask" in sys.argv[1:]:
        import ast
        prompt_mask_bench([int(v) for v in ast.literal_eval(sys.argv[sys.argv.index("--prompt-mask") + 1])])
    elif "--masked" in sys.argv[1:]:
        masked_bench()
    elif "--decode" in sys.argv[1:]:
        decode_bench()
    elif "--vae-encode" in sys.argv[1:]:
        vae_encode_bench()
    elif "--encode" in sys.argv[1:]:
        encode_bench()
    elif "--clip-image" in sys.argv[1:]:
        clip_image_bench()
    else:
        main()
