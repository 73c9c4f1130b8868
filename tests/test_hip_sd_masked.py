"""GPU half of masked sampling (latent inpainting) and PLMS ``prompt_mask`` on the HIP path: ``masked_blend`` against ``torch.where``
to the bit, ``DDIMSampler`` / ``PLMSSampler`` with ``mask=, x0=`` and ``prompt_mask=`` against latents captured from the reference's
own samplers (tests/golden/capture_sd_masked.py; tests/test_sd_masked_host.py pins what the fixture means), the number and size of
the model calls a ``prompt_mask`` makes, bitwise identities over the tiny HIP latent UNet, and scripts/sd_inpaint.py end to end.

Bounds: the blend is exact (integer comparison of the bit patterns; the one stated exception is the sign of a selected zero, which
the sum of the two disjoint halves -- like the reference's ``orig * mask + (1 - mask) * img`` -- makes positive).  Fixture runs:
rtol = atol = 2e-5, what test_hip_sd.py::test_latent_samplers_match_reference_goldens holds this toy model to.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from helpers import golden
from test_sd_masked_host import RUNS, parse_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ the blend
def _special(shape, seed):
    """Normal draws with -0.0, +0.0, denormals and large values planted every few elements."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3
    flat = x.view(-1)
    plant = torch.tensor([-0.0, 0.0, 1e-40, -1e-41, 1.4e-45, -1.17549435e-38, 3.0e38, -65504.0])
    idx = torch.arange(seed % 3, flat.numel(), 5)
    flat[idx] = plant[torch.arange(idx.numel()) % plant.numel()]
    return x


@pytest.mark.parametrize("layout", ["N1HW", "11HW", "NCHW", "all_keep", "all_drop"])
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (1, 4, 5, 7), (2, 4, 9, 29)])   # 768; 140 (< one block); 2088 (not a multiple of 256)
def test_masked_blend_is_torch_where_to_the_bit(shape, layout):
    from autodiffusion_amd.sd_sampler import axpby_noise, masked_blend
    n, c, h, w = shape
    g = torch.Generator().manual_seed(h * w)
    mshape = {"N1HW": (n, 1, h, w), "11HW": (1, 1, h, w)}.get(layout, shape)
    mask = (torch.rand(mshape, generator=g) < 0.5).float()
    if layout in ("all_keep", "all_drop"):
        mask = torch.full(shape, 1.0 if layout == "all_keep" else 0.0)
    orig, img = _special(shape, 1), _special(shape, 2)
    assert int(((orig == 0) & torch.signbit(orig)).sum()) > 0 and int((orig.abs() < 1e-38).sum()) > 4   # -0.0 and denormals are in
    keep = mask.expand(shape).contiguous().to(DEV)
    drop = axpby_noise(keep, -1.0, torch.ones_like(keep), 1.0)
    assert torch.equal(drop.cpu(), 1.0 - mask.expand(shape))
    got = masked_blend(img.to(DEV), orig.to(DEV), keep, drop)
    want = torch.where(mask.expand(shape) > 0, orig, img)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    pos = want.clone()
    pos[want == 0] = 0.0                       # the sum of the halves gives a selected zero the sign +, whatever it had
    same = _bits(got) == _bits(pos)
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} elements differ in their bits"
    if layout == "all_keep":
        assert bool((_bits(got) == _bits(torch.where(orig == 0, torch.zeros(()), orig))).all())


# ------------------------------------------------------------------ the samplers against the reference's
class _Toy:
    """The attributes of LatentDiffusion the samplers read; apply_model = the capture script's toy model on the GPU, q_sample = the
    library's own on the fixture's stored noises, one per call."""

    def __init__(self, q_noise=None):
        from autodiffusion_amd.sd_sampler import LatentDiffusion
        self._base = base = LatentDiffusion(None, device=DEV)
        self.num_timesteps, self.device = base.num_timesteps, base.device
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = base.betas, base.alphas_cumprod, base.alphas_cumprod_prev
        self.q_noise, self.q_calls, self.batches = q_noise, 0, []

    def apply_model(self, x, t, c):
        from oracle.sd_sampler import toy_model
        self.batches.append(int(x.shape[0]))
        return toy_model(x, t, c)

    def q_sample(self, x0, t):
        noise = self.q_noise[self.q_calls]
        self.q_calls += 1
        return self._base.q_sample(x0, t, noise=noise)


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = golden("sd_masked")
    return g, {k: torch.from_numpy(g[k]).to(DEV) for k in ("x_T", "c", "uc", "x0", "q_noise", "mask_blocks", "mask_half", "mask_chan")}


@pytest.mark.parametrize("key", RUNS)
def test_masked_and_prompt_masked_sampling_matches_the_reference(fx, key):
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler
    g, t = fx
    name, tag, gtag, mask, pm = parse_run(key)
    cand = g[f"cand_{tag}"]
    scale, uc = {"cfg": (7.5, t["uc"]), "plain": (1.0, None)}[gtag]
    m = _Toy(list(t["q_noise"]))
    kw = {}
    if mask is not None:
        kw.update(mask=t[f"mask_{mask}"], x0=t["x0"])
    if pm is not None:
        kw.update(prompt_mask=pm)
    st = np.array(sorted(cand)) if name == "plms" else cand
    got, inter = {"ddim": DDIMSampler, "plms": PLMSSampler}[name](m).sample(
        S=len(cand), batch_size=3, shape=[4, 8, 8], conditioning=t["c"], verbose=False, eta=0.0, x_T=t["x_T"],
        unconditional_guidance_scale=scale, unconditional_conditioning=uc, sampled_timestep=st, **kw)
    err = np.abs(got.cpu().numpy() - g[key]).max()
    print(f"{key}: max |err| {err:.3g}")
    np.testing.assert_allclose(got.cpu().numpy(), g[key], rtol=2e-5, atol=2e-5, err_msg=key)
    assert m.q_calls == (len(cand) if mask is not None else 0)      # one blend per loop iteration, none after the last update
    assert torch.equal(inter["x_inter"][-1], got)                   # x_inter stays the post-step latent
    if mask is not None:   # the result's kept region is the model's last update of it, not x0 (the reference does not re-blend)
        keep = t[f"mask_{mask}"].expand_as(got) > 0
        assert not torch.equal(got[keep], t["x0"][keep])


class _Counting:
    """A toy model that takes ``context_key`` (so guidance may split over two streams) and records every call."""
    accepts_context_key = True

    def __init__(self):
        self._toy = _Toy()
        for k in ("num_timesteps", "device", "betas", "alphas_cumprod", "alphas_cumprod_prev"):
            setattr(self, k, getattr(self._toy, k))
        self.calls = []

    def apply_model(self, x, t, c, context_key=None):
        on_cur = torch.cuda.current_stream().cuda_stream == self.main_stream
        self.calls.append((int(x.shape[0]), context_key[1] if isinstance(context_key, tuple) and isinstance(context_key[0], tuple) else "-",
                           "cur" if on_cur else "side"))
        return self._toy.apply_model(x, t, c)


@pytest.mark.parametrize("pm", [[1, 0, 1, 0], [0, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]])
def test_prompt_mask_makes_the_expected_model_calls(fx, pm):
    """S = 4 steps; the first (pseudo-Euler) step calls the model twice, so a run has 5 evaluation points.  An entry of 1 costs, per
    point, one call of 2N (single guidance batch, ADM_SD_SPLIT_GUIDANCE=0) or two calls of N on two streams (split guidance:
    'u' on the side stream, 'c' on the current one); an entry of 0 costs ONE call of N on the current stream under key 'u' either
    way.  With z zeros among entries 1..3 and z0 = 1 if entry 0 is zero: N-calls of the unguided kind = z + 2 * z0."""
    from autodiffusion_amd.sd_sampler import PLMSSampler
    g, t = fx
    n = 3
    points = [pm[0], pm[0]] + pm[1:]     # the doubled first step
    for split in (True, False):
        m = _Counting()
        m.main_stream = torch.cuda.current_stream().cuda_stream
        s = PLMSSampler(m)
        s.split_guidance = split       # what ADM_SD_SPLIT_GUIDANCE=0 sets for the process
        got, _ = s.sample(S=4, batch_size=n, shape=[4, 8, 8], conditioning=t["c"], verbose=False, x_T=t["x_T"],
                          unconditional_guidance_scale=7.5, unconditional_conditioning=t["uc"],
                          sampled_timestep=np.array(sorted(g["cand_k4"])), prompt_mask=pm)
        torch.cuda.synchronize()
        want = []
        for p in points:
            if p == 0:
                want.append((n, "u", "cur"))
            elif split:
                want += [(n, "u", "side"), (n, "c", "cur")]
            else:
                want.append((2 * n, "-", "cur"))
        assert m.calls == want, (split, m.calls)
        assert len(m.calls) == sum(1 if p == 0 else (2 if split else 1) for p in points)
        np.testing.assert_allclose(got.cpu().numpy(), g["plms_k4_cfg_pm" + "".join(map(str, pm))], rtol=2e-5, atol=2e-5)


def test_mask_value_and_layout_refusals(fx):
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler
    g, t = fx
    kw = dict(S=4, batch_size=3, shape=[4, 8, 8], conditioning=t["c"], x_T=t["x_T"], verbose=False)
    soft = t["mask_half"].clone()
    soft[0, 0, 3, 3] = 0.5
    for cls in (DDIMSampler, PLMSSampler):
        m = _Toy(list(t["q_noise"]))
        with pytest.raises(NotImplementedError, match="soft masks"):
            cls(m).sample(mask=soft, x0=t["x0"], **kw)
        with pytest.raises(NotImplementedError):
            cls(m).sample(mask=torch.ones(1), **kw)         # the pin of test_hip_sd.py / test_hip_sd_vae_encode.py
        assert m.batches == [] and m.q_calls == 0           # refused before the first model call


# ------------------------------------------------------------------ over the tiny HIP latent UNet
@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    from autodiffusion_amd.sd_unet import UNetModel
    from test_sd_oracle import sd_case
    g, plan, P = sd_case("sd_unet_tiny")
    unet = UNetModel(image_size=32, use_spatial_transformer=True, **ast.literal_eval(str(g["cfg"])))
    unet.load_state_dict(P)
    unet.to(DEV).eval()
    ctx = torch.from_numpy(g["context"]).to(DEV)
    return unet, LatentDiffusion(unet, device=DEV), torch.from_numpy(g["x"]).to(DEV), ctx, (ctx.flip(1).contiguous() * 0.5)


def _plms(ld, x_T, c, uc, scale, split=True, **kw):
    from autodiffusion_amd.sd_sampler import PLMSSampler
    s = PLMSSampler(ld)
    s.split_guidance = split
    out, _ = s.sample(S=4, batch_size=x_T.shape[0], shape=list(x_T.shape[1:]), conditioning=c, verbose=False, x_T=x_T,
                      unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                      sampled_timestep=np.array([153, 424, 690, 926]), **kw)
    torch.cuda.synchronize()
    return out.clone()


def test_prompt_mask_identities_over_the_hip_unet(tiny):
    unet, ld, x_T, c, uc = tiny
    unet.enable_graph(False)
    plain = _plms(ld, x_T, c, uc, 3.0)
    assert torch.equal(_plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 1, 1, 1]), plain)           # all ones: the run without the keyword
    on_uc = _plms(ld, x_T, uc, None, 1.0)
    assert torch.equal(_plms(ld, x_T, c, uc, 3.0, prompt_mask=[0, 0, 0, 0]), on_uc)           # all zeros: a plain run on uc, scale 1
    assert not torch.equal(on_uc, plain)
    mixed = _plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 0, 0, 1])
    assert not torch.equal(mixed, plain) and not torch.equal(mixed, on_uc) and bool(torch.isfinite(mixed).all())
    assert torch.equal(_plms(ld, x_T, c, uc, 3.0, split=False, prompt_mask=[1, 0, 0, 1]), mixed)   # one batch of 2N: the same bits


def test_mixed_prompt_mask_replays_disjoint_graphs_per_stream(tiny):
    """Graph mode, split guidance: guided and unguided evaluations all have batch N, so the launching stream alone tells the
    captured graphs apart -- one on the current stream (the 'c' half and the unguided steps, in stream order), one on the side
    stream (the 'u' half).  Bitwise the eager result, twice."""
    unet, ld, x_T, c, uc = tiny
    unet.enable_graph(False)
    eager = _plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 0, 0, 1])
    try:
        unet.enable_graph()
        unet._packed.graphs.clear()
        a = _plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 0, 0, 1])
        assert len(unet._packed.graphs) == 2
        assert len({k[5] for k in unet._packed.graphs}) == 2       # ... on two different streams
        b = _plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 0, 0, 1])
        assert len(unet._packed.graphs) == 2
        assert torch.equal(a, eager) and torch.equal(b, eager)
        x0 = (x_T * 0.3).contiguous()
        mask = torch.zeros(1, 1, *x_T.shape[2:], device=DEV)
        mask[..., : x_T.shape[3] // 2] = 1.0
        runs = []
        for graph in (True, False):     # masked, with a prompt mask, graph replay against eager on the same q_sample noise
            unet.enable_graph(graph)
            torch.manual_seed(5)
            runs.append(_plms(ld, x_T, c, uc, 3.0, prompt_mask=[1, 0, 0, 1], mask=mask, x0=x0))
        assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], eager)
    finally:
        unet.enable_graph(False)


# ------------------------------------------------------------------ scripts/sd_inpaint.py
@pytest.fixture(scope="module")
def inpaint():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("sd_inpaint", os.path.join(ROOT, "scripts", "sd_inpaint.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def test_inpaint_cli_synthetic_tiny(inpaint, tmp_path):
    rs = np.random.RandomState(4)
    init = rs.randint(0, 256, size=(1, 64, 64, 3)).astype(np.uint8)
    mask = np.zeros((1, 64, 64), np.uint8)
    mask[0, 16:48, 8:40] = 255                       # repaint a 32 x 32 square, keep the rest
    np.save(tmp_path / "init.npy", init)
    np.save(tmp_path / "mask.npy", mask)
    np.save(tmp_path / "ids.npy", rs.randint(0, 500, size=(1, 8)).astype(np.int64))
    common = ["--synthetic", "tiny", "--init-img", str(tmp_path / "init.npy"), "--mask", str(tmp_path / "mask.npy"),
              "--prompt_ids", str(tmp_path / "ids.npy"), "--n_samples", "2", "--ddim_steps", "4", "--use_timestep", "[153, 424, 926, 690]",
              "--scale", "3.0", "--seed", "7"]
    repaint = mask[0] >= 128
    arr = inpaint.main(common + ["--outdir", str(tmp_path / "a")])
    assert arr.shape == (2, 64, 64, 3) and arr.dtype == np.uint8
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "samples_2x64x64x3.npz")["arr_0"], arr)
    for i in range(2):
        np.testing.assert_array_equal(arr[i][~repaint], init[0][~repaint])        # kept pixels: the input's bytes
        assert (arr[i][repaint] != init[0][repaint]).mean() > 0.5                 # repainted ones: generated
    raw = inpaint.main(common + ["--outdir", str(tmp_path / "b"), "--no_composite"])
    assert raw.shape == arr.shape and raw.dtype == np.uint8
    np.testing.assert_array_equal(raw[:, repaint], arr[:, repaint])               # the same seed: the same samples under the mask
    assert (raw[:, ~repaint] != init[:, ~repaint]).mean() > 0.5                   # a VAE round trip does not return the bytes
    pl = inpaint.main(common + ["--outdir", str(tmp_path / "c"), "--plms", "--prompt_mask", "[1, 0, 1, 0]"])
    assert pl.shape == arr.shape and pl.dtype == np.uint8 and not np.array_equal(pl, arr)
    np.testing.assert_array_equal(pl[:, ~repaint], np.repeat(init, 2, 0)[:, ~repaint])
    with pytest.raises(SystemExit, match="--plms"):
        inpaint.main(common + ["--outdir", str(tmp_path / "d"), "--prompt_mask", "[1, 0, 1, 0]"])
