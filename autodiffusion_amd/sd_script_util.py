"""What more than one Stable-Diffusion command line (scripts/sd_*.py) uses: the model builders, the prompt and image loaders, the
sampling scripts' shared flags and a few helpers -- the latent path's counterpart of script_util.py.  A helper that refuses its input
raises ``SystemExit`` and takes ``prog``, the running script's name, for the message's prefix."""
import argparse
import ast
import json
import os
import random

import numpy as np
import torch

from . import dist_util, logger, sd_clip
from .inception import InceptionV3
from .script_util import str2bool
from .sd_arch import SD_V1, SD_V2
from .sd_clip import CLIP_VIT_L14_TEXT, OPENCLIP_VIT_H14_TEXT, FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder
from .sd_sampler import DDIMSampler, DPMSolverSampler, LatentDiffusion, PLMSSampler, UniPCSampler
from .sd_unet import UNetModel
from .sd_vae import SD_V1_VAE, AutoencoderKL

# --synthetic tiny: the smallest networks the test suite runs (a 64-wide two-level UNet, a three-level decoder that turns an
# h x w latent into a 4h x 4w image, a one-layer text transformer of the UNet's context width over 512 token ids)
TINY_UNET = dict(in_channels=4, out_channels=4, model_channels=64, attention_resolutions=[1, 2], num_res_blocks=1,
                 channel_mult=[1, 2], num_heads=2, transformer_depth=1, context_dim=128, legacy=False)
TINY_VAE = dict(ddconfig=dict(ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3,
                              resolution=32, z_channels=4), embed_dim=4)
TINY_CLIP = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                 max_position_embeddings=77)
# --synthetic tiny2: the same sizes in the Stable Diffusion 2.x form -- 64-wide heads named by num_head_channels, linear proj_in /
# proj_out, a two-layer OpenCLIP-style tower (exact GELU, penultimate exit, pad id 0) and a v-predicting UNet
TINY2_UNET = dict({k: v for k, v in TINY_UNET.items() if k != "num_heads"}, num_head_channels=64, use_linear_in_transformer=True)
TINY2_CLIP = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                  max_position_embeddings=77, hidden_act="gelu")
COND_STAGES = {"FrozenCLIPEmbedder": FrozenCLIPEmbedder, "FrozenOpenCLIPEmbedder": FrozenOpenCLIPEmbedder}

# ------------------------------------------------------------------ the flags sd_img2img.py and sd_inpaint.py share
SD_SAMPLING_FLAGS = {
    "--prompt": dict(type=str, nargs="?", default="a painting of a virus monster playing guitar", help="the prompt to render"),
    "--init-img": dict(type=str, nargs="?", required=True, help="path to the input image (image file, or uint8 NHWC .npy / .npz)"),
    "--ddim_eta": dict(type=float, default=0.0, help="ddim eta (eta=0.0 corresponds to deterministic sampling)"),
    "--n_iter": dict(type=int, default=1, help="sample this often"),
    "--n_samples": dict(type=int, default=2, help="how many samples to produce for each given prompt. A.k.a batch size"),
    "--scale": dict(type=float, default=5.0, help="unconditional guidance scale: eps = eps(x, empty) + scale * (eps(x, cond) - eps(x, empty))"),
    "--config": dict(type=str, default="configs/stable-diffusion/v1-inference.yaml",
                     help="path to config which constructs model (read when the file exists; else the SD-v1 constants)"),
    "--ckpt": dict(type=str, default="models/ldm/stable-diffusion-v1/model.ckpt", help="path to checkpoint of model"),
    "--seed": dict(type=int, default=42, help="the seed (for reproducible sampling)"),
    "--tokenizer_dir": dict(type=str, default="", help="LOCAL directory of the transformers CLIP tokenizer (nothing is fetched)"),
    "--prompt_ids": dict(type=str, default="", help=".npy int64 [num, T] token ids (num = 1 or --n_samples); replaces --prompt"),
    "--torso": dict(choices=["bf16", "fp16"], default="bf16", help="16-bit type of activations and weights between kernels"),
    "--synthetic": dict(choices=["tiny", "v1", "tiny2", "v2"], default="",
                        help="build the networks with randomize_() instead of reading --ckpt (tiny2 / v2: the SD 2.x family, v-prediction)"),
    "--use_timestep": dict(type=str, default="", help="'[t0, t1, ...]': a searched schedule of --ddim_steps timesteps"),
    "--side_multiple": dict(type=int, default=64, help="an image FILE is resized down to a multiple of this many pixels"),
    # absent from the namespace unless given (as the flags below): the argument line of every other run stays what it was
    "--skip_layers": dict(type=str, default=argparse.SUPPRESS,
                          help="'[[ids], [ids], ...]': per-step layer-skip lists, list i belonging to entry i of --use_timestep as written "
                               "(without --use_timestep: to step i of the uniform schedule, ascending)"),
}
# scripts/sd_search_ea.py's joint timestep / layer-skip search: scripts/search_ea.py's names and meaning
SD_SKIP_SEARCH_FLAGS = {
    "--use_dynamic_unet": dict(type=str2bool, default=argparse.SUPPRESS,
                               help="search per-step layer-skip lists together with the timesteps (DDIM / PLMS)"),
    "--max_prun": dict(type=float, default=argparse.SUPPRESS, help="largest fraction of the UNet's layers one step may skip"),
    "--min_prun": dict(type=float, default=argparse.SUPPRESS, help="smallest fraction, from epoch 6 on"),
    "--index_step": dict(type=str, default=argparse.SUPPRESS,
                         help="budget of evaluated layers per candidate (default: time_step * layer_num); a number, no arithmetic"),
}


def add_sd_sampling_flags(parser, first, last):
    """Adds SD_SAMPLING_FLAGS from `first` to `last`, in the table's order.  A script calls it once per run of shared flags and
    defines its own in between: argparse lists its help and fills the namespace in definition order, which the scripts keep."""
    names = list(SD_SAMPLING_FLAGS)
    for name in names[names.index(first):names.index(last) + 1]:
        parser.add_argument(name, **SD_SAMPLING_FLAGS[name])


def add_skip_search_flags(parser):
    for name, kw in SD_SKIP_SEARCH_FLAGS.items():
        parser.add_argument(name, **kw)


def skip_search_options(opt, prog):
    """The joint search's (max_prun, min_prun, index_step | None), or None with --use_dynamic_unet off; its flags without it, and
    the continuous-time samplers beside it, are refused."""
    if not getattr(opt, "use_dynamic_unet", False):
        given = [k for k in ("max_prun", "min_prun", "index_step") if hasattr(opt, k)]
        if given:
            raise SystemExit(f"{prog}: --{given[0]} needs --use_dynamic_unet True")
        return None
    if getattr(opt, "dpm_solver", False) or getattr(opt, "unipc", False):
        raise SystemExit(f"{prog}: --use_dynamic_unet searches the integer timestep space (DDIM / PLMS): not with --dpm_solver / --unipc")
    if not (hasattr(opt, "max_prun") and hasattr(opt, "min_prun")):
        raise SystemExit(f"{prog}: --use_dynamic_unet True needs --max_prun F --min_prun F")
    if not 0.0 <= opt.min_prun <= opt.max_prun < 1.0:
        raise SystemExit(f"{prog}: expected 0 <= --min_prun <= --max_prun < 1, got {opt.min_prun} and {opt.max_prun}")
    index_step = None
    if hasattr(opt, "index_step"):
        from .evaluate import parse_index_step
        try:
            index_step = parse_index_step(opt.index_step, "--index_step")
        except ValueError as e:
            raise SystemExit(f"{prog}: {e}") from e
    return opt.max_prun, opt.min_prun, index_step


def read_skip_layers(text, use_timestep, steps, prog):
    """--skip_layers "[[ids], ...]" -> one list of ints per step in ASCENDING timestep order (read_use_timestep's order), or None when
    the flag is empty.  List i belongs to entry i of --use_timestep as written and moves with it through the sort."""
    if not text:
        return None
    try:
        v = ast.literal_eval(text)
    except (ValueError, SyntaxError) as e:
        raise SystemExit(f"{prog}: --skip_layers: expected a list of lists of layer ids, got {text!r}") from e
    ok = isinstance(v, (list, tuple)) and all(isinstance(s, (list, tuple)) and all(isinstance(i, int) and not isinstance(i, bool) for i in s)
                                              for s in v)
    if not ok:
        raise SystemExit(f"{prog}: --skip_layers: expected a list of lists of layer ids, got {text!r}")
    if len(v) != steps:
        raise SystemExit(f"{prog}: --skip_layers holds {len(v)} lists; --ddim_steps is {steps}")
    lists = [list(s) for s in v]
    if use_timestep:
        ts = [int(t) for t in ast.literal_eval(use_timestep)]
        if len(ts) != len(lists):
            raise SystemExit(f"{prog}: --skip_layers holds {len(lists)} lists; --use_timestep {len(ts)} entries")
        lists = [lists[i] for i in sorted(range(len(ts)), key=lambda i: ts[i])]
    return lists


def read_use_timestep(text, ddim_steps, prog):
    """--use_timestep "[t0, t1, ...]" -> the sorted int array of --ddim_steps entries, or None when the flag is empty."""
    if not text:
        return None
    sched = np.array(sorted(int(t) for t in ast.literal_eval(text)))
    if sched.shape[0] != ddim_steps:
        raise SystemExit(f"{prog}: --use_timestep holds {sched.shape[0]} entries; --ddim_steps is {ddim_steps}")
    return sched


def seed_everything(seed):
    """pytorch_lightning.seed_everything(seed): random, numpy, torch."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def require_gpu(prog):
    """-> this rank's device, made current."""
    device = dist_util.dev()
    if device.type != "cuda":
        raise SystemExit(f"{prog}: no GPU is visible (the HIP path has no CPU fallback)")
    torch.cuda.set_device(device)
    return device


def save_samples(outdir, arr):
    """uint8 NHWC `arr` -> OUTDIR/samples_{N}x{H}x{W}x3.npz (``arr_0``); returns `arr`."""
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "samples_%s.npz" % "x".join(str(v) for v in arr.shape))
    np.savez(path, arr)
    logger.log(f"saved {arr.shape[0]} images to {path}")
    return arr


# ------------------------------------------------------------------ prompts and images
def read_captions(path):
    """COCO-style JSON -> annotations[i]['caption'].lower() in file order (ldm/data/coco.py:36-46); otherwise one caption per line."""
    with open(path, "r", encoding="utf-8") as f:
        text = f.read()
    if text.lstrip().startswith("{"):
        return [a["caption"].lower() for a in json.loads(text)["annotations"]]
    return [line.strip() for line in text.splitlines() if line.strip()]


def read_prompt_ids(path, prog, n_samples=None):
    """--prompt_ids FILE.npy -> int64 [num, T] token ids (host).  n_samples: the file must then hold one row or that many."""
    ids = np.load(path, allow_pickle=False)
    if ids.ndim != 2 or not np.issubdtype(ids.dtype, np.integer) or (n_samples is not None and ids.shape[0] not in (1, n_samples)):
        raise SystemExit(f"{prog}: --prompt_ids must hold an integer [{'1 | n_samples' if n_samples else 'num'}, T] array, "
                         f"got {ids.dtype} {ids.shape}")
    return torch.from_numpy(ids.astype(np.int64))


def load_prompts(opt, device, prog):
    """-> (what get_learned_conditioning takes for the batch, for the empty prompt, T of --prompt_ids | None)."""
    if opt.prompt_ids:
        ids = read_prompt_ids(opt.prompt_ids, prog, opt.n_samples).expand(opt.n_samples, -1).contiguous().to(device)   # one row: repeated
        return ids, opt.n_samples * [""], ids.shape[1]
    if not opt.tokenizer_dir:
        raise SystemExit(f"{prog}: --prompt needs --tokenizer_dir (a local CLIP tokenizer directory); or pass token ids with --prompt_ids")
    return opt.n_samples * [opt.prompt], opt.n_samples * [""], None


def load_images(path, n_samples, side_multiple, prog):
    """-> fp32 NCHW [n_samples, 3, H, W] in [-1, 1] (host), as img2img.py:39-49 load_img builds it."""
    if path.endswith((".npy", ".npz")):
        arr = np.load(path, allow_pickle=False)
        arr = arr["arr_0"] if path.endswith(".npz") else arr
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
            raise SystemExit(f"{prog}: --init-img must hold a uint8 [N, H, W, 3] batch, got {arr.dtype} {arr.shape}")
    else:
        from PIL import Image
        image = Image.open(path).convert("RGB")
        w, h = (v - v % side_multiple for v in image.size)
        print(f"loaded input image of size {image.size} from {path}, resized to ({w}, {h})")
        arr = np.asarray(image.resize((w, h), resample=Image.LANCZOS), dtype=np.uint8)[None]
    if arr.shape[0] == 1:
        arr = np.repeat(arr, n_samples, axis=0)
    if arr.shape[0] != n_samples:
        raise SystemExit(f"{prog}: --init-img holds {arr.shape[0]} images; one or --n_samples {n_samples} expected")
    x = arr.astype(np.float32) / 255.0
    return torch.from_numpy(2.0 * x - 1.0).permute(0, 3, 1, 2).contiguous()


class EmptyPromptTokenizer:
    """Stands in for the CLIP tokenizer in a --prompt_ids run, which has one string left to tokenise: the empty prompt of
    classifier-free guidance.  CLIP's tokenizer turns "" into <|startoftext|> followed by <|endoftext|> up to max_length (its pad
    token is <|endoftext|>), and those two are the last two ids of its vocabulary (49406 and 49407 of 49408).  pad: the id behind the
    first <|endoftext|> (None: <|endoftext|> itself, CLIP's; 0 for OpenCLIP's tokenizer: [bos, eos, 0, 0, ...])."""

    def __init__(self, vocab_size, prog="sd_search_ea.py", pad=None):
        self.bos, self.eos, self.prog = int(vocab_size) - 2, int(vocab_size) - 1, prog
        self.pad = self.eos if pad is None else int(pad)

    def __call__(self, text, max_length, **kw):
        if any(t != "" for t in text):
            raise SystemExit(f"{self.prog}: a --prompt_ids run has no tokenizer for strings; give --tokenizer_dir")
        ids = torch.full((len(text), max_length), self.pad, dtype=torch.int64)
        ids[:, 0] = self.bos
        ids[:, 1:2] = self.eos
        return {"input_ids": ids}


# ------------------------------------------------------------------ networks
def build_model(opt, device, prompt_len=None, with_encoder=False):
    """LatentDiffusion (UNet + first stage + cond stage) on `device`: synthetic weights, or --ckpt under --config / the v1 constants.
    prompt_len: the T of --prompt_ids; without --tokenizer_dir the empty prompt is then built as T ids by EmptyPromptTokenizer.
    with_encoder: the first stage also gets its image encoder."""
    unet_cfg = dict(image_size=32, use_spatial_transformer=True, **SD_V1)
    vae_cfg, clip_cfg, ld_cfg = dict(SD_V1_VAE), dict(config=CLIP_VIT_L14_TEXT), {}
    cond_cls = FrozenCLIPEmbedder
    if opt.synthetic == "tiny":
        unet_cfg = dict(image_size=32, use_spatial_transformer=True, **TINY_UNET)
        vae_cfg, clip_cfg = dict(TINY_VAE), dict(config=TINY_CLIP)
    elif opt.synthetic == "tiny2":
        unet_cfg = dict(image_size=32, use_spatial_transformer=True, **TINY2_UNET)
        vae_cfg, clip_cfg, cond_cls = dict(TINY_VAE), dict(config=TINY2_CLIP, layer="penultimate"), FrozenOpenCLIPEmbedder
        ld_cfg = dict(parameterization="v")
    elif opt.synthetic == "v2":
        unet_cfg = dict(image_size=32, use_spatial_transformer=True, **SD_V2)
        clip_cfg, cond_cls = dict(config=OPENCLIP_VIT_H14_TEXT, layer="penultimate"), FrozenOpenCLIPEmbedder
        ld_cfg = dict(parameterization="v")
    elif not opt.synthetic and opt.config and os.path.isfile(opt.config):
        import yaml
        with open(opt.config, "r", encoding="utf-8") as f:
            params = yaml.safe_load(f)["model"]["params"]
        ld_cfg = {k: params[k] for k in ("timesteps", "linear_start", "linear_end", "scale_factor", "parameterization") if k in params}
        unet_cfg = dict(params["unet_config"].get("params") or {})
        vae_cfg = dict(params["first_stage_config"].get("params") or {})
        clip_cfg = dict(params["cond_stage_config"].get("params") or {})
        clip_cfg.pop("device", None)
        clip_cfg.pop("freeze", None)
        target = str(params["cond_stage_config"].get("target") or "FrozenCLIPEmbedder")
        if target.rsplit(".", 1)[-1] not in COND_STAGES:
            raise SystemExit(f"build_model: cond_stage_config.target {target!r} is not built (one of {sorted(COND_STAGES)})")
        cond_cls = COND_STAGES[target.rsplit(".", 1)[-1]]
        logger.log(f"model configuration from {opt.config}")
    elif not opt.synthetic:
        logger.log(f"--config {opt.config} is not a file: using the SD-v1 constants of the package")
    if opt.tokenizer_dir:
        clip_cfg["version"] = opt.tokenizer_dir
    unet = UNetModel(**unet_cfg).set_torso(opt.torso)
    vae = AutoencoderKL(**vae_cfg, with_encoder=with_encoder).set_torso(opt.torso)
    if prompt_len is not None and not opt.tokenizer_dir:
        clip_cfg["max_length"] = int(prompt_len)
    clip = cond_cls(device="cpu", **clip_cfg).set_torso(opt.torso)
    if prompt_len is not None and not opt.tokenizer_dir:
        clip._tokenizer = EmptyPromptTokenizer(clip.transformer.plan.vocab_size, pad=0 if cond_cls is FrozenOpenCLIPEmbedder else None)
    if opt.synthetic:
        unet.randomize_(1234)
        vae.randomize_(4321)
        clip.randomize_(2468)
        logger.log(f"--synthetic {opt.synthetic}: the networks hold RANDOM weights (randomize_()); --ckpt is not read")
    unet.to(device)
    vae.to(device)
    clip.to(device)
    model = LatentDiffusion(unet, device=device, first_stage=vae, cond_stage=clip, **ld_cfg)
    if not opt.synthetic:
        print(f"Loading model from {opt.ckpt}")
        pl_sd = torch.load(opt.ckpt, map_location="cpu")
        if "global_step" in pl_sd:
            print(f"Global Step: {pl_sd['global_step']}")
        model.load_state_dict(pl_sd["state_dict"] if "state_dict" in pl_sd else pl_sd, strict=False)
    return model


def build_inception(opt, device, prog="sd_search_ea.py"):
    if not opt.inception_path and not opt.allow_random_inception:
        raise SystemExit(f"{prog}: give --inception_path (the pytorch_fid pt_inception-2015-12-05 state_dict); FID on "
                         "random Inception weights ranks candidates on a meaningless metric (--allow_random_inception opts in "
                         "for throughput runs and tests)")
    net = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[2048]]).to(device)
    if opt.inception_path:
        net.load_state_dict(dist_util.load_state_dict(opt.inception_path))
    else:
        logger.log("WARNING: FID features come from an Inception-v3 with RANDOM weights (--allow_random_inception): "
                   "every fid value below is NOT a quality metric")
    return net


def build_clip_scorer(opt, device, prompt_len=None):
    """--clip_ckpt: the CLIPScorer of both towers from one file (the tiny towers under --synthetic tiny / tiny2)."""
    tiny = opt.synthetic in ("tiny", "tiny2")
    return sd_clip.build_clip_scorer(dist_util.load_state_dict(opt.clip_ckpt),
                                     sd_clip.CLIP_TINY_VISION if tiny else None, sd_clip.CLIP_TINY_TEXT_PROJ if tiny else None,
                                     device=device, torso=opt.torso, tokenizer_dir=opt.tokenizer_dir or None,
                                     max_length=77 if prompt_len is None or opt.tokenizer_dir else int(prompt_len))


# ------------------------------------------------------------------ CMMD (autodiffusion_amd/cmmd.py)
def require_cmmd_flags(opt, prog):
    """--fitness cmmd: the reference embeddings and the CLIP towers that embed the candidate's images."""
    if not getattr(opt, "ref_clip_feats", ""):
        raise SystemExit(f"{prog}: --fitness cmmd needs --ref_clip_feats FILE.npz (scripts/sd_clip_score.py --save_clip_feats writes it)")
    if not opt.clip_ckpt:
        raise SystemExit(f"{prog}: --fitness cmmd needs --clip_ckpt CLIP.pt (the image tower produces the embeddings)")


def save_clip_feats(path, rows):
    """fp32 [N, E] image embeddings -> the .npz array `clip_feats` that cmmd.load_ref_clip_feats reads."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float32))
    if rows.ndim != 2 or rows.shape[0] < 2:
        raise SystemExit(f"--save_clip_feats: need at least 2 images, got rows {rows.shape}")
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:      # an open file: np.savez appends no suffix to the name given
        np.savez(f, clip_feats=rows)
    return path


def add_unipc_flags(parser):
    """--unipc [--unipc_order --unipc_variant --unipc_corrector]: sample with UniPCSampler over DPM-Solver's candidate space.  Absent
    from the namespace unless given: the argument line of log.txt of every other run stays what it was."""
    parser.add_argument("--unipc", action="store_true", default=argparse.SUPPRESS, help="use UniPC sampling (sd_sampler.UniPCSampler)")
    parser.add_argument("--unipc_order", type=int, choices=[1, 2, 3], default=argparse.SUPPRESS, help="UniPC order (2)")
    parser.add_argument("--unipc_variant", choices=["bh1", "bh2"], default=argparse.SUPPRESS, help="UniPC B(h): bh1 = h, bh2 = e^h - 1 (bh2)")
    parser.add_argument("--unipc_corrector", type=str2bool, default=argparse.SUPPRESS, help="apply the corrector (true)")


def unipc_options(opt, prog):
    """The UniPCSampler keywords of the flags, or None with --unipc off; --unipc with --dpm_solver / --plms is refused."""
    if not getattr(opt, "unipc", False):
        given = [k for k in ("unipc_order", "unipc_variant", "unipc_corrector") if hasattr(opt, k)]
        if given:
            raise SystemExit(f"{prog}: --{given[0]} needs --unipc")
        return None
    if getattr(opt, "dpm_solver", False) or getattr(opt, "plms", False):
        raise SystemExit(f"{prog}: --unipc and --dpm_solver / --plms all name the sampler: give one of them")
    return dict(order=getattr(opt, "unipc_order", 2), variant=getattr(opt, "unipc_variant", "bh2"),
                corrector=getattr(opt, "unipc_corrector", True))


def build_sampler(opt, model):
    if getattr(opt, "unipc", False):
        return UniPCSampler(model, **unipc_options(opt, "build_sampler"))
    if opt.dpm_solver:
        return DPMSolverSampler(model)
    if opt.plms:
        return PLMSSampler(model)
    return DDIMSampler(model)
