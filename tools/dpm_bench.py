"""Time the pixel-space DPM-Solver launches (csrc/adm_dpm.hip) beside adm_ddim_step, and a guided 64 x 64 DPM loop beside DDIM.

Shapes 256 x 3 x 64^2, 32 x 3 x 128^2, 16 x 3 x 256^2 in one process.  A launch of 10-20 us is shorter than the host takes to issue
it from Python, so every variant is captured once as a hipGraph of GRAPH_LAUNCHES back-to-back launches (they are capturable: no
host synchronisation, no copy) and a timed window is REPLAYS replays of it between two HIP events, a few tenths of a second.  Per
shape the variants' windows alternate (median of --reps, after a warm-up of every graph):
  ddim        adm_ddim_step, guided, want_xstart: reads x, eps (the first C of 2C channels), grad; writes x_prev, pred_xstart
  dpm1        adm_pix_dpm_step, first-order update, unthresholded: reads x, eps, grad; writes m, x_next -- the same five arrays
  dpm2        the same with one history term (a sixth array read)
  dpm2_thr    the thresholded pair: the selection over |x0| (reads x, eps, grad; larger images also write and re-read their keys
              through the work buffer) and the update
  quantile    adm_abs_quantile alone on a plain [n, C h w] array
Bytes are computed from the shapes (4-byte elements; the uint8 pack is off); rate = bytes / time, next to the 8 TB/s HBM3E peak
of the MI355X.  The thresholded pair is also given as a multiple of dpm2 and as a share of one guided step of the headline
(README: 795 images/s at batch 256 = 322 ms per step of 256 images).
--loop: images/s of a guided ADM-G-64 candidate evaluation (synthetic weights, batch --batch, 10 timesteps) under DDIM, DPM-Solver++
order 2, and the same with thresholding, alternating.  Without a GPU the tool fails; it has no fallback.
Usage: python tools/dpm_bench.py [--reps 7] [--loop] [--out profiles/dpm_solver/dpm_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autodiffusion_amd import ops  # noqa: E402
from autodiffusion_amd.sampler import step_coefs  # noqa: E402
from autodiffusion_amd.script_util import create_gaussian_diffusion  # noqa: E402

HBM_PEAK = 8.0e12
HEADLINE_STEP_S = 256 / 795.0
SHAPES = [(256, 3, 64, 64), (32, 3, 128, 128), (16, 3, 256, 256)]
GRAPH_LAUNCHES, REPLAYS = 50, 200


def graphed(fn):
    """GRAPH_LAUNCHES back-to-back calls of fn as one captured graph -> its replay function."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_LAUNCHES):
            fn()
    return g.replay


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def med(v):
    return sorted(v)[len(v) // 2]


def step_rows(reps):
    diffusion = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule="cosine")
    cf = step_coefs(diffusion, 500, learned_range=True, clip_denoised=False)
    rows = []
    for n, c, h, w in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n)
        x, grad, h1 = (torch.randn((n, c, h, w), generator=g, device="cuda") for _ in range(3))
        mo = torch.randn((n, 2 * c, h, w), generator=g, device="cuda")
        per = c * h * w
        work = ops.abs_quantile_work(n, per, x.device)
        kw = dict(alpha_s=0.7, sigma_s=0.714, a=0.9, b0=0.2, b1=-0.05)
        fns = {
            "ddim": lambda: ops.sampler_step("ddim", x, mo, cf, grad, None, want_xstart=True),
            "dpm1": lambda: ops.pix_dpm_step(x, mo, grad, x, None, None, **kw),
            "dpm2": lambda: ops.pix_dpm_step(x, mo, grad, x, h1, None, **kw),
            "dpm2_thr": lambda: ops.pix_dpm_step(x, mo, grad, x, h1, None, thresholding=True, work=work, **kw),
            "quantile": lambda: ops.abs_quantile(x.view(n, per), 0.995, work),
        }
        arrays = {"ddim": 5, "dpm1": 5, "dpm2": 6, "dpm2_thr": 6 + 3 + (3 if per > 12288 else 0), "quantile": 1 if per <= 12288 else 4}
        fns = {k: graphed(f) for k, f in fns.items()}
        for f in fns.values():
            window(f, 3)
        iters = GRAPH_LAUNCHES * REPLAYS
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t[k].append(window(f, REPLAYS) / GRAPH_LAUNCHES)
        row = {"shape": [n, c, h, w], "launches_per_window": iters}
        for k in fns:
            s = med(t[k])
            nbytes = arrays[k] * n * per * 4
            row[k] = {"s": s, "window_s": s * iters, "spread": (max(t[k]) - min(t[k])) / s, "bytes": nbytes,
                      "bytes_per_s": nbytes / s, "frac_hbm_peak": nbytes / s / HBM_PEAK}
        row["dpm1_over_ddim"] = row["dpm1"]["s"] / row["ddim"]["s"]
        row["dpm2_over_ddim"] = row["dpm2"]["s"] / row["ddim"]["s"]
        row["thr_pair_over_dpm2"] = row["dpm2_thr"]["s"] / row["dpm2"]["s"]
        if (n, h) == (256, 64):
            row["thr_pair_share_of_headline_guided_step"] = row["dpm2_thr"]["s"] / HEADLINE_STEP_S
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fns, x, grad, h1, mo, work
        torch.cuda.empty_cache()
    return rows


def loop_rows(reps, batch):
    import bench
    from autodiffusion_amd.evaluate import CandidateEvaluator
    dev = torch.device("cuda:0")
    model, diffusion, clf = bench.build_guided(bench.adm64_flags(class_cond=True), 64, 4, "bf16", "bf16", dev)
    cand = [20, 110, 215, 320, 430, 540, 650, 745, 840, 900]
    evs = {"ddim": CandidateEvaluator(model, diffusion, clf, image_size=64, use_ddim=True, device=dev),
           "dpm2": CandidateEvaluator(model, diffusion, clf, image_size=64, device=dev, sampler="dpm_solver"),
           "dpm2_thr": CandidateEvaluator(model, diffusion, clf, image_size=64, device=dev, sampler="dpm_solver", dpm_thresholding=True)}
    for ev in evs.values():
        ev.set_candidate(cand)
        ev.sample_batch(batch, seed=0)
    torch.cuda.synchronize()
    t = {k: [] for k in evs}
    for r in range(reps):
        for k, ev in evs.items():
            t[k].append(window(lambda: ev.sample_batch(batch, seed=r), 1))
    row = {"loop": "guided ADM-G-64, synthetic weights", "batch": batch, "timesteps": len(cand)}
    for k in evs:
        s = med(t[k])
        row[k] = {"s_per_candidate_batch": s, "images_per_s": batch / s, "spread": (max(t[k]) - min(t[k])) / s}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_bench.py: no GPU (timings are taken on the device or not at all)")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": args.reps,
           "command": "python tools/dpm_bench.py " + " ".join(sys.argv[1:]), "rows": step_rows(args.reps)}
    if args.loop:
        res["loop"] = loop_rows(max(3, args.reps // 2), args.batch)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
