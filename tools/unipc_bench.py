"""Time the fused UniPC launch (adm_pix_unipc_step, csrc/adm_dpm.hip) beside the two adm_pix_dpm_step launches that compute the same
two states, and beside adm_ddim_step; and a guided 64 x 64 candidate under --unipc beside --dpm_solver.

tools/dpm_bench.py's protocol: shapes 256 x 3 x 64^2, 32 x 3 x 128^2, 16 x 3 x 256^2 in one process; every variant is captured once
as a hipGraph of GRAPH_LAUNCHES back-to-back calls and a timed window is REPLAYS replays of it between two HIP events; per shape the
variants' windows alternate (median of --reps, after a warm-up of every graph).  An evaluation of order 2 with the corrector on:
  ddim          adm_ddim_step, guided, want_xstart: 5 arrays (reads x, eps, grad; writes x_prev, pred_xstart)
  unipc         one adm_pix_unipc_step: reads x_eval, eps, grad, x_base, h1, h2; writes m, x_corr, x_pred -- 9 arrays
  dpm_pair      adm_pix_dpm_step twice: x_corr = ac x_base + c0 m + c1 h1 + c2 h2 (6 reads, 2 writes), then x_pred = ap x_corr + p0 m +
                p1 h1 (5 reads, 2 writes) -- 15 arrays; the only formulation without the fused kernel
  unipc_thr     the thresholded fused evaluation: the selection launch and the update
  dpm_pair_thr  the thresholded pair: the selection runs twice
Bytes are computed from the shapes (4-byte elements; the uint8 pack is off; the selection's traffic as tools/dpm_bench.py counts
it); rate = bytes / time next to the 8 TB/s HBM3E peak of the MI355X.
--loop: images/s of a guided ADM-G-64 candidate evaluation (synthetic weights, batch --batch, 10 timesteps) under DPM-Solver++
order 2 and UniPC order 2 (bh2, corrector on), alternating.  Without a GPU the tool fails; it has no fallback.
Usage: python tools/unipc_bench.py [--reps 7] [--loop] [--out profiles/unipc/unipc_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from autodiffusion_amd import ops  # noqa: E402
from autodiffusion_amd.sampler import step_coefs  # noqa: E402
from autodiffusion_amd.script_util import create_gaussian_diffusion  # noqa: E402
from dpm_bench import GRAPH_LAUNCHES, HBM_PEAK, REPLAYS, SHAPES, graphed, med, window  # noqa: E402

CORR = (0.9, 0.2, -0.15, 0.03, 0.0)
PRED = (0.8, 0.3, -0.1, 0.0)


def step_rows(reps):
    diffusion = create_gaussian_diffusion(steps=1000, learn_sigma=True, noise_schedule="cosine")
    cf = step_coefs(diffusion, 500, learned_range=True, clip_denoised=False)
    rows = []
    for n, c, h, w in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n)
        x, xb, grad, h1, h2 = (torch.randn((n, c, h, w), generator=g, device="cuda") for _ in range(5))
        mo = torch.randn((n, 2 * c, h, w), generator=g, device="cuda")
        per = c * h * w
        work = ops.abs_quantile_work(n, per, x.device)
        kw = dict(alpha_s=0.7, sigma_s=0.714)

        def pair(**thr):
            _, x_corr, _, _ = ops.pix_dpm_step(x, mo, grad, xb, h1, h2, a=CORR[0], b0=CORR[1], b1=CORR[2], b2=CORR[3], **kw, **thr)
            return ops.pix_dpm_step(x, mo, grad, x_corr, h1, None, a=PRED[0], b0=PRED[1], b1=PRED[2], **kw, **thr)

        fns = {
            "ddim": lambda: ops.sampler_step("ddim", x, mo, cf, grad, None, want_xstart=True),
            "unipc": lambda: ops.pix_unipc_step(x, mo, grad, xb, h1, h2, None, corr=CORR, pred=PRED, **kw),
            "dpm_pair": pair,
            "unipc_thr": lambda: ops.pix_unipc_step(x, mo, grad, xb, h1, h2, None, corr=CORR, pred=PRED, thresholding=True, work=work, **kw),
            "dpm_pair_thr": lambda: pair(thresholding=True, work=work),
        }
        sel = 3 + (3 if per > 12288 else 0)      # one selection: reads x, eps, grad; larger images write and re-read their keys twice
        arrays = {"ddim": 5, "unipc": 9, "dpm_pair": 15, "unipc_thr": 9 + sel, "dpm_pair_thr": 15 + 2 * sel}
        # the same two states from both formulations, on the operands that are timed
        _, uc, up, _, _ = fns["unipc"]()
        _, pp, _, _ = fns["dpm_pair"]()
        same = bool(torch.equal(up, pp))
        fns = {k: graphed(f) for k, f in fns.items()}
        for f in fns.values():
            window(f, 3)
        iters = GRAPH_LAUNCHES * REPLAYS
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t[k].append(window(f, REPLAYS) / GRAPH_LAUNCHES)
        row = {"shape": [n, c, h, w], "evaluations_per_window": iters, "fused_equals_pair_bitwise": same}
        for k in fns:
            s = med(t[k])
            nbytes = arrays[k] * n * per * 4
            row[k] = {"s": s, "window_s": s * iters, "spread": (max(t[k]) - min(t[k])) / s, "bytes": nbytes,
                      "bytes_per_s": nbytes / s, "frac_hbm_peak": nbytes / s / HBM_PEAK}
        row["unipc_over_dpm_pair"] = row["unipc"]["s"] / row["dpm_pair"]["s"]
        row["unipc_thr_over_dpm_pair_thr"] = row["unipc_thr"]["s"] / row["dpm_pair_thr"]["s"]
        row["unipc_over_ddim"] = row["unipc"]["s"] / row["ddim"]["s"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fns, x, xb, grad, h1, h2, mo, work
        torch.cuda.empty_cache()
    return rows


def loop_rows(reps, batch):
    import bench
    from autodiffusion_amd.evaluate import CandidateEvaluator
    dev = torch.device("cuda:0")
    model, diffusion, clf = bench.build_guided(bench.adm64_flags(class_cond=True), 64, 4, "bf16", "bf16", dev)
    cand = [20, 110, 215, 320, 430, 540, 650, 745, 840, 900]
    evs = {"dpm2": CandidateEvaluator(model, diffusion, clf, image_size=64, device=dev, sampler="dpm_solver"),
           "unipc2": CandidateEvaluator(model, diffusion, clf, image_size=64, device=dev, sampler="unipc")}
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
    row["unipc2_over_dpm2"] = row["unipc2"]["s_per_candidate_batch"] / row["dpm2"]["s_per_candidate_batch"]
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
        raise SystemExit("unipc_bench.py: no GPU (timings are taken on the device or not at all)")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "reps": args.reps,
           "command": "python tools/unipc_bench.py " + " ".join(sys.argv[1:]), "rows": step_rows(args.reps)}
    if args.loop:
        res["loop"] = loop_rows(max(3, args.reps // 2), args.batch)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
