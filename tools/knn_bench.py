"""Time the evaluation suite's k-NN kernels (csrc/adm_knn.hip) against a torch-composed baseline, D = 2048.

  manifold_radii   N = 10 000 and 50 000   (adm_knn_smallest, kk = 4)   vs fp16 torch.mm blocks + torch.topk
  evaluate_pr      10 000 x 50 000 and 50 000 x 50 000 (adm_knn_cover, K = 1)  vs fp16 torch.mm blocks + the comparisons

Rate = 2 n1 n2 D / time as TFLOP/s and as a fraction of the 2.5 PF/s dense fp16 peak.  Kernel and baseline runs alternate in
one process (each timed with HIP events around the whole call, after one warm-up), median of --reps.
Usage: python tools/knn_bench.py [--reps 5] [--out profiles/knn_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autodiffusion_amd import evaluator as ev  # noqa: E402

PEAK = 2.5e15
D = 2048
BLOCK = 10000      # the reference's row / column batch


def feats(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, D), generator=g, device="cuda", dtype=torch.float32) * 0.5


def baseline_radii(x16, kk):
    xn = x16.float().pow(2).sum(1)
    out = []
    for i in range(0, x16.shape[0], BLOCK):
        blk = torch.cat([torch.clamp_min(xn[i:i + BLOCK, None] - 2 * torch.mm(x16[i:i + BLOCK], x16[j:j + BLOCK].T).float()
                                         + xn[None, j:j + BLOCK], 0) for j in range(0, x16.shape[0], BLOCK)], 1)
        out.append(torch.topk(blk, kk, dim=1, largest=False).values)
    return torch.cat(out)


def baseline_cover(a16, ra, b16, rb):
    an, bn = a16.float().pow(2).sum(1), b16.float().pow(2).sum(1)
    a_in = torch.zeros(a16.shape[0], dtype=torch.bool, device="cuda")
    b_in = torch.zeros(b16.shape[0], dtype=torch.bool, device="cuda")
    for i in range(0, a16.shape[0], BLOCK):
        for j in range(0, b16.shape[0], BLOCK):
            d = torch.clamp_min(an[i:i + BLOCK, None] - 2 * torch.mm(a16[i:i + BLOCK], b16[j:j + BLOCK].T).float() + bn[None, j:j + BLOCK], 0)
            a_in[i:i + BLOCK] |= (d <= rb[None, j:j + BLOCK, 0]).any(1)
            b_in[j:j + BLOCK] |= (d <= ra[i:i + BLOCK, 0, None]).any(0)
    return a_in, b_in


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    cases = [("manifold_radii", 10000, 10000), ("manifold_radii", 50000, 50000),
             ("evaluate_pr", 10000, 50000), ("evaluate_pr", 50000, 50000)]
    for what, n1, n2 in cases:
        a = ev._Prepared(feats(n1, 1))
        b = a if (what == "manifold_radii") else ev._Prepared(feats(n2, 2))
        if what == "manifold_radii":
            kern = lambda: ev.knn_smallest(a.x16, a.norm, a.x16, a.norm, 4)
            base = lambda: baseline_radii(a.x16, 4)
        else:
            ra = ev.knn_smallest(a.x16, a.norm, a.x16, a.norm, 4)[:, 3:4].contiguous()
            rb = ev.knn_smallest(b.x16, b.norm, b.x16, b.norm, 4)[:, 3:4].contiguous()
            kern = lambda: ev.knn_cover(a.x16, a.norm, ra, b.x16, b.norm, rb)
            base = lambda: baseline_cover(a.x16, ra, b.x16, rb)
        kern(), base()            # warm-up (code objects, allocator)
        tk, tb = [], []
        for _ in range(args.reps):   # alternate: the same clocks / thermals for both
            tk.append(timed(kern)[0])
            tb.append(timed(base)[0])
        # agreement of the two (the baseline's fp16 torch.mm output is rounded to fp16: a few ties may move)
        rk, rb_ = kern(), base()
        if what == "manifold_radii":
            agree = float((rk - rb_).abs().max())
        else:
            agree = float(sum((x.view(-1) != y.view(-1)).float().mean() for x, y in zip(rk, rb_)) / 2)
        tk, tb = sorted(tk)[len(tk) // 2], sorted(tb)[len(tb) // 2]
        flop = 2.0 * n1 * n2 * D
        row = {"case": what, "n1": n1, "n2": n2, "d": D, "kernel_s": tk, "baseline_s": tb,
               "kernel_tflops": flop / tk / 1e12, "baseline_tflops": flop / tb / 1e12,
               "kernel_frac_fp16_peak": flop / tk / PEAK, "speedup_vs_baseline": tb / tk,
               "splits": ev.knn_splits(n1, n1) if what == "manifold_radii" else None,
               "max_abs_diff_or_flag_mismatch": agree}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del a, b
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "peak_fp16_flops": PEAK, "reps": args.reps, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
