"""Time the CMMD kernel sums (csrc/adm_cmmd.hip, adm_rbf_sums) against the plain torch formulation, d = 768 (CLIP ViT-L/14's
projection width) -- the three calls a candidate makes against a 30 000-image reference set:

  cross sum   (n, m) = (1000, 30000) and (5000, 30000)    S_xy: a candidate's embeddings against the reference's
              (64, 30000)                                  one row tile: 469 blocks for 256 CUs (recorded, not tuned)
  self sum    n = 30000                                     S_yy: computed once per reference set

Baseline, on the same device: rows normalised in float64, torch.expm1(-g * (2 - 2 * (xn @ yn.T)).clamp_min(0)).sum() -- a float64
rocBLAS GEMM that writes the n x m matrix (7.2 GB at 30000 x 30000) and elementwise passes over it; for the self sum the diagonal's
terms are subtracted afterwards.  Rate = the Gram's algorithmic FLOP / time: 2 n m d for a cross sum, n (n - 1) d for the self sum
(each unordered pair once), as TFLOP/s and as a fraction of the 78.6 TFLOP/s float64 matrix peak AMD publishes for the MI355X.  The
rate leaves out the epilogue (a float64 sqrt, division and expm1 per entry, on the vector pipe): at d = 768 it is a visible share of
the kernel's time, so the fraction of the matrix peak is lower than KID's at d = 2048 by construction.  Each timed window is a fixed
number of back-to-back calls (CASES) between two HIP events ending in a synchronise; kernel and baseline windows alternate in one
process after a warm-up of both, median of --reps.  Without a GPU the tool fails; it has no fallback.
Usage: python tools/cmmd_bench.py [--reps 7] [--out profiles/cmmd/cmmd_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autodiffusion_amd import cmmd, ops  # noqa: E402

PEAK_F64_MATRIX = 78.6e12
D = 768
GAMMA = cmmd.gamma_of(cmmd.SIGMA)
CASES = [("cross", 64, 30000, 4000), ("cross", 1000, 30000, 600), ("cross", 5000, 30000, 120), ("self", 30000, 30000, 40)]     # (mode, n, m, calls per timed window)


def feats(n, seed):
    """CLIP-like rows: a common direction plus noise, norms near 10."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mu = torch.randn((1, D), generator=torch.Generator(device="cuda").manual_seed(99), device="cuda", dtype=torch.float32)
    z = torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)
    return (10.0 * (0.8 * mu / mu.norm() + 0.6 * z / z.norm(dim=1, keepdim=True))).contiguous()


def baseline(x, y):
    xn = x.double()
    xn = xn / xn.norm(dim=1, keepdim=True)
    if y is None:
        full = torch.expm1(-GAMMA * (2 - 2 * (xn @ xn.T)).clamp_min(0)).sum()
        return full - torch.expm1(-GAMMA * (2 - 2 * (xn * xn).sum(1)).clamp_min(0)).sum()
    yn = y.double()
    yn = yn / yn.norm(dim=1, keepdim=True)
    return torch.expm1(-GAMMA * (2 - 2 * (xn @ yn.T)).clamp_min(0)).sum()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cmmd_bench.py: no GPU (timings are taken on the device or not at all)")
    torch.cuda.set_device(0)
    rows = []
    for mode, n, m, iters in CASES:
        x = feats(n, 1)
        y = None if mode == "self" else feats(m, 2)
        kern = lambda: ops.rbf_sums(x, y, GAMMA)      # noqa: E731
        base = lambda: baseline(x, y)                 # noqa: E731
        base_iters = max(1, iters // 2)
        window(kern, 2), window(base, 2)              # warm-up: code objects, rocBLAS's algorithm choice, the allocator
        tk, tb = [], []
        for _ in range(args.reps):                    # alternate: the same clocks for both
            tk.append(window(kern, iters)[0])
            tb.append(window(base, base_iters)[0])
        sk, sb = float(kern().item()), float(base().item())
        spread = (max(tk) - min(tk)) / sorted(tk)[len(tk) // 2]
        tk, tb = sorted(tk)[len(tk) // 2], sorted(tb)[len(tb) // 2]
        flop = float(n) * (n - 1) * D if mode == "self" else 2.0 * n * m * D
        row = {"case": mode, "n": n, "m": m, "d": D, "blocks": cmmd.rbf_blocks(n, m, mode == "self"), "kernel_s": tk, "baseline_s": tb,
               "kernel_window_s": tk * iters, "baseline_window_s": tb * base_iters, "kernel_spread": spread,
               "kernel_tflops": flop / tk / 1e12, "baseline_tflops": flop / tb / 1e12, "kernel_frac_f64_matrix_peak": flop / tk / PEAK_F64_MATRIX,
               "speedup_vs_baseline": tb / tk, "rel_diff_kernel_vs_baseline": abs(sk - sb) / abs(sb),
               "matrix_bytes_not_written": 8.0 * n * m}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, y
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "peak_f64_matrix_flops": PEAK_F64_MATRIX, "reps": args.reps, "sigma": cmmd.SIGMA,
           "command": "python tools/cmmd_bench.py " + " ".join(sys.argv[1:]), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
