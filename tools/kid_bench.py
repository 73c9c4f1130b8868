"""Time the KID kernel sums (csrc/adm_kid.hip, adm_poly3_sums) against the plain torch formulation, d = 2048.

  cross sum   (n, m) = (64, 10000) and (1000, 10000)    S_xy: the search's per-candidate call, and one subset of the evaluator's
  self sum    n = 10000                                  S_yy: computed once per reference set

Baseline, on the same device: ((x.double() @ y.double().T) / d + 1).pow(3).sum() -- a float64 rocBLAS GEMM that writes the n x m
matrix (800 MB at 10000 x 10000) and elementwise passes over it; for the self sum the diagonal's terms are subtracted afterwards.
Rate = algorithmic FLOP / time: 2 n m d for a cross sum, n (n - 1) d for the self sum (each unordered pair once), as TFLOP/s and
as a fraction of the 78.6 TFLOP/s float64 matrix peak AMD publishes for the MI355X (the MFMA bound; the inputs are a few tens of
MB, so HBM does not bound any of the three).  Each timed window is a fixed number of back-to-back calls (CASES) between two HIP events ending in
a synchronise (a few tenths of a second: printed per row as kernel_window_s / baseline_window_s), kernel and baseline windows alternate in
one process after a warm-up of both, median of --reps.  Without a GPU the tool fails; it has no fallback.
Usage: python tools/kid_bench.py [--reps 7] [--out profiles/kid/kid_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autodiffusion_amd import kid, ops  # noqa: E402

PEAK_F64_MATRIX = 78.6e12
D = 2048
CASES = [("cross", 64, 10000, 2000), ("cross", 1000, 10000, 400), ("self", 10000, 10000, 80)]     # (mode, n, m, calls per timed window)


def feats(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.relu(torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)) * 0.6


def baseline(x, y):
    if y is None:
        xd = x.double()
        full = ((xd @ xd.T) / D + 1).pow(3).sum()
        return full - ((xd * xd).sum(1) / D + 1).pow(3).sum()
    return ((x.double() @ y.double().T) / D + 1).pow(3).sum()


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
        raise SystemExit("kid_bench.py: no GPU (timings are taken on the device or not at all)")
    torch.cuda.set_device(0)
    rows = []
    for mode, n, m, iters in CASES:
        x = feats(n, 1)
        y = None if mode == "self" else feats(m, 2)
        kern = lambda: ops.poly3_sums(x, y)           # noqa: E731
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
        row = {"case": mode, "n": n, "m": m, "d": D, "blocks": kid.poly3_blocks(n, m, mode == "self"), "kernel_s": tk, "baseline_s": tb,
               "kernel_window_s": tk * iters, "baseline_window_s": tb * base_iters, "kernel_spread": spread,
               "kernel_tflops": flop / tk / 1e12, "baseline_tflops": flop / tb / 1e12, "kernel_frac_f64_matrix_peak": flop / tk / PEAK_F64_MATRIX,
               "speedup_vs_baseline": tb / tk, "rel_diff_kernel_vs_baseline": abs(sk - sb) / abs(sb),
               "matrix_bytes_not_written": 8.0 * n * m}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, y
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "peak_f64_matrix_flops": PEAK_F64_MATRIX, "reps": args.reps,
           "command": "python tools/kid_bench.py " + " ".join(sys.argv[1:]), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
