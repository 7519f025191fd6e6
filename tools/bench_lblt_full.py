"""Timing of lblt_factor_in_place with the Full pivoting strategy (csrc/lblt.hip), with the full-pivot LU (csrc/fplu.hip) on the same
matrices beside it: both are level-2 algorithms whose every step is one pass over the trailing matrix, the LU over the whole trailing
square (about twice the bytes of the trailing triangle).  Symmetric Gaussian matrices, fp64 and fp32, device-resident operands, one
process.  Every factorization works on a fresh device copy of its input (the copy is outside the timed region); a call is timed with
the host clock around a synchronised call, which is what a caller sees.  Median of `--reps` after one warm-up.

Modelled traffic of the Full strategy: every step reads and writes the strict lower triangle of the trailing matrix once, so a run
whose steps leave trailing sizes m_1, m_2, ... moves sum 2 (m_s (m_s - 1) / 2) sizeof(T) bytes; with 1 x 1 pivots only that is
about n^3 / 3 sizeof(T), and a 2 x 2 pivot saves one of two passes.  The model below takes the 1 x 1 sum over the rows the
multi-workgroup path handled (an upper bound of its traffic), and reports it against the HBM rate bench.py uses (HBM_PEAK_GBS).
Launches: 3 before the loop, 2 per launched step (steps are launched for the host's lower bound of k, so a run with 2 x 2 pivots
launches surplus steps that return at once), the leaf, the unscaling.  Prints one JSON object; `--out FILE` also writes it.

    python tools/bench_lblt_full.py [--sizes 1024 2048 4096] [--reps 5] [--out profiles/lblt_full.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import init_gpu, to_dev  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 2048, 4096])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
F = init_gpu()


def median_ms(src, fn, reps):
    work = src.clone()
    times = []
    for i in range(reps + 1):
        work.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(work)
        F.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


res = {"reps": args.reps, "hbm_peak_gbs": HBM_PEAK_GBS, "sizes": {}}
for n in args.sizes:
    g = np.random.default_rng(n).standard_normal((n, n))
    a = (g + g.T) / 2.0
    res["sizes"][str(n)] = {}
    for dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        dev = to_dev(np.asfortranarray(a.astype(dtype)))
        sub = torch.zeros(n, dtype=tdt, device="cuda")
        isz = np.dtype(dtype).itemsize
        r = {}
        r["lblt_full_ms"] = median_ms(dev, lambda w: F.lblt_factor_in_place(w, subdiag=sub, pivoting="full"), args.reps)
        steps, leaf_rows, n2, syncs = F.debug_lblt_last()
        rows = n - leaf_rows  # rows of the multi-workgroup path
        model_bytes = sum(2.0 * (n - k - 1) * (n - k - 2) / 2.0 * isz for k in range(rows))
        gbs = model_bytes / (r["lblt_full_ms"][0] * 1e-3) / 1e9
        r.update({"steps": steps, "leaf_rows": leaf_rows, "pivots_2x2": n2, "host_syncs": syncs, "model_bytes": model_bytes,
                  "model_gbs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)})
        r["launches_lower_bound"] = 3 + 2 * steps + 2
        r["launches_upper_bound"] = 3 + 2 * rows + 2
        r["us_per_step"] = round(r["lblt_full_ms"][0] * 1e3 / max(steps, 1), 2)
        r["lblt_partial_diag_ms"] = median_ms(dev, lambda w: F.lblt_factor_in_place(w, subdiag=sub), args.reps)
        r["fplu_ms"] = median_ms(dev, lambda w: F.full_piv_lu_factor_in_place(w), args.reps)
        r["fplu_model_bytes"] = sum(2.0 * (n - k - 1) ** 2 * isz for k in range(n))
        r["fplu_model_gbs"] = round(r["fplu_model_bytes"] / (r["fplu_ms"][0] * 1e-3) / 1e9, 1)
        res["sizes"][str(n)][np.dtype(dtype).name] = r
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
