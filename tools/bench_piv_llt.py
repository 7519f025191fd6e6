"""A/B timing of piv_llt_factor_in_place against llt_factor_in_place and lblt_factor_in_place (PartialDiag) on the same matrices, fp64,
device-resident operands, one process.  Two inputs per size: full rank (G G^T + n I) and rank n / 8 (G G^T with G n x n / 8), on which
llt reports NonPositivePivot -- its time is still printed, for the columns it got through -- and piv_llt stops at the rank.  Every
factorization works on a fresh device copy of its input (the copy is outside the timed region); a call is timed with the host clock
around a synchronised call, which is what a caller sees -- the pivoted drivers read a few words back per panel.  Median of `--reps`
after one warm-up.  Prints one JSON object; `--out FILE` also writes it.

    python tools/bench_piv_llt.py [--sizes 4096 8192] [--reps 5] [--out profiles/piv_llt_ab.json]
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

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
F = init_gpu()
NB = 64  # panel width of csrc/piv_llt.hip


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


def llt(w):
    try:
        F.llt_factor_in_place(w)
    except F.LltError:
        pass  # the low-rank input


res = {"dtype": "f64", "reps": args.reps, "sizes": {}}
for n in args.sizes:
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    inputs = {"full_rank": g @ g.T + n * np.eye(n), "rank_n_8": g[:, :n // 8] @ g[:, :n // 8].T}
    res["sizes"][str(n)] = {}
    for kind, a in inputs.items():
        dev = to_dev(np.asfortranarray(a))
        sub = torch.zeros(n, dtype=torch.float64, device="cuda")
        r = {}
        r["piv_llt_ms"] = median_ms(dev, lambda w: F.piv_llt_factor_in_place(w), args.reps)
        r["piv_llt_last"] = F.debug_piv_llt_last()
        r["llt_ms"] = median_ms(dev, llt, args.reps)
        r["lblt_ms"] = median_ms(dev, lambda w: F.lblt_factor_in_place(w, subdiag=sub), args.reps)
        r["piv_llt_over_llt"] = r["piv_llt_ms"][0] / r["llt_ms"][0]
        r["launches_per_panel"] = 1 + 2 * NB + 2  # diagonal scan, NB x (pivot, column), interchange, product
        res["sizes"][str(n)][kind] = r
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
