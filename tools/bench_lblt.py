"""A/B timing of lblt_factor_in_place (PartialDiag, Gaussian symmetric) against the unpivoted ldlt_factor_in_place (SPD input) and
partial_piv_lu_factor_in_place (the same Gaussian matrix), fp64, device-resident operands, one process.  Every factorization works
on a fresh device copy of its input (the copy is outside the timed region); a call is timed with the host clock around a
synchronised call, which is what a caller sees -- the pivoted drivers read a few words back.  Median of `--reps` after one warm-up.
The lblt time is split with the kernel-class profile: class 0 holds the MFMA products (the trailing triangular updates), the rest
is the panel chain, the interchanges and the leaf.  Prints one JSON object; `--out FILE` also writes it.

    python tools/bench_lblt.py [--sizes 1024 4096 8192] [--reps 5] [--out profiles/lblt_ab.json]
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
ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096, 8192])
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


res = {"dtype": "f64", "reps": args.reps, "sizes": {}}
for n in args.sizes:
    g = np.random.default_rng(n).standard_normal((n, n))
    sym = to_dev(np.asfortranarray((g + g.T) / 2))
    spd = to_dev(np.asfortranarray(g @ g.T + n * np.eye(n)))
    sub = torch.zeros(n, dtype=torch.float64, device="cuda")
    r = {}
    r["lblt_ms"] = median_ms(sym, lambda w: F.lblt_factor_in_place(w, subdiag=sub), args.reps)
    r["lblt_last"] = F.debug_lblt_last()
    r["ldlt_ms"] = median_ms(spd, lambda w: F.ldlt_factor_in_place(w), args.reps)
    r["lu_ms"] = median_ms(sym, lambda w: F.partial_piv_lu_factor_in_place(w), args.reps)
    work = sym.clone()
    F.synchronize()
    F.prof_begin()
    t0 = time.perf_counter()
    F.lblt_factor_in_place(work, subdiag=sub)
    F.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    prof = F.prof_end()
    r["lblt_profiled"] = {"total_ms": total, "classes": prof}
    panels = r["lblt_last"][0]
    r["launches_per_panel"] = 1 + 3 * 63 + 2  # init, 63 x (two column passes, pivot), product, interchange
    r["panels"] = panels
    res["sizes"][str(n)] = r
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
