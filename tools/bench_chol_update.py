"""LLT rank-r update (csrc/chol_update.hip) against refactoring, fp64: for every (N, r) the time of
llt_rank_r_update_clobber, the time of the same call with the tail launches left out (faer_hip_debug_chol_update_diag_only: the
serial chain of diagonal kernels), their difference as the time of the tail kernels with the bytes/s it stands for against the
2 * (N^2 / 2) * 8 B per chunk of W the tails must move, and the time of llt_factor_in_place at the same N from the same run.

Host clock around calls that end in a device synchronise; every shape is warmed up first; the two variants alternate and the
best and the median of `--reps` repetitions are printed.  One JSON line per (N, r) at the end.

    python tools/bench_chol_update.py [--n 4096 16384] [--r 1 8 32] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--r", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    F = ge.load_package()
    torch.cuda.set_device(0)
    F.lib()
    F.use_torch_stream()
    nb, rc = F.chol_update_shape("float64")
    results = []
    for n in args.n:
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=g)
        a = torch.mm(x, x.t())
        a.diagonal().add_(float(n))
        del x
        l0 = a.clone().t()  # (symmetric: the transpose is the same matrix, column major)
        del a
        work = l0.clone()
        t_factor = []
        for rep in range(args.reps + 1):
            work.copy_(l0)
            t = timed(lambda: F.llt_factor_in_place(work))
            if rep:
                t_factor.append(t)
        factor = work.clone()  # the factor the updates start from
        print(f"N={n}: llt_factor_in_place best {min(t_factor):.2f} ms, median {statistics.median(t_factor):.2f} ms", flush=True)
        for r in args.r:
            w0 = torch.randn((r, n), dtype=torch.float64, device="cuda", generator=g).t()
            al0 = torch.rand(r, dtype=torch.float64, device="cuda", generator=g) + 0.5
            w, al = w0.clone(), al0.clone()
            full, diag = [], []
            for rep in range(args.reps + 1):
                for only, out in ((0, full), (1, diag)):
                    work.copy_(factor)
                    w.copy_(w0)
                    al.copy_(al0)
                    F.debug_chol_update_diag_only(bool(only))
                    try:
                        t = timed(lambda: F.llt_rank_r_update_clobber(work, w, al, raise_on_error=False))
                    finally:
                        F.debug_chol_update_diag_only(False)
                    if rep:
                        out.append(t)
            last = F.debug_chol_update_last()
            chunks = -(-r // rc)
            t_full, t_diag = min(full), min(diag)
            t_tail = max(t_full - t_diag, 1e-6)
            nbytes = 2 * (n * n / 2) * 8 * chunks
            rec = {"n": n, "r": r, "nb": nb, "rc": rc, "chunks": chunks, "blocks": last["blocks"], "update_ms_best": round(t_full, 3),
                   "update_ms_median": round(statistics.median(full), 3), "diag_chain_ms_best": round(t_diag, 3),
                   "diag_chain_share": round(t_diag / t_full, 3), "tail_ms": round(t_tail, 3), "tail_bytes": nbytes,
                   "tail_gbytes_per_s": round(nbytes / (t_tail * 1e-3) / 1e9, 1), "llt_factor_ms_best": round(min(t_factor), 3),
                   "llt_factor_ms_median": round(statistics.median(t_factor), 3), "update_over_factor": round(t_full / min(t_factor), 3)}
            results.append(rec)
            print(f"  r={r}: update best {t_full:.2f} ms (median {statistics.median(full):.2f}), diagonal chain alone {t_diag:.2f} ms "
                  f"({100 * t_diag / t_full:.0f} %), tails {t_tail:.2f} ms = {rec['tail_gbytes_per_s']:.0f} GB/s of {nbytes / 1e9:.2f} GB; "
                  f"refactoring {min(t_factor):.2f} ms", flush=True)
        del l0, work, factor
    for rec in results:
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
