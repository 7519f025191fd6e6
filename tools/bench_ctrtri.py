"""Complex triangular inverse (csrc/ctrtri.hip) next to what a caller had to do without it: solve_triangular_lower_in_place(T, I) on an
identity right-hand side.  For c32 / c64 and lower-triangular T of order N, from the same run on the same box: the time of one
inverse_triangular_in_place into a fresh destination, the time of the solve on a fresh identity, and the ratio t_inverse / t_solve.

Timed with events on the caller's (non-blocking) stream around the call alone -- the refill of the destination / the identity is
outside the events; every case is warmed up first; best and median of `--reps` repetitions.  One JSON line per case at the end.

    python tools/bench_ctrtri.py [--n 1024 4096 8192] [--reps 9]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

DTYPES = (("c32", torch.complex64), ("c64", torch.complex128))


def lower(n, dtype):
    """tril(randn + i randn) / n + I, column major: the matrix of the tests"""
    g = torch.Generator(device="cuda").manual_seed(n)
    a = torch.randn((n, n), dtype=dtype, device="cuda", generator=g).t()
    return (torch.tril(a) / n + torch.eye(n, dtype=dtype, device="cuda")).t().contiguous().t()


def series(reps, prepare, fn):
    out = []
    for i in range(reps + 2):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 2:  # the first two warm up
            out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1024, 4096, 8192])
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    F = ge.load_package()
    torch.cuda.set_device(0)
    F.lib()
    results = []
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        F.use_torch_stream()
        for name, dt in DTYPES:
            for n in args.n:
                t = lower(n, dt)
                w = torch.zeros((n, n), dtype=dt, device="cuda").t()
                x = torch.zeros((n, n), dtype=dt, device="cuda").t()
                eye = torch.eye(n, dtype=dt, device="cuda")
                ti = series(args.reps, lambda: w.zero_(), lambda: F.inverse_triangular_in_place(w, t, upper=False, unit=False))
                ts = series(args.reps, lambda: x.copy_(eye), lambda: F.solve_lower_triangular_in_place(t, x))
                err = float((torch.tril(w) - x).abs().max())
                rec = {"dtype": name, "n": n, "inverse_ms_best": min(ti), "inverse_ms_median": statistics.median(ti), "solve_ms_best": min(ts),
                       "solve_ms_median": statistics.median(ts), "ratio_best": min(ti) / min(ts), "max_abs_diff": err}
                print(f"{name} n={n}: inverse best {min(ti):.3f} ms (median {statistics.median(ti):.3f}); solve on I best {min(ts):.3f} ms "
                      f"(median {statistics.median(ts):.3f}); t_inverse / t_solve = {rec['ratio_best']:.2f}; max |W - X| {err:.2e}", flush=True)
                results.append(rec)
                del t, w, x, eye
    F.use_torch_stream()
    for rec in results:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
