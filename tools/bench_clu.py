"""Complex partial-pivot LU (csrc/cgetrf.hip) next to the real one of the same shape, from the same run on the same box: for
c64 / f64 and c32 / f32, square matrices at N and one tall shape, the time of one partial_piv_lu_factor_in_place on a fresh copy of
the same random matrix, the ratio t_complex / t_real, and -- where torch.linalg.lu_factor takes complex tensors on the box -- its
time as a third column (else the reason it does not).

Host clock around calls that end in a device synchronise (the factorization ends with the read-back of its pivots; the restoring copy
of the input is outside the clock); every shape is warmed up first; best and median of `--reps` repetitions.  A complex LU does
4x the real flops: real TFLOP/s are counted as 4 times the real LU's 2 (m n k - (m + n) k^2 / 2 + k^3 / 3), k = min(m, n) -- (8 / 3) n^3
for a square complex matrix.
One JSON line per case at the end.  `--only N DTYPE` runs one square case a few times and nothing else (the profiler's workload).

    python tools/bench_clu.py [--n 1024 4096 8192] [--tall 16384 512] [--reps 7] [--only 4096 c64]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

PAIRS = (("c64", torch.complex128, "f64", torch.float64), ("c32", torch.complex64, "f32", torch.float32))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def col_major(m, n, dtype, seed):
    return torch.randn((n, m), dtype=dtype, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)).t()


def series(F, src, reps, fn):
    work = torch.empty_like(src.t()).t()
    out = []
    for i in range(reps + 1):
        work.copy_(src)
        t = timed(lambda: fn(work))
        if i:  # the first one warms up
            out.append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1024, 4096, 8192])
    ap.add_argument("--tall", type=int, nargs=2, default=[16384, 512], metavar=("M", "N"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", nargs=2, default=None, metavar=("N", "DTYPE"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    F = ge.load_package()
    torch.cuda.set_device(0)
    F.lib()
    F.use_torch_stream()
    if args.only:
        n, name = int(args.only[0]), args.only[1]
        cdt = dict((p[0], p[1]) for p in PAIRS)[name]
        t = series(F, col_major(n, n, cdt, n), 3, lambda w: F.partial_piv_lu_factor_in_place(w))
        print(f"{name} {n}x{n}: best {min(t):.3f} ms; last call {F.debug_clu_last()}")
        return
    results = []
    shapes = [(n, n) for n in args.n] + [tuple(args.tall)]
    for cname, cdt, rname, rdt in PAIRS:
        for m, n in shapes:
            tc = series(F, col_major(m, n, cdt, m + n), args.reps, lambda w: F.partial_piv_lu_factor_in_place(w))
            last = F.debug_clu_last()
            tr = series(F, col_major(m, n, rdt, m + n), args.reps, lambda w: F.partial_piv_lu_factor_in_place(w))
            k = min(m, n)
            flops = 4.0 * 2.0 * (m * n * k - (m + n) * k * k / 2.0 + k ** 3 / 3.0)
            rec = {"dtype": cname, "real_dtype": rname, "m": m, "n": n, "complex_ms_best": min(tc), "complex_ms_median": statistics.median(tc),
                   "real_ms_best": min(tr), "real_ms_median": statistics.median(tr), "ratio_best": min(tc) / min(tr),
                   "complex_real_tflops": flops / (min(tc) * 1e-3) / 1e12, "panels": last}
            try:
                tt = series(F, col_major(m, n, cdt, m + n), min(args.reps, 3), lambda w: torch.linalg.lu_factor(w))
                rec["torch_ms_best"] = min(tt)
                third = f"torch.linalg.lu_factor best {min(tt):.3f} ms"
            except Exception as e:  # noqa: BLE001 (whatever the box's torch raises: it is reported, not hidden)
                rec["torch_ms_best"] = None
                rec["torch_error"] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
                third = f"torch.linalg.lu_factor does not run here ({rec['torch_error']})"
            print(f"{cname} {m}x{n}: best {min(tc):.3f} ms (median {statistics.median(tc):.3f}, {rec['complex_real_tflops']:.2f} real TFLOP/s); "
                  f"{rname} best {min(tr):.3f} ms; t_complex / t_real = {rec['ratio_best']:.2f}; {third}; panels {last}", flush=True)
            results.append(rec)
    for rec in results:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
