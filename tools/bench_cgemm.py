"""Complex GEMM (csrc/cgemm.hip) against the composition a caller had to write without it: for c64 and c32, square products at N
and one tall shape, the time of one fused F.matmul on interleaved operands and the time of the same product from real pieces --
the torch passes that split A and B into re / im planes, four real F.matmul calls (Cr = Ar Br - Ai Bi, Ci = Ar Bi + Ai Br, the
second of each pair accumulating) and the torch pass that merges Cr / Ci into the interleaved result.

Host clock around calls that end in a device synchronise; every shape is warmed up first; the two variants alternate and the best
and the median of `--reps` repetitions are printed, with real TFLOP/s counted as 8 m n k flops.  One JSON line per case at the end.

    python tools/bench_cgemm.py [--n 4096] [--tall 16384 512 512] [--reps 7]"""
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


def col_major(shape, dtype, gen=None):
    """a column-major device matrix (faer::Mat order), random if a generator is given"""
    m, n = shape
    if gen is None:
        return torch.empty((n, m), dtype=dtype, device="cuda").t()
    return torch.randn((n, m), dtype=dtype, device="cuda", generator=gen).t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096])
    ap.add_argument("--tall", type=int, nargs=3, default=[16384, 512, 512], metavar=("M", "N", "K"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    F = ge.load_package()
    torch.cuda.set_device(0)
    F.lib()
    F.use_torch_stream()
    results = []
    shapes = [(n, n, n) for n in args.n] + [tuple(args.tall)]
    for cdt, rdt in ((torch.complex128, torch.float64), (torch.complex64, torch.float32)):
        for m, n, k in shapes:
            g = torch.Generator(device="cuda").manual_seed(m + n + k)
            a, b, c = col_major((m, k), cdt, g), col_major((k, n), cdt, g), col_major((m, n), cdt)
            c2 = col_major((m, n), cdt)
            planes = {nm: col_major(sh, rdt) for nm, sh in (("ar", (m, k)), ("ai", (m, k)), ("br", (k, n)), ("bi", (k, n)), ("cr", (m, n)), ("ci", (m, n)))}

            def fused():
                F.matmul(c, F.ACCUM_REPLACE, a, b, 1.0)

            def composed():
                p = planes
                p["ar"].copy_(a.real)
                p["ai"].copy_(a.imag)
                p["br"].copy_(b.real)
                p["bi"].copy_(b.imag)
                F.matmul(p["cr"], F.ACCUM_REPLACE, p["ar"], p["br"], 1.0)
                F.matmul(p["cr"], F.ACCUM_ADD, p["ai"], p["bi"], -1.0)
                F.matmul(p["ci"], F.ACCUM_REPLACE, p["ar"], p["bi"], 1.0)
                F.matmul(p["ci"], F.ACCUM_ADD, p["ai"], p["br"], 1.0)
                c2.real.copy_(p["cr"])
                c2.imag.copy_(p["ci"])

            timed(fused)
            timed(composed)
            scale = float(c2.abs().max())
            diff = float((c - c2).abs().max())
            tf, tc = [], []
            for _ in range(args.reps):
                tf.append(timed(fused))
                tc.append(timed(composed))
            flops = 8.0 * m * n * k
            rec = {"dtype": "c64" if cdt == torch.complex128 else "c32", "m": m, "n": n, "k": k, "fused_ms_best": min(tf),
                   "fused_ms_median": statistics.median(tf), "composed_ms_best": min(tc), "composed_ms_median": statistics.median(tc),
                   "fused_tflops": flops / (min(tf) * 1e-3) / 1e12, "composed_tflops": flops / (min(tc) * 1e-3) / 1e12,
                   "speedup_best": min(tc) / min(tf), "max_abs_diff_over_max_abs": diff / scale if scale else 0.0}
            print(f"{rec['dtype']} {m}x{n}x{k}: fused best {min(tf):.3f} ms ({rec['fused_tflops']:.1f} real TFLOP/s), four real products + "
                  f"split / merge best {min(tc):.3f} ms ({rec['composed_tflops']:.1f}); fused is {rec['speedup_best']:.2f}x; results differ by "
                  f"{rec['max_abs_diff_over_max_abs']:.1e} of the largest entry", flush=True)
            results.append(rec)
            del a, b, c, c2, planes
    for rec in results:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
