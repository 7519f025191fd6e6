"""timing of libfaer_v0_23_evd_f64 (device operands, N(0,1) entries, N = 512 / 1024 / 2048), both vector sets, split into the
Hessenberg reduction (faer_hip_hessenberg_in_place: the driver's first stage), the real Schur decomposition (with the number
of sweeps, window steps, leaf launches and host read-backs of faer_hip_debug_evd_last_counts) and the eigenvectors.  The
split comes from four calls: both vector sets (t_both), UL only (t_left), values only (t_vals), the reduction alone (t_hess):
  vectors      = 2 (t_both - t_left)            one back substitution + one triangular product each
  schur with Z = t_both - t_hess - vectors      includes forming Z from the reflectors
  schur, no Z  = t_vals - t_hess
One timed call each after a warm-up at the smallest size (a sweep count does not change between calls); numpy's eig (LAPACK
geev, all host cores) on the same matrix is printed beside it for orientation only."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from gpu_util import init_gpu, to_dev  # noqa: E402
import torch  # noqa: E402

F = init_gpu()


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


sizes = [int(x) for x in sys.argv[1:]] or [512, 1024, 2048]
dtype, td = np.float64, torch.float64
warm = True
for n in sizes:
    a = np.asarray(np.random.default_rng(n).standard_normal((n, n)), dtype=dtype, order="F")
    ad = to_dev(a)
    s, si = torch.empty(n, dtype=td, device="cuda"), torch.empty(n, dtype=td, device="cuda")
    ul, ur = to_dev(np.zeros((n, n), dtype=dtype)), to_dev(np.zeros((n, n), dtype=dtype))
    bs = F.qr_recommended_block_size(n - 1, n - 1, dtype)
    work, h = ad.clone(), torch.zeros((n - 1, bs), dtype=td, device="cuda").t()

    def hess():
        work.copy_(ad)
        F.hessenberg_in_place(work, h)

    if warm:
        assert F.evd(ad, s, si, ul, ur) == F.EVD_OK
        hess()
        warm = False
    t_both = timed_ms(lambda: F.evd(ad, s, si, ul, ur))
    counts = F.debug_evd_last_counts()
    t_left = timed_ms(lambda: F.evd(ad, s, si, ul, None))
    t_vals = timed_ms(lambda: F.evd(ad, s, si, None, None))
    t_hess = timed_ms(hess)
    t0 = time.perf_counter()
    np.linalg.eig(a)
    t_np = (time.perf_counter() - t0) * 1e3
    vec = 2 * (t_both - t_left)
    row = {"n": n, "dtype": "float64", "total_ms": round(t_both, 1), "hessenberg_ms": round(t_hess, 1), "schur_with_z_ms": round(t_both - t_hess - vec, 1),
           "vectors_ms": round(vec, 1), "values_only_ms": round(t_vals, 1), "schur_no_z_ms": round(t_vals - t_hess, 1), **counts,
           "numpy_eig_host_ms": round(t_np, 1)}
    print("general_evd " + json.dumps(row), flush=True)
