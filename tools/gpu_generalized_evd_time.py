"""timing of libfaer_v0_23_generalized_evd_f64 (device operands, N(0,1) entries, N = 256 / 512 / 1024), both vector sets, with the
counters of faer_hip_debug_gevd_last_counts.  The split by stage comes from separate calls:
  values_only  = the QR of B, the reduction and the QZ iteration without the two orthogonal factors
  factors      = t_left - values_only - vectors / 2    what accumulating Q and Z costs in the reduction and the iteration
  vectors      = 2 (t_both - t_left)                    one back substitution + one product each
  qr_of_b      = faer_hip QR of B alone (stage 0 without the applies)
One timed call each after a warm-up at the smallest size; scipy.linalg.eig(a, b) on the same host (LAPACK ggev, all host cores) is
printed beside it for orientation where scipy is installed."""
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


sizes = [int(x) for x in sys.argv[1:]] or [256, 512, 1024]
dtype, td = np.float64, torch.float64
warm = True
for n in sizes:
    rng = np.random.default_rng(n)
    a = np.asarray(rng.standard_normal((n, n)), dtype=dtype, order="F")
    b = np.asarray(rng.standard_normal((n, n)), dtype=dtype, order="F")
    ad, bd = to_dev(a), to_dev(b)
    al, ai, be = (torch.empty(n, dtype=td, device="cuda") for _ in range(3))
    ul, ur = to_dev(np.zeros((n, n), dtype=dtype)), to_dev(np.zeros((n, n), dtype=dtype))
    bs = F.qr_recommended_block_size(n, n, dtype)
    work, h = bd.clone(), torch.zeros((n, bs), dtype=td, device="cuda").t()

    def qr_b():
        work.copy_(bd)
        F.qr_factor_in_place(work, h)

    if warm:
        assert F.generalized_evd(ad, bd, al, ai, be, ul, ur) == F.GEVD_OK
        qr_b()
        warm = False
    t_both = timed_ms(lambda: F.generalized_evd(ad, bd, al, ai, be, ul, ur))
    counts = F.debug_gevd_last_counts()
    t_left = timed_ms(lambda: F.generalized_evd(ad, bd, al, ai, be, ul, None))
    t_vals = timed_ms(lambda: F.generalized_evd(ad, bd, al, ai, be, None, None))
    t_qr = timed_ms(qr_b)
    vec = 2 * (t_both - t_left)
    row = {"n": n, "dtype": "float64", "total_ms": round(t_both, 1), "qr_of_b_ms": round(t_qr, 1), "values_only_ms": round(t_vals, 1),
           "factors_ms": round(t_left - t_vals - vec / 2, 1), "vectors_ms": round(vec, 1), **counts}
    try:
        import scipy.linalg

        t0 = time.perf_counter()
        scipy.linalg.eig(a, b)
        row["scipy_eig_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    except ImportError:
        pass
    print("generalized_evd " + json.dumps(row), flush=True)
