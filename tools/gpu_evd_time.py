"""timing of libfaer_v0_23_self_adjoint_evd_{f64,f32} (device operands, N = 1024 / 2048 / 4096, with and without U), split
into the tridiagonalization (faer_hip_tridiag_in_place: the driver's first stage), the block Householder back-transform
(apply_householder_on_the_left on the rows 1..n of an n x n U, the driver's last stage) and the rest: the tridiagonal
divide and conquer plus the O(n^2) copies.  Best of 3 after one warm-up call."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from gpu_util import init_gpu, to_dev  # noqa: E402
import torch  # noqa: E402

F = init_gpu()


def best_ms(fn, reps=3):
    fn()
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


args = sys.argv[1:]
rt = None
if args[:1] == ["--rt"]:
    rt, args = int(args[1]), args[2:]
sizes = [int(x) for x in args] or [1024, 2048, 4096]
for dtype in (np.float64, np.float32):
    td = torch.float64 if dtype == np.float64 else torch.float32
    for n in sizes:
        rng = np.random.default_rng(n)
        a = rng.standard_normal((n, n))
        a = np.asarray(a + a.T, dtype=dtype, order="F")
        ad = to_dev(a)
        s = torch.empty(n, dtype=td, device="cuda")
        u = to_dev(np.zeros((n, n), dtype=dtype))
        bs = F.qr_recommended_block_size(n, n, dtype)
        prm = None
        if rt is not None:
            pf = getattr(F.lib(), "libfaer_v0_23_SelfAdjointEvdParams_" + ("f64" if dtype == np.float64 else "f32"))
            pf.restype = F.SelfAdjointEvdParams
            prm = pf()
            prm.recursion_threshold = rt
        t_u = best_ms(lambda: F.self_adjoint_evd(ad, s, u, prm))
        t_no = best_ms(lambda: F.self_adjoint_evd(ad, s, None, prm))
        work, h = ad.clone(), torch.zeros((n - 1, bs), dtype=td, device="cuda").t()

        def trid():
            work.copy_(ad)
            F.tridiag_in_place(work, h)

        t_tr = best_ms(trid)
        t_bt = best_ms(lambda: F.apply_block_householder_sequence_on_the_left_in_place(work[1:, :n - 1], h, u[1:, :]))
        print(f"self_adjoint_evd {np.dtype(dtype).name} n={n}: with U {t_u:.1f} ms = tridiag {t_tr:.1f} + solve {t_u - t_tr - t_bt:.1f} "
              f"+ back-transform {t_bt:.1f}; values only {t_no:.1f} ms = tridiag {t_tr:.1f} + solve {t_no - t_tr:.1f}", flush=True)
