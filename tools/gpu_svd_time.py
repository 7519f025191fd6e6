"""timing of libfaer_v0_23_svd_{f64,f32} (device operands, 1024^2 / 2048^2 / 4096^2 and 16384 x 1024, with thin vectors and
values only), split into the bidiagonalization (faer_hip_bidiag_in_place: the driver's first stage of a squareish matrix),
the two block Householder back-transforms (apply_householder_on_the_left with the left reflectors on U and with the right
ones on rows 1.. of V, the driver's last stage) and the rest: the bidiagonal divide and conquer plus the O(n^2) copies.
A tall matrix (m / n > 11 / 6) goes through the QR factorization first: its split takes the n x n reduction of R and puts
the QR factorization and the application of Q into the rest.  Best of 3 after one warm-up call."""
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
shapes = [tuple(int(v) for v in x.split("x")) for x in args] or [(1024, 1024), (2048, 2048), (4096, 4096), (16384, 1024)]
for dtype in (np.float64, np.float32):
    td = torch.float64 if dtype == np.float64 else torch.float32
    for m, n in shapes:
        rng = np.random.default_rng(m + n)
        ad = to_dev(np.asarray(rng.standard_normal((m, n)), dtype=dtype, order="F"))
        s = torch.empty(n, dtype=td, device="cuda")
        u = to_dev(np.zeros((m, n), dtype=dtype))
        v = to_dev(np.zeros((n, n), dtype=dtype))
        t_uv = best_ms(lambda: F.svd(ad, s, u, v))
        t_no = best_ms(lambda: F.svd(ad, s))
        # the reduction the driver runs: the matrix itself when squareish, the n x n factor R behind the QR pre-step
        mr = m if m / n <= 11.0 / 6.0 else n
        bs = F.qr_recommended_block_size(mr, n, dtype)
        src = ad[:mr, :]
        work = src.clone()
        hl = torch.zeros((n, bs), dtype=td, device="cuda").t()
        hr = torch.zeros((n - 1, bs), dtype=td, device="cuda").t()

        def bid():
            work.copy_(src)
            F.bidiag_in_place(work, hl, hr)

        t_bd = best_ms(bid)
        ur = u[:mr, :]
        t_bu = best_ms(lambda: F.apply_block_householder_sequence_on_the_left_in_place(work, hl, ur))
        t_bv = best_ms(lambda: F.apply_block_householder_sequence_on_the_left_in_place(work[: n - 1, 1:].t(), hr, v[1:, :]))
        print(f"svd {np.dtype(dtype).name} {m}x{n}: with U, V {t_uv:.1f} ms = bidiag {t_bd:.1f} + solve {t_uv - t_bd - t_bu - t_bv:.1f} "
              f"+ back-transforms {t_bu:.1f} + {t_bv:.1f}; values only {t_no:.1f} ms = bidiag {t_bd:.1f} + solve {t_no - t_bd:.1f}", flush=True)
