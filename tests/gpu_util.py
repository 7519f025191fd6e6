"""helpers shared by the -m gpu parity tests (device tensors are column major like faer::Mat)."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

EPS = {np.dtype(np.float64): np.finfo(np.float64).eps, np.dtype(np.float32): np.finfo(np.float32).eps}


def fa():
    return ge.load_package()


def init_gpu():
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    m = fa()
    m.lib()
    m.use_torch_stream()
    return m


def to_dev(x, order="F"):
    """numpy 2-D array -> torch cuda tensor with the requested memory order (same logical values)."""
    import torch

    x = np.asarray(x)
    if order == "F":
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(t):
    fa().synchronize()
    return t.detach().cpu().numpy()


def rnd(rng, m, n, dtype=np.float64, order="F"):
    return np.asarray(rng.standard_normal((m, n)), dtype=dtype, order=order)


def spd(rng, n, dtype=np.float64):
    a = rng.standard_normal((n, n))
    return np.asarray(a @ a.T + n * np.eye(n), dtype=dtype, order="F")


# ---- route counters of the GEMM / TRSM dispatch (faer_hip_debug_route_counts)
def route_names():
    """FaerHipRoute_* in enum order, read from the header (like test_cabi.py reads the exports)"""
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    vals = {int(v): k for k, v in re.findall(r"FaerHipRoute_(\w+)\s*=\s*(\d+)", hdr) if k != "Count"}
    assert sorted(vals) == list(range(len(vals)))
    return [vals[i] for i in range(len(vals))]


ROUTES = route_names()


class Routes:
    """with Routes(F) as r: ...  -- r.hits: {route name: launches} of the calls inside (this thread)"""

    def __init__(self, F):
        self.F = F
        self.lib = F.lib()
        self.lib.faer_hip_debug_route_counts.restype = C.c_size_t

    def __enter__(self):
        self.F.synchronize()
        self.lib.faer_hip_debug_route_reset()
        return self

    def __exit__(self, *exc):
        self.F.synchronize()
        buf = (C.c_longlong * len(ROUTES))()
        assert self.lib.faer_hip_debug_route_counts(buf, len(ROUTES)) == len(ROUTES)
        self.hits = dict(zip(ROUTES, buf))
        return False

    def assert_hit(self, *names):
        missing = [r for r in names if self.hits[r] <= 0]
        assert not missing, (missing, {k: v for k, v in self.hits.items() if v})
