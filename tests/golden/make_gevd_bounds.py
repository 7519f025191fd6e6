#!/usr/bin/env python3
"""Writes tests/golden/gevd_bounds.json and tests/golden/gevd_spectra.npz: for every (kind, n, dtype, seed) of the generalized EVD tests, the residuals of the reference
solver (scipy.linalg.eig on the pair) in the dtype of the case (the JSON file), and its fp64 spectrum (alpha, beta) with the condition numbers
kappa_i of tests/gevd_cases.py (the binary file).  Recorded results only; needs scipy.  Run after changing a case:  python tests/golden/make_gevd_bounds.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gevd_cases as gc  # noqa: E402

EDGES = {np.dtype(np.float64): 64, np.dtype(np.float32): 96}  # faer_hip_gevd_window_edge


def sizes(dtype):
    W = EDGES[np.dtype(dtype)]
    return sorted(set([1, 2, 3, W - 1, W, W + 1, 2 * W + 3, 3 * W + 5] + gc.HOST_SIZES))


def vector_sizes(dtype):
    """sizes of gc.VECTOR_KINDS: the size at which the guard fires, the host's 15 and 35, the GPU's W + 1 for the rotations"""
    return sorted({gc.GUARD_N, 15, 35, EDGES[np.dtype(dtype)] + 1})


def cases(dtype):
    return gc.all_cases(sizes(dtype)) + gc.vector_cases(vector_sizes(dtype))


def main():
    out, arrays = {}, {}
    for dtype in gc.DTYPES:
        for kind, n in cases(dtype):
            key = gc._key(kind, n, dtype)
            out[key], arr = gc.encode(gc._compute(kind, n, dtype))
            arrays[key] = arr
    with open(gc.GOLDEN, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k])}" for k in sorted(out)) + "\n}\n")
    np.savez_compressed(gc.GOLDEN_SPECTRA, **{name: np.concatenate([arrays[k][name] for k in sorted(out)]) for name in ("alpha", "beta", "kappa")})
    print(f"{len(out)} cases, {os.path.getsize(gc.GOLDEN)} + {os.path.getsize(gc.GOLDEN_SPECTRA)} bytes")


if __name__ == "__main__":
    main()
