"""The bodies of csrc/qz_core.h on the host: tests/host/qz_host.cpp instantiates them with HostGroup (one thread, no barrier) and
runs the Hessenberg-triangular reduction, the sweep driver (scan, shifts, window steps, leaves) and the eigenvectors of a pair whose B is triangular (stage 0, the QR of
B, is numpy's here).  No GPU.  Every kind of tests/gevd_cases.py at n = 1, 2, 3, 15, 16, 17, 35 with edge 16, under both verdicts;
the decomposition itself (A = Q S Z^T, B = Q P Z^T, the form of S and P); the iteration cap; the deflation of an infinite
eigenvalue at the bottom and in the interior of the pair; the `random` kind as (A 2^ka, B 2^kb) at every row of gc.RANGE_SCALES,
n = 15 (one leaf), 17 and 35 (windows); the kinds built for the eigenvector stage (gc.VECTOR_KINDS)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gevd_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "qz_host.cpp")
INC = os.path.join(ROOT, "faer-rs_amd", "csrc")
EDGE = 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("qz_host") / "qz_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", str(out)], check=True, capture_output=True, text=True)
    return str(out)


def run(exe, tmp_path, a, b, dtype, cap=0, pre_qr=True):
    """the host program on (a, b) in `dtype`: stage 0 in numpy (fp64, rounded to dtype), stages 1 to 3 in the program"""
    n = a.shape[0]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    q0 = np.eye(n)
    if pre_qr:
        q0, r = np.linalg.qr(b64)
        a64, b64 = q0.T @ a64, np.triu(r)
    a64, b64 = a64.astype(dtype).astype(np.float64), b64.astype(dtype).astype(np.float64)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([[float(n)], a64.ravel(order="F"), b64.ravel(order="F")]).tofile(fin)
    subprocess.run([exe, "f64" if np.dtype(dtype) == np.float64 else "f32", str(EDGE), str(cap), str(fin), str(fout)], check=True)
    o = np.fromfile(fout)
    out = {"status": int(o[0]), "sweeps": int(o[1]), "infinite": int(o[2]), "leaves": int(o[3]), "a_in": a64, "b_in": b64}
    out["window_steps"] = int(o[4])
    o = o[5:]
    out["alpha"], out["alpha_im"], out["beta"] = (o[k * n:(k + 1) * n].astype(dtype) for k in range(3))
    o = o[3 * n:]
    names = ["ur", "ul", "s", "p", "q", "z"]
    for k, name in enumerate(names):
        out[name] = o[k * n * n:(k + 1) * n * n].reshape(n, n, order="F")
    out["ul"] = q0 @ out["ul"]
    return out


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind,n", gc.all_cases(gc.HOST_SIZES))
def test_kinds_pass_both_verdicts(exe, tmp_path, kind, n, dtype):
    a, b = gc.generate(kind, n, dtype)
    r = run(exe, tmp_path, a, b, dtype)
    assert r["status"] == 0
    e = gc.eps_of(dtype)
    # the decomposition of the pair the program was given
    for m, f in ((r["a_in"], r["s"]), (r["b_in"], r["p"])):
        assert np.abs(r["q"] @ f @ r["z"].T - m).max() <= 40 * n * e * max(np.abs(m).max(), 1e-300)
    assert np.abs(r["q"].T @ r["q"] - np.eye(n)).max() <= 40 * n * e and np.abs(r["z"].T @ r["z"] - np.eye(n)).max() <= 40 * n * e
    assert (np.tril(r["s"], -2) == 0).all() and (np.tril(r["p"], -1) == 0).all() and (r["beta"] >= 0).all()
    sub = np.nonzero(np.diag(r["s"], -1))[0]
    assert (np.diff(sub) > 1).all()  # no two 2 x 2 blocks overlap
    for i in sub:  # a 2 x 2 block is a conjugate pair over a positive diagonal block of P
        assert r["p"][i, i + 1] == 0 and r["p"][i, i] > 0 and r["p"][i + 1, i + 1] > 0 and r["alpha_im"][i] > 0
    gc.check(kind, n, dtype, a, b, r["alpha"], r["alpha_im"], r["beta"], r["ur"].astype(dtype), r["ul"].astype(dtype))
    if kind == "triangular_pair":
        assert r["sweeps"] == 0
    elif n - (gc.singular_count(kind, n) if kind.startswith("singular_b") else 0) > EDGE:  # a block of more than EDGE rows takes multishift sweeps in windows
        assert r["sweeps"] > 0 and r["window_steps"] > r["sweeps"]
    if kind == "scaled":  # A 2^k, B 2^-k: every step scales by a power of two, so alpha and beta scale exactly
        r0 = run(exe, tmp_path, *gc.generate("random", n, dtype), dtype)
        assert np.array_equal(np.ldexp(r0["alpha"], gc.SCALE_K), r["alpha"]) and np.array_equal(np.ldexp(r0["beta"], -gc.SCALE_K), r["beta"])
    if kind.startswith("singular_b"):
        assert r["infinite"] >= gc.singular_count(kind, n)
    if kind == "identity_b":
        lam = np.sort_complex((r["alpha"].astype(np.float64) + 1j * r["alpha_im"]) / r["beta"])
        assert np.abs(lam - np.sort_complex(np.linalg.eigvals(a.astype(np.float64)))).max() <= 1e3 * n * e * np.linalg.norm(a)


_UNSCALED = {}


def unscaled_run(exe, tmp_path, n, dtype):
    """the result on the `random` pair itself, once per size and dtype"""
    key = (n, np.dtype(dtype).name)
    if key not in _UNSCALED:
        _UNSCALED[key] = run(exe, tmp_path, *gc.generate("random", n, dtype), dtype)
    return _UNSCALED[key]


RANGE = [(n, dtype, group, ka, kb) for dtype in gc.DTYPES for n in gc.RANGE_HOST_SIZES for group, ka, kb in gc.range_rows(dtype)]


@pytest.mark.parametrize("n,dtype,group,ka,kb", RANGE, ids=[f"{n}-{np.dtype(d).name}-{g}-{ka}-{kb}" for n, d, g, ka, kb in RANGE])
def test_range_rows(exe, tmp_path, n, dtype, group, ka, kb):
    """(A 2^ka, B 2^kb) at the ends of the range: convergence, both verdicts on unscaled quantities, and alpha 2^ka, beta 2^kb and
    the vectors of the unscaled pair bit for bit.  Beyond sqrt(max) the square of a shift lambda is not representable: shifts
    carried as lambda itself end a block of more than EDGE rows at the iteration cap."""
    _, _, a, b = gc.range_generate(n, dtype, ka, kb)
    r = run(exe, tmp_path, a, b, dtype)
    assert r["status"] == 0, (r["status"], r["sweeps"])
    assert (r["sweeps"] > 0 and r["window_steps"] > r["sweeps"]) if n > EDGE else r["sweeps"] == 0
    gc.range_check(n, dtype, ka, kb, r["alpha"], r["alpha_im"], r["beta"], r["ur"].astype(dtype), r["ul"].astype(dtype))
    r0 = unscaled_run(exe, tmp_path, n, dtype)
    assert r["sweeps"] == r0["sweeps"] and r["window_steps"] == r0["window_steps"] and r["leaves"] == r0["leaves"]
    assert np.array_equal(np.ldexp(r0["alpha"], ka), r["alpha"]) and np.array_equal(np.ldexp(r0["alpha_im"], ka), r["alpha_im"])
    assert np.array_equal(np.ldexp(r0["beta"], kb), r["beta"])
    assert np.array_equal(r0["ur"], r["ur"]) and np.array_equal(r0["ul"], r["ul"])


def vector_sizes(kind):
    """the size at which the guard fires, or 15 and 35 where no firing is needed"""
    return [n for n in ([gc.GUARD_N] if kind.endswith("graded_triangular_pair") else [15, 35, gc.GUARD_N]) if gc.exists(kind, n)]


VECTOR = [(kind, n, dtype) for dtype in gc.DTYPES for kind in gc.VECTOR_KINDS for n in vector_sizes(kind)]


@pytest.mark.parametrize("kind,n,dtype", VECTOR, ids=[f"{k}-{n}-{np.dtype(d).name}" for k, n, d in VECTOR])
def test_vector_kinds(exe, tmp_path, kind, n, dtype):
    """the kinds built for the back substitution: the overflow rescale, the pivot floor at every divisor, the vectors of
    infinite eigenvalues; triangular pairs take zero sweeps and keep their diagonals (gc.check asserts alpha and beta exactly)"""
    a, b = gc.generate(kind, n, dtype)
    r = run(exe, tmp_path, a, b, dtype, pre_qr=kind.startswith("rotated_"))
    assert r["status"] == 0
    for x in ("alpha", "alpha_im", "beta", "ur", "ul"):
        assert np.isfinite(r[x]).all()
    gc.check(kind, n, dtype, a, b, r["alpha"], r["alpha_im"], r["beta"], r["ur"].astype(dtype), r["ul"].astype(dtype))
    if kind in gc.TRIANGLE_KINDS:
        assert r["sweeps"] == 0 and r["window_steps"] == 0
    if kind == "infinite_in_triangle":
        assert r["infinite"] == len(gc.infinite_rows(n))


def test_iteration_cap_reports_no_convergence(exe, tmp_path):
    a, b = gc.generate("random", 17, np.float64)
    assert run(exe, tmp_path, a, b, np.float64, cap=3)["status"] > 0
    assert run(exe, tmp_path, a, b, np.float64)["status"] == 0


@pytest.mark.parametrize("where", ["bottom", "interior", "top"])
def test_infinite_eigenvalue_deflation(exe, tmp_path, where):
    """an exact zero on the diagonal of the triangular factor: at the bottom (one column rotation), in the interior of an
    unreduced block (the zero is chased down) and at the top"""
    n = 12
    rng = np.random.default_rng(5)
    a, b = np.triu(rng.standard_normal((n, n)), -1), np.triu(rng.standard_normal((n, n)))
    zero = {"bottom": [n - 1], "interior": [5], "top": [0]}[where]
    for i in zero:
        b[i, i] = 0.0
    r = run(exe, tmp_path, a, b, np.float64, pre_qr=False)
    assert r["status"] == 0 and r["infinite"] >= len(zero)
    assert int((r["beta"] == 0).sum()) == len(zero)
    al, VR = gc.unpack(r["alpha"], r["alpha_im"], r["beta"], r["ur"])
    _, VL = gc.unpack(r["alpha"], r["alpha_im"], r["beta"], r["ul"])
    bound = 4 * 4 * n * gc.eps_of(np.float64)  # (no recorded reference for these pairs: four times the floor n eps of the rule)
    assert gc.pair_residuals(a, b, al, r["beta"], VR).max() <= bound
    assert gc.pair_residuals(a, b, al, r["beta"], VL, "left").max() <= bound
