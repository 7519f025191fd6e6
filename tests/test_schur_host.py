"""The bodies of csrc/schur_core.h on the host: tests/host/schur_host.cpp instantiates them with HostGroup (one thread, no
barrier) and runs the whole sweep loop -- prepare, shifts, window steps, leaves, finish, eigenvectors -- with a small window
edge, so that matrices of a few dozen rows take every path.  No GPU.

Checked against numpy in fp64: the decomposition H = Z T Z^T, the form of T, the eigenvalues and the eigenvector residual.
Bound: 4 max(numpy's own residual, n eps), as in test_gpu_evd_general.py.

The non-normal kinds of tests/evd_cases.py run here first, under the per-column verdict and the assignment of the spectrum: the
overflow guard and the divisor floor of eigvec_block are reached by them alone, and a defect there shows without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import evd_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "schur_host.cpp")
INC = os.path.join(ROOT, "faer-rs_amd", "csrc")
W = 24


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("schur_host") / "schur_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", str(out)], check=True, capture_output=True, text=True)
    return str(out)


def hessenberg(kind, n, rng):
    if kind == "normal":
        return np.triu(rng.standard_normal((n, n)), -1)
    if kind == "split":  # exact zeros on the subdiagonal, an active block that does not start at 0
        h = np.triu(rng.standard_normal((n, n)), -1)
        h[n // 3, n // 3 - 1] = 0
        h[n // 3 + 2, n // 3 + 1] = 0
        return h
    if kind == "cyclic":  # converges only through the exceptional shifts
        return np.roll(np.eye(n), 1, axis=0)
    raise ValueError(kind)


def run(exe, tmp_path, h, dtype, w=W):
    n = h.shape[0]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([[float(n)], h.ravel(order="F")]).astype(np.float64).tofile(fin)
    subprocess.run([exe, dtype, str(w), str(fin), str(fout)], check=True)
    o = np.fromfile(fout)
    status, counts, o = int(o[0]), o[1:4].astype(int), o[4:]
    wr, wi = o[:n], o[n:2 * n]
    t, z, x = (o[2 * n + k * n * n:2 * n + (k + 1) * n * n].reshape(n, n, order="F") for k in range(3))
    return status, counts, wr, wi, t, z, x


def complex_vectors(wi, v):
    n = len(wi)
    c = np.zeros((n, n), dtype=complex)
    k = 0
    while k < n:
        if wi[k] == 0:
            c[:, k] = v[:, k]
            k += 1
        else:
            c[:, k] = v[:, k] + 1j * v[:, k + 1]
            c[:, k + 1] = v[:, k] - 1j * v[:, k + 1]
            k += 2
    return c


def residual(a, lam, v):
    return np.linalg.norm(a @ v - v * lam) / (np.linalg.norm(a) * np.linalg.norm(v))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind,n", [("normal", 3), ("normal", W), ("normal", W + 1), ("normal", 2 * W + 3), ("normal", 85),
                                    ("split", 2 * W + 3), ("cyclic", W + 1), ("cyclic", 2 * W + 3)])
def test_sweep_loop_on_the_host(exe, tmp_path, kind, n, dtype):
    rng = np.random.default_rng(1000 + n)
    np_t = np.float64 if dtype == "f64" else np.float32
    eps = np.finfo(np_t).eps
    h = hessenberg(kind, n, rng).astype(np_t).astype(np.float64)
    status, counts, wr, wi, t, z, x = run(exe, tmp_path, h, dtype)
    assert status == 0
    if n > W and kind != "split":
        assert counts[0] > 0 and counts[1] > 0, counts  # sweeps and window steps were taken
    lam_np, v_np = np.linalg.eig(h.astype(np_t))
    bound = 4 * max(residual(h, lam_np.astype(complex), v_np.astype(complex)), n * eps)
    print(f"{kind} n={n} {dtype}: sweeps/steps/leaves {counts}, bound {bound:.3e}")

    # T: quasi upper triangular, 2 x 2 blocks standardised, (wr, wi) read off its diagonal blocks
    assert np.all(np.tril(t, -2) == 0)
    sub = np.diag(t, -1)
    assert not np.any((sub[:-1] != 0) & (sub[1:] != 0))
    for k in np.nonzero(sub)[0]:
        assert t[k, k] == t[k + 1, k + 1] and t[k, k + 1] * t[k + 1, k] < 0
        assert wi[k] > 0 and wi[k + 1] == -wi[k] and wr[k] == wr[k + 1] == t[k, k]
    real = np.ones(n, dtype=bool)
    real[np.nonzero(sub)[0]] = False
    real[np.nonzero(sub)[0] + 1] = False
    assert np.all(wi[real] == 0) and np.all(wr[real] == np.diag(t)[real])

    # H = Z T Z^T with Z orthogonal
    err_orth = np.linalg.norm(z.T @ z - np.eye(n)) / np.sqrt(n)
    err_dec = np.linalg.norm(z @ t @ z.T - h) / np.linalg.norm(h)
    print(f"  orthogonality {err_orth:.3e}, decomposition {err_dec:.3e}")
    assert err_orth <= bound and err_dec <= bound

    # eigenvectors of H: Z X, packed as the public interface packs them
    lam = wr + 1j * wi
    v = complex_vectors(wi, z @ x)
    assert np.all(np.linalg.norm(v, axis=0) > 0)
    res = residual(h, lam, v)
    print(f"  eigenvector residual {res:.3e}")
    assert res <= bound


def test_iteration_cap_is_reported(exe, tmp_path):
    """A NaN never deflates: the loop ends at its cap with status 1 instead of running on."""
    h = np.triu(np.ones((W + 5, W + 5)), -1)
    h[3, 3] = np.nan
    status = run(exe, tmp_path, h, "f64")[0]
    assert status == 1


def hessenberg_form(a):
    """Q^T a Q upper Hessenberg, by Householder reflectors in fp64"""
    h = np.array(a, dtype=np.float64)
    n = h.shape[0]
    for k in range(n - 2):
        x = h[k + 1:, k].copy()
        if not x[1:].any():
            continue
        x[0] += np.copysign(np.linalg.norm(x), x[0])
        x /= np.linalg.norm(x)
        h[k + 1:, :] -= 2 * np.outer(x, x @ h[k + 1:, :])
        h[:, k + 1:] -= 2 * np.outer(h[:, k + 1:] @ x, x)
        h[k + 2:, k] = 0
    return h


NON_NORMAL = [(k, n) for k in ec.NEW_KINDS for n in (W, 2 * W + 3)] + [(k, "guard") for k in ("graded_triangular", "graded_quasi")]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind,n", NON_NORMAL)
def test_non_normal_kinds_on_the_host(exe, tmp_path, kind, n, dtype):
    np_t = np.float64 if dtype == "f64" else np.float32
    eps = ec.eps_of(np_t)
    n = ec.GUARD_N[np.dtype(np_t)] if n == "guard" else n
    a, known, defective = ec.generate(kind, n, np_t)
    unrotated = kind in ec.TRIANGULAR_KINDS
    h = a if unrotated else hessenberg_form(a).astype(np_t)  # (the triangular kinds are Hessenberg matrices already)
    assert np.array_equal(np.tril(h, -2), np.zeros_like(h))
    status, counts, wr, wi, t, z, x = run(exe, tmp_path, h.astype(np.float64), dtype)
    assert status == 0
    assert np.isfinite(x).all() and np.isfinite(z).all()
    lam = wr + 1j * wi
    v = complex_vectors(wi, z @ x)
    assert (np.abs(v).max(axis=0) > 0).all()
    key = ("host", kind, n, dtype)
    _, bc = ec.bounds(h, key)
    np_col = ec.numpy_same_dtype(h, key)[2]
    r = ec.column_residuals(h, lam, v)
    norms = np.linalg.norm(v / np.abs(v).max(), axis=0) * np.abs(v).max()
    print(f"{kind} n={n} {dtype}: sweeps/steps/leaves {counts}, numpy's worst column {np_col / eps:.2f} eps, worst column {r.max() / eps:.2f} eps, "
          f"bound {bc / eps:.0f} eps, column norms {norms.min():.3g} .. {norms.max():.3g}")
    assert r.max() <= bc, (r.argmax(), r.max() / eps, bc / eps)
    if not defective:
        ref, radius = ec.reference_spectrum(h, key)
        assert ec.assign_spectrum(lam, ref, radius)
    if unrotated:
        # nothing to do for the sweeps: T is the input, the real eigenvalues are its diagonal entries exactly and an imaginary part
        # is a product of two square roots (three roundings)
        assert np.array_equal(t, h.astype(np.float64))
        assert np.array_equal(wr, np.diag(h).astype(np.float64))
        assert ec.assign_spectrum(lam, known, 4 * eps * np.abs(known).max())
    if kind in ("graded_triangular", "graded_quasi"):
        # the guard fired: in extended precision the unscaled vectors pass its threshold, here no component does, and the
        # largest one is what the same substitution with the same rescalings leaves
        big = ec.guard_threshold(np_t)
        top, sites, out = ec.guard_sites(h, np_t)
        print(f"  largest unscaled component {float(top):.3e}, guard at {sorted(sites)}, largest component {np.abs(x).max():.3e}, "
              f"in extended precision {float(out):.3e}, threshold {big:.3e}")
        assert top > big or (dtype == "f64" and n == W)  # (24 rows do not reach the fp64 threshold)
        assert np.abs(x).max() <= big
        assert np.abs(x).max() == pytest.approx(float(out), rel=1e-3)
        if n == ec.GUARD_N[np.dtype(np_t)]:
            assert len(sites) == (4 if kind == "graded_quasi" else 1)
