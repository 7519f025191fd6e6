"""The bodies of csrc/chol_update_core.h on the host: tests/host/chol_update_host.cpp instantiates the coefficient step, the row
step, the diagonal-block loop and the tail loop with HostGroup and a small block (NB = 8 columns, RC = 2 columns of W per chunk),
so that a matrix of 30 rows crosses block and chunk borders the way one of a few hundred rows does on the device.  No GPU.

Checked: the residual of both factorizations and of the deletion against 64 n eps max|A| (tests/test_chol_update_ref.py), and
every entry of the factor against tests/chol_update_ref.py.  The element-wise bound is 4 n eps of max|L_ref|: the two compute the
same recurrence with differently rounded steps (the restatement rounds its fused multiply-adds from extended precision, the
compiler may contract d * d + alpha p * p), so each entry carries a few roundings per column in front of it.  Measured here:
at most 0.07 n eps (fp64) and below 0.005 n eps (fp32) over all cases of this file, so 4 n eps is the larger of the two rules."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chol_update_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "chol_update_host.cpp")
INC = os.path.join(ROOT, "faer-rs_amd", "csrc")
SIZES = [1, 7, 8, 9, 17, 30]
RANKS = [1, 2, 3, 5]
NP = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("chol_update_host") / "chol_update_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", str(out)], check=True, capture_output=True, text=True)
    return str(out)


def run(exe, tmp_path, dtype, mode, f, *rest):
    n = f.shape[0]
    r = rest[0].shape[1] if mode != "delete" else len(rest[0])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    parts = [[float(n), float(r)], f.ravel(order="F")] + [np.asarray(x, dtype=np.float64).ravel(order="F") for x in rest]
    np.concatenate(parts).astype(np.float64).tofile(fin)
    subprocess.run([exe, dtype, mode, str(fin), str(fout)], check=True)
    o = np.fromfile(fout)
    return int(o[0]), o[1:].reshape(n, n, order="F").astype(NP[dtype])


def parity(got, want, n, dtype):
    """max |got - want| over the lower triangle in units of n eps max|want|"""
    d = np.abs(np.tril(got).astype(np.float64) - np.tril(want).astype(np.float64)).max()
    return d / (n * np.finfo(NP[dtype]).eps * np.abs(np.tril(want)).max())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("downdate", [False, True])
@pytest.mark.parametrize("ldlt", [False, True])
def test_update_on_the_host(exe, tmp_path, ldlt, downdate, dtype):
    worst_res = worst_par = 0.0
    for n in SIZES:
        for r in RANKS:
            f, w, alpha, target, amax = ref.case_update(n, r, NP[dtype], ldlt, downdate)
            status, got = run(exe, tmp_path, dtype, "ldlt" if ldlt else "llt", f, w, alpha)
            assert status == -1
            assert np.array_equal(np.triu(got, 1), np.triu(f, 1))
            err = np.abs((ref.ldlt_product if ldlt else ref.llt_product)(got) - target).max()
            assert err <= ref.residual_bound(n, amax, NP[dtype]), (n, r, err)
            worst_res = max(worst_res, err / (n * np.finfo(NP[dtype]).eps * amax))
            (ref.ldlt_rank_r_update_clobber if ldlt else ref.llt_rank_r_update_clobber)(f, w, alpha)
            p = parity(got, f, n, dtype)
            worst_par = max(worst_par, p)
            assert p <= 4, (n, r, p)
    print(f"ldlt={ldlt} downdate={downdate} {dtype}: worst residual {worst_res:.2f} n eps max|A|, worst distance to the restatement {worst_par:.2f} n eps")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [3, 9, 17, 30])
def test_deletion_on_the_host(exe, tmp_path, n, dtype):
    """the zero-filled W with the plain update against the reference's staircase (rank_update_indices)"""
    worst = 0.0
    for name, idx in ref.index_sets(n):
        ld, a = ref.case_delete(n, NP[dtype])
        status, got = run(exe, tmp_path, dtype, "delete", ld, sorted(idx))
        keep = np.setdiff1d(np.arange(n), idx)
        m = len(keep)
        assert np.array_equal(np.triu(got, 1), np.triu(ld, 1))
        if m == 0:
            continue
        err = np.abs(ref.ldlt_product(got[:m, :m]) - a[np.ix_(keep, keep)]).max()
        assert err <= ref.residual_bound(n, a, NP[dtype]), (name, err)
        ref.ldlt_delete_rows_and_cols_clobber(ld, idx)
        p = parity(got[:m, :m], ld[:m, :m], n, dtype)
        worst = max(worst, p)
        assert p <= 4, (name, p)
    print(f"n={n} {dtype}: worst distance to the restatement {worst:.2f} n eps")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,j,r,k", [(5, 2, 1, 0), (30, 0, 1, 0), (30, 9, 1, 0), (30, 29, 1, 0), (30, 9, 5, 4), (30, 9, 5, 0)])
def test_failure_index_on_the_host(exe, tmp_path, n, j, r, k, dtype):
    """L = 2 I, column k of W = 3 e_j, alpha = -1: the pivot of column j fails by a wide margin, in whichever chunk k lies"""
    l = np.asfortranarray(2 * np.eye(n, dtype=NP[dtype]))
    w = np.zeros((n, r), dtype=NP[dtype], order="F")
    w[j, k] = 3
    alpha = -np.ones(r, dtype=NP[dtype])
    status, _ = run(exe, tmp_path, dtype, "llt", l, w, alpha)
    with pytest.raises(ref.NonPositivePivot) as e:
        ref.llt_rank_r_update_clobber(l, w, alpha)
    assert status == e.value.index == j


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_later_chunk_fails_at_a_smaller_column(exe, tmp_path, dtype):
    """column 3 of W (second chunk) fails at column 2, column 0 (first chunk) at column 5 of the same block: the reference, which
    runs all of W column by column, reports 2"""
    n = 12
    l = np.asfortranarray(2 * np.eye(n, dtype=NP[dtype]))
    w = np.zeros((n, 4), dtype=NP[dtype], order="F")
    w[5, 0] = 3
    w[2, 3] = 3
    alpha = -np.ones(4, dtype=NP[dtype])
    status, _ = run(exe, tmp_path, dtype, "llt", l, w, alpha)
    with pytest.raises(ref.NonPositivePivot) as e:
        ref.llt_rank_r_update_clobber(l, w, alpha)
    assert status == e.value.index == 2


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_cases_on_the_host(exe, tmp_path, dtype):
    t = NP[dtype]
    l = np.asfortranarray(np.diag(np.array([3, 5, 8], dtype=t)))
    status, got = run(exe, tmp_path, dtype, "llt", l, np.asfortranarray(np.diag(np.array([4, 12, 15], dtype=t))), np.ones(3, dtype=t))
    assert status == -1 and np.array_equal(got, np.diag(np.array([5, 13, 17], dtype=t)))
    ld = np.asfortranarray(np.diag(np.array([1, 0, 1], dtype=t)))
    status, got = run(exe, tmp_path, dtype, "ldlt", ld, np.asfortranarray(np.diag(np.array([1, 0, 1], dtype=t))), np.ones(3, dtype=t))
    assert np.array_equal(got, np.diag(np.array([2, 0, 2], dtype=t)))
    status, got = run(exe, tmp_path, dtype, "ldlt", ld, np.array([[1], [0], [1]], dtype=t), np.ones(1, dtype=t))
    assert np.array_equal(got, np.array([[2, 0, 0], [0, 0, 0], [0.5, 0, 1.5]], dtype=t))
    # a NaN passes the pivot test (<= 0 is false) and reaches L without an error
    l = np.asfortranarray(2 * np.eye(9, dtype=t))
    w = np.ones((9, 1), dtype=t)
    w[4, 0] = np.nan
    status, got = run(exe, tmp_path, dtype, "llt", l, w, np.ones(1, dtype=t))
    assert status == -1 and np.isnan(got[4, 4]) and np.isnan(np.tril(got)[5:, 4]).all()
