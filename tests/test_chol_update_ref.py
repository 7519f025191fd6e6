"""tests/chol_update_ref.py against fresh factorizations: the numpy restatement of the reference's Cholesky update routines is what
the host build and the GPU kernels are compared with element by element, so it is checked first, on its own.  No GPU.

Bound: the new factor reproduces the modified matrix to 64 n eps max|A| (the restatement itself stays below 3 n eps on these
families; the figures are printed)."""
import numpy as np
import pytest

import chol_update_ref as ref

SIZES = [1, 2, 3, 7, 8, 9, 17, 30, 65]
RANKS = [1, 2, 3, 5, 9]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("downdate", [False, True])
@pytest.mark.parametrize("ldlt", [False, True])
def test_update_reproduces_the_modified_matrix(ldlt, downdate, dtype):
    worst = 0.0
    for n in SIZES:
        for r in RANKS:
            f, w, alpha, target, amax = ref.case_update(n, r, dtype, ldlt, downdate)
            upper = np.triu(f, 1).copy()
            if ldlt:
                ref.ldlt_rank_r_update_clobber(f, w, alpha)
            else:
                ref.llt_rank_r_update_clobber(f, w, alpha)
            assert np.array_equal(np.triu(f, 1), upper)
            got = (ref.ldlt_product if ldlt else ref.llt_product)(f)
            err = np.abs(got - target).max()
            worst = max(worst, err / (n * np.finfo(dtype).eps * amax))
            assert err <= ref.residual_bound(n, amax, dtype), (n, r, err)
    print(f"ldlt={ldlt} downdate={downdate} {np.dtype(dtype).name}: worst residual {worst:.2f} n eps max|A|")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [3, 9, 17, 65, 129])
def test_deletion_reproduces_the_submatrix(n, dtype):
    worst = 0.0
    for name, idx in ref.index_sets(n):
        ld, a = ref.case_delete(n, dtype)
        out = ref.ldlt_delete_rows_and_cols_clobber(ld, idx)
        assert out == sorted(idx)
        keep = np.setdiff1d(np.arange(n), idx)
        m = len(keep)
        got = ref.ldlt_product(ld[:m, :m])
        want = a[np.ix_(keep, keep)]
        err = np.abs(got - want).max() if m else 0.0
        worst = max(worst, err / (n * np.finfo(dtype).eps * np.abs(a).max()))
        assert err <= ref.residual_bound(n, a, dtype), (name, err)
    print(f"n={n} {np.dtype(dtype).name}: worst residual {worst:.2f} n eps max|A|")


def test_rank_update_indices_counts_the_columns_in_front():
    """column c of the trailing block (new numbering, from `first`) sees the removed columns whose old index lies in front of it"""
    for n, idx in [(10, [0]), (10, [2, 3, 7]), (12, [0, 1, 6, 11]), (9, [8])]:
        first, r = idx[0], len(idx)
        nxt = ref.rank_update_indices(first, idx)
        keep = [i for i in range(n) if i not in idx]
        for c in range(first, n - r):
            assert nxt() == sum(1 for j in idx if j < keep[c]), (n, idx, c)


def test_failure_index():
    for dtype in (np.float64, np.float32):
        l = np.asfortranarray(2 * np.eye(5, dtype=dtype))
        w = np.zeros((5, 1), dtype=dtype)
        w[2, 0] = 3
        with pytest.raises(ref.NonPositivePivot) as e:
            ref.llt_rank_r_update_clobber(l, w, np.array([-1], dtype=dtype))
        assert e.value.index == 2


def test_exact_cases():
    for dtype in (np.float64, np.float32):
        l = np.asfortranarray(np.diag(np.array([3, 5, 8], dtype=dtype)))
        w = np.asfortranarray(np.diag(np.array([4, 12, 15], dtype=dtype)))
        ref.llt_rank_r_update_clobber(l, w, np.ones(3, dtype=dtype))
        assert np.array_equal(l, np.diag(np.array([5, 13, 17], dtype=dtype)))
        l = np.asfortranarray(np.diag(np.array([3, 7], dtype=dtype)))
        w = np.array([[4, 12], [0, 0]], dtype=dtype, order="F")
        ref.llt_rank_r_update_clobber(l, w, np.ones(2, dtype=dtype))
        assert np.array_equal(l, np.diag(np.array([13, 7], dtype=dtype)))
        # d == 0 && nd == 0 (ldlt/update.rs:281): one nonzero per column of W again, so that the result stays diagonal
        ld = np.asfortranarray(np.diag(np.array([1, 0, 1], dtype=dtype)))
        w = np.asfortranarray(np.diag(np.array([1, 0, 1], dtype=dtype)))
        ref.ldlt_rank_r_update_clobber(ld, w, np.ones(3, dtype=dtype))
        assert np.array_equal(ld, np.diag(np.array([2, 0, 2], dtype=dtype)))
        # the same branch with the single column (1, 0, 1): [[2, 0, 1], [0, 0, 0], [1, 0, 2]] = L diag(2, 0, 1.5) L^T, l_20 = 0.5
        ld = np.asfortranarray(np.diag(np.array([1, 0, 1], dtype=dtype)))
        ref.ldlt_rank_r_update_clobber(ld, np.array([[1], [0], [1]], dtype=dtype, order="F"), np.ones(1, dtype=dtype))
        assert np.array_equal(ld, np.array([[2, 0, 0], [0, 0, 0], [0.5, 0, 1.5]], dtype=dtype))
