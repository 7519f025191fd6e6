"""tests/evd_cases.py alone (no GPU): the two verdicts on hand-made decompositions, the controls that show what each of them
catches and the Frobenius quotient does not, numpy's eig in the dtype of the input under the assignment on every non-defective
input of tests/test_gpu_evd_general.py (so a miss there is the code's, not the radius'), and the sizes of the graded kinds: in
extended precision the unscaled eigenvectors pass the guard's threshold, in graded_quasi at all four places of the guard."""
import numpy as np
import pytest

import evd_cases as ec

WEDGE = {np.dtype(np.float64): 96, np.dtype(np.float32): 128}  # csrc/schur.hip schur_w


def gpu_cases(dtype):
    """(kind, n) of every non-defective case that tests/test_gpu_evd_general.py puts under assign_spectrum"""
    d = np.dtype(dtype)
    W = WEDGE[d]
    out = [(k, n) for k in ec.KINDS for n in (1, 2, 3, W - 1, W, W + 1, 2 * W + 3, {96: 337, 128: 449}[W])]
    out += [(k, ec.GUARD_N[d]) for k in ("graded_triangular", "graded_quasi")]
    out += [("scaled_similarity", n) for n in (W - 1, W + 1, 2 * W + 3)]
    return out


def test_column_residuals_do_not_mix_columns():
    rng = np.random.default_rng(1)
    n = 12
    a = rng.standard_normal((n, n))
    lam, v = np.linalg.eig(a)
    base = ec.column_residuals(a, lam, v)
    assert base.max() < 50 * np.finfo(np.float64).eps
    # a column of norm 1e152 next to one of norm 1e-150 (powers of two: the same mantissas): the same values, and nothing
    # overflows (|v|^2 alone would)
    scale = np.ones(n)
    scale[3], scale[5] = 2.0 ** 505, 2.0 ** -498
    with np.errstate(over="raise", invalid="raise"):
        r = ec.column_residuals(a, lam, v * scale)
    assert np.allclose(r, base, rtol=1e-6, atol=1e-18)
    # one wrong column shows in its own entry alone, whatever the norm of the others
    w = (v * scale).copy()
    w[:, 5] = rng.standard_normal(n) * 2.0 ** -498
    r = ec.column_residuals(a, lam, w)
    assert r[5] > 1e-2 and np.allclose(np.delete(r, 5), np.delete(base, 5), rtol=1e-6, atol=1e-18)
    # left vectors: the rows of inv(V)
    y = np.linalg.inv(v).conj().T
    assert ec.column_residuals(a, lam, y * scale, "left").max() < 1e3 * np.finfo(np.float64).eps
    assert ec.column_residuals(a, lam, y, "right").max() > 1e-3
    # a zero and a non-finite column
    w = v.copy()
    w[:, 0] = 0
    w[2, 1] = np.inf
    r = ec.column_residuals(a, lam, w)
    assert np.isinf(r[0]) and np.isinf(r[1]) and np.allclose(r[2:], base[2:], rtol=1e-6, atol=1e-18)
    # float32 inputs are measured in fp64
    assert ec.column_residuals(a.astype(np.float32), lam, v).max() < 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("use_scipy", [True, False])
def test_assign_spectrum(use_scipy):
    ref = np.array([1.0, 1.0 + 1e-3, 2.0 + 1j, 2.0 - 1j])
    rad = np.array([1e-6, 1e-6, 1e-6, 1e-6])
    perm = ref[[2, 0, 3, 1]]
    assert ec.assign_spectrum(perm, ref, rad, use_scipy)
    assert ec.assign_spectrum(perm + 5e-7, ref, rad, use_scipy) and not ec.assign_spectrum(perm + 2e-6, ref, rad, use_scipy)
    dup = perm.copy()
    dup[0] = dup[2]  # 2 - i twice, 2 + i missing
    assert not ec.assign_spectrum(dup, ref, rad, use_scipy)
    assert not ec.assign_spectrum(perm[:3], ref, rad, use_scipy)
    nan = perm.copy()
    nan[1] = np.nan
    assert not ec.assign_spectrum(nan, ref, rad, use_scipy)
    # the radius belongs to the reference value: two values halfway between the first two need both of their radii
    mid = np.array([1.0005, 1.0005, 2.0 + 1j, 2.0 - 1j])
    assert ec.assign_spectrum(mid, ref, np.array([2e-3, 2e-3, 0, 0]), use_scipy)
    assert not ec.assign_spectrum(mid, ref, np.array([2e-3, 1e-6, 0, 0]), use_scipy)
    # a matching that the first choice of every row does not find: rows 0 and 1 both reach value 0, only row 0 reaches value 1
    assert ec.assign_spectrum(np.array([0.0, 1.0]), np.array([0.5, 0.0]), np.array([0.6, 0.1]), use_scipy)
    assert not ec.assign_spectrum(np.array([0.0, 1.0]), np.array([0.5, 0.0]), np.array([0.4, 0.1]), use_scipy)
    assert ec.assign_spectrum(np.zeros(0), np.zeros(0), np.zeros(0), use_scipy)


def test_augmenting_paths_against_random_graphs():
    """sizes of maximum matchings: chains that need every path flipped, and random graphs against a brute-force count"""
    import itertools

    n = 9
    chain = np.eye(n, dtype=bool) | np.eye(n, k=-1, dtype=bool)  # row i reaches i - 1 and i; tried in that order
    assert ec._augmenting_paths(chain) == n
    chain[0, 0] = False
    assert ec._augmenting_paths(chain) == n - 1
    rng = np.random.default_rng(3)
    for _ in range(40):
        adj = rng.random((6, 6)) < 0.3
        best = max(sum(adj[i, p[i]] for i in range(6)) for p in itertools.permutations(range(6)))
        assert ec._augmenting_paths(adj) == best


@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_numpy_in_the_same_dtype_passes_the_assignment(dtype):
    """on every input the GPU file holds to it; prints numpy's own residuals, which are the source of the bounds"""
    e = ec.eps_of(dtype)
    for kind, n in gpu_cases(dtype):
        a, known, defective = ec.generate(kind, n, dtype)
        assert not defective
        key = (kind, n, np.dtype(dtype).name)
        w, rf, rc = ec.numpy_same_dtype(a, key)
        ref, radius = ec.reference_spectrum(a, key)
        print(f"{kind} n={n} {np.dtype(dtype).name}: numpy Frobenius {rf / e:.2f} eps, worst column {rc / e:.2f} eps, "
              f"smallest radius {radius.min() / max(np.linalg.norm(a.astype(np.float64)), 1e-300) / e:.3g} eps |A|_F")
        assert (radius > 0).all() or n == 1
        assert ec.assign_spectrum(w, ref, radius), (kind, n)
        if known is not None:
            assert ec.assign_spectrum(known, ref, radius), (kind, n, "the known spectrum")


def test_generators():
    for dtype in ec.DTYPES:
        for kind in ec.NEW_KINDS:
            for n in (5, 30):
                a, known, defective = ec.generate(kind, n, dtype)
                assert a.shape == (n, n) and a.dtype == dtype and np.isfinite(a).all()
                assert defective == (kind in ec.DEFECTIVE or kind.startswith("rotated_"))
                assert (known is None) == kind.startswith("rotated_")
                if kind in ec.TRIANGULAR_KINDS:
                    sub = np.diag(a, -1)
                    assert (np.tril(a, -2) == 0).all() and not ((sub[:-1] != 0) & (sub[1:] != 0)).any()
                    for i in np.nonzero(sub)[0]:  # standard form
                        assert a[i, i] == a[i + 1, i + 1] and a[i, i + 1] * a[i + 1, i] < 0
                    ref = np.linalg.eigvals(a.astype(np.float64))
                    if not defective:
                        assert ec.assign_spectrum(known, ref, 1e-6)
        # graded_quasi: every other pair of rows is a block, the rows between are 1 x 1
        sub = np.diag(ec.graded_quasi(12, dtype)[0], -1) != 0
        assert sub.tolist() == [True, False, False, False] * 2 + [True, False, False]
        # repeated_blocks: one eigenvalue pair, repeated
        assert set(np.round(ec.repeated_blocks(8, dtype)[1], 12)) == {1 + 1j, 1 - 1j}
        # scaled_similarity: the similarity is exact, the spectrum is that of the normal kind's matrix, and it is far from normal
        a, known, _ = ec.scaled_similarity(30, dtype)
        b, _ = ec.make("normal", 30, dtype)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        assert (b64[0, :] != 0).all()
        d = a64[0, :] / b64[0, :]
        assert np.array_equal(np.ldexp(1.0, np.round(np.log2(np.abs(d))).astype(int)), np.abs(d))  # powers of two
        assert np.linalg.norm(a64 @ a64.T - a64.T @ a64) > 1e3 * np.linalg.norm(b64 @ b64.T - b64.T @ b64) + 1.0
        assert ec.assign_spectrum(np.linalg.eigvals(a64), known, 1e-6)


@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_guard_fires_at_the_guard_size(dtype):
    n = ec.GUARD_N[np.dtype(dtype)]
    assert n <= min(WEDGE.values())  # one leaf
    big = ec.guard_threshold(dtype)
    assert big == pytest.approx({np.float64: 6.7e153, np.float32: 9.2e18}[dtype], rel=1e-2)
    top, sites, out = ec.guard_sites(ec.graded_triangular(n, dtype)[0], dtype)
    print(f"graded_triangular n={n} {np.dtype(dtype).name}: largest unscaled component {top:.3e}, threshold {big:.3e}")
    assert top > big and sites == {("real", 1)}
    top, sites, out = ec.guard_sites(ec.graded_quasi(n, dtype)[0], dtype)
    print(f"graded_quasi n={n} {np.dtype(dtype).name}: largest unscaled component {top:.3e}, guard fires at {sorted(sites)}")
    assert top > big and sites == {("real", 1), ("real", 2), ("pair", 1), ("pair", 2)}
    # and not where nothing grows
    top, sites, out = ec.guard_sites(np.diag(np.arange(1.0, 41.0)) + 0.1 * np.triu(np.ones((40, 40)), 1), dtype)
    assert top < big and not sites


def code_like_columns(v, decades):
    """columns of norm 1 scaled as the back substitution leaves them: norms from 1 up to 10^decades"""
    n = v.shape[1]
    return v * 10.0 ** (decades * np.arange(n) / (n - 1))


def test_control_a_wrong_small_column():
    """one column of ordinary norm replaced by noise, among columns of up to 1e18 times its norm: the Frobenius quotient stays
    under the bound, the per-column verdict does not"""
    dtype = np.float32
    n = ec.GUARD_N[np.dtype(dtype)]
    a, _, _ = ec.graded_triangular(n, dtype)
    bf, bc = ec.bounds(a, ("control a", n))
    lam, v = np.linalg.eig(a.astype(np.float64))
    v = code_like_columns(v, 18)
    assert ec.frobenius_quotient(a, lam, v) <= bf and ec.column_residuals(a, lam, v).max() <= bc
    v[:, 0] = np.random.default_rng(5).standard_normal(n) / np.sqrt(n)
    assert ec.frobenius_quotient(a, lam, v) <= bf
    r = ec.column_residuals(a, lam, v)
    assert r[0] > bc and r[1:].max() <= bc


def test_control_b_an_eigenpair_twice():
    """pair j replaced by a copy of pair i: every column residual passes, the assignment does not"""
    dtype = np.float64
    n = 40
    a, _ = ec.make("normal01", n, dtype)
    bf, bc = ec.bounds(a, ("control b", n))
    ref, radius = ec.reference_spectrum(a, ("control b", n))
    lam, v = np.linalg.eig(a)
    assert ec.column_residuals(a, lam, v).max() <= bc and ec.assign_spectrum(lam, ref, radius)
    i, j = 0, n - 1
    assert abs(lam[i] - lam[j]) > 1e-3
    lam[j], v[:, j] = lam[i], v[:, i]
    assert ec.frobenius_quotient(a, lam, v) <= bf and ec.column_residuals(a, lam, v).max() <= bc
    assert not ec.assign_spectrum(lam, ref, radius)
    assert not ec.assign_spectrum(lam, ref, radius, use_scipy=False)
