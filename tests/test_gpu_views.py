"""Every factorization, solve and reconstruction on padded and offset DEVICE views (tests/gpu_util.py: place / place_host /
guard_intact; the layouts are listed there and pinned by tests/test_view_helpers.py).

A device view's ptr / row_stride / col_stride go straight to the kernels (csrc/api.hip stages host operands only), and
faer hands over exactly such views: faer::Mat pads its column stride to 64 bytes, every blocked algorithm works on
submatrices of a bigger parent.  Each test places every matrix operand of the C-ABI call inside a parent filled with a
NaN of a recognisable payload and asserts
  a. the permutations, counts, ranks and failure indices of the oracle run on place_host of the SAME layout (the pivot searches
     of the full-pivot LU and the column-pivot QR depend on the view's major direction, in the reference and here);
  b. the factors within the bound of the dense test of that entry point -- every bound below names the test it repeats;
  c. guard_intact for every parent (bitwise), and a second sentinel (-7.5) in the triangle an entry point must not touch;
  d. no NaN inside any view afterwards where the oracle's result has none.
An over-read that matters shows up as a NaN or a wrong pivot, an over-write bitwise; nothing here tries to fault."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import EPS, GUARD_BITS, bits, guard_intact, init_gpu, place, place_host, rnd, same_bits, spd, to_host, view_box
from test_bidiag_oracle import bidiag_of
from test_gpu_self_adjoint_evd import check as evd_check
from test_hessenberg_oracle import hess_of
from test_tridiag_oracle import tridiag_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
MAIN = ["mat", "sub", "rowpad"]  # every shape
EXTRA = ["odd", "step2"]  # the two smallest shapes of an entry point and one that reaches its blocked driver


def cases(shapes, extra):
    """(shape..., layout) parameters: MAIN for every shape, EXTRA for the shapes whose index is in `extra`"""
    out = []
    for i, s in enumerate(shapes):
        s = s if isinstance(s, tuple) else (s,)
        for lay in MAIN + (EXTRA if i in extra else []):
            out.append(pytest.param(*s, lay, id="-".join(str(x) for x in s) + "-" + lay))
    return out


class Held:
    """a numpy matrix placed on the device inside a guarded parent, with the snapshot guard_intact compares against"""

    def __init__(self, a, layout, fill=None):
        a = np.asarray(a)
        self.parent, self.view = place(a, layout, fill)
        self.before = self.parent.clone()
        self.box = view_box(a.shape, layout, a.dtype)

    def host(self):
        return to_host(self.view)

    def intact(self, what=""):
        guard_intact(self.parent, self.before, self.box, what)

    def untouched(self, what=""):
        """a read-only operand: not one bit of the parent, view included, has changed"""
        assert same_bits(self.parent, self.before), f"{what}: a read-only operand was written"


def no_new_nan(got, ref=None, what=""):
    bad = np.isnan(got) if ref is None else np.isnan(got) & ~np.isnan(ref)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist())


def block_upper(bs, size):
    """the upper triangles of the bs-wide diagonal blocks of a Householder coefficient matrix (the part the reference defines)"""
    up = np.zeros((bs, size), bool)
    for j0 in range(0, size, bs):
        w = min(bs, size - j0)
        up[:w, j0:j0 + w] = np.triu(np.ones((w, w), bool))
    return up


# ------------------------------------------------------------------------------------------ partial-pivot LU (getrf.hip)
# (40, 17), (300, 8): single-workgroup leaf; (600, 5): cooperative leaf; (257, 257); (1000, 1000): recursion with 128-column
# nodes; (2000, 64): flat panel; (8, 300): wide
LU_SHAPES = [(40, 17), (300, 8), (600, 5), (257, 257), (1000, 1000), (2000, 64), (8, 300)]


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,layout", cases(LU_SHAPES, {0, 1, 4, 5}))
def test_plu_on_views(oracle, m, n, layout, dtype, general):
    F = init_gpu()
    rng = np.random.default_rng(m * 7 + n)
    a = rnd(rng, m, n, dtype)
    _, ref = place_host(a, layout)
    rperm, rinv, rnt = oracle.lu_in_place(ref)
    A = Held(a, layout)
    F.lib().faer_hip_debug_lu_force_general(general)
    try:
        perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(A.view)
        lu = A.host()
    finally:
        F.lib().faer_hip_debug_lu_force_general(0)
    A.intact("lu")
    no_new_nan(lu, ref, "lu")
    perm, perm_inv = perm.astype(np.int64), perm_inv.astype(np.int64)
    assert np.array_equal(perm, rperm) and np.array_equal(perm_inv, rinv) and nt == rnt
    size = min(m, n)
    e = EPS[np.dtype(dtype)]
    # test_plu_vs_oracle: P A == L U, |L| <= 1, factor-level agreement at the forward error of the factorization
    L = (np.tril(lu[:, :size], -1) + np.eye(m, size)).astype(np.float64)
    U = np.triu(lu[:size, :]).astype(np.float64)
    assert np.abs(L @ U - a[perm]).max() <= 16 * max(m, n) * e * np.abs(a).max()
    assert np.abs(np.tril(lu, -1)).max(initial=0) <= 1.0 + 4 * e
    kappa = np.linalg.cond(a[perm][:size, :size].astype(np.float64))
    # test_plu_vs_oracle / test_plu_non_cooperative_leaves_vs_oracle
    assert np.abs(lu - ref).max() <= 4 * max(m, n) * e * kappa * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["mat", "rowpad"])
def test_plu_lookahead_driver_on_views(oracle, layout, dtype):
    """n = 3072 under faer_hip_debug_lu_plan(512, 1536, 2048): the look-ahead driver with all three phases, as
    test_plu_lookahead_phases_and_transitions_at_small_n runs it -- flat panels for `mat`, the recursion and staged panels for
    `rowpad` (row stride != 1)"""
    import torch

    F = init_gpu()
    n = 3072
    rng = np.random.default_rng(n + 11)
    a = rnd(rng, n, n, dtype)
    A = Held(a, layout)
    F.lib().faer_hip_debug_lu_plan(C.c_size_t(512), C.c_size_t(1536), C.c_size_t(2048))
    try:
        perm, perm_inv, _ = F.partial_piv_lu_factor_in_place(A.view)
        F.synchronize()
    finally:
        F.lib().faer_hip_debug_lu_plan(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))
    A.intact("lu look-ahead")
    lu = A.view
    assert not torch.isnan(lu).any().item()
    perm = perm.astype(np.int64)
    assert sorted(perm.tolist()) == list(range(n)) and np.array_equal(perm_inv.astype(np.int64)[perm], np.arange(n))
    k = 256
    _, ref = place_host(a[:, :k], layout)
    rperm, _, _ = oracle.lu_in_place(ref)
    assert np.array_equal(perm[:k], rperm[:k])
    ad = torch.from_numpy(a).cuda()
    p = torch.as_tensor(perm, device="cuda")
    Lm = (torch.tril(lu, -1) + torch.eye(n, dtype=lu.dtype, device="cuda")).double()
    U = torch.triu(lu).double()
    err = (Lm @ U - ad.double()[p]).abs().max().item()
    scale = (Lm.abs() @ U.abs()).max().item()
    if dtype == np.float64:  # test_plu_lookahead_phases_and_transitions_at_small_n
        assert err <= 16 * n * 2.3e-16 * scale
    else:  # test_lookahead_paths_fp32
        assert err <= 8 * n * 1.2e-7 * scale


# ------------------------------------------------------------------------------------------ Cholesky, LDLT (potrf.hip)
def quasi_definite(rng, n, dtype=np.float64):
    """the matrices of test_ldlt_vs_oracle: [[H, B^T], [B, -G]] with H, G positive definite"""
    n1 = n // 2
    h = rng.standard_normal((n, n))
    H = h[:n1, :n1] @ h[:n1, :n1].T + n * np.eye(n1)
    G = h[n1:, n1:] @ h[n1:, n1:].T + n * np.eye(n - n1)
    B = h[n1:, :n1]
    return np.asarray(np.block([[H, B.T], [B, -G]]), dtype=dtype, order="F"), n1


def _llt_checks(a, got, ref, n, dtype):
    e = EPS[np.dtype(dtype)]
    iu = np.triu_indices(n, 1)
    assert (got[iu] == -7.5).all(), "the strict upper triangle was written"
    no_new_nan(got, ref, "llt")
    # test_llt_vs_oracle (max|ref| there includes the untouched upper triangle of A; the lower triangle alone is no larger)
    L = np.tril(got).astype(np.float64)
    assert np.abs(np.tril(L @ L.T - a)).max() <= 8 * n * e * np.abs(a).max()
    assert np.abs(np.tril(got) - np.tril(ref)).max() <= 64 * n * e * np.abs(np.tril(ref)).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,layout", cases([31, 128, 129, 300, 1024], {0, 1, 4}))
def test_llt_on_views(oracle, n, layout, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n)
    a = spd(rng, n, dtype)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5
    _, ref = place_host(marked, layout)
    assert oracle.llt_in_place(ref) == ("ok", 0)
    A = Held(marked, layout)
    assert F.llt_factor_in_place(A.view) == 0
    got = A.host()
    A.intact("llt")
    _llt_checks(a, got, ref, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", MAIN)
def test_llt_lookahead_driver_on_views(oracle, layout, dtype, monkeypatch):
    """n = 2304 with FAER_HIP_LLT_LA_MIN=2048 and FAER_HIP_LLT_TAIL=0: the two-stream look-ahead driver, whose merged trailing
    update asks the GEMM for a tile skip (test_llt_lookahead_path, test_llt_lookahead_on_a_view_with_reversed_rows_and_columns)"""
    F = init_gpu()
    monkeypatch.setenv("FAER_HIP_LLT_LA_MIN", "2048")
    monkeypatch.setenv("FAER_HIP_LLT_TAIL", "0")
    n = 2304
    rng = np.random.default_rng(77)
    a = spd(rng, n, dtype)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5
    _, ref = place_host(marked, layout)
    assert oracle.llt_in_place(ref) == ("ok", 0)
    A = Held(marked, layout)
    assert F.llt_factor_in_place(A.view) == 0
    got = A.host()
    A.intact("llt look-ahead")
    _llt_checks(a, got, ref, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", MAIN + EXTRA)
def test_llt_non_positive_pivot_on_views(oracle, layout, dtype):
    """test_llt_non_positive_pivot on a view: the index of the first non-positive pivot"""
    F = init_gpu()
    n, bad = 300, 211
    a = spd(np.random.default_rng(7), n, dtype)
    a[bad, bad] = -1.0
    a[np.triu_indices(n, 1)] = -7.5
    _, ref = place_host(a, layout)
    assert oracle.llt_in_place(ref) == ("non_positive_pivot", bad)
    A = Held(a, layout)
    with pytest.raises(F.LltError) as ei:
        F.llt_factor_in_place(A.view)
    assert ei.value.index == bad
    A.intact("llt failure")
    assert (A.host()[np.triu_indices(n, 1)] == -7.5).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,layout", cases([31, 128, 129, 300, 1024], {0, 1, 4}))
def test_ldlt_on_views(oracle, n, layout, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n)
    a, n1 = quasi_definite(rng, n, dtype)
    iu = np.triu_indices(n, 1)
    marked = a.copy()
    marked[iu] = -7.5
    _, ref = place_host(marked, layout)
    assert oracle.ldlt_in_place(ref) == ("ok", 0)
    A = Held(marked, layout)
    assert F.ldlt_factor_in_place(A.view) == 0
    got = A.host()
    A.intact("ldlt")
    assert (got[iu] == -7.5).all()
    no_new_nan(got, ref, "ldlt")
    # test_ldlt_vs_oracle
    tol = 64 * n * EPS[np.dtype(dtype)]
    assert np.abs(np.tril(got) - np.tril(ref)).max() <= tol * max(1.0, np.abs(np.tril(ref)).max())
    D = np.diag(got).astype(np.float64)
    assert (D[:n1] > 0).all() and (D[n1:] < 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", MAIN + EXTRA)
def test_ldlt_zero_pivot_on_views(oracle, layout, dtype):
    """A = L D L^T from small integers with d_bad = 0: every intermediate of the elimination is an exact integer in both
    precisions and in any order, so pivot `bad` is exactly zero (the condition of LdltError::ZeroPivot)"""
    F = init_gpu()
    n, bad = 150, 131
    rng = np.random.default_rng(5)
    L = np.tril(rng.integers(-1, 2, (n, n)), -1) * (rng.random((n, n)) < 0.1) + np.eye(n)
    d = rng.choice([1.0, 2.0, -1.0, -2.0], n)
    d[bad] = 0.0
    a = np.asarray((L * d) @ L.T, dtype=dtype)
    assert np.abs(a).max() < 2 ** 20 and np.array_equal(a, np.round(a))
    a[np.triu_indices(n, 1)] = -7.5
    _, ref = place_host(a, layout)
    assert oracle.ldlt_in_place(ref) == ("zero_pivot", bad)
    A = Held(a, layout)
    with pytest.raises(F.LdltError) as ei:
        F.ldlt_factor_in_place(A.view)
    assert ei.value.index == bad
    A.intact("ldlt failure")
    assert (A.host()[np.triu_indices(n, 1)] == -7.5).all()


@pytest.mark.parametrize("layout", MAIN)
def test_ldlt_signs_and_regularization_on_views(oracle, layout):
    """test_ldlt_zero_pivot_regularization_and_solve: a singular leading minor, regularized with the expected signs"""
    F = init_gpu()
    rng = np.random.default_rng(3)
    n, bad = 300, 211
    a, _ = quasi_definite(rng, n)
    s = a.copy()
    s[bad, :] = s[5, :]
    s[:, bad] = s[:, 5]
    s[bad, bad] = s[5, 5]
    s[np.triu_indices(n, 1)] = -7.5
    signs = np.where(np.arange(n) < n // 2, 1, -1).astype(np.int8)
    _, ref = place_host(s, layout)
    r = oracle.ldlt_in_place(ref, 1e-2, 1e-9, signs=signs)
    assert r[0] == "ok"
    A = Held(s, layout)
    assert F.ldlt_factor_in_place(A.view, (1e-2, 1e-9), signs=signs) == r[1]
    got = A.host()
    A.intact("ldlt regularized")
    assert (got[np.triu_indices(n, 1)] == -7.5).all()
    no_new_nan(got, ref, "ldlt regularized")
    # test_ldlt_zero_pivot_regularization_and_solve
    assert np.abs(np.tril(got) - np.tril(ref)).max() <= 1e-6 * max(1.0, np.abs(np.tril(ref)).max())


# ------------------------------------------------------------------------------------------ full-pivot LU (fplu.hip)
@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,layout", cases([(40, 30), (30, 40), (300, 300), (1030, 700)], {0, 1, 2}))
def test_full_piv_lu_on_views(oracle, m, n, layout, dtype, inplace):
    """both settings of faer_hip_debug_fplu_inplace: the default one-launch path copies between scratch matrices and the view;
    `rowpad` is factored transposed (fplu.hip: transpose = !(|rs| < |cs|)), like the reference does it"""
    F = init_gpu()
    rng = np.random.default_rng(m * 31 + n)
    a = np.asarray(rng.standard_normal((m, n)), dtype=dtype)
    _, ref = place_host(a, layout)
    rp, rpi, cp, cpi, nt = oracle.full_piv_lu_in_place(ref)
    A = Held(a, layout)
    F.lib().faer_hip_debug_fplu_inplace(inplace)
    try:
        rf, rb, cf, cb, cnt = F.full_piv_lu_factor_in_place(A.view)
        got = A.host()
    finally:
        F.lib().faer_hip_debug_fplu_inplace(0)
    A.intact("full-pivot lu")
    no_new_nan(got, ref, "full-pivot lu")
    assert np.array_equal(rf.astype(np.int64), rp) and np.array_equal(rb.astype(np.int64), rpi)
    assert np.array_equal(cf.astype(np.int64), cp) and np.array_equal(cb.astype(np.int64), cpi) and cnt == nt
    # test_full_piv_lu_vs_oracle
    assert np.abs(got - ref).max() <= 64 * max(m, n) * EPS[np.dtype(dtype)] * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------ QR (qr.hip, tsqr.hip panels)
def q_from(F, basis, coeff, m, dtype, layout):
    """Q = Q I through the left application, the identity placed like everything else"""
    Q = Held(np.eye(m, dtype=dtype), layout)
    F.apply_block_householder_sequence_on_the_left_in_place(basis, coeff, Q.view, transpose=False)
    q = Q.host()
    Q.intact("apply on the left")
    return q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,bs,layout", cases([(100, 40, 4), (40, 100, 15), (512, 200, 32), (1024, 256, 32), (2500, 700, 128)], {0, 1, 3}))
def test_qr_on_views(oracle, m, n, bs, layout, dtype):
    """(1024, 256, 32): the whole-matrix one-pass path of tsqr.hip; (2500, 700, 128): one-pass panels inside the classic
    recursion; the others: the classic path down to its leaves.  H is placed as well"""
    F = init_gpu()
    rng = np.random.default_rng(m * 131 + n)
    a = rnd(rng, m, n, dtype)
    size = min(m, n)
    _, ref = place_host(a, layout)
    _, rh = place_host(np.zeros((bs, size), dtype=dtype), layout)
    assert oracle.qr_in_place(ref, rh) == size
    A, H = Held(a, layout), Held(np.zeros((bs, size), dtype=dtype), layout)
    assert F.qr_factor_in_place(A.view, H.view) == size
    qr, h = A.host(), H.host()
    A.intact("qr")
    H.intact("qr coefficients")
    no_new_nan(qr, ref, "qr")
    no_new_nan(h, rh, "qr coefficients")
    e = EPS[np.dtype(dtype)]
    # test_qr_full_rank_vs_oracle (the same expressions in test_qr_moderately_tall_one_pass_shape_rule and
    # test_qr_classic_path_one_pass_panels_vs_oracle, which cover the two larger shapes densely)
    tol = 64 * max(m, n) * e * max(1.0, np.abs(a).max())
    q = q_from(F, A.view[:, :size], H.view, m, dtype, layout).astype(np.float64)
    A.intact("qr basis read by the application")
    assert np.abs(q @ np.triu(qr).astype(np.float64) - a).max() <= tol
    assert np.abs(q.T @ q - np.eye(m)).max() <= tol
    assert np.abs(qr.astype(np.float64) - ref).max() <= 8 * tol
    fin = np.isfinite(rh)
    assert (np.isfinite(h) == fin).all()
    up = block_upper(bs, size)
    assert np.abs(h.astype(np.float64) - np.where(fin, rh, 0.0))[fin & up].max(initial=0) <= 8 * tol * max(1.0, np.abs(rh[fin & up]).max(initial=0))


# ------------------------------------------------------------------------------------------ column-pivot QR (colpiv_qr.hip)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,layout", cases([(40, 30), (30, 40), (200, 50), (400, 400)], {0, 1, 3}))
def test_colpiv_qr_on_views(oracle, m, n, layout, dtype):
    """`rowpad` and `step2` have row stride != 1: no delayed updates (colpiv_qr.hip delayed_ok, the reference's rule)"""
    F = init_gpu()
    rng = np.random.default_rng(m * n)
    a = np.asarray(rng.standard_normal((m, n)) * np.logspace(0, -3, n)[None, :], dtype=dtype)
    size = min(m, n)
    bs = oracle.qr_recommended_block_size(m, n, dtype)
    _, ref = place_host(a, layout)
    _, href = place_host(np.zeros((bs, size), dtype=dtype), layout)
    cp, cpi, nt = oracle.colpiv_qr_in_place(ref, href)
    A, H = Held(a, layout), Held(np.zeros((bs, size), dtype=dtype), layout)
    cf, cb, cnt = F.colpiv_qr_factor_in_place(A.view, H.view)
    got, hg = A.host(), H.host()
    A.intact("colpiv qr")
    H.intact("colpiv qr coefficients")
    no_new_nan(got, ref, "colpiv qr")
    no_new_nan(hg, href, "colpiv qr coefficients")
    assert np.array_equal(cf.astype(np.int64), cp) and np.array_equal(cb.astype(np.int64), cpi) and cnt == nt
    # test_colpiv_qr_vs_oracle
    tol = 256 * max(m, n) * EPS[np.dtype(dtype)] * max(1.0, np.abs(a).max())
    assert np.abs(got - ref).max() <= tol
    fin = np.isfinite(href)
    assert np.array_equal(np.isfinite(hg), fin) and np.array_equal(hg[~fin], href[~fin])
    assert np.abs(hg[fin] - href[fin]).max(initial=0) <= tol * 4


# ------------------------------------------------------------------------------------------ condensed forms (condense.hip)
CONDENSE = cases([(17, 1), (129, 32), (700, 32)], {0, 1, 2})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b,layout", CONDENSE)
def test_tridiag_on_views(n, b, layout, dtype):
    from oracle import oracle as O

    F = init_gpu()
    rng = np.random.default_rng(n * 7 + b)
    x = rng.standard_normal((n, n))
    a = np.asarray(x + x.T, dtype=dtype)
    iu = np.triu_indices(n, 1)
    marked = a.copy()
    marked[iu] = -7.5  # tridiag.rs works on the lower triangle
    _, vo = place_host(marked, layout)
    _, ho = place_host(np.zeros((b, n - 1), dtype=dtype), layout)
    O.tridiag_in_place(vo, ho)
    A, H = Held(marked, layout), Held(np.zeros((b, n - 1), dtype=dtype), layout)
    F.tridiag_in_place(A.view, H.view)
    v, h = A.host(), H.host()
    A.intact("tridiag")
    H.intact("tridiag coefficients")
    assert (v[iu] == -7.5).all()
    no_new_nan(v, vo, "tridiag")
    no_new_nan(h, ho, "tridiag coefficients")
    # test_tridiag_vs_oracle
    eps = EPS[np.dtype(dtype)]
    scale = np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(tridiag_of(v) - tridiag_of(vo)).max() <= 64 * n * eps * scale
    il = np.tril_indices(n, -2)
    assert np.abs(v[il] - vo[il]).max(initial=0.0) <= 64 * n * eps
    fin = np.isfinite(ho)
    assert np.array_equal(np.isfinite(h), fin)
    assert np.abs(h[fin] - ho[fin]).max(initial=0.0) <= 64 * n * eps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b,layout", CONDENSE)
def test_hessenberg_on_views(n, b, layout, dtype):
    from oracle import oracle as O

    F = init_gpu()
    rng = np.random.default_rng(n * 5 + b)
    a = np.asarray(rng.standard_normal((n, n)), dtype=dtype)
    _, vo = place_host(a, layout)
    _, ho = place_host(np.zeros((b, n - 1), dtype=dtype), layout)
    O.hessenberg_in_place(vo, ho)
    A, H = Held(a, layout), Held(np.zeros((b, n - 1), dtype=dtype), layout)
    F.hessenberg_in_place(A.view, H.view)
    v, h = A.host(), H.host()
    A.intact("hessenberg")
    H.intact("hessenberg coefficients")
    no_new_nan(v, vo, "hessenberg")
    no_new_nan(h, ho, "hessenberg coefficients")
    # test_hessenberg_vs_oracle (tests/test_gpu_hessenberg.py _vs_oracle): H normwise, reflectors and block factors per column
    eps = EPS[np.dtype(dtype)]
    scale = np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(hess_of(v) - hess_of(vo)).max() <= 64 * n * eps * scale
    sub = np.abs(np.diag(vo, -1)).astype(np.float64)
    cond = np.maximum(1.0, scale / np.where(sub != 0, sub, scale))
    for j in range(n - 2):
        assert np.abs(v[j + 2:, j] - vo[j + 2:, j]).max(initial=0.0) <= 64 * n * eps * cond[j], j
    fin = np.isfinite(ho)
    assert np.array_equal(np.isfinite(h), fin)
    for j in range(n - 1):
        cj = cond[(j // b) * b:j + 1].max()
        fj = fin[:, j]
        assert np.abs(h[fj, j] - ho[fj, j]).max(initial=0.0) <= 64 * n * eps * cj, j


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,bl,br,layout", cases([(130, 129, 32, 16), (515, 515, 32, 32)], {0, 1}))
def test_bidiag_on_views(m, n, bl, br, layout, dtype):
    from oracle import oracle as O

    F = init_gpu()
    rng = np.random.default_rng(m * 13 + n)
    a = np.asarray(rng.standard_normal((m, n)), dtype=dtype)
    zl, zr = np.zeros((bl, n), dtype=dtype), np.zeros((br, n - 1), dtype=dtype)
    (_, uo), (_, hlo), (_, hro) = place_host(a, layout), place_host(zl, layout), place_host(zr, layout)
    O.bidiag_in_place(uo, hlo, hro)
    A, HL, HR = Held(a, layout), Held(zl, layout), Held(zr, layout)
    F.bidiag_in_place(A.view, HL.view, HR.view)
    u, hl, hr = A.host(), HL.host(), HR.host()
    for held, what in ((A, "bidiag"), (HL, "bidiag left coefficients"), (HR, "bidiag right coefficients")):
        held.intact(what)
    no_new_nan(u, uo, "bidiag")
    no_new_nan(hl, hlo, "bidiag left coefficients")
    no_new_nan(hr, hro, "bidiag right coefficients")
    # test_bidiag_vs_oracle: B normwise, reflectors and block factors with the conditioning of the entry each one produces
    eps = EPS[np.dtype(dtype)]
    scale = np.linalg.norm(a.astype(np.float64), 2)
    mx = max(m, n)
    assert np.abs(bidiag_of(u) - bidiag_of(uo)).max() <= 64 * mx * eps * scale
    bo = bidiag_of(uo).astype(np.float64)
    dg = np.abs(np.diag(bo))[:min(m, n)]
    sg = np.abs(np.diag(bo, 1))
    cl = np.maximum(1.0, scale / np.where(dg != 0, dg, scale))
    cr = np.maximum(1.0, scale / np.where(sg != 0, sg, scale))
    for j in range(min(m, n)):
        assert np.abs(u[j + 1:, j] - uo[j + 1:, j]).max(initial=0.0) <= 64 * mx * eps * cl[j], ("left", j)
        if j + 2 < n:
            assert np.abs(u[j, j + 2:] - uo[j, j + 2:]).max(initial=0.0) <= 64 * mx * eps * cr[j], ("right", j)
    for h, ho, cc, bb in ((hl, hlo, cl, bl), (hr, hro, cr, br)):
        fin = np.isfinite(ho)
        assert np.array_equal(np.isfinite(h), fin)
        for j in range(ho.shape[1]):
            cj = cc[(j // bb) * bb:j + 1].max(initial=1.0)
            fj = fin[:, j]
            assert np.abs(h[fj, j] - ho[fj, j]).max(initial=0.0) <= 64 * mx * eps * cj, j


# ------------------------------------------------------------------------------------------ self-adjoint EVD (evd.hip)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,layout", cases([5, 257, 1000], {0, 1, 2}))
def test_self_adjoint_evd_on_views(n, layout, dtype):
    """A with a sentinel strict upper triangle (never read, never written), U placed, S with stride 3 inside a guarded vector"""
    import torch

    F = init_gpu()
    x = np.random.default_rng(n).standard_normal((n, n))
    a = np.asarray(x + x.T, dtype=dtype)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5
    A, U = Held(marked, layout), Held(np.zeros((n, n), dtype=dtype), layout)
    isz = np.dtype(dtype).itemsize
    s_buf = torch.full((3 * n + 2,), GUARD_BITS[isz], dtype=torch.int64 if isz == 8 else torch.int32, device="cuda").view(A.view.dtype)
    s_before = s_buf.clone()
    sv = s_buf[1::3][:n]
    assert sv.stride(0) == 3 and sv.shape[0] == n
    assert F.self_adjoint_evd(A.view, sv, U.view) == F.EVD_OK
    s, u = to_host(sv), U.host()
    A.untouched("evd")
    U.intact("evd eigenvectors")
    gaps = torch.ones(3 * n + 2, dtype=torch.bool, device="cuda")
    gaps[1:1 + 3 * n:3] = False
    assert torch.equal(bits(s_buf)[gaps], bits(s_before)[gaps]), "S's gaps were written"
    no_new_nan(s, None, "eigenvalues")
    no_new_nan(u, None, "eigenvectors")
    evd_check(a, s, u)  # test_random_against_lapack: values, residual per column and orthogonality at C_TOL n eps


# ------------------------------------------------------------------------------------------ solves and applications
SOLVES = cases([(257, 64), (600, 9)], {0})


def well_conditioned(rng, n, dtype):
    return np.asarray(rng.standard_normal((n, n)) + 2 * np.sqrt(n) * np.eye(n), dtype=dtype, order="F")


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_partial_piv_lu_solve_on_views(oracle, n, k, layout, dtype, transpose):
    F = init_gpu()
    rng = np.random.default_rng(3 * n + k)
    a, b = well_conditioned(rng, n, dtype), rnd(rng, n, k, dtype)
    lu = a.copy(order="F")
    perm, perm_inv, _ = oracle.lu_in_place(lu)
    if not transpose:
        ref = np.asfortranarray(b[perm])
        oracle.trsm(lu, ref, unit=True)
        oracle.trsm(lu, ref, upper=True)
    else:
        ref = b.copy(order="F")
        oracle.trsm(lu.T, ref)
        oracle.trsm(lu.T, ref, upper=True, unit=True)
        ref = np.asfortranarray(ref[perm_inv])
    A = Held(a, layout)
    pf, pb, _ = F.partial_piv_lu_factor_in_place(A.view)
    assert np.array_equal(pf.astype(np.int64), perm)
    A.intact("lu")
    LU, X = Held(A.host(), layout), Held(b, layout)
    F.partial_piv_lu_solve_in_place(LU.view, pf, pb, X.view, transpose=transpose)
    x = X.host()
    LU.untouched("lu solve")
    X.intact("lu solve rhs")
    no_new_nan(x, None, "lu solve")
    kappa = np.linalg.cond(a.astype(np.float64))
    # test_partial_piv_lu_solve_vs_oracle
    assert np.abs(x.astype(np.float64) - ref).max() <= 64 * n * EPS[np.dtype(dtype)] * kappa * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_full_piv_lu_solve_on_views(n, k, layout, dtype, transpose):
    F = init_gpu()
    rng = np.random.default_rng(n * 31 + n)
    a, b = np.asarray(rng.standard_normal((n, n)), dtype=dtype), rnd(rng, n, k, dtype)
    A = Held(a, layout)
    rf, rb, cf, cb, _ = F.full_piv_lu_factor_in_place(A.view)
    A.intact("full-pivot lu")
    LU, X = Held(A.host(), layout), Held(b, layout)
    F.full_piv_lu_solve_in_place(LU.view, rf, rb, cf, cb, X.view, transpose=transpose)
    x = X.host()
    LU.untouched("full-pivot lu solve")
    X.intact("full-pivot lu solve rhs")
    no_new_nan(x, None, "full-pivot lu solve")
    # test_full_piv_lu_vs_oracle: the residual of the solve and of the transpose solve
    a64 = a.astype(np.float64)
    tol = 256 * n * EPS[np.dtype(dtype)] * np.linalg.cond(a64)
    assert np.abs((a64.T if transpose else a64) @ x - b).max() <= tol * np.abs(b).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_llt_solve_on_views(oracle, n, k, layout, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n + k)
    a, b = spd(rng, n, dtype), rnd(rng, n, k, dtype)
    l = a.copy(order="F")
    assert oracle.llt_in_place(l) == ("ok", 0)
    ref = b.copy(order="F")
    oracle.trsm(l, ref)
    oracle.trsm(l.T, ref, upper=True)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5  # the solve reads the lower triangle only
    A = Held(marked, layout)
    assert F.llt_factor_in_place(A.view) == 0
    Lf, X = Held(A.host(), layout), Held(b, layout)
    F.llt_solve_in_place(Lf.view, X.view)
    x = X.host()
    Lf.untouched("llt solve")
    X.intact("llt solve rhs")
    no_new_nan(x, None, "llt solve")
    kappa = np.linalg.cond(a.astype(np.float64))
    # test_llt_solve_vs_oracle
    assert np.abs(x.astype(np.float64) - ref).max() <= 64 * n * EPS[np.dtype(dtype)] * kappa * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_ldlt_solve_on_views(n, k, layout, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n + 2 * k)
    a, _ = quasi_definite(rng, n, dtype)
    b = rnd(rng, n, k, dtype)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5
    A = Held(marked, layout)
    assert F.ldlt_factor_in_place(A.view) == 0
    LD, X = Held(A.host(), layout), Held(b, layout)
    F.ldlt_solve_in_place(LD.view, X.view)
    x = X.host().astype(np.float64)
    LD.untouched("ldlt solve")
    X.intact("ldlt solve rhs")
    no_new_nan(x, None, "ldlt solve")
    a64 = a.astype(np.float64)
    ref = np.linalg.solve(a64, b.astype(np.float64))
    if dtype == np.float64:  # test_ldlt_zero_pivot_regularization_and_solve (the only dense LDLT solve, fp64, same matrices)
        assert np.abs(x - ref).max() <= 1e-9
    else:
        # no dense fp32 LDLT solve exists.  The solve is two unit-triangular substitutions and a diagonal scaling with factors
        # that agree with the exact ones to c n eps kappa, the situation of test_llt_solve_vs_oracle: its expression
        assert np.abs(x - ref).max() <= 64 * n * EPS[np.dtype(dtype)] * np.linalg.cond(a64) * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_qr_solve_lstsq_on_views(oracle, n, k, layout, dtype):
    F = init_gpu()
    m = n + 43
    rng = np.random.default_rng(m + n + k)
    a, b = rnd(rng, m, n, dtype), rnd(rng, m, k, dtype)
    bs = oracle.qr_recommended_block_size(m, n, dtype)
    qr, h = a.copy(order="F"), np.zeros((bs, n), dtype=dtype, order="F")
    assert oracle.qr_in_place(qr, h) == n
    ref = b.copy(order="F")
    oracle.apply_householder_sequence_left(qr, h, ref, True)
    top = np.asfortranarray(ref[:n])
    oracle.trsm(qr[:n, :n], top, upper=True)
    A, H = Held(a, layout), Held(np.zeros((bs, n), dtype=dtype), layout)
    assert F.qr_factor_in_place(A.view, H.view) == n
    QR, HC, X = Held(A.host(), layout), Held(H.host(), layout), Held(b, layout)
    F.qr_solve_lstsq_in_place(QR.view, HC.view, X.view)
    x = X.host()
    QR.untouched("qr lstsq")
    HC.untouched("qr lstsq coefficients")
    X.intact("qr lstsq rhs")
    no_new_nan(x, None, "qr lstsq")
    kappa = np.linalg.cond(a.astype(np.float64))
    # test_qr_solve_lstsq_vs_oracle
    assert np.abs(x[:n].astype(np.float64) - top).max() <= 64 * max(m, n) * EPS[np.dtype(dtype)] * kappa * max(1.0, np.abs(top).max())


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,layout", SOLVES)
def test_apply_householder_sequences_on_views(n, k, layout, dtype, transpose):
    """test_apply_householder_on_the_right with basis, coefficients and both operands placed: Q from the left application on I
    is orthogonal, M Q / M Q^H and Q B / Q^H B agree with products by that Q"""
    F = init_gpu()
    m = n + 43
    rng = np.random.default_rng(m + n + k)
    a = rnd(rng, m, n, dtype)
    bs = F.qr_recommended_block_size(m, n, dtype)
    A, H = Held(a, layout), Held(np.zeros((bs, n), dtype=dtype), layout)
    assert F.qr_factor_in_place(A.view, H.view) == n
    V, T = Held(A.host(), layout), Held(H.host(), layout)
    e = float(EPS[np.dtype(dtype)])
    Q = q_from(F, V.view, T.view, m, dtype, layout).astype(np.float64)
    # test_apply_householder_on_the_right (2.3e-16 there is the fp64 eps)
    assert np.abs(Q.T @ Q - np.eye(m)).max() <= 64 * m * e
    Qop = Q.T if transpose else Q
    mat = rnd(rng, k, m, dtype)
    M = Held(mat, layout)
    F.apply_block_householder_sequence_on_the_right_in_place(V.view, T.view, M.view, transpose=transpose)
    got = M.host()
    M.intact("apply on the right")
    no_new_nan(got, None, "apply on the right")
    ref = mat.astype(np.float64) @ Qop
    assert np.abs(got - ref).max() <= 64 * m * e * np.abs(ref).max()
    # the left application on a right-hand side: the mirror image of the product above, held to the same expression
    b = rnd(rng, m, k, dtype)
    B = Held(b, layout)
    F.apply_block_householder_sequence_on_the_left_in_place(V.view, T.view, B.view, transpose=transpose)
    got = B.host()
    B.intact("apply on the left")
    no_new_nan(got, None, "apply on the left")
    ref = Qop @ b.astype(np.float64)
    assert np.abs(got - ref).max() <= 64 * m * e * np.abs(ref).max()
    V.untouched("householder basis")
    T.untouched("householder coefficients")


# ------------------------------------------------------------------------------------------ extras.hip
EXTRAS = cases([129, 300], {0})


def tol(n, dtype, c=64):
    """tests/test_gpu_extras.py tol()"""
    return c * max(n, 1) * EPS[np.dtype(dtype)]


def full_of(shape, value, dtype):
    return np.full(shape, value, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("n,layout", EXTRAS)
def test_triangular_inverse_on_views(n, layout, unit, upper, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n * 4 + 2 * unit + upper)
    t = (rnd(rng, n, n, dtype) / n ** 0.5 + 2 * np.eye(n, dtype=dtype)).astype(dtype)
    tri = np.triu(t) if upper else np.tril(t)
    if unit:
        np.fill_diagonal(tri, 1.0)
    mask = (np.triu(np.ones((n, n), bool), 1 if unit else 0) if upper else np.tril(np.ones((n, n), bool), -1 if unit else 0))
    junk = t.copy() if not unit else t + 3 * np.eye(n, dtype=dtype)  # the other triangle (and a unit diagonal) hold values never to be read
    T, Out = Held(junk, layout), Held(full_of((n, n), -7.5, dtype), layout)
    F.inverse_triangular_in_place(Out.view, T.view, upper=upper, unit=unit)
    got = Out.host()
    T.untouched("triangular inverse")
    Out.intact("triangular inverse")
    assert (got[~mask] == -7.5).all()
    no_new_nan(got, None, "triangular inverse")
    # test_triangular_inverse
    ref = np.linalg.inv(tri.astype(np.float64))
    assert np.abs(got[mask] - ref[mask]).max(initial=0) <= tol(n, dtype) * max(1.0, np.abs(ref).max())


def _lower_outputs(F, fn, factor, n, dtype, layout, what):
    """reconstruct / inverse into the lower triangle of a placed Out full of -7.5"""
    Out = Held(full_of((n, n), -7.5, dtype), layout)
    fn(Out.view, factor.view)
    got = Out.host()
    factor.untouched(what)
    Out.intact(what)
    assert (got[np.triu_indices(n, 1)] == -7.5).all()
    no_new_nan(got, None, what)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["llt", "ldlt"])
@pytest.mark.parametrize("n,layout", EXTRAS)
def test_cholesky_reconstruct_and_inverse_on_views(n, layout, kind, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n + (kind == "ldlt"))
    a = spd(rng, n, dtype)
    marked = a.copy()
    marked[np.triu_indices(n, 1)] = -7.5
    A = Held(marked, layout)
    assert (F.llt_factor_in_place if kind == "llt" else F.ldlt_factor_in_place)(A.view) == 0
    Fac = Held(A.host(), layout)
    il = np.tril_indices(n)
    # test_llt_reconstruct_and_inverse / test_ldlt_reconstruct_and_inverse
    got = _lower_outputs(F, F.llt_reconstruct if kind == "llt" else F.ldlt_reconstruct, Fac, n, dtype, layout, kind + " reconstruct")
    assert np.abs(got[il] - a[il]).max() <= tol(n, dtype) * np.abs(a).max()
    got = _lower_outputs(F, F.llt_inverse if kind == "llt" else F.ldlt_inverse, Fac, n, dtype, layout, kind + " inverse")
    ainv = np.tril(got.astype(np.float64)) + np.tril(got.astype(np.float64), -1).T
    a64 = a.astype(np.float64)
    assert np.abs(ainv @ a64 - np.eye(n)).max() <= tol(n, dtype, 256) * np.linalg.cond(a64)


def _full_outputs(fn, held, shape, dtype, layout, what):
    """reconstruct / inverse into a placed Out whose view starts as plain NaNs (test_gpu_extras.py starts from NaN as well)"""
    Out = Held(full_of(shape, np.nan, dtype), layout)
    fn(Out.view)
    got = Out.host()
    for h in held:
        h.untouched(what)
    Out.intact(what)
    no_new_nan(got, None, what)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["lu", "full_piv_lu", "qr", "colpiv_qr"])
@pytest.mark.parametrize("n,layout", EXTRAS)
def test_reconstruct_and_inverse_on_views(n, layout, kind, dtype):
    """partial_piv_lu_, full_piv_lu_, qr_ and colpiv_qr_ reconstruct and inverse: test_lu_reconstruct_and_inverse,
    test_full_piv_lu_reconstruct_and_inverse, test_qr_reconstruct_and_inverse, test_colpiv_qr_reconstruct_and_inverse"""
    F = init_gpu()
    rng = np.random.default_rng(n * 3 + len(kind))
    a = rnd(rng, n, n, dtype)
    if kind != "full_piv_lu":
        a = (a + n ** 0.5 * np.eye(n, dtype=dtype)).astype(dtype)
    A = Held(a, layout)
    if kind == "lu":
        fwd, bwd, _ = F.partial_piv_lu_factor_in_place(A.view)
        Fac = Held(A.host(), layout)
        held = [Fac]
        rec = lambda out: F.partial_piv_lu_reconstruct(out, Fac.view, fwd, bwd)
        inv = lambda out: F.partial_piv_lu_inverse(out, Fac.view, fwd, bwd)
    elif kind == "full_piv_lu":
        rf, rb, cf, cb, _ = F.full_piv_lu_factor_in_place(A.view)
        Fac = Held(A.host(), layout)
        held = [Fac]
        rec = lambda out: F.full_piv_lu_reconstruct(out, Fac.view, rf, rb, cf, cb)
        inv = lambda out: F.full_piv_lu_inverse(out, Fac.view, rf, rb, cf, cb)
    else:
        bs = F.qr_recommended_block_size(n, n, dtype)
        H = Held(np.zeros((bs, n), dtype=dtype), layout)
        if kind == "qr":
            F.qr_factor_in_place(A.view, H.view)
        else:
            cf, cb, _ = F.colpiv_qr_factor_in_place(A.view, H.view)
        Fac, T = Held(A.host(), layout), Held(H.host(), layout)
        held = [Fac, T]
        if kind == "qr":
            rec = lambda out: F.qr_reconstruct(out, Fac.view, T.view)
            inv = lambda out: F.qr_inverse(out, Fac.view, T.view)
        else:
            rec = lambda out: F.colpiv_qr_reconstruct(out, Fac.view, T.view, cf, cb)
            inv = lambda out: F.colpiv_qr_inverse(out, Fac.view, T.view, cf, cb)
    A.intact(kind)
    got = _full_outputs(rec, held, (n, n), dtype, layout, kind + " reconstruct")
    assert np.abs(got - a).max() <= tol(n, dtype) * np.abs(a).max()
    got = _full_outputs(inv, held, (n, n), dtype, layout, kind + " inverse")
    a64 = a.astype(np.float64)
    assert np.abs(got.astype(np.float64) @ a64 - np.eye(n)).max() <= tol(n, dtype, 256) * np.linalg.cond(a64)
