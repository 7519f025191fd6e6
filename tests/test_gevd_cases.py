"""tests/gevd_cases.py alone (CPU): the recorded results of tests/golden/gevd_bounds.json and gevd_spectra.npz are current where scipy is installed, and
the reference solver passes both verdicts on every listed case and size, within the cap on pairs left out of the assignment."""
import importlib.util
import os

import numpy as np
import pytest

import gevd_cases as gc

spec = importlib.util.spec_from_file_location("make_gevd_bounds", os.path.join(os.path.dirname(gc.GOLDEN), "make_gevd_bounds.py"))
mk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mk)

CASES = [(kind, n, dtype) for dtype in gc.DTYPES for kind, n in gc.all_cases(mk.sizes(dtype))]
IDS = [f"{k}-{n}-{np.dtype(d).name}" for k, n, d in CASES]


def test_golden_file_lists_exactly_the_cases():
    import json

    keys = set(json.load(open(gc.GOLDEN)))
    assert keys == {gc._key(k, n, d) for k, n, d in CASES}
    z = np.load(gc.GOLDEN_SPECTRA)
    total = sum(int(k.split("/")[1]) for k in keys)
    assert set(z.files) == {"alpha", "beta", "kappa"} and all(z[name].shape == (total,) for name in z.files)
    assert os.path.getsize(gc.GOLDEN) < (1 << 20) and os.path.getsize(gc.GOLDEN_SPECTRA) < (1 << 20)


@pytest.mark.parametrize("kind,n,dtype", CASES, ids=IDS)
def test_reference_passes_its_own_verdicts(kind, n, dtype):
    pytest.importorskip("scipy")
    a, b = gc.generate(kind, n, dtype)
    own = gc._compute(kind, n, dtype)
    ref = gc.reference(kind, n, dtype)
    gold = gc.reference(kind, n, dtype, prefer_golden=True)
    # the recorded results are current
    # the recorded results are current: the recorded spectrum is the live one to well within the radii (another build of LAPACK
    # rounds differently), the residuals and condition numbers agree in magnitude
    cur = dict(ref, radius=np.minimum(ref["radius"], 1.0) / 16)
    assert gc.assign_pairs(gold["alpha"], gold["beta"], cur)[0]
    e = gc.eps_of(dtype)
    assert abs(gold["res_right"] - ref["res_right"]) <= n * e and abs(gold["res_left"] - ref["res_left"]) <= n * e
    assert np.allclose(np.sort(np.log2(gold["kappa"])), np.sort(np.log2(np.minimum(ref["kappa"], 3e38))), atol=1.0)
    # the reference in the dtype of the case against the fp64 reference: the assignment, and the cap on pairs left out
    ok, left_out = gc.assign_pairs(own["own_alpha"], own["own_beta"], ref)
    assert ok and left_out <= 0.1 * n, (left_out, n)
    br, bl = gc.bounds(kind, n, dtype)
    assert own["res_right"] <= br and own["res_left"] <= bl
    if kind.startswith("singular_b"):
        k = gc.singular_count(kind, n)
        assert int((own["own_beta"] == 0).sum()) == k


def test_verdicts_reject_wrong_results():
    n, dtype = 17, np.float64
    a, b = gc.generate("random", n, dtype)
    own = gc._compute("random", n, dtype) if gc._sla is not None else None
    ref = gc.reference("random", n, dtype)
    al, be = ref["alpha"].copy(), ref["beta"].copy()
    assert gc.assign_pairs(al, be, ref)[0]
    assert gc.assign_pairs(al * 3.0, be * 3.0, ref)[0]  # a scaling of (alpha, beta) is the same eigenvalue
    al2 = al.copy()
    al2[0] = al2[1]
    be2 = be.copy()
    be2[0] = be2[1]
    assert not gc.assign_pairs(al2, be2, ref)[0]  # an eigenvalue reported twice, another one missing
    if own is not None:
        x = np.linalg.solve(a.astype(complex) * be[0] - b * al[0] + 1e-9 * np.eye(n), np.ones(n, complex))
        assert gc.pair_residuals(a, b, al[:1], be[:1], x[:, None]).max() < 1e-6
        assert gc.pair_residuals(a, b, al[:1], be[:1], np.ones((n, 1))).max() > 1e-3
