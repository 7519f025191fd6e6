"""CPU tests of the Full strategy at the LBLT boundary (include/faer_hip.h sections 2g and 3): the query that tells a caller which
pivoting strategies the factorization runs, without a device and without a call into the factorization itself."""
import os
import re

import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pivoting_supported():
    F = fa()
    assert [F.lblt_pivoting_supported(p) for p in range(5)] == [1] * 5
    assert F.lblt_pivoting_supported(-1) == 0 and F.lblt_pivoting_supported(5) == 0
    assert all(F.lblt_pivoting_supported(name) == 1 for name in F.PivotingStrategy)
    assert F.lblt_pivoting_supported("no_such_strategy") == 0


def test_query_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    assert re.search(r"FAER_HIP_API int faer_hip_lblt_pivoting_supported\(FaerPivotingStrategy \w+\);", hdr)
    assert hasattr(fa().lib(), "faer_hip_lblt_pivoting_supported")


def test_unsupported_value_raises_before_the_library_is_entered():
    import numpy as np

    F = fa()
    with pytest.raises(ValueError):
        F.lblt_factor_in_place(np.eye(3, order="F"), pivoting=5)
    with pytest.raises(KeyError):
        F.lblt_factor_in_place(np.eye(3, order="F"), pivoting="fullest")
