"""Writes bidiag_svd_cases.json: the bidiagonal test matrices of the reference's divide-and-conquer SVD tests (data only).

Sources (faer 0.24, run where the reference tree is present; the GPU tests read the JSON, never the tree):
  * faer/test_data/svd/svd64.txt, svd128.txt, svd512.txt -- `diag` / `subdiag` columns read by
    svd/bidiag_svd.rs parse_bidiag (test_divide_and_conquer);
  * the diag / col0 literals of test_deflation43, test_deflation44 and test_both_deflation in the same file, kept as
    (diag, offdiag) pairs of 7 entries.
`offdiag` has as many entries as `diag`; an n x n upper bidiagonal matrix uses its first n - 1.
"""
import json
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FAER_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


def parse_bidiag(path):
    diag, sub, cur = [], [], None
    for line in open(path):
        line = line.strip().rstrip(",")
        if line.startswith("subdiag"):
            cur = sub
        elif line.startswith("diag"):
            cur = diag
        elif line:
            cur.append(float(line))
    assert len(diag) == len(sub)
    return {"diag": diag, "offdiag": sub}


cases = {}
for name in ("svd64", "svd128", "svd512"):
    cases[name] = parse_bidiag(os.path.join(REF, "faer", "test_data", "svd", name + ".txt"))
ones = [1.0] * 7
cases["deflation43"] = {"diag": [1.0, 5.0, 3.0, 1e-7, 4.0, 2.0, 2e-7], "offdiag": ones}
cases["deflation44"] = {"diag": [1.0, 5.0, 3.0, 1.0, 4.0, 2.0, 1.0], "offdiag": ones}
cases["both_deflations"] = {"diag": [1.0, 5.0, 3.0, 2.0, 4.0, 2.0, 0.0], "offdiag": ones}
out = {"source": "bidiagonal test matrices of faer's divide-and-conquer SVD tests (diag, offdiag)", "cases": cases}
with open(os.path.join(HERE, "bidiag_svd_cases.json"), "w") as f:
    json.dump(out, f)
    f.write("\n")
print({k: len(v["diag"]) for k, v in cases.items()})
