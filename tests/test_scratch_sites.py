"""Keeps the scratch-site table complete: every object under faer-rs_amd/csrc that creates device scratch -- each declarator of a `Scratch`
declaration, a direct call of Ctx::alloc, a `Staged` operand in whichever file declares it -- is counted per file and compared with SCRATCH_SITES at the top of
tests/test_gpu_scratch_poison.py, which names next to each count the poison cases that run the file's sites ("Scratch
sites", says what lives in each buffer and how it is initialised).  A new allocation site changes a count: its author adds or names
the case that covers it and a row of the table."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faer-rs_amd", "csrc")
DECL = re.compile(r"\b(?:Scratch|Staged<[^>]+>)\s+(?=\w+\s*[({])")
OTHER = re.compile(r"\.alloc\(|optional<Scratch>")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declarators(stmt):
    """the objects one declaration statement creates: identifiers directly followed by ( or { outside every bracket"""
    n = depth = 0
    for m in re.finditer(r"\w+\s*(?=[({])|[(){}]", stmt):
        tok = m.group(0)
        if tok in "({":
            depth += 1
        elif tok in ")}":
            depth -= 1
        elif depth == 0:
            n += 1
    return n


def count_sites(path):
    """scratch objects one source file creates: every declarator of a `Scratch a(..), b{..};` or `Staged<T> a(..), b(..);` statement (one
    line may hold several; api.hip and the drivers that stage their own operands), every direct call of Ctx::alloc, every optional<Scratch>"""
    text = strip_comments(open(path).read())
    n = len(OTHER.findall(text))
    for m in DECL.finditer(text):
        n += declarators(text[m.end():text.index(";", m.end())])
    return n


def table():
    """SCRATCH_SITES read from the source of the GPU test (importing it would need torch and a device)"""
    src = open(os.path.join(ROOT, "tests", "test_gpu_scratch_poison.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "SCRATCH_SITES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("SCRATCH_SITES not found in tests/test_gpu_scratch_poison.py")


def counted(csrc=CSRC):
    out = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            n = count_sites(os.path.join(csrc, name))
            if n:
                out[name] = n
    return out


def test_every_scratch_site_is_in_the_table():
    tab = table()
    got = counted()
    assert got == {k: v[0] for k, v in tab.items()}, (
        "scratch sites changed: update SCRATCH_SITES in tests/test_gpu_scratch_poison.py (and the table in DESIGN.md) and name the "
        f"poison case that covers the new site; counted {got}")


def test_every_table_row_names_its_cases():
    src = open(os.path.join(ROOT, "tests", "test_gpu_scratch_poison.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", src, re.M))
    for name, (_, cases) in table().items():
        named = set(re.findall(r"\btest_\w+", cases))
        assert named <= defined, (name, sorted(named - defined))
        assert named or "every test" in cases or "measurement aid" in cases, name
