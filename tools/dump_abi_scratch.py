#!/usr/bin/env python3
"""Calls every scratch query and every params getter of include/faer_hip.h and prints what they return, as JSON.

The header pins the names and signatures of the boundary (a conflicting definition does not compile); it does not pin what the
small bodies return.  tests/test_abi_scratch_snapshot.py compares a build with tests/abi_scratch_snapshot.json, which this tool
wrote from a build of the commit BEFORE a change of the boundary -- never from the code under test:

    python tools/dump_abi_scratch.py --label <commit> [--lib path/to/libfaer_hip.so] > tests/abi_scratch_snapshot.json

What is enumerated (from the header alone, no list to maintain): every FAER_HIP_API prototype that returns FaerLayout and every
`*Params_<scalar>(void)` getter.  None of them needs a device.  Arguments: size_t arguments get small distinct primes by position
(a swapped or dropped argument shows), FaerPar is Seq, a params struct is what its own getter returns for the scalar type of the
query, and an enum argument takes every one of its values (one entry per combination).  A function pointer in a params struct is
recorded as the exported symbol it points to and its value at (13, 7)."""
import argparse
import ctypes as C
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "faer_hip.h")
DEFAULT_LIB = os.path.join(ROOT, "faer-rs_amd", "libfaer_hip.so")
PRIMES = (13, 7, 5, 3, 2, 11)
FNPTR = C.CFUNCTYPE(C.c_size_t, C.c_size_t, C.c_size_t)
PLAIN = {"size_t": C.c_size_t, "double": C.c_double}


class Header:
    """the structs, enums and prototypes of the header that the queries need, as ctypes"""

    def __init__(self, path=HEADER):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
        self.enums = {m.group(1): [int(v) for v in re.findall(r"=\s*(\d+)", m.group(2))]
                      for m in re.finditer(r"typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S)}
        self.bodies = {m.group(1): m.group(2) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S)}
        self.structs = {}
        # (return type, name, [(type, name)]) of every exported prototype
        self.protos = {}
        for m in re.finditer(r"FAER_HIP_API\s+([\w\s\*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*;", text):
            args = [] if m.group(3).strip() == "void" else [tuple(a.strip().rsplit(None, 1)) for a in m.group(3).split(",")]
            self.protos[m.group(2)] = (" ".join(m.group(1).split()), args)

    def ctype(self, name):
        if name in PLAIN:
            return PLAIN[name]
        if name in self.enums:
            return C.c_int
        if name not in self.structs:
            fields = []
            for f in filter(None, (f.strip() for f in self.bodies[name].split(";"))):
                fp = re.fullmatch(r"size_t\s*\(\s*\*\s*(\w+)\s*\)\s*\(\s*size_t\s+\w+\s*,\s*size_t\s+\w+\s*\)", f)
                if fp:
                    fields.append((fp.group(1), FNPTR))
                else:
                    m = re.fullmatch(r"(\w+)\s+(\w+)", f)
                    assert m, f"{name}: a field this tool cannot read: {f!r}"
                    fields.append((m.group(2), self.ctype(m.group(1))))
            self.structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        return self.structs[name]

    def queries(self):
        """names of the scratch queries and of the params getters, sorted"""
        out = []
        for name, (ret, args) in self.protos.items():
            if ret == "FaerLayout" or (re.search(r"Params_\w+$", name) and not args and re.fullmatch(r"Faer\w+Params", ret)):
                out.append(name)
        return sorted(out)


def symbol_at(addr):
    """the exported symbol at an address of a loaded library (dladdr), or None"""

    class DlInfo(C.Structure):
        _fields_ = [("fname", C.c_char_p), ("fbase", C.c_void_p), ("sname", C.c_char_p), ("saddr", C.c_void_p)]

    dladdr = C.CDLL(None).dladdr
    dladdr.argtypes, dladdr.restype = [C.c_void_p, C.POINTER(DlInfo)], C.c_int
    info = DlInfo()
    if not dladdr(addr, C.byref(info)) or info.saddr != addr or not info.sname:
        return None
    return info.sname.decode()


def plain(v):
    """a returned ctypes value as JSON data"""
    if isinstance(v, C.Structure):
        return {f: plain(getattr(v, f)) for f, _ in v._fields_}
    if isinstance(v, FNPTR):
        addr = C.cast(v, C.c_void_p).value
        return {"symbol": symbol_at(addr), "at_13_7": v(13, 7)} if addr else None
    return v


def bind(lib, hdr, name, spelled=None):
    """the ctypes function of prototype `name`, looked up under `spelled` (its v0_24 alias) if given"""
    ret, args = hdr.protos[name]
    fn = getattr(lib, spelled or name)
    fn.restype = hdr.ctype(ret)
    fn.argtypes = [hdr.ctype(t) for t, _ in args]
    return fn


def call(lib, hdr, name, spelled=None):
    """{call key: result} of one query: one entry, or one per combination of its enum arguments"""
    ret, args = hdr.protos[name]
    fn = bind(lib, hdr, name, spelled)
    suffix = name.rsplit("_", 1)[1]
    primes = iter(PRIMES)
    fixed, enum_at = [], []
    for i, (t, _) in enumerate(args):
        if t == "size_t":
            fixed.append(next(primes))
        elif t == "FaerPar":
            fixed.append(hdr.ctype(t)(0, 1))  # FaerParTag_Seq
        elif t in hdr.enums:
            enum_at.append(i)
            fixed.append(None)
        else:
            assert t.endswith("Params"), f"{name}: an argument this tool cannot make: {t}"
            getter = f"libfaer_v0_23_{t[len('Faer'):]}_{suffix}"
            fixed.append(bind(lib, hdr, getter)())
    out = {}
    for combo in itertools.product(*(hdr.enums[args[i][0]] for i in enum_at)):
        a = list(fixed)
        for i, v in zip(enum_at, combo):
            a[i] = v
        key = name + ("(" + ",".join(map(str, combo)) + ")" if combo else "")
        out[key] = plain(fn(*a))
    return out


def dump(lib_path=DEFAULT_LIB, spelling="v0_23"):
    """{call key: result} of every query of the header; spelling="v0_24": through the exported v0_24 aliases only (keys stay v0_23)"""
    lib, hdr = C.CDLL(lib_path), Header()
    out = {}
    for name in hdr.queries():
        if spelling == "v0_23":
            out.update(call(lib, hdr, name))
        elif name.startswith("libfaer_v0_23_") and hasattr(lib, name.replace("v0_23", spelling)):
            out.update(call(lib, hdr, name, name.replace("v0_23", spelling)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=os.environ.get("FAER_HIP_LIB", DEFAULT_LIB))
    ap.add_argument("--label", required=True, help="the commit the library was built from")
    a = ap.parse_args()
    json.dump({"generated_from": a.label, "entries": dump(a.lib)}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
