"""CPU test of the Python front ends' shape: every launching entry point of the C ABI is marshalled by ONE function of the package (the
`ops.*_raw` helpers and the few Functions that own an entry point outright), and torch_ops.py holds no call into the library at all.  Reads
only the package's own Python source."""
import ast
import os
from collections import defaultdict

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "facialmmt_amd")

# entry points that may be called from more than one function: name -> the one-line reason (at most three; `*_workspace` size queries are exempt
# by rule: an allocator and its consumer may both ask for a size)
ALLOWED_TWICE: dict = {}


def _fmmt_call_sites():
    """{entry point: {"file.py::Qualified.function", ...}} over every `<expr>.fmmt_*(...)` call of the package"""
    sites = defaultdict(set)

    def walk(node, where, rel):
        for child in ast.iter_child_nodes(node):
            inner = where
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                inner = f"{where}.{child.name}" if where else child.name
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr.startswith("fmmt_"):
                sites[child.func.attr].add(f"{rel}::{inner or '<module>'}")
            walk(child, inner, rel)

    for d, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(d, f)
                with open(path) as fh:
                    walk(ast.parse(fh.read(), path), "", os.path.relpath(path, PKG))
    return sites


def test_each_entry_point_is_marshalled_by_one_function():
    sites = _fmmt_call_sites()
    assert len(sites) > 50, "the walk found too few entry points to mean anything"
    assert len(ALLOWED_TWICE) <= 3
    in_torch_ops = {name: sorted(w for w in where if w.startswith("torch_ops.py::")) for name, where in sites.items()}
    assert not {n: w for n, w in in_torch_ops.items() if w}, "torch_ops.py calls the library itself; its operators go through ops.*_raw"
    twice = {name: sorted(where) for name, where in sites.items()
             if len(where) > 1 and not name.endswith("_workspace") and name not in ALLOWED_TWICE}
    assert not twice, "entry points marshalled by hand in more than one function:\n" + "\n".join(f"  {n}: {w}" for n, w in sorted(twice.items()))
