#!/usr/bin/env python3
"""Record how the reference's run / eval scripts use this package, as data: tests/golden/reference_surface.json.

    python tests/golden/make_surface.py <reference checkout>

The scripts are only PARSED (ast).  Per script the fixture lists what tests/test_reference_surface_cpu.py checks
against the package: the names imported from `future_od`, `runs` and `config`, the attributes read from those names,
and, for every call of one of them, the keyword names and the number of positional arguments.  Names and counts
only; no source text is kept.
"""
import ast
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OURS = ("future_od", "runs", "config")


def surface(source):
    tree = ast.parse(source)
    imports, bound = [], set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in OURS:
            for a in node.names:
                imports.append({"from": node.module, "name": a.name, "as": a.asname})
                bound.add(a.asname or a.name)
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.split(".")[0] in OURS:
                    imports.append({"import": a.name, "as": a.asname})
                    bound.add(a.asname or a.name.split(".")[0])
    attrs, calls = [], []
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in bound:
            attrs.append([node.value.id, node.attr])
        if isinstance(node, ast.Call):
            if isinstance(node.func, ast.Name) and node.func.id in bound:
                func = [node.func.id]
            elif (isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name)
                  and node.func.value.id in bound):
                func = [node.func.value.id, node.func.attr]
            else:
                continue
            calls.append({"func": func, "keywords": [kw.arg for kw in node.keywords if kw.arg is not None],
                          "positional": len(node.args)})
    return {"imports": imports, "attributes": attrs, "calls": calls}


def main(ref):
    scripts = sorted(p for p in glob.glob(os.path.join(ref, "runs", "*.py")) + glob.glob(os.path.join(ref, "runs", "eval", "*.py"))
                     if not os.path.basename(p).startswith("_"))
    assert scripts, f"no run scripts under {ref}"
    out = {}
    for p in scripts:
        with open(p) as f:
            out[os.path.relpath(p, ref)] = surface(f.read())
    with open(os.path.join(HERE, "reference_surface.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} scripts -> reference_surface.json")


if __name__ == "__main__":
    main(sys.argv[1])
