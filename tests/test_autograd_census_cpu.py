"""Census of the autograd nodes: every torch.autograd.Function defined in future_od/native/functional.py and
future_od/native/backbone.py has an entry in tests/autograd_node_cases.py -- its float64 cases in
tests/test_autograd_nodes_gpu.py, or the test that already compares its gradients with torch.  A node added without one
fails here.  The sources are parsed, not imported: no library is loaded."""
import ast
import os

import autograd_node_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "future-object-detection_amd", "future_od", "native", f) for f in ("functional.py", "backbone.py")]


def _parse(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def _is_function_base(node):
    """`Function`, `autograd.Function`, `torch.autograd.Function`"""
    if isinstance(node, ast.Name):
        return node.id == "Function"
    return isinstance(node, ast.Attribute) and node.attr == "Function"


def function_classes_of(tree):
    return {n.name for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and any(_is_function_base(b) for b in n.bases)}


def function_classes(paths=SOURCES):
    return {name for p in paths for name in function_classes_of(_parse(p))}


def _functions(path):
    return {n.name for n in ast.walk(_parse(path)) if isinstance(n, ast.FunctionDef)}


def _classes(path):
    return {n.name for n in ast.walk(_parse(path)) if isinstance(n, ast.ClassDef)}


def test_every_autograd_node_has_an_entry():
    found = function_classes()
    assert len(found) >= 24 and {"LinearFn", "BackboneFn"} <= found, found       # (the parser still finds them)
    assert found == set(NC.NODES), f"without an entry: {sorted(found - set(NC.NODES))}; no such node: {sorted(set(NC.NODES) - found)}"


def test_the_census_finds_a_node_however_its_base_is_written():
    """A source with one more node than the table knows, in each spelling of the base class: all are found (so the set
    comparison above fails for it), a class of another base is not."""
    src = ("import torch\nfrom torch.autograd import Function\nfrom torch import autograd\n"
           "class LinearFn(Function): pass\n"
           "class NewFn(torch.autograd.Function): pass\n"
           "class OtherFn(autograd.Function): pass\n"
           "def f():\n    class _InnerFn(Function): pass\n"
           "class Holder(torch.nn.Module): pass\nclass Plain: pass\n")
    found = function_classes_of(ast.parse(src))
    assert found == {"LinearFn", "NewFn", "OtherFn", "_InnerFn"}
    assert found - set(NC.NODES) == {"NewFn", "OtherFn", "_InnerFn"}


def test_every_entry_names_cases_or_a_test_that_exists():
    defined = _classes(os.path.join(ROOT, "tests", "test_autograd_nodes_gpu.py"))
    used = set()
    for node, entry in NC.NODES.items():
        if isinstance(entry, NC.CoveredElsewhere):
            continue
        assert isinstance(entry, list) and entry, node
        for name in entry:
            assert name in NC.CASES, (node, name)
            assert name in defined, f"{node}: no case class {name} in tests/test_autograd_nodes_gpu.py"
            used.add(name)
    assert used == set(NC.CASES), f"cases of no node: {sorted(set(NC.CASES) - used)}"


def test_every_test_cited_exists():
    targets = [e.target for e in NC.NODES.values() if isinstance(e, NC.CoveredElsewhere)] + list(NC.ALSO_COVERED)
    assert targets
    for target in targets:
        path, _, name = target.partition("::")
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), target
        assert name in _functions(full), target
