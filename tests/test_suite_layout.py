"""The layout of the suite itself (CPU, no GPU): a test module is nobody's library.  What two test modules share lives in a support
module (tests/util.py, gpu_support.py, live.py, checkers.py, the *_ref.py checkers), whose name does not start with test_ and which
defines no test.  tests/ has no __init__.py, so pytest imports tests/test_x.py as `test_x`, and `from tests import test_x` in another
module would load it a second time as `tests.test_x`: its module-level code runs twice, and a module-scoped fixture taken from it
is built once per importer."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def modules():
    return {os.path.basename(p)[:-3]: ast.parse(open(p).read(), p) for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def imported_test_modules(tree):
    """every test_* module an import statement of `tree` names, at any depth: import test_x, import tests.test_x,
    from test_x import y, from tests.test_x import y, from tests import test_x, from . import test_x"""
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names = [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names = [node.module or ""] + [f"{node.module or ''}.{a.name}" for a in node.names if (node.module or "") in ("", "tests")]
        else:
            continue
        found += [n for n in names if any(part.startswith("test_") for part in n.split("."))]
    return found


def test_no_test_module_imports_another():
    mods = modules()
    assert sum(1 for m in mods if m.startswith("test_")) > 50, sorted(mods)
    bad = {m: imported_test_modules(tree) for m, tree in mods.items() if imported_test_modules(tree)}
    assert not bad, f"test modules imported as libraries: {bad}"
    tests_in_support = {m: [n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test_")]
                        for m, tree in mods.items() if not m.startswith("test_")}
    assert not any(tests_in_support.values()), f"support modules that define tests: { {m: t for m, t in tests_in_support.items() if t} }"
