"""The suite's one layering rule: no module under tests/ or tools/ imports a test module.  What tests share lives in the plain modules
beside them (helpers.py, parity.py, kernel_leaves.py, leaf_states.py, mode_walk.py, policy_checks.py, ...)."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _test_modules_imported(node, test_modules):
    """The test modules an import statement names: `import test_x`, `from test_x import y`, `from tests import test_x`."""
    if isinstance(node, ast.Import):
        return [a.name for a in node.names if any(p.startswith("test_") for p in a.name.split("."))]
    if isinstance(node, ast.ImportFrom):
        base = node.module or ""
        if any(p.startswith("test_") for p in base.split(".")):
            return [base]
        return [f"{base}.{a.name}" for a in node.names if a.name in test_modules]
    return []


def test_no_module_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True))
    test_modules = {os.path.basename(f)[:-3] for f in files if os.path.basename(f).startswith("test_")}
    assert len(files) > 50 and len(test_modules) > 30
    found = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            found += [f"{os.path.relpath(path, ROOT)}:{node.lineno}: {name}" for name in _test_modules_imported(node, test_modules)]
    assert not found, "\n".join(found)
