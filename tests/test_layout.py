"""No module under tests/ imports a test module: what test files share lives in tests/mirrors.py (the yardsticks), tests/cases.py (inputs and
small drivers) and tests/support.py (generic helpers).  Source text only; it names no test module itself."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_module_imports_a_test_module():
    found = []
    for path in sorted(glob.glob(os.path.join(HERE, "**", "*.py"), recursive=True)):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = []
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                names = [a.name for a in node.names] + [getattr(node, "module", None) or ""]
            found += ["%s:%d imports %s" % (os.path.relpath(path, HERE), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not found, "test modules are not imported from; move what is shared to mirrors.py, cases.py or support.py:\n" + "\n".join(found)
