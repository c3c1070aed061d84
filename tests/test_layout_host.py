"""The layout of the test tree: what more than one file uses lives in a helper module (query_model.py, *_model.py, *_scenes.py,
*_routes.py, scan_clouds.py, dropin_build.py beside window_model.py, reg_cases.py and oracle_lib.py), never in a test module.  A
model inside a test_*.py is an oracle that an edit to that file's own tests can change for every file that borrowed it."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_file_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(files) > 60, files
    found = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
                names = [node.module]
            for name in names:
                if any(part.startswith("test_") for part in name.split(".")):
                    found.append(f"{os.path.relpath(path, ROOT)}:{node.lineno}: imports {name}")
    assert not found, "\n".join(found)
