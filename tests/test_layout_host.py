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


# The package has the same rule for its own files: api.py is the list of names, the code lives in one module per subsystem
# (the cut of csrc/api_*.hip), and those modules import one another in one direction only.
SUBSYSTEM_MODULES = ["_abi", "records", "context", "scan", "queries", "global_map", "store", "device_map", "registration", "mapping"]


def _package_trees():
    files = sorted(glob.glob(os.path.join(ROOT, "warpsense_amd", "*.py")))
    trees = {}
    for path in files:
        with open(path) as f:
            trees[os.path.splitext(os.path.basename(path))[0]] = ast.parse(f.read(), path)
    assert set(SUBSYSTEM_MODULES + ["api", "app", "_lib"]) <= set(trees), sorted(trees)
    return trees


def _relative_imports(node, modules):
    """the modules of the package that one import statement names: `from .m import x`, `from . import m`"""
    if not isinstance(node, ast.ImportFrom) or node.level != 1:
        return []
    if node.module:
        return [node.module.split(".")[0]]
    return [a.name for a in node.names if a.name in modules]


def test_package_modules_are_layered():
    trees = _package_trees()
    top, inner = {}, []
    for name, tree in trees.items():
        top[name] = set()
        at_top = set()
        for node in tree.body:
            at_top.add(node)
            top[name].update(_relative_imports(node, trees))
        for node in ast.walk(tree):
            if node not in at_top:
                inner += [(name, m) for m in _relative_imports(node, trees)]
    # no cycle: every module can be numbered after all it imports
    done = set()
    while len(done) < len(top):
        ready = sorted(n for n in top if n not in done and top[n] - {n} <= done)
        assert ready, "import cycle among " + ", ".join(sorted(set(top) - done))
        done.update(ready)
    for name in SUBSYSTEM_MODULES:
        assert not top[name] & {"api", "app"}, (name, sorted(top[name]))
    # an import inside a function is how a cycle gets hidden: only the OS1-128 table and dist's WsError are taken that way
    assert sorted(set(inner)) == [("dist", "_lib"), ("mapping", "synthetic")], inner


API_NAMES = ["Context", "DeviceGlobalMap", "DeviceMap", "DeviceMapMemWrapper", "DevicePoints", "GlobalMap", "LocalMap", "MATRIX_RESOLUTION",
             "MapParams", "Params", "RAY", "RegistrationCuda", "RegistrationParams", "SAMPLE", "SAMPLE_CLASSES", "SURFACE_RECORD",
             "ScanPreprocessor", "TSDFCuda", "TSDFMapping", "TSDFRegistration", "VERT", "WEIGHT_RESOLUTION", "WS_INTEGRATE_DENSE",
             "WS_INTEGRATE_SPARSE", "WS_MAP_AVG", "WS_MAP_NEW", "WS_REG_ALL_POINTS", "WS_REG_COMPAT_REFERENCE_LAUNCH", "WsError", "annotations",
             "batch_best", "candidate_poses", "check", "chunks_of_box", "cleanup", "distance_class", "distance_d2", "distance_mm", "pack_entry",
             "pause", "pose_to_values", "preprocess_sweep_host", "sweep_bins", "sweep_poses", "to_int_mat", "to_map", "unpack_entry",
             "write_mesh_ply", "write_raycast_ply", "write_surface_ply"]


def test_api_facade_keeps_its_names():
    """API_NAMES is dir(warpsense_amd.api) without underscore names as it was while api.py held all the code (less the modules it had
    imported: C, np, threading, _lib); `annotations` is the __future__ import's and is in the list because it was."""
    import warpsense_amd
    import warpsense_amd.api
    missing = [n for n in API_NAMES if not hasattr(warpsense_amd.api, n)]
    assert not missing, missing
    taken = []
    for node in _package_trees()["__init__"].body:
        if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module == "api":
            taken += [a.name for a in node.names]
    assert len(taken) > 35 and set(taken) <= set(API_NAMES), taken
    other = [n for n in taken if getattr(warpsense_amd, n) is not getattr(warpsense_amd.api, n)]
    assert not other, other


def test_no_module_is_a_grab_bag():
    trees = _package_trees()
    for name in trees:
        if name in ("_lib", "dist", "synthetic"):
            continue
        with open(os.path.join(ROOT, "warpsense_amd", name + ".py")) as f:
            lines = len(f.read().splitlines())
        assert lines <= 500, (name, lines)
    defs = [node.name for node in ast.walk(trees["api"]) if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))]
    assert not defs, defs
