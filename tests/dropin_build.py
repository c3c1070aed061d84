"""The build of a C++ drop-in program of tests/cpp/: one g++ line against include/ and the built library, for every test that runs
such a program next to the Python route.  No cache: every caller builds into a directory of its own (its tmp_path, or a module's
tmp_path_factory directory)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dropin(name, directory):
    """compile tests/cpp/<name>.cpp into directory / name (a pathlib.Path) and return that path"""
    cxx = shutil.which("g++")
    assert cxx is not None, "the C++ drop-in needs g++"
    exe = directory / name
    lib = os.path.join(ROOT, "warpsense_amd")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cpp", f"{name}.cpp"), "-o", str(exe), f"-L{lib}", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-lwarpsense_hip", "-lpthread"])
    return exe
