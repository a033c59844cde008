"""Builds one of the plain-C restatements under tests/ (homography_ref.c, homography_refine_ref.c, affine_ref.c), or a C++
shim over a host-only header of the library (knn_l2_plan_shim.cpp), with
the host compiler into a temporary directory and loads it with ctypes; each *_ref.py loader does this once, on first
use, with its own table of signatures."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
_tmps = []          # the build directories live as long as the process (the libraries stay mapped)


def load(name, argtypes, restypes=None, include=()):
    """Compiles tests/<name>.c (or, where there is none, tests/<name>.cpp as C++17 with the `include` directories) and
    returns the CDLL, its functions typed by the two tables (function name -> argtypes, function name -> restype;
    ctypes' int where none is given)."""
    src = os.path.join(HERE, name + ".c")
    if os.path.exists(src):
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        std = []
    else:
        src += "pp"
        cc = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
        std = ["-std=c++17"]
    assert cc, "no host compiler"
    tmp = tempfile.TemporaryDirectory(prefix=name + "_")
    _tmps.append(tmp)
    so = os.path.join(tmp.name, "lib%s.so" % name)
    r = subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC"] + std + ["-I" + d for d in include] +
                       ["-o", so, src, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    for fn, types in argtypes.items():
        getattr(L, fn).argtypes = types
    for fn, restype in (restypes or {}).items():
        getattr(L, fn).restype = restype
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
