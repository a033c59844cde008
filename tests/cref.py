"""Builds one of the plain-C restatements under tests/ (homography_ref.c, homography_refine_ref.c, affine_ref.c) with
the host C compiler into a temporary directory and loads it with ctypes; each *_ref.py loader does this once, on first
use, with its own table of signatures."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
_tmps = []          # the build directories live as long as the process (the libraries stay mapped)


def load(name, argtypes, restypes=None):
    """Compiles tests/<name>.c and returns the CDLL, its functions typed by the two tables (function name -> argtypes,
    function name -> restype; ctypes' int where none is given)."""
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    tmp = tempfile.TemporaryDirectory(prefix=name + "_")
    _tmps.append(tmp)
    so = os.path.join(tmp.name, "lib%s.so" % name)
    r = subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, name + ".c"),
                        "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    for fn, types in argtypes.items():
        getattr(L, fn).argtypes = types
    for fn, restype in (restypes or {}).items():
        getattr(L, fn).restype = restype
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
