"""TEST INFRASTRUCTURE: the one g++ recipe of the x86 probes the tests build for themselves (tests/emu/<name>.cpp), the process-wide
cache that builds each of them once (shared), and the ctypes pointer helpers of their callers (ptr, desc_ptrs).  The flags are
the Makefile's own CXXFLAGS, asked for with `make flags`, -mfma detection included."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
_PACK = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "micro_raytracer_amd", "csrc", "mrt_pack.cpp")
_CACHE = {}          # (name, build arguments) -> the bound CDLL
_DIR = []            # the one temporary directory of this process's probes
BUILDS = []          # every name build_probe compiled in this process, in order


def build_probe(name, out_dir, with_pack=True, pthread=True):
    """tests/emu/<name>.cpp (with the host packer: with_pack) as <out_dir>/lib<name>.so, loaded with ctypes; None without g++."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    flags = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", _HERE, "flags"], text=True).split()
    out = os.path.join(str(out_dir), f"lib{name}.so")
    subprocess.check_call([cxx, *flags, "-shared", "-o", out, os.path.join(_HERE, name + ".cpp"), *([_PACK] if with_pack else []),
                           *(["-lpthread"] if pthread else [])])
    BUILDS.append(name)
    return C.CDLL(out)


def shared(name, bind=None, **kw):
    """The probe `name` of this process: built once (build_probe's arguments in kw) into a temporary directory that goes at exit,
    bind(L) called once to set argtypes and restype, the same CDLL from then on.  Skips the test where there is no g++."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        if not _DIR:
            _DIR.append(tempfile.mkdtemp(prefix="mrt_probes_"))
            atexit.register(shutil.rmtree, _DIR[0], ignore_errors=True)
        L = build_probe(name, tempfile.mkdtemp(dir=_DIR[0]), **kw)          # a directory per key: no build overwrites a loaded library
        if L is None:
            import pytest
            pytest.skip("no g++")
        if bind:
            bind(L)
        _CACHE[key] = L
    return _CACHE[key]


def ptr(a, t=C.c_float):
    """A numpy array as a ctypes pointer to t"""
    return a.ctypes.data_as(C.POINTER(t))


def desc_ptrs(holder, with_ext=True):
    """(render-desc pointer, ext pointer or None) of an _abi.build_desc holder, as every probe takes them"""
    return C.cast(holder.ptr(), C.c_void_p), (holder.ext_ptr() if with_ext else None)
