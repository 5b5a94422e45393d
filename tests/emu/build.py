"""TEST INFRASTRUCTURE: the one g++ recipe of the x86 probes the tests build for themselves (tests/emu/<name>.cpp).  The flags are
the Makefile's own CXXFLAGS, asked for with `make flags`, -mfma detection included."""
import ctypes as C
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_PACK = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "micro_raytracer_amd", "csrc", "mrt_pack.cpp")


def build_probe(name, out_dir, with_pack=True, pthread=True):
    """tests/emu/<name>.cpp (with the host packer: with_pack) as <out_dir>/lib<name>.so, loaded with ctypes; None without g++."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    flags = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", _HERE, "flags"], text=True).split()
    out = os.path.join(str(out_dir), f"lib{name}.so")
    subprocess.check_call([cxx, *flags, "-shared", "-o", out, os.path.join(_HERE, name + ".cpp"), *([_PACK] if with_pack else []),
                           *(["-lpthread"] if pthread else [])])
    return C.CDLL(out)


def probe_or_skip(name, out_dir, **kw):
    """build_probe for a test: skips where there is no g++."""
    import pytest
    return build_probe(name, out_dir, **kw) or pytest.skip("no g++")
