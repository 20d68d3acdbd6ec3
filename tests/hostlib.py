"""The one g++ line of the test-suite: a C++ source (a wrapper around a csrc/*_math.hpp serial restatement) built into a shared
library at test time, once per process."""
import ctypes
import functools
import os
import subprocess
import tempfile


@functools.lru_cache(maxsize=None)
def build(tag, source):
    """g++ -O2 -std=c++17 -ffp-contract=off build of `source` -> ctypes.CDLL (the caller sets argtypes / restype)"""
    d = tempfile.mkdtemp(prefix=f"danbo_{tag}_")
    src, so = os.path.join(d, tag + ".cpp"), os.path.join(d, f"lib{tag}.so")
    with open(src, "w") as f:
        f.write(source)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)
