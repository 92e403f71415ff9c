"""ctypes binding of tests/cpp/update_ref_ld.cpp: update_ref.update_core in compiled `long double` (and in `double`: the fp64 loop
restatement of the large cases) -- TEST INFRASTRUCTURE ONLY.  The library is built on first use with g++ -O2 -fopenmp into a
temporary directory; np.longdouble arrays pass through untouched (asserted at load time: 64-bit mantissa, 16 bytes, same layout).
Threads: OMP_NUM_THREADS, capped at 16 (4 where it is not set); the bits do not depend on it (see the .cpp)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import update_ref as ur

LD = np.longdouble
_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "cpp", "update_ref_ld.cpp")
CXXFLAGS = ["-std=c++17", "-O2", "-fopenmp", "-ffp-contract=off", "-shared", "-fPIC"]
_lib = None


def threads_from_env():
    try:
        t = int(os.environ.get("OMP_NUM_THREADS", "4").split(",")[0])
    except ValueError:
        t = 4
    return max(1, min(16, t))


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="update_ref_ld_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libupdate_ref_ld.so")
        subprocess.check_call(["g++", *CXXFLAGS, "-o", so, SOURCE])
        L = C.CDLL(so)
        assert L.urld_mant_dig() == 64, "long double is not the x87 extended type"
        assert np.finfo(LD).nmant == 63 and np.dtype(LD).itemsize == L.urld_sizeof_long_double() == 16
        third = np.zeros(1, LD)
        L.urld_third(third.ctypes.data_as(C.c_void_p))
        assert third[0] == LD(1) / LD(3) and third.tobytes()[:10] == (LD(1) / LD(3)).tobytes()[:10], "np.longdouble has another layout"
        vp, i32 = C.c_void_p, C.c_int
        for f in (L.urld_update_core_ld, L.urld_update_core_f64):
            f.restype = i32
            f.argtypes = [i32, i32] + [vp] * 14 + [i32]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update_arith(P, rows, residual, R, dtype=LD, threads=None):
    """A, S, L, W, B, z, dx, P6 of update_core in `dtype` (np.longdouble or np.float64) -> dict of arrays of that type"""
    L = lib()
    P64 = np.ascontiguousarray(P, dtype=np.float64)
    n = len(P64)
    row_start, col, val = (np.ascontiguousarray(rows[0], dtype=np.int32), np.ascontiguousarray(rows[1], dtype=np.int32),
                           np.ascontiguousarray(rows[2], dtype=np.float64))
    m = len(row_start) - 1
    assert row_start[0] == 0 and row_start[-1] == len(col) == len(val) and np.all(np.diff(row_start) >= 0)
    assert len(col) == 0 or (col.min() >= 0 and col.max() < n)
    res = np.ascontiguousarray(np.atleast_1d(residual), dtype=np.float64)
    R64 = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(m, m))
    assert len(res) == m
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(LD), np.dtype(np.float64))
    out = {"A": np.zeros((m, n), dtype), "S": np.zeros((m, m), dtype), "L": np.zeros((m, m), dtype), "W": np.zeros((m, m), dtype),
           "B": np.zeros((m, n), dtype), "z": np.zeros(m, dtype), "dx": np.zeros(n, dtype), "P6": np.zeros((n, n), dtype)}
    f = L.urld_update_core_ld if dtype == np.dtype(LD) else L.urld_update_core_f64
    rc = f(n, m, _p(P64), _p(row_start), _p(col), _p(val), _p(res), _p(R64), *(_p(out[k]) for k in ("A", "S", "L", "W", "B", "z", "dx", "P6")),
           threads_from_env() if threads is None else int(threads))
    assert rc == 0, f"pivot {rc - 1} of S is not positive"
    return out


def update_core(x13, feature_pos, P, rows, residual, R, threads=None):
    """update_ref.update_core with the arithmetic compiled: the same keys, so that update_ref.with_bounds is used unchanged"""
    a = update_arith(P, rows, residual, R, LD, threads)
    return ur.core_of(x13, feature_pos, P, a["A"], a["S"], a["L"], a["W"], a["B"], a["z"], a["dx"], a["P6"])
