"""ctypes front-end of the pose-math probe (oracle/pose_math_probe.hip): the closed-form device functions of the product header
csrc/pose_math.h, callable with chosen float64 arguments.

TEST INFRASTRUCTURE ONLY.  Imported by tests/test_pose_math_gpu.py; never by the product package, which cannot reach the library.
Every function takes an (n, NI) float64 array of cases and returns the (n, NO) float64 results computed on the GPU.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libancsh_pose_probe.so")
_lib = None

# name -> (doubles in, doubles out) per case
ENTRIES = {
    "horn_quat": (9, 4), "horn_quat_fast": (9, 4),                      # M (row-major, M[a][b] = sum tgt_a src_b) -> (w, x, y, z)
    "quat_to_mat": (4, 9), "quat_to_rotvec": (4, 3), "rotvec_to_mat": (3, 9),
    "rodrigues": (6, 3),                                                # rotation vector, point -> rod_apply(rod_prepare(rv), p)
    "sincos": (1, 2),                                                   # x -> sin, cos (sincos_compact)
    "rcp": (1, 1), "rsqrt": (1, 1),
    "chol_solve": (28, 7),                                              # A (21 packed lower), par, b (6) -> x (6), ok
    "lmpar": (28, 7),                                                   # A (21 packed lower), g (6), delta -> par, z (6)
}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(f"{_SO} is missing: build it with `make -C oracle probe` (or __graft_entry__.build()); "
                               "the pose-math tests do not run without it")
        L = ctypes.CDLL(_SO)
        for name in ENTRIES:
            fn = getattr(L, "ancsh_probe_" + name)
            fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            fn.restype = ctypes.c_int
        _lib = L
    return _lib


def call(name, cases):
    ni, no = ENTRIES[name]
    a = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, ni)
    out = np.full((len(a), no), np.nan)
    rc = getattr(lib(), "ancsh_probe_" + name)(len(a), a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError(f"ancsh_probe_{name}: HIP error {rc}")
    return out
