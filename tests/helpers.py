"""Shared test inputs for the network-half operators."""
import numpy as np


def cloud(rng, b, n, kind="uniform"):
    """Point clouds in [-1,1]^3.  kinds: uniform floats; grid = coordinates on a 2^-8 lattice (all
    squared-distance arithmetic exact in float32 -> every FMA-contraction pattern agrees, and exact
    distance ties are common); tiled = a small cloud repeated to n points (the reference loader
    tiles small clouds, lib/dataset.py:290-317 -> duplicated points)."""
    if kind == "uniform":
        return rng.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    if kind == "grid":
        return (rng.randint(-256, 257, (b, n, 3)) / 256.0).astype(np.float32)
    if kind == "coarse":   # very coarse lattice: massive ties
        return (rng.randint(-8, 9, (b, n, 3)) / 8.0).astype(np.float32)
    if kind == "tiled":
        base = rng.uniform(-1, 1, (b, max(1, n // 3), 3)).astype(np.float32)
        reps = -(-n // base.shape[1])
        return np.tile(base, (1, reps, 1))[:, :n].copy()
    raise ValueError(kind)


# ---- hand-built weights for the coupled (production) data-flow tests: the builder lives in the package so that bench.py
# --pose-inputs network can use it too
from articulated_pose_amd.synthetic import passthrough_pose_problem  # noqa: E402,F401


# ---- the reference's own operator code on the tests' seeded inputs, stored as digests (tests/golden/ref_ops.json, written by
# tests/golden/gen_ref_ops_golden.py from the reference sources compiled into oracle/_ref): a test holds an output to the reference
# bit for bit without the reference being present
def digest(a):
    """dtype, shape and SHA-256 of an array's bytes: equal digests <=> bit-equal arrays (integers compared as int64)."""
    import hashlib
    a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    a = np.ascontiguousarray(a.astype(np.int64) if a.dtype.kind in "iu" else a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


_REF_OPS = None


def ref_ops(key):
    """The stored digest of the reference's output for one test case (KeyError: the fixture lacks the case -- regenerate it)."""
    global _REF_OPS
    if _REF_OPS is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ops.json")) as f:
            _REF_OPS = json.load(f)
    return _REF_OPS[key]
