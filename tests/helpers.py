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


# ---- the streamed record's layout on a prepared pipeline (the GPU stream tests)
def check_record_layout(pipe, names=None):
    """A prepared streaming AncshPipeline: in every slot the tensor the record output copies is out[layout.key], layout.width columns wide,
    every block's carried record is the out[...] entry of that width, and (names) the blocks are these.  -> the layout."""
    L = pipe.record_layout
    assert names is None or L.names == tuple(names), L
    for sl in pipe.slots:
        for f32 in (False, True) if sl.out32 is not None else (False,):
            out = sl.pick("out", f32)
            src = sl.outputs["record"].source(sl, f32)[0]
            assert src is out[L.key] and src.shape[2] == L.width == sl.record_width == len(L.columns), L
            assert out["record"].shape[2] == L.span("pose").stop == 26
            for name in L.names[1:]:
                key, width = L.carried(name)
                assert out[key].shape[2] == width == L.span(name).start, (name, key, width)
    return L
