#!/usr/bin/env python
"""Generates the golden vectors of the fit quality (ancsh_fit_quality_rec) by IMPORTING the reference's own verifiers,
single_transformation_verifier and joint_transformation_verifier, from where they lie (gen_pose_golden.py's import_reference() shims are
reused by import).

Run in the build container only (it needs the reference tree):
    python tests/golden/gen_fit_quality_golden.py

The verifiers return a score and the inlier masks and drop the residual norms in between.  To store the reference's OWN norms, and not a
restatement of them, the imported module's `np` is replaced for the duration of a call by a pass-through that records what its `sqrt`
returns: the verifiers take exactly one square root per part, of the norm.

Problems (float32 source / target like the fit's packed rows, a random similarity as the model, noise of the order of inlier_th so that
both outcomes occur): single parts of 1, 2, 3, 64, 65, 257 and 1024 points, one part without an inlier and one with nothing else; joint
problems over pairs of them.  The generator asserts that no stored norm lies within 1e-9 of inlier_th: the condition under which the masks
do not depend on the implementation.

Writes (arrays only): fit_quality.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE), HERE]
sys.dont_write_bytecode = True

from gen_pose_golden import import_reference, rand_rot  # noqa: E402

TH = 0.1
CLEAR = 1e-9
SIZES = (1, 2, 3, 64, 65, 257, 1024)


class _Tap(object):
    """numpy, except that every sqrt result is kept."""

    def __init__(self):
        self.roots = []

    def __getattr__(self, name):
        return getattr(np, name)

    def sqrt(self, x):
        r = np.sqrt(x)
        self.roots.append(np.array(r, np.float64))
        return r


def make_part(rng, n, noise):
    """(source, target float32 (n, 3), model [R | s | t] float64 (13,)): target = s R source + t + noise * N(0, 1)."""
    R, s, t = rand_rot(rng), rng.uniform(0.6, 1.2), rng.uniform(-0.3, 0.3, 3)
    src = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    tgt = (s * src.astype(np.float64) @ R.T + t + noise * rng.randn(n, 3)).astype(np.float32)
    return src, tgt, np.concatenate([R.ravel(), [s], t])


def main():
    _, pose, _ = import_reference()
    rng = np.random.RandomState(20261018)
    out = dict(th=np.float64(TH))
    # noise 0.06: |N(0, 0.06^2 I_3)| has its median at 0.092, so about half the points fall on either side of 0.1
    parts = [make_part(rng, n, 0.06) for n in SIZES]
    far = make_part(rng, 65, 0.01)
    far[2][10:13] += 0.5                                          # no inlier: the model's translation is off by 0.87
    parts += [far, make_part(rng, 64, 1e-3)]                      # ... and all inliers
    tap = _Tap()
    real_np = pose.np
    pose.np = tap
    try:
        for i, (src, tgt, m) in enumerate(parts):
            del tap.roots[:]
            score, inl = pose.single_transformation_verifier(dict(source=src, target=tgt, nsource=len(src), ntarget=len(tgt)),
                                                             dict(rotation=m[:9].reshape(3, 3), scale=m[9], translation=m[10:13]), TH)
            assert len(tap.roots) == 1 and tap.roots[0].shape == (len(src),)
            out.update({"s%d_source" % i: src, "s%d_target" % i: tgt, "s%d_model" % i: m, "s%d_norms" % i: tap.roots[0],
                        "s%d_inliers" % i: np.asarray(inl), "s%d_score" % i: np.asarray(score)})
        pairs = [(6, 5), (3, 4), (2, 1), (0, 0), (7, 8), (8, 6)]          # (part 0, part j) of `parts`
        for i, (a, b) in enumerate(pairs):
            (s0, t0, m0), (s1, t1, m1) = parts[a], parts[b]
            del tap.roots[:]
            score, inl = pose.joint_transformation_verifier(
                dict(source0=s0, target0=t0, nsource0=len(s0), source1=s1, target1=t1, nsource1=len(s1)),
                dict(rotation0=m0[:9].reshape(3, 3), scale0=m0[9], translation0=m0[10:13],
                     rotation1=m1[:9].reshape(3, 3), scale1=m1[9], translation1=m1[10:13]), TH)
            assert len(tap.roots) == 2
            out.update({"j%d_parts" % i: np.asarray([a, b]), "j%d_norms0" % i: tap.roots[0], "j%d_norms1" % i: tap.roots[1],
                        "j%d_inliers0" % i: np.asarray(inl[0]), "j%d_inliers1" % i: np.asarray(inl[1]), "j%d_score" % i: np.asarray(score)})
    finally:
        pose.np = real_np
    out["n_single"], out["n_joint"] = np.asarray(len(parts)), np.asarray(len(pairs))
    norms = np.concatenate([v for k, v in out.items() if "_norms" in k])
    assert np.abs(norms - TH).min() > CLEAR, np.abs(norms - TH).min()
    counts = [int(out["s%d_inliers" % i].sum()) for i in range(len(parts))]
    assert counts[7] == 0 and counts[8] == 64 and any(0 < c < n for c, n in zip(counts, SIZES))
    path = os.path.join(HERE, "fit_quality.npz")
    np.savez_compressed(path, **out)
    print("fit_quality.npz", os.path.getsize(path), "inliers per part", counts, "closest norm to th", np.abs(norms - TH).min())


if __name__ == "__main__":
    main()
