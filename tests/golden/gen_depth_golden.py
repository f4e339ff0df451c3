"""Generator of tests/golden/depth_unproject.npz -- BUILD CONTAINER ONLY (needs the reference checkout).

The depth-to-cloud rule of tools/preprocess_data.py is part of a method body: lines 271-276 build the projected maps of a 512 x 512 frame
and lines 288-296 (inside the loop over parts) index them with one part's pixels and back-project those through projMat into
cloud_cam_real.  This generator EXECUTES THOSE LINES AS THEY LIE in the reference file -- read at run time, dedented, exec'd in a namespace
that holds what the preceding lines would have set (the pixel maps of :167-168, a synthetic float depth image, projMat, and a single
"part" whose choose_x / choose_y are np.where of the object mask, as :263 and :283-284 make them).  Nothing of the reference is written to
disk; the .npz holds the mask pixels' (row, col, depth), the matrices and the reference's float64 cloud_cam_real only.  Guards check that
both ranges still start and end on the expected statements.

    python tests/golden/gen_depth_golden.py        # rewrites tests/golden/depth_unproject.npz
"""
import os
import textwrap

import numpy as np

REF = os.environ.get("ANCSH_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
MAPS, CLOUD = (271, 276), (288, 296)


def reference_blocks():
    lines = open(os.path.join(REF, "tools", "preprocess_data.py")).read().splitlines()

    def block(first, last, head, tail):
        assert lines[first - 1].strip().startswith(head), lines[first - 1]
        assert lines[last - 1].strip().startswith(tail), lines[last - 1]
        return compile(textwrap.dedent("\n".join(lines[first - 1:last])), "preprocess_data.py:%d-%d" % (first, last), "exec")
    return (block(MAPS[0], MAPS[1], "u_map     = ymap * 2 / w -1", "projected_map1 = np.stack("),
            block(CLOUD[0], CLOUD[1], "projected_points = projected_map[", "cloud_cam_real    = np.concatenate("))


def perspective(fov_deg, aspect, near, far):
    """The matrix PyBullet's computeProjectionMatrixFOV returns, in the `.reshape(4, 4).T` form of :229 (symmetric frustum)."""
    f = 1.0 / np.tan(np.radians(fov_deg) / 2.0)
    return np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)],
                     [0, 0, -1, 0]], np.float64)


def general():
    """Off-centre principal point (P02, P12 != 0) and a non-diagonal upper 2 x 2: all six coefficients are exercised."""
    P = perspective(50.0, 1.2, 0.1, 50.0)
    P[0, 1], P[1, 0] = 0.05, -0.03
    P[0, 2], P[1, 2] = 0.13, -0.07
    return P


def main():
    maps, cloud = reference_blocks()
    rng = np.random.RandomState(7)
    H = W = 512
    rr, cc = np.mgrid[0:H, 0:W]
    depth = (1.5 + 0.4 * np.sin(rr / 37.0) * np.cos(cc / 53.0) + 0.05 * rng.rand(H, W)).astype(np.float32)
    # the object: an off-centre ellipse that reaches the image corner region, thinned to a few thousand pixels
    obj = (((rr - 300) / 170.0) ** 2 + ((cc - 210) / 120.0) ** 2 < 1.0) & (rng.rand(H, W) < 0.06)
    obj[0, 0] = obj[511, 511] = obj[0, 511] = obj[511, 0] = obj[256, 256] = True
    out = dict(height=np.int64(H), width=np.int64(W))
    rows, cols = np.where(obj)
    out["row"], out["col"], out["depth"] = rows.astype(np.int32), cols.astype(np.int32), depth[rows, cols]
    for tag, P in (("pybullet", perspective(35.0, 1.0, 0.1, 100.0)), ("general", general())):
        ns = dict(np=np, ymap=np.array([[i for i in range(W)] for j in range(H)]), xmap=np.array([[j for i in range(W)] for j in range(H)]),
                  h=H, w=W, depth=depth, projMat=P, s=0)
        exec(maps, ns)
        ns["choose_x"], ns["choose_y"] = {0: rows}, {0: cols}
        exec(cloud, ns)
        got = np.asarray(ns["cloud_cam_real"], np.float64)
        assert got.shape == (len(rows), 3), got.shape
        out["projMat_" + tag], out["cloud_cam_real_" + tag] = P, got
        print(tag, got.shape, "x range", got[:, 0].min(), got[:, 0].max())
    np.savez_compressed(os.path.join(HERE, "depth_unproject.npz"), **out)


if __name__ == "__main__":
    main()
