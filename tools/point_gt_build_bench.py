"""ancsh_point_gt_build alone at the streaming shape (32 clouds x 3000 rows, K = 3, two revolute joints on part 0): microseconds a launch
with its operands in the Infinity Cache (one operand set, launched back to back) and beyond it (enough operand sets in rotation to
exceed 256 MiB), next to bench.py's float4-copy HBM yardstick for the same 100 bytes a row (28 read + 72 written).  Prints one JSON line.

    python tools/point_gt_build_bench.py [--clouds 32] [--rows 3000] [--reps 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import articulated_pose_amd  # noqa: E402,F401
import bench  # noqa: E402
from articulated_pose_amd.dataset import RIG_WIDTH, pack_joint_rig, point_gt_build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    K, B, n, dev = 3, args.clouds, args.rows, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    corners = np.array([[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]]] + [[[-0.3, -0.3, -0.3], [0.3, 0.3, 0.3]]] * K)
    factors = 1.0 / np.linalg.norm(corners[:, 1] - corners[:, 0], axis=1)
    joints = {"link": {"xyz": [[0, 0, 0], [0.05, 0, 0], [0, -0.05, 0.1]]}, "joint": {"axis": [[0, 0, 0], [1.0, 0.05, 0], [0, 0.1, 1.0]], "parent": [-1, 0, 0]}}
    rig = torch.from_numpy(np.tile(pack_joint_rig(corners, factors, joints, [[j] for j in range(K)])[0], (B, 1))).to(dev)
    assert rig.shape[1] == RIG_WIDTH(K)
    cap = B * n
    host = np.concatenate([rs.uniform(-1, 1, (cap, 3)), rs.uniform(-0.3, 0.3, (cap, 3)), np.sort(rs.randint(0, K, (B, n)), axis=1).reshape(cap, 1)], 1)
    off = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
    row_bytes = 100
    sets_beyond = (3 * (256 << 20)) // (cap * row_bytes) + 1          # three times the Infinity Cache
    out = {}
    for label, sets in (("in_cache", 1), ("beyond_cache", sets_beyond)):
        src = [torch.from_numpy(host.astype(np.float32)).to(dev) for _ in range(sets)]
        rows = [torch.empty((cap, 18), dtype=torch.float32, device=dev) for _ in range(sets)]
        for s in range(min(sets, 8)):
            point_gt_build(src[s], off, rig, K, rows[s])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(args.reps):
            point_gt_build(src[r % sets], off, rig, K, rows[r % sets])
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / args.reps
        out[label] = {"operand_sets": sets, "us_per_launch": round(us, 2), "GBps": round(cap * row_bytes / us / 1e3, 1)}
        del src, rows
    copy = bench.measured_hbm_copy(dev)
    out["hbm_copy_measured_GBps"] = copy
    out["frac_of_measured_copy_beyond_cache"] = round(out["beyond_cache"]["GBps"] / copy, 3)
    print(json.dumps(dict(metric="ancsh_point_gt_build alone, back-to-back launches timed with HIP events (launch overhead included)",
                          shape={"K": K, "clouds": B, "rows_per_cloud": n, "bytes_per_row": row_bytes, "reps": args.reps}, **out)))


if __name__ == "__main__":
    main()
