"""Step time of annotated depth frames (AncshPipeline(depth_capacity=..., point_ground_truth=True, build_point_gt=True): uint16 depth crops,
link-label crops and one scene table per frame in; the annotation -- ancsh_depth_annotate_stream -- runs inside the captured step) against
the xyz build_point_gt stream fed the same frames' annotated clouds from host memory, at equal frames and configs[2]'s shape (K = 3,
32 x 1024, 10000 / 200 hypotheses, couple=True, synthetic weights, predicted joints).  Two legs, alternated in one process for --rounds
rounds:
  f: the annotated depth stream (3 bytes per pixel and 1920 bytes of scene per frame cross to the device);
  g: the xyz build_point_gt stream on the 7-column clouds the operator made of the same frames BEFORE the clock starts (28 bytes per row;
     the reference's preprocessing that would make them on the host is not in the timed loop: the best case without the new entry).
Prints one JSON line: a record, not a gate.

    python tools/depth_annotate_bench.py [--rounds 3] [--passes 4] [--slots 8] [--clouds 320]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_stream_bench import SCALE, SIDE, POINTS, make_frame  # noqa: E402  (puts the repository root on sys.path)
from articulated_pose_amd import depth as D  # noqa: E402
from articulated_pose_amd.dataset import identity_rig  # noqa: E402
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.synthetic import make_cloud  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402


def annotate(frame, focal, K):
    """A mask frame of depth_stream_bench -> (depth crop, link-label crop, origin) and its scene table: the object's pixels cut into K
    links by column, link l = part l with the identity map, behind the frame's pinhole camera."""
    d, m, org = frame
    cols = np.flatnonzero(m.any(0))
    edges = np.linspace(cols.min(), cols.max() + 1, K + 1)
    link = np.clip(np.searchsorted(edges, np.arange(d.shape[1]), side="right") - 1, 0, K - 1).astype(np.uint8)
    lab = np.where(m, link[None, :], D.NOT_OBJECT).astype(np.uint8)
    sc = np.zeros(D.SCENE_WIDTH)
    sc[0:6] = sc[7:13] = D.unprojection_from_intrinsics(focal, focal, SIDE / 2, SIDE / 2)
    sc[6], sc[13], sc[14] = SCALE, 10, K
    for l in range(K):
        at = D.SCENE_HEAD + D.SCENE_LINK * l
        sc[at], sc[at + 1] = l, l
        sc[at + 2:at + 14] = np.eye(4)[:3].reshape(12)
    return (d, lab, org), sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=4, help="passes over the frames per timed leg")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--clouds", type=int, default=320)
    args = ap.parse_args()
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    sizes = rs.randint(700, 3001, args.clouds)
    made = [annotate(*make_frame(rs, make_cloud(i, N=POINTS, K=K)["P"], int(n)), K) for i, n in enumerate(sizes)]
    nf, rigs, jf = np.ones(B, np.float32), np.tile(identity_rig(K), (B, 1)), rs.normal(size=(B, 13))
    fbatches, cbatches, rows, pixels = [], [], [], []
    for i in range(0, len(made) - B + 1, B):
        frames, tables = [m[0] for m in made[i:i + B]], np.stack([m[1] for m in made[i:i + B]])
        fbatches.append((frames, nf, dict(scene=tables, rig=rigs, frame=jf)))
        r7, off, cnt, _ = D.annotate_depth_batch(frames, tables, "uint16", K)
        assert (cnt > 0).all()
        cbatches.append(([np.ascontiguousarray(r7[off[b]:off[b + 1]]) for b in range(B)], nf, jf, rigs))
        rows.append(int(off[-1]))
        pixels.append(sum(f[0].size for f in frames))
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    depth = AncshPipeline(K, wa, wn, B, N, dev, depth_capacity=max(pixels), depth_dtype="uint16", **kw).prepare()
    xyz = AncshPipeline(K, wa, wn, B, N, dev, raw_capacity=max(rows), **kw).prepare()
    torch.cuda.synchronize()

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        gen = (depth.stream_depth_batches(fbatches[k] for _ in range(passes) for k in range(len(fbatches))) if name == "f" else
               xyz.stream_batches(cbatches[k] for _ in range(passes) for k in range(len(cbatches))))
        for _ in gen:
            n += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n          # ms per batch of B frames, steady state over the slots

    for name in "fg":                                         # warm-up: every slot replayed with real input
        leg(name, 1)
    ms = {name: [] for name in "fg"}
    for _ in range(args.rounds):
        for name in "fg":
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"metric": "ms per batch: annotated depth stream (f) vs xyz build_point_gt stream on the same frames' clouds (g)",
                      "device": torch.cuda.get_device_name(0), "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "f_over_g": round(med["f"] / med["g"], 4),
                      "h2d_bytes_per_batch_f": int(round(3 * np.mean(pixels) + 8 * D.SCENE_WIDTH * B)), "h2d_bytes_per_batch_g": int(round(28 * np.mean(rows))),
                      "rows_per_frame": round(float(np.mean(rows)) / B, 1), "crop_pixels_per_frame": round(float(np.mean(pixels)) / B, 1),
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(fbatches) * B,
                                "passes": args.passes, "rounds": args.rounds}}))


if __name__ == "__main__":
    main()
