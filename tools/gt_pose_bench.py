"""What build_gt_pose=True costs a stream, at tools/stream_bench.py's shape (K = 3, 32 x 1024, raw clouds of 700-3000 rows of 18 columns,
synthetic weights, articulation, ground_truth and point_ground_truth on): two pipelines in one process, timed in alternation --
  (a) build_gt_pose=True: the step fits the ground-truth poses (ancsh_gt_pose_build); gt carries the box extents only, no frame travels in;
  (b) the option off, fed (32, K, 19) / (32, 13) host tables prepared before the clock starts.
Leg (b) leaves out what the option removes from a real consumer -- the host Umeyama fits and the two device round trips per batch that
reproduce the sampler's points -- so the ratio is the cost of the launch alone, not the gain of the feature.  Prints one JSON line.

    python tools/gt_pose_bench.py [--rounds 3] [--passes 3] [--slots 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import articulated_pose_amd  # noqa: E402,F401
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.synthetic import make_cloud  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations a, b, a, b, ...")
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the 640 clouds (20 batches each) per leg and round")
    ap.add_argument("--slots", type=int, default=20)
    ap.add_argument("--clouds", type=int, default=640)
    args = ap.parse_args()
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    raw = []
    for i, n in enumerate(rs.randint(700, 3001, args.clouds)):
        c = make_cloud(i, N=int(n), K=K)
        lab = c["cls_gt"][:, None].astype(np.float32)
        raw.append(np.concatenate([c["P"], lab, rs.uniform(0, 1, (int(n), 13)).astype(np.float32), lab], 1))
    batches = [(raw[i:i + B], np.ones(B, np.float32)) for i in range(0, len(raw) - B + 1, B)]
    gts = rs.uniform(0.3, 0.9, (len(batches), B, K, 19))
    frames = rs.normal(size=(len(batches), B, 13))
    boxes = np.full_like(gts, np.nan)
    boxes[..., 13:16] = gts[..., 13:16]
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, raw_capacity=B * 3000, articulation=True, ground_truth=True, point_ground_truth=True)
    legs = {"a": (AncshPipeline(K, wa, wn, B, N, dev, build_gt_pose=True, **kw).prepare(),
                  [(c, nf, boxes[k]) for k, (c, nf) in enumerate(batches)]),
            "b": (AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare(),
                  [(c, nf, gts[k], frames[k]) for k, (c, nf) in enumerate(batches)])}
    for pipe, items in legs.values():               # warm-up: every slot replayed with real input
        for _ in pipe.stream_batches(items):
            pass
    torch.cuda.synchronize()
    rates = {"a": [], "b": []}
    for _ in range(args.rounds):
        for name, (pipe, items) in legs.items():
            t0 = time.perf_counter()
            n = sum(rec.shape[0] for _, _, rec in pipe.stream_batches(items * args.passes))
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps({"metric": "clouds/s through AncshPipeline.stream_batches, build_gt_pose on (a) against off with host tables prepared (b)",
                      "a_clouds_per_s": [round(x, 1) for x in rates["a"]], "b_clouds_per_s": [round(x, 1) for x in rates["b"]],
                      "a_median": round(med["a"], 1), "b_median": round(med["b"], 1), "a_over_b": round(med["a"] / med["b"], 4),
                      "shape": {"K": K, "B": B, "N": N, "slots": args.slots, "rounds": args.rounds, "passes": args.passes,
                                "distinct_clouds": len(batches) * B, "record_columns": 59},
                      "note": "leg b leaves out the host Umeyama fits and the two device round trips per batch the option removes"}))


if __name__ == "__main__":
    main()
