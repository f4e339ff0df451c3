"""Throughput of the streaming pipeline (AncshPipeline.stream: raw clouds of varied sizes in, pose records out, H2D + on-GPU sampling +
fit + record D2H per batch) against load_inputs + step() on the same clouds, at configs[2]'s shape (K = 3, 32 x 1024, 10000 / 200
hypotheses, couple=True, synthetic weights, 20 slots).  Prints one JSON line.

    python tools/stream_bench.py [--passes 5] [--slots 20]
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
from articulated_pose_amd.dataset import sample_raw_batch  # noqa: E402
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.synthetic import make_cloud  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5, help="timed passes over the 640 clouds (20 batches each)")
    ap.add_argument("--slots", type=int, default=20)
    ap.add_argument("--clouds", type=int, default=640)
    args = ap.parse_args()
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    sizes = rs.randint(700, 3001, args.clouds)
    raw = []
    for i, n in enumerate(sizes):
        c = make_cloud(i, N=int(n), K=K)
        raw.append(np.concatenate([c["P"], c["cls_gt"][:, None].astype(np.float32)], 1))
    batches = [(raw[i:i + B], np.ones(B, np.float32)) for i in range(0, len(raw) - B + 1, B)]
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)

    # streaming
    pipe = AncshPipeline(K, wa, wn, B, N, dev, couple=True, slots=args.slots, raw_capacity=B * 3000).prepare()
    for _ in pipe.stream_batches(batches):          # warm-up: every slot replayed with real input
        pass
    torch.cuda.synchronize()
    t_sub, lat = {}, []
    work = [(c, nf, (p, k)) for p in range(args.passes) for k, (c, nf) in enumerate(batches)]

    def timed(items):
        for it in items:
            t_sub[it[2]] = time.perf_counter()
            yield it
    t0 = time.perf_counter()
    n_out = 0
    for tag, seed, rec in pipe.stream_batches(timed(work)):
        lat.append(time.perf_counter() - t_sub[tag])
        n_out += rec.shape[0]
    torch.cuda.synchronize()
    t_stream = time.perf_counter() - t0
    del pipe
    torch.cuda.synchronize()

    # baseline: the same clouds sampled once up front, then load_inputs + step() per batch, the slot's previous record read back
    pre = []
    for k, (c, nf) in enumerate(batches):
        s = sample_raw_batch(c, N, nf, k, dev)
        pre.append((s["P"].cpu().numpy(), s["joint_cls"].cpu().numpy()))
    base = AncshPipeline(K, wa, wn, B, N, dev, couple=True, slots=args.slots)
    base.load_inputs(*pre[0])
    base.prepare()

    def run_steps(items):
        n = 0
        for P, J in items:
            i = base._next
            sl = base.next_slot()
            sl.stream.synchronize()
            if sl.out is not None:
                n += sl.out["record"].cpu().shape[0]
            base.load_inputs(P, J, slot=i)
            base.step()
        base.synchronize()
        return n
    run_steps(pre)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps([pre[k] for _ in range(args.passes) for k in range(len(pre))])
    torch.cuda.synchronize()
    t_step = time.perf_counter() - t0

    n_clouds = args.passes * len(batches) * B
    line = {"metric": "clouds/s through AncshPipeline.stream_batches (raw clouds %d-%d rows, H2D + sampling + fit + record D2H)" % (sizes.min(), sizes.max()),
            "stream_clouds_per_s": round(n_clouds / t_stream, 1), "step_clouds_per_s": round(n_clouds / t_step, 1),
            "ratio": round(t_step / t_stream, 4), "records_out": n_out,
            "batch_latency_ms_min": round(1e3 * min(lat), 2), "batch_latency_ms_max": round(1e3 * max(lat), 2),
            "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "couple": True,
                      "distinct_clouds": len(batches) * B, "timed_batches": args.passes * len(batches)},
            "baseline": "load_inputs (pageable, synchronous) + step(), the slot's previous record read back before its next batch"}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
