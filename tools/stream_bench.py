"""Throughput of the streaming pipeline (AncshPipeline.stream: raw clouds of varied sizes in, pose records out, H2D + on-GPU sampling +
fit + record D2H per batch) against load_inputs + step() on the same clouds, at configs[2]'s shape (K = 3, 32 x 1024, 10000 / 200
hypotheses, couple=True, synthetic weights, 20 slots).  Prints one JSON line.

    python tools/stream_bench.py [--passes 5] [--slots 20] [--arithmetic {f32,f16x2}] [--range-guard] [--overflow-every K] [--articulation] [--dense]
                                 [--joint-source {gt,predicted}] [--joint-states] [--fit-quality] [--ground-truth] [--point-gt [--build-point-gt] [--build-gt-pose]]
                                 [--no-baseline]

--arithmetic pins both pipelines' arithmetic; --range-guard streams through AncshPipeline(arithmetic="f16x2", range_guard=True); with
--overflow-every K, one cloud of every K-th batch has a norm factor of 1e6 (absolute xyz beyond f16's range: flagged, refit in f32).  The
line then also carries the rerun count, the latency of the batches that reran and the device memory the streaming pipeline holds.
--articulation streams with AncshPipeline(articulation=True) (the record plus the (n, K, 12) articulation block per cloud).
--joint-states (with --articulation) streams with AncshPipeline(joint_states=True): the block is the (n, K, 20) one, one more launch a step.
--fit-quality streams with AncshPipeline(fit_quality=True): the record is the (n, K, 39) wide one, one more launch a step.
--ground-truth streams with AncshPipeline(ground_truth=True): every batch carries a (32, K, 19) ground truth in, the record comes back 12
columns wider (the errors against it, ancsh_gt_error_rec), one more launch a step.
--point-gt (with --articulation) streams with AncshPipeline(point_ground_truth=True): the clouds are (n_raw, 18) rows with per-point ground
truth (4.5 times the bytes of an [x y z joint_cls] row over the link), every batch carries (32, 13) frames in, the record comes back 21
columns wider (both networks' test losses and the joint errors, ancsh_point_gt_rec), one more launch a step.
--build-point-gt (with --point-gt) streams with AncshPipeline(build_point_gt=True): the clouds are (n_raw, 7) annotated rows [x y z | cx cy cz |
part] (28 bytes a row over the link instead of 72), every batch carries (32, RIG_WIDTH) rigs in (two revolute joints on part 0,
dataset.pack_joint_rig), and the step's first launch builds the 18-column rows on the device (ancsh_point_gt_build), one more launch a step.
--build-gt-pose (with --point-gt) streams with AncshPipeline(build_gt_pose=True): no frames travel in, a ground truth carries only its box
extents, and one more launch behind the sampler (ancsh_gt_pose_build) fits the ground-truth poses the error launches read.
--no-baseline skips the load_inputs + step() leg (step_clouds_per_s and ratio are then null): for A/B runs of the stream alone.
--dense streams with AncshPipeline(dense=True) (the record plus every raw row's label and 7 head values: ancsh_raw_point_labels).
--joint-source predicted builds both pipelines with joint_source="predicted" (stage B's joint association from the ANCSH network's index
head) and submits (n_raw, 3) xyz clouds: no label column crosses to the device.
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
    ap.add_argument("--arithmetic", choices=("f32", "f16x2"), default=None)
    ap.add_argument("--range-guard", action="store_true")
    ap.add_argument("--overflow-every", type=int, default=0)
    ap.add_argument("--articulation", action="store_true", help="stream with AncshPipeline(articulation=True) and retire the blocks too")
    ap.add_argument("--joint-states", action="store_true", help="with --articulation: AncshPipeline(joint_states=True), the (n, K, 20) block")
    ap.add_argument("--fit-quality", action="store_true", help="AncshPipeline(fit_quality=True): the streamed record is the (n, K, 39) wide one")
    ap.add_argument("--ground-truth", action="store_true",
                    help="AncshPipeline(ground_truth=True): a ground truth per batch in, the streamed record 12 error columns wider")
    ap.add_argument("--point-gt", action="store_true",
                    help="with --articulation: AncshPipeline(point_ground_truth=True): 18-column clouds and frames in, the record 21 columns wider")
    ap.add_argument("--build-point-gt", action="store_true",
                    help="with --point-gt: AncshPipeline(build_point_gt=True): 7-column annotated clouds and rigs in, the rows built on the device")
    ap.add_argument("--build-gt-pose", action="store_true",
                    help="with --point-gt: AncshPipeline(build_gt_pose=True): the ground-truth poses fitted on the device, no frames in")
    ap.add_argument("--no-baseline", action="store_true", help="skip the load_inputs + step() leg")
    ap.add_argument("--dense", action="store_true", help="stream with AncshPipeline(dense=True) and retire every raw row's labels too")
    ap.add_argument("--joint-source", choices=("gt", "predicted"), default="gt",
                    help="predicted: the joint association from the network's index head; (n_raw, 3) xyz clouds are submitted")
    args = ap.parse_args()
    if args.range_guard and args.arithmetic != "f16x2":
        ap.error("--range-guard needs --arithmetic f16x2")
    if args.joint_states and not args.articulation:
        ap.error("--joint-states needs --articulation")
    if args.point_gt and not args.articulation:
        ap.error("--point-gt needs --articulation")
    if args.build_point_gt and not args.point_gt:
        ap.error("--build-point-gt needs --point-gt")
    if args.build_gt_pose and not args.point_gt:
        ap.error("--build-gt-pose needs --point-gt")
    extra = args.arithmetic is not None
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    sizes = rs.randint(700, 3001, args.clouds)
    raw = []
    for i, n in enumerate(sizes):
        c = make_cloud(i, N=int(n), K=K)
        raw.append(np.concatenate([c["P"], c["cls_gt"][:, None].astype(np.float32)], 1))
    predicted = args.joint_source == "predicted"
    rigs = None
    if args.build_point_gt:      # 7-column rows: random canonical coordinates, the part label; one rig for every cloud (the launch's cost does not depend on it)
        from articulated_pose_amd.dataset import pack_joint_rig
        raw = [np.concatenate([r[:, :3], rs.uniform(-0.3, 0.3, (r.shape[0], 3)).astype(np.float32), r[:, 3:]], 1) for r in raw]
        corners = np.array([[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]]] + [[[-0.3, -0.3, -0.3], [0.3, 0.3, 0.3]]] * K)
        factors = 1.0 / np.linalg.norm(corners[:, 1] - corners[:, 0], axis=1)
        joints = {"link": {"xyz": [[0, 0, 0], [0.05, 0, 0], [0, -0.05, 0.1]]},
                  "joint": {"axis": [[0, 0, 0], [1.0, 0.05, 0], [0, 0.1, 1.0]], "parent": [-1, 0, 0]}}
        rigs = np.tile(pack_joint_rig(corners, factors, joints, [[j] for j in range(K)])[0], (B, 1))
    elif args.point_gt:          # 18-column rows: the part label, random ground-truth channels (the launch's cost does not depend on them), the joint label
        raw = [np.concatenate([r[:, :4], rs.uniform(0, 1, (r.shape[0], 13)).astype(np.float32), r[:, 3:]], 1) for r in raw]
    elif predicted:
        raw = [np.ascontiguousarray(r[:, :3]) for r in raw]
    batches = [(raw[i:i + B], np.ones(B, np.float32)) for i in range(0, len(raw) - B + 1, B)]
    if args.overflow_every:
        for k in range(0, len(batches), args.overflow_every):
            batches[k][1][k % B] = 1.0e6
    gts = None
    if args.ground_truth:        # a rotation about z, a scale, translations and box extents per part: the launch's cost does not depend on them
        a = rs.uniform(0, 2 * np.pi, (len(batches), B, K))
        z, o = np.zeros_like(a), np.ones_like(a)
        R = np.stack([np.cos(a), -np.sin(a), z, np.sin(a), np.cos(a), z, z, z, o], -1)
        gts = np.concatenate([R, rs.uniform(0.5, 1.5, a.shape + (1,)), rs.uniform(-0.3, 0.3, a.shape + (3,)), rs.uniform(0.3, 0.9, a.shape + (3,)),
                              rs.uniform(-0.3, 0.3, a.shape + (3,))], -1)
    frames = rs.normal(size=(len(batches), B, 13)) if args.point_gt and not args.build_gt_pose else None
    if gts is not None and args.build_gt_pose:      # only the box extents travel in
        gts[..., :13] = gts[..., 16:] = np.nan
    with_gt = lambda k, c, nf: (c, nf) + ((gts[k],) if args.ground_truth else ()) + ((frames[k],) if frames is not None else ()) + \
        ((rigs,) if args.build_point_gt else ())
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)

    # streaming
    torch.cuda.synchronize()
    mem0 = torch.cuda.mem_get_info(dev)[0]
    pipe = AncshPipeline(K, wa, wn, B, N, dev, couple=True, slots=args.slots, raw_capacity=B * 3000, arithmetic=args.arithmetic,
                         range_guard=args.range_guard, articulation=args.articulation, dense=args.dense,
                         joint_source=args.joint_source, joint_states=args.joint_states, fit_quality=args.fit_quality,
                         ground_truth=args.ground_truth, point_ground_truth=args.point_gt,
                         **(dict(build_point_gt=True) if args.build_point_gt else {}),
                         **(dict(build_gt_pose=True) if args.build_gt_pose else {})).prepare()
    torch.cuda.synchronize()
    pipe_bytes = mem0 - torch.cuda.mem_get_info(dev)[0]
    for _ in pipe.stream_batches([with_gt(k, c, nf) for k, (c, nf) in enumerate(batches)]):          # warm-up: every slot replayed with real input
        pass
    torch.cuda.synchronize()
    t_sub, lat = {}, []
    work = [with_gt(k, c, nf) + ((p, k),) for p in range(args.passes) for k, (c, nf) in enumerate(batches)]

    def timed(items):
        for it in items:
            t_sub[it[-1]] = time.perf_counter()
            yield it
    t0 = time.perf_counter()
    n_out, rerun_lat, n_blocks, n_rows = 0, [], 0, 0
    reruns0 = pipe.f32_reruns
    for item in pipe.stream_batches(timed(work), articulation=args.articulation, dense=args.dense):
        tag, seed, rec = item[:3]
        n_blocks += item[-2 if args.dense else -1].shape[0] if args.articulation else 0
        n_rows += item[-1][0].shape[0] if args.dense else 0
        lat.append(time.perf_counter() - t_sub[tag])
        if pipe.f32_reruns != reruns0:
            rerun_lat.append(lat[-1])
            reruns0 = pipe.f32_reruns
        n_out += rec.shape[0]
    torch.cuda.synchronize()
    t_stream = time.perf_counter() - t0
    pipe_reruns, pipe_paired = pipe.f32_reruns, pipe.paired is not None
    del pipe
    torch.cuda.synchronize()

    # baseline: the same clouds sampled once up front, then load_inputs + step() per batch, the slot's previous record read back
    pre = []
    for k, (c, nf) in enumerate([] if args.no_baseline else batches):
        if args.point_gt:
            c = [np.ascontiguousarray(r[:, [0, 1, 2, 6 if args.build_point_gt else 17]]) for r in c]
        s = sample_raw_batch(c, N, nf, k, dev, xyz_only=predicted)
        pre.append((s["P"].cpu().numpy(), None if predicted else s["joint_cls"].cpu().numpy()))
    base = None
    if not args.no_baseline:
        base = AncshPipeline(K, wa, wn, B, N, dev, couple=True, slots=args.slots, arithmetic=args.arithmetic, joint_source=args.joint_source)
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
    t_step = None
    if base is not None:
        run_steps(pre)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps([pre[k] for _ in range(args.passes) for k in range(len(pre))])
        torch.cuda.synchronize()
        t_step = time.perf_counter() - t0

    n_clouds = args.passes * len(batches) * B
    line = {"metric": "clouds/s through AncshPipeline.stream_batches (raw clouds %d-%d rows, H2D + sampling + fit + record D2H)" % (sizes.min(), sizes.max()),
            "stream_clouds_per_s": round(n_clouds / t_stream, 1), "step_clouds_per_s": round(n_clouds / t_step, 1) if t_step else None,
            "ratio": round(t_step / t_stream, 4) if t_step else None, "records_out": n_out,
            "batch_latency_ms_min": round(1e3 * min(lat), 2), "batch_latency_ms_max": round(1e3 * max(lat), 2),
            "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "couple": True,
                      "distinct_clouds": len(batches) * B, "timed_batches": args.passes * len(batches)},
            "baseline": "load_inputs (pageable, synchronous) + step(), the slot's previous record read back before its next batch"}
    if extra:
        line.update({"arithmetic": args.arithmetic, "range_guard": args.range_guard, "overflow_every": args.overflow_every,
                     "f32_reruns": pipe_reruns, "paired": pipe_paired, "stream_device_bytes": int(pipe_bytes),
                     "rerun_batch_latency_ms": [round(1e3 * x, 2) for x in rerun_lat[:8]],
                     "batch_latency_ms_median": round(1e3 * float(np.median(lat)), 2)})
    if args.articulation:
        line.update({"articulation": True, "blocks_out": n_blocks})
    if args.joint_states:
        line.update({"joint_states": True})
    if args.fit_quality:
        line.update({"fit_quality": True})
    if args.ground_truth:
        line.update({"ground_truth": True, "record_columns": int(rec.shape[2])})
    if args.point_gt:
        line.update({"point_ground_truth": True, "record_columns": int(rec.shape[2]), "h2d_row_bytes": 28 if args.build_point_gt else 72})
    if args.build_point_gt:
        line.update({"build_point_gt": True})
    if args.build_gt_pose:
        line.update({"build_gt_pose": True})
    if predicted:
        line.update({"joint_source": "predicted"})
    if args.dense:
        line.update({"dense": True, "raw_rows_out": n_rows, "dense_d2h_bytes_per_batch": round(n_rows * 32 / (args.passes * len(batches)))})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
