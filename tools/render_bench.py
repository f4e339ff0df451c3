"""Throughput of the GPU renderer (ancsh_render_depth_labels) and of the stream it feeds: AncshPipeline(..., render_mesh=mesh), whose step
renders its own depth and link-label crops, against the annotated depth stream fed the SAME frames from host memory, at equal frames and
configs[2]'s shape (K = 3, 32 x 1024, 10000 / 200 hypotheses, couple=True, synthetic weights, predicted joints).  The object: three
tessellated boxes, one per link, under random views and openings; one SIDE x SIDE uint16 crop per frame.  Measured:
  operator: frames/s of the entry alone on one batch of 32 frames (HIP events around --calls back-to-back calls);
  two legs, alternated in one process for --rounds rounds:
    r: the rendered stream (geometry, render table and scene table per frame cross to the device: 20 + 1664 + 1920 bytes);
    d: the annotated depth stream on the frames depth.render_depth_frames made of the same tables BEFORE the clock starts (3 bytes per
       pixel more; whatever renderer made them on the host is not in the timed loop: the best case without the new entry).
Prints one JSON line: a record, not a gate.

--sensor measures the depth sensor model (ancsh_depth_sensor_model) instead: the entry alone on one batch of 32 rendered crops with the
identity table and with a noisy one (every term on), and two legs of the rendered stream, alternated like r and d above:
    r: the rendered stream without the option;   s: the rendered stream built with sensor=<the noisy table>.

--reprojection measures render-and-compare (reprojection=True) instead: two legs of the rendered stream, alternated like r and d above:
    r: the rendered stream without the option;   p: the rendered stream built with reprojection=True;
and the option's three calls alone on one batch of 32 frames: ancsh_reproject_scene_build, the renderer on the 64 predicted frames, and
ancsh_reproject_compare_rec, with the record the stream fitted for that batch.

--refine N measures render-and-compare ICP (refine=pack_refine(iters=N)) instead: two legs of the rendered stream, alternated like r and d:
    r: the rendered stream without the option;   f: the rendered stream built with refine=;
one ancsh_refine_pass alone on one batch of 32 frames whose record draws every part (the exact poses moved by 0.01), one whole loop of the
device wrappers (pose.refinement.refine_batch) on it, and the eager operator depth.refine_frames from host arrays.
--refine N --silhouette adds a third leg, s: the rendered stream built with refine=pack_refine(iters=N, silhouette=dict(weight=1, dist=0.1,
slack=1)), and times ancsh_silhouette_field, one ancsh_refine_pass_sil and the whole loop with the term on the same batch and record.
--refine N --silhouette --coverage adds a fourth leg, c: the rendered stream built with the same table and coverage=dict(weight=1, dist=0.1,
slack=1), next to silhouette-only (s) and plain (f), and times ancsh_coverage_field, one ancsh_refine_pass_cov and the whole loop with both terms.
--refine N --silhouette --coverage --scale adds a fifth leg, g: the rendered stream built with the same table and scale=dict(max_step=0.05,
max_total=0.25), alternated with the coverage-only stream (c) of the same build, and times one ancsh_refine_pass_scale and the whole loop with it.
--refine N --joints measures the joint step (refine=pack_refine(iters=N, joints=dict(weight=1, axis_length=0.5))) instead, on the POSED stream
(the option needs the kinematic table: link 1 hangs on a revolute, link 2 on a prismatic joint of link 0): two legs, alternated:
    f: the posed stream built with refine=pack_refine(iters=N);   j: the same with joints=;
ancsh_refine_joint_step alone on one batch of 32 frames whose record draws every part a different distance off its place, and the share of
that batch's objects whose joints' position residual (obj's gap_rms) is lower at the last pass than at the first.

    python tools/render_bench.py [--sensor | --reprojection | --refine N [--silhouette [--coverage [--scale]] | --joints]] [--rounds 3] [--passes 4] [--slots 8] [--frames 320] [--side 128] [--tess 8]
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
from articulated_pose_amd import depth as D  # noqa: E402
from articulated_pose_amd.dataset import identity_rig  # noqa: E402
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402

SCALE = 1e-3
NOISY_SENSOR = dict(sigma=(0.001, 0.002, 0.001), z0=1.0, p_hole=0.05, p_edge=0.5, edge_rel=0.05, disparity=(35.0, 8), z_range=(0.2, 10.0))
LO, HI = np.array([-0.16, -0.11, -0.06]), np.array([0.16, 0.11, 0.06])


def tessellated_box(lo, hi, n):
    """(vertices, faces) of the box [lo, hi], every face an n x n grid of quads, two triangles each: 12 n^2 triangles."""
    verts, faces = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (lo, hi):
            base = len(verts)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = np.empty(3)
                    p[axis], p[u], p[v] = side[axis], lo[u] + (hi[u] - lo[u]) * i / n, lo[v] + (hi[v] - lo[v]) * j / n
                    verts.append(p)
            for i in range(n):
                for j in range(n):
                    a = base + i * (n + 1) + j
                    faces += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return np.asarray(verts), np.asarray(faces, np.int64)


def make_scene(rs, side):
    """One frame: (render table, scene table) of the three-link object seen from about 1.5 units under a slightly random view."""
    t, near, far = np.tan(np.radians(20.0)), 0.1, 100.0
    P = np.array([[1.0 / t, 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1.0, 0]])
    V = np.eye(4)
    V[:3, :3] = D._rotation_from_rpy(*rs.uniform(-0.5, 0.5, 3))[:3, :3]
    V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
    opening = rs.uniform(0.1, 1.2)
    pos = np.array([[0.0, 0.0, 0.0], [0.3, 0.02, 0.12], [-0.34, -0.03, 0.02]])
    orn = np.array([[0, 0, 0, 1.0], [0, np.sin(opening / 2), 0, np.cos(opening / 2)], [0, 0, np.sin(0.2), np.cos(0.2)]])
    zero = np.zeros((3, 3))
    return (D.pack_render_scene(V, P, pos, orn, side, side, depth_scale=SCALE),
            D.pack_frame_scene(V, P, pos, orn, zero, zero, zero[:2], [[0], [1], [2]], side, side, depth_scale=SCALE))


def timed_calls(call, rounds, calls):
    """ms per call over `calls` back-to-back calls between two HIP events, once per round, after 20 warm-up calls."""
    for _ in range(20):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(rounds):
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return ms


def sensor_bench(args, K, B, N, dev, mesh, rbatches, d_geom, d_sc, clean, cap):
    """--sensor: the entry alone (identity and noisy table) on `clean`, the rendered crops of one batch; the rendered stream with and without
    sensor=noisy, alternated."""
    seed = torch.tensor([12345], dtype=torch.int64, device=dev)
    out = (torch.zeros_like(clean[0]), torch.zeros_like(clean[1]))
    tables = {"identity": D.pack_sensor(), "noisy": D.pack_sensor(**NOISY_SENSOR)}
    op_ms, dropped = {}, {}
    for name, table in tables.items():
        d_table = torch.from_numpy(table).to(dev)
        op_ms[name] = timed_calls(lambda: D.depth_sensor_model(clean[0], clean[1], d_geom, d_sc, d_table, seed, out=out), args.rounds, args.calls)
        dropped[name] = int(((out[1] == D.NOT_OBJECT) & (clean[1] != D.NOT_OBJECT)).sum())
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16", render_mesh=mesh)
    pipes = {"r": AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare(), "s": AncshPipeline(K, wa, wn, B, N, dev, sensor=tables["noisy"], **kw).prepare()}
    torch.cuda.synchronize()

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        for _ in pipes[name].stream_render_batches(rbatches[k] for _ in range(passes) for k in range(len(rbatches))):
            n += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for name in "rs":
        leg(name, 1)
    ms = {name: [] for name in "rs"}
    for _ in range(args.rounds):
        for name in "rs":
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"metric": "the depth sensor model: ms per launch of the entry alone on one batch (identity / noisy table); frames/s of the "
                                "rendered stream without (r) and with (s) sensor=noisy",
                      "device": torch.cuda.get_device_name(0), "operator_ms_per_batch": {k: round(float(np.median(v)), 4) for k, v in op_ms.items()},
                      "operator_ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in op_ms.items()},
                      "operator_bytes_per_batch": 2 * 3 * cap, "object_pixels_dropped_per_batch": dropped,
                      "stream_frames_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "s_over_r": round(med["s"] / med["r"], 4),
                      "sensor": NOISY_SENSOR, "crop_pixels_per_frame": args.side * args.side,
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(rbatches) * B,
                                "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


def reprojection_bench(args, K, B, N, dev, mesh, d_mesh, rbatches, d_geom, d_rt, d_sc, clean, cap):
    """--reprojection: the rendered stream with and without reprojection=True, alternated; then the option's three calls alone (the table
    builder, the renderer on 2 B predicted frames, the comparison) on the last batch, with the record the stream fitted for it."""
    from articulated_pose_amd.pose import reprojection as R
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16", render_mesh=mesh)
    pipes = {"r": AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare(), "p": AncshPipeline(K, wa, wn, B, N, dev, reprojection=True, **kw).prepare()}
    torch.cuda.synchronize()
    last = {}

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        for got in pipes[name].stream_render_batches(rbatches[k] for _ in range(passes) for k in range(len(rbatches))):
            n += 1
        torch.cuda.synchronize()
        last[name] = got[2]
        return 1e3 * (time.perf_counter() - t0) / n

    for name in "rp":
        leg(name, 1)
    ms = {name: [] for name in "rp"}
    for _ in range(args.rounds):
        for name in "rp":
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    W = last["r"].shape[2]
    assert last["p"].shape[2] == W + R.REPROJECTION_WIDTH and last["p"][:, :, :W].tobytes() == last["r"].tobytes()
    # the record the three calls are timed on: the stream's own last one with both poses of every part replaced by the pose that undoes the
    # frame's scene map (the rig and the norm factor are the identity here: [s R | t] = D M^-1), so that every part is drawn and scored
    # twice -- random-weight networks leave most poses NaN, and a NaN pose draws nothing
    exact = np.ascontiguousarray(last["p"][:, :, :W])
    sc = rbatches[-1][2]["scene"]
    for f in range(B):
        for j in range(K):
            M = np.vstack([sc[f, D.SCENE_HEAD + D.SCENE_LINK * j + 2:D.SCENE_HEAD + D.SCENE_LINK * (j + 1)].reshape(3, 4), [0, 0, 0, 1.0]])
            pose = np.diag([1.0, -1.0, 1.0, 1.0]) @ np.linalg.inv(M)
            exact[f, j, :13] = exact[f, j, 13:26] = np.concatenate([pose[:3, :3].reshape(9), [1.0], pose[:3, 3]])
    carried = torch.from_numpy(exact).to(dev)
    d_rig, d_nf = torch.from_numpy(rbatches[-1][2]["rig"]).to(dev), torch.from_numpy(rbatches[-1][1]).to(dev)
    tables, pred = R.predicted_frames(B, cap, "uint16", dev)
    wide = torch.empty((B, K, W + R.REPROJECTION_WIDTH), dtype=torch.float64, device=dev)
    calls = {"scene_build": lambda: R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables),
             "render_2B_frames": lambda: D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2]),
             "compare": lambda: R.reproject_compare(clean[0], clean[1], pred[0], pred[1], d_geom, d_sc, carried, out=wide)}
    op_ms = {name: timed_calls(call, args.rounds, args.calls) for name, call in calls.items()}
    cols, timed = R.named_columns(last["p"]), R.named_columns(wide.cpu().numpy())
    print(json.dumps({"metric": "render-and-compare: ms per batch of the rendered stream without (r) and with (p) reprojection=True; ms per call of the "
                                "option's three calls alone on one batch",
                      "device": torch.cuda.get_device_name(0), "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "stream_frames_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "added_ms_per_batch": round(med["p"] - med["r"], 4),
                      "p_over_r": round(med["p"] / med["r"], 4), "operator_ms_per_batch": {k: round(float(np.median(v)), 4) for k, v in op_ms.items()},
                      "operator_ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in op_ms.items()},
                      "device_bytes_per_pixel_of_capacity_and_slot": 2 * (2 + 1 + 8),
                      "streamed_last_batch": {"parts": B * K, "parts_with_a_finite_baseline_pose": int(np.isfinite(cols["baseline_n_pred"]).sum()),
                                              "parts_with_a_finite_nonlinear_pose": int(np.isfinite(cols["nonlinear_n_pred"]).sum()),
                                              "predicted_pixels": float(np.nansum(cols["baseline_n_pred"]) + np.nansum(cols["nonlinear_n_pred"]))},
                      "operator_record": {"median_iou": float(np.median(timed["nonlinear_iou"])),
                                          "predicted_pixels": float(timed["baseline_n_pred"].sum() + timed["nonlinear_n_pred"].sum()),
                                          "max_abs_d": float(timed["nonlinear_max_abs"].max())},
                      "crop_pixels_per_frame": args.side * args.side, "triangles": int(mesh[1].shape[0]),
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(rbatches) * B,
                                "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


def refine_bench(args, K, B, N, dev, mesh, d_mesh, rbatches, d_geom, d_rt, d_sc, clean, cap):
    """--refine N: the rendered stream with and without refine=pack_refine(iters=N), alternated; then one ancsh_refine_pass, one whole loop on
    device tensors and the eager operator on the last batch, with a record that draws every part 0.01 off its place."""
    from articulated_pose_amd.pose import refinement as F, reprojection as R
    table = F.pack_refine(iters=args.refine)
    sil_table = F.pack_refine(iters=args.refine, silhouette=dict(weight=1.0, dist=0.1, slack=1.0)) if args.silhouette else None
    cov_table = F.pack_refine(iters=args.refine, silhouette=dict(weight=1.0, dist=0.1, slack=1.0), coverage=dict(weight=1.0, dist=0.1, slack=1.0)) if args.coverage else None
    scl_table = F.pack_refine(iters=args.refine, silhouette=dict(weight=1.0, dist=0.1, slack=1.0), coverage=dict(weight=1.0, dist=0.1, slack=1.0),
                              scale=dict(max_step=0.05, max_total=0.25)) if args.scale else None
    legs = "rfscg" if args.scale else "rfsc" if args.coverage else "rfs" if args.silhouette else "rf"
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16", render_mesh=mesh)
    pipes = {"r": AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare(), "f": AncshPipeline(K, wa, wn, B, N, dev, refine=table, **kw).prepare()}
    if args.silhouette:
        pipes["s"] = AncshPipeline(K, wa, wn, B, N, dev, refine=sil_table, **kw).prepare()
    if args.coverage:
        pipes["c"] = AncshPipeline(K, wa, wn, B, N, dev, refine=cov_table, **kw).prepare()
    if args.scale:
        pipes["g"] = AncshPipeline(K, wa, wn, B, N, dev, refine=scl_table, **kw).prepare()
    torch.cuda.synchronize()
    last = {}

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        for got in pipes[name].stream_render_batches(rbatches[k] for _ in range(passes) for k in range(len(rbatches))):
            n += 1
        torch.cuda.synchronize()
        last[name] = got[2]
        return 1e3 * (time.perf_counter() - t0) / n

    for name in legs:
        leg(name, 1)
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    W = last["r"].shape[2]
    assert last["f"].shape[2] == W + F.REFINE_WIDTH and last["f"][:, :, :W].tobytes() == last["r"].tobytes()
    # the record the calls are timed on: the pose that undoes the frame's scene map (reprojection_bench's), moved 0.01 along the view axis
    moved = np.ascontiguousarray(last["r"][:, :, :26])
    sc = rbatches[-1][2]["scene"]
    for f in range(B):
        for j in range(K):
            M = np.vstack([sc[f, D.SCENE_HEAD + D.SCENE_LINK * j + 2:D.SCENE_HEAD + D.SCENE_LINK * (j + 1)].reshape(3, 4), [0, 0, 0, 1.0]])
            pose = np.diag([1.0, -1.0, 1.0, 1.0]) @ np.linalg.inv(M)
            moved[f, j, :13] = moved[f, j, 13:26] = np.concatenate([pose[:3, :3].reshape(9), [1.0], pose[:3, 3] + [0.0, 0.0, 0.01]])
    carried = torch.from_numpy(moved).to(dev)
    rigs, nf = rbatches[-1][2]["rig"], rbatches[-1][1]
    d_rig, d_nf, d_par = torch.from_numpy(rigs).to(dev), torch.from_numpy(nf).to(dev), torch.from_numpy(table).to(dev)
    tables, pred = R.predicted_frames(B, cap, "uint16", dev)
    bufs = F.refine_buffers(B, K, dev)
    R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables)
    D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2])
    calls = {"refine_pass": lambda: F.refine_pass(d_mesh, clean[0], clean[1], pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, carried,
                                                  bufs.work[0], bufs.best, bufs.sums[0]),
             "refine_rec": lambda: F.refine_rec(bufs.best, carried)}
    op_ms = {name: timed_calls(call, args.rounds, args.calls) for name, call in calls.items()}
    used = bufs.sums[0][..., 28].cpu().numpy()
    loop = lambda: F.refine_batch(d_mesh, d_rt, d_sc, d_rig, d_nf, d_geom, clean, carried, "uint16", tables, pred, d_par, args.refine, bufs)
    op_ms["whole_loop"] = timed_calls(loop, args.rounds, max(1, args.calls // 10))
    cols = F.named_columns(loop().cpu().numpy())
    sil = {}
    if args.silhouette:                                                   # the same batch and record with the term: the field, one pass, the loop
        d_spar, sbufs = torch.from_numpy(sil_table).to(dev), F.refine_buffers(B, K, dev, silhouette=True, pixel_capacity=cap)
        R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables)
        D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2])
        op_ms["silhouette_field"] = timed_calls(lambda: F.silhouette_field(clean[0], clean[1], d_geom, d_sc, K, out=sbufs.field), args.rounds, args.calls)
        op_ms["refine_pass_sil"] = timed_calls(lambda: F.refine_pass(d_mesh, clean[0], clean[1], pred, d_geom, d_sc, tables[0], d_nf, d_spar, 0, False,
                                                                     carried, sbufs.work[0], sbufs.best, sbufs.sums[0], field=sbufs.field), args.rounds, args.calls)
        s0 = sbufs.sums[0].cpu().numpy()
        sloop = lambda: F.refine_batch(d_mesh, d_rt, d_sc, d_rig, d_nf, d_geom, clean, carried, "uint16", tables, pred, d_spar, args.refine, sbufs)
        op_ms["whole_loop_sil"] = timed_calls(sloop, args.rounds, max(1, args.calls // 10))
        scols = F.named_columns(sloop().cpu().numpy())
        sil = {"silhouette": {"table": sil_table[8:11].tolist(), "launches_added": 5 * (args.refine + 1) + 2, "field_bytes_per_slot": 4 * K * cap,
                              "added_ms_per_batch_over_plain_refine": round(med["s"] - med["f"], 4), "s_over_r": round(med["s"] / med["r"], 4),
                              "overhang_rows_per_part_and_pose": float(s0[..., 33].mean()), "far_pixels_per_part_and_pose": float(s0[..., 34].mean()),
                              "median_cost_start": float(np.median(scols["baseline_cost_start"])),
                              "median_cost_best": float(np.median(scols["baseline_cost_best"])),
                              "parts_improved": int((scols["baseline_cost_best"] < scols["baseline_cost_start"]).sum()), "parts": B * K}}
    if args.coverage:                                                     # ... and with both terms: the predicted field, one pass, the loop
        d_cpar = torch.from_numpy(cov_table).to(dev)
        cbufs = F.refine_buffers(B, K, dev, silhouette=True, pixel_capacity=cap, coverage=True)
        R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables)
        D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2])
        F.silhouette_field(clean[0], clean[1], d_geom, d_sc, K, out=cbufs.field)
        op_ms["coverage_field"] = timed_calls(lambda: F.coverage_field(pred, tables[1], d_sc, K, out=cbufs.cover), args.rounds, args.calls)
        op_ms["refine_pass_cov"] = timed_calls(lambda: F.refine_pass(d_mesh, clean[0], clean[1], pred, d_geom, d_sc, tables[0], d_nf, d_cpar, 0, False,
                                                                     carried, cbufs.work[0], cbufs.best, cbufs.sums[0], field=cbufs.field,
                                                                     cover=cbufs.cover), args.rounds, args.calls)
        c0 = cbufs.sums[0].cpu().numpy()
        cloop = lambda: F.refine_batch(d_mesh, d_rt, d_sc, d_rig, d_nf, d_geom, clean, carried, "uint16", tables, pred, d_cpar, args.refine, cbufs)
        op_ms["whole_loop_cov"] = timed_calls(cloop, args.rounds, max(1, args.calls // 10))
        ccols = F.named_columns(cloop().cpu().numpy())
        sil["coverage"] = {"table": cov_table[24:27].tolist(), "launches_added": 6 * (args.refine + 1) + 2, "cover_bytes_per_slot": 8 * K * cap,
                           "added_ms_per_batch_over_silhouette": round(med["c"] - med["s"], 4), "c_over_s": round(med["c"] / med["s"], 4),
                           "c_over_r": round(med["c"] / med["r"], 4), "gap_rows_per_part_and_pose": float(c0[..., 37].mean()),
                           "far_gap_pixels_per_part_and_pose": float(c0[..., 38].mean()),
                           "median_cost_start": float(np.median(ccols["baseline_cost_start"])),
                           "median_cost_best": float(np.median(ccols["baseline_cost_best"])),
                           "parts_improved": int((ccols["baseline_cost_best"] < ccols["baseline_cost_start"]).sum()), "parts": B * K}
    if args.scale:                                                        # ... and with s solved as well: one pass and the loop, on the same batch and record
        d_gpar = torch.from_numpy(scl_table).to(dev)
        gbufs = F.refine_buffers(B, K, dev, silhouette=True, pixel_capacity=cap, coverage=True, scale=True)
        R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables)
        D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2])
        F.silhouette_field(clean[0], clean[1], d_geom, d_sc, K, out=gbufs.field)
        F.coverage_field(pred, tables[1], d_sc, K, out=gbufs.cover)
        op_ms["refine_pass_scale"] = timed_calls(lambda: F.refine_pass(d_mesh, clean[0], clean[1], pred, d_geom, d_sc, tables[0], d_nf, d_gpar, 0, False,
                                                                       carried, gbufs.work[0], gbufs.best, gbufs.sums[0], field=gbufs.field,
                                                                       cover=gbufs.cover, fitted=carried), args.rounds, args.calls)
        gloop = lambda: F.refine_batch(d_mesh, d_rt, d_sc, d_rig, d_nf, d_geom, clean, carried, "uint16", tables, pred, d_gpar, args.refine, gbufs)
        op_ms["whole_loop_scale"] = timed_calls(gloop, args.rounds, max(1, args.calls // 10))
        gcols = F.named_columns(gloop().cpu().numpy())
        sil["scale"] = {"table": scl_table[32:34].tolist(), "launches_added_over_coverage": 0,
                        "added_ms_per_batch_over_coverage": round(med["g"] - med["c"], 4), "g_over_c": round(med["g"] / med["c"], 4),
                        "g_over_r": round(med["g"] / med["r"], 4),
                        "refine_pass_scale_over_cov": round(float(np.median(op_ms["refine_pass_scale"]) / np.median(op_ms["refine_pass_cov"])), 4),
                        "median_s_kept_over_s_fitted": float(np.median(gcols["baseline_s"] / moved[:, :, 9])),
                        "median_cost_start": float(np.median(gcols["baseline_cost_start"])),
                        "median_cost_best": float(np.median(gcols["baseline_cost_best"])),
                        "parts_improved": int((gcols["baseline_cost_best"] < gcols["baseline_cost_start"]).sum()), "parts": B * K}
    frames = D._cut_frames(clean[0].cpu().numpy().view(np.uint16), clean[1].cpu().numpy(), d_geom.cpu().numpy(), "uint16")
    eager = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        D.refine_frames(mesh, rbatches[-1][2]["render"], sc, rigs, nf, moved, frames, "uint16", table, device=dev)
        eager.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"metric": "render-and-compare ICP: ms per batch of the rendered stream without (r) and with (f) refine=pack_refine(iters=N); ms "
                                "per call of ancsh_refine_pass, ancsh_refine_rec and the whole loop alone on one batch; ms of the eager operator",
                      "device": torch.cuda.get_device_name(0), "iters": args.refine, "launches_added": 5 * (args.refine + 1) + 1,
                      "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "stream_frames_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "added_ms_per_batch": round(med["f"] - med["r"], 4),
                      "f_over_r": round(med["f"] / med["r"], 4), "operator_ms_per_batch": {k: round(float(np.median(v)), 4) for k, v in op_ms.items()},
                      "operator_ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in op_ms.items()},
                      "eager_operator_ms": [round(x, 3) for x in eager],
                      "operator_record": {"pixels_used_per_part_and_pose": float(used.mean()), "median_cost_start": float(np.median(cols["baseline_cost_start"])),
                                          "median_cost_best": float(np.median(cols["baseline_cost_best"])),
                                          "parts_improved": int((cols["baseline_cost_best"] < cols["baseline_cost_start"]).sum()), "parts": B * K},
                      "streamed_last_batch": {"parts": B * K, "parts_with_a_finite_refined_pose": int(np.isfinite(F.named_columns(last["f"])["baseline_s"]).sum())},
                      "crop_pixels_per_frame": args.side * args.side, "triangles": int(mesh[1].shape[0]), **sil,
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(rbatches) * B,
                                "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


def joints_bench(args, K, B, N, dev, mesh, d_mesh):
    """--refine N --joints: the posed stream with refine=pack_refine(iters=N) without and with joints=, alternated; then the new launch alone and
    the whole loop with it on the last batch, with a record that draws part j (j - 1) * 0.01 off its place along the view axis."""
    from articulated_pose_amd.pose import refinement as F, reprojection as R
    rs, side = np.random.RandomState(1), args.side
    t, near, far = np.tan(np.radians(20.0)), 0.1, 100.0
    P = np.array([[1.0 / t, 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1.0, 0]])
    zero = np.zeros((3, 3))
    kin = D.pack_kinematics(P, side, side, [-1, 0, 0], ["fixed", "revolute", "prismatic"], [(0, 0, 0), (0.3, 0.02, 0.12), (-0.34, -0.03, 0.02)],
                            [(0, 0, 0)] * 3, [(0, 0, 0), (0, 1, 0), (1, 0, 0)], zero, zero, zero[:2], [[0], [1], [2]], depth_scale=SCALE)
    crops = [(side, side, (0, 0))] * B
    nf, rigs, jf = np.ones(B, np.float32), np.tile(identity_rig(K), (B, 1)), rs.normal(size=(B, 13))
    batches = []
    for _ in range(args.frames // B):
        ps = []
        for _ in range(B):
            V = np.eye(4)
            V[:3, :3] = D._rotation_from_rpy(*rs.uniform(-0.5, 0.5, 3))[:3, :3]
            V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
            ps.append(D.pack_pose([0.0, rs.uniform(0.1, 1.2), rs.uniform(-0.03, 0.03)], V))
        batches.append((crops, nf, dict(pose=np.stack(ps), rig=rigs, frame=jf)))
    geom = np.zeros((B, D.GEOM_WORDS), np.int32)
    cap = D.pack_crop_geometry([c[:2] for c in crops], [c[2] for c in crops], geom)
    tables_off, tables_on = F.pack_refine(iters=args.refine), F.pack_refine(iters=args.refine, joints=dict(weight=1.0, axis_length=0.5))
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16", render_mesh=mesh, kinematics=kin)
    pipes = {"f": AncshPipeline(K, wa, wn, B, N, dev, refine=tables_off, **kw).prepare(),
             "j": AncshPipeline(K, wa, wn, B, N, dev, refine=tables_on, **kw).prepare()}
    torch.cuda.synchronize()
    last = {}

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        for got in pipes[name].stream_posed_batches(batches[k] for _ in range(passes) for k in range(len(batches))):
            n += 1
        torch.cuda.synchronize()
        last[name] = got[2]
        return 1e3 * (time.perf_counter() - t0) / n

    for name in "fj":
        leg(name, 1)
    ms = {name: [] for name in "fj"}
    for r in range(args.rounds):
        for name in ("fj", "jf")[r % 2]:                                  # the order swaps from round to round: neither leg is always first
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    W = last["f"].shape[2] - F.REFINE_WIDTH
    assert last["j"].shape == last["f"].shape and last["j"][:, :, :W].tobytes() == last["f"][:, :, :W].tobytes()
    # the last batch on device tensors: its own tables, its rendered frames, and the record that undoes each scene map, part j moved (j - 1) * 0.01
    rt, sc = D.pose_scene_tables(kin, batches[-1][2]["pose"], dev)
    d_geom, d_rt, d_sc = torch.from_numpy(geom).to(dev), torch.from_numpy(rt).to(dev), torch.from_numpy(sc).to(dev)
    clean = (torch.zeros(cap, dtype=torch.int16, device=dev), torch.zeros(cap, dtype=torch.uint8, device=dev))
    D.render_depth(d_mesh, d_geom, d_rt, "uint16", out=clean, scratch=torch.zeros(cap, dtype=torch.int64, device=dev))
    moved = np.zeros((B, K, 26))
    for f in range(B):
        for j in range(K):
            M = np.vstack([sc[f, D.SCENE_HEAD + D.SCENE_LINK * j + 2:D.SCENE_HEAD + D.SCENE_LINK * (j + 1)].reshape(3, 4), [0, 0, 0, 1.0]])
            pose = np.diag([1.0, -1.0, 1.0, 1.0]) @ np.linalg.inv(M)
            moved[f, j, :13] = moved[f, j, 13:26] = np.concatenate([pose[:3, :3].reshape(9), [1.0], pose[:3, 3] + [0.0, 0.0, 0.01 * (j - 1)]])
    carried = torch.from_numpy(moved).to(dev)
    d_rig, d_nf, d_kin = torch.from_numpy(rigs).to(dev), torch.from_numpy(nf).to(dev), torch.from_numpy(kin).to(dev)
    d_par = torch.from_numpy(tables_on).to(dev)
    tables, pred = R.predicted_frames(B, cap, "uint16", dev)
    bufs = F.refine_buffers(B, K, dev, passes=args.refine + 1, joints=True)
    loop = lambda: F.refine_batch(d_mesh, d_rt, d_sc, d_rig, d_nf, d_geom, clean, carried, "uint16", tables, pred, d_par, args.refine, bufs, kin=d_kin)
    op_ms = {"whole_loop_joints": timed_calls(loop, args.rounds, max(1, args.calls // 10))}
    obj = bufs.obj.cpu().numpy()
    R.reproject_scene_build(d_rt, d_sc, d_rig, d_nf, carried, d_geom, cap, out=tables)
    D.render_depth(d_mesh, tables[1], tables[0], "uint16", out=pred[:2], scratch=pred[2])
    F.refine_pass(d_mesh, clean[0], clean[1], pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, carried, bufs.work[0], bufs.best, bufs.sums[0])
    step = lambda: F.refine_joint_step(d_kin, d_sc, tables[0], d_nf, d_par, 0, False, carried, bufs.sums[0], bufs.work[0], bufs.best, bufs.state, bufs.obj[0])
    op_ms["refine_joint_step"] = timed_calls(step, args.rounds, args.calls)
    fell = obj[-1, :, :, 7] < obj[0, :, :, 7]
    print(json.dumps({"metric": "the joint step of render-and-compare ICP: ms per batch of the posed stream with refine=pack_refine(iters=N) without (f) "
                                "and with (j) joints=; ms per call of ancsh_refine_joint_step and of the whole loop with it on one batch",
                      "device": torch.cuda.get_device_name(0), "iters": args.refine, "launches_added": args.refine + 1,
                      "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "added_ms_per_batch": round(med["j"] - med["f"], 4), "j_over_f": round(med["j"] / med["f"], 4),
                      "operator_ms_per_batch": {k: round(float(np.median(v)), 4) for k, v in op_ms.items()},
                      "operator_ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in op_ms.items()},
                      "operator_record": {"objects": int(fell.size), "objects_whose_gap_rms_fell": int(fell.sum()),
                                          "share": round(float(fell.mean()), 4), "active_joints_per_object": float(obj[0, :, :, 5].mean()),
                                          "passes_the_step_solved": float(obj[:-1, :, :, 6].mean()),
                                          "median_gap_rms_first_pass": float(np.median(obj[0, :, :, 7])),
                                          "median_gap_rms_last_pass": float(np.median(obj[-1, :, :, 7])),
                                          "objects_whose_cost_fell": int((obj[-1, :, :, 1] < obj[-1, :, :, 0]).sum())},
                      "streamed_last_batch": {name: {"parts_with_a_finite_refined_pose": int(np.isfinite(F.named_columns(last[name])["baseline_s"]).sum()),
                                                     "pixels_used_at_the_kept_pose": float(np.nansum(F.named_columns(last[name])["baseline_n_used"])),
                                                     "passes_solved": float(np.nanmean(F.named_columns(last[name])["baseline_passes_solved"]))}
                                              for name in "fj"},
                      "crop_pixels_per_frame": side * side, "triangles": int(mesh[1].shape[0]),
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(batches) * B,
                                "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sensor", action="store_true", help="measure the depth sensor model instead of the renderer")
    ap.add_argument("--reprojection", action="store_true", help="measure render-and-compare (reprojection=True) instead of the renderer")
    ap.add_argument("--refine", type=int, default=0, metavar="N", help="measure render-and-compare ICP (refine=pack_refine(iters=N)) instead of the renderer")
    ap.add_argument("--silhouette", action="store_true", help="with --refine N: measure the silhouette term as well (a third leg and its launches)")
    ap.add_argument("--coverage", action="store_true", help="with --refine N --silhouette: measure the coverage term as well (a fourth leg and its launches)")
    ap.add_argument("--scale", action="store_true", help="with --refine N --silhouette --coverage: measure the scale unknown as well (a fifth leg beside the coverage-only stream)")
    ap.add_argument("--joints", action="store_true", help="with --refine N: measure the joint step on the posed stream (joints= off and on, alternated)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=4, help="passes over the frames per timed leg")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--side", type=int, default=128, help="the image and the crop: side x side pixels")
    ap.add_argument("--tess", type=int, default=8, help="quads per box edge: 12 tess^2 triangles per link")
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls of the operator between its two events")
    args = ap.parse_args()
    if args.scale and not (args.refine and args.silhouette and args.coverage):
        ap.error("--scale goes with --refine N --silhouette --coverage: the scale unknown runs with both pixel terms")
    if args.coverage and not (args.refine and args.silhouette):
        ap.error("--coverage goes with --refine N --silhouette: the coverage term runs with the silhouette term")
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    mesh = D.pack_mesh([tessellated_box(LO, HI, args.tess)] * K)
    if args.refine and args.joints:
        return joints_bench(args, K, B, N, dev, mesh, D.mesh_to_device(mesh, dev))
    crops = [(args.side, args.side, (0, 0))] * B
    nf, rigs, jf = np.ones(B, np.float32), np.tile(identity_rig(K), (B, 1)), rs.normal(size=(B, 13))
    rbatches, dbatches, valid = [], [], []
    for _ in range(args.frames // B):
        tables = [make_scene(rs, args.side) for _ in range(B)]
        rt, sc = np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables])
        frames = D.render_depth_frames(mesh, rt, crops, "uint16", dev)
        valid.append(np.mean([(f[1] != D.NOT_OBJECT).sum() for f in frames]))
        rbatches.append((crops, nf, dict(render=rt, scene=sc, rig=rigs, frame=jf)))
        dbatches.append((frames, nf, dict(scene=sc, rig=rigs, frame=jf)))
    # the operator alone, on the last batch
    d_mesh = D.mesh_to_device(mesh, dev)
    geom = np.zeros((B, D.GEOM_WORDS), np.int32)
    cap = D.pack_crop_geometry([c[:2] for c in crops], [c[2] for c in crops], geom)
    d_geom, d_rt = torch.from_numpy(geom).to(dev), torch.from_numpy(rt).to(dev)
    out = (torch.zeros(cap, dtype=torch.int16, device=dev), torch.zeros(cap, dtype=torch.uint8, device=dev))
    zbuf = torch.zeros(cap, dtype=torch.int64, device=dev)
    if args.sensor:
        D.render_depth(d_mesh, d_geom, d_rt, "uint16", out=out, scratch=zbuf)
        return sensor_bench(args, K, B, N, dev, mesh, rbatches, d_geom, torch.from_numpy(sc).to(dev), out, cap)
    if args.reprojection:
        D.render_depth(d_mesh, d_geom, d_rt, "uint16", out=out, scratch=zbuf)
        return reprojection_bench(args, K, B, N, dev, mesh, d_mesh, rbatches, d_geom, d_rt, torch.from_numpy(sc).to(dev), out, cap)
    if args.refine:
        D.render_depth(d_mesh, d_geom, d_rt, "uint16", out=out, scratch=zbuf)
        return refine_bench(args, K, B, N, dev, mesh, d_mesh, rbatches, d_geom, d_rt, torch.from_numpy(sc).to(dev), out, cap)
    op_ms = timed_calls(lambda: D.render_depth(d_mesh, d_geom, d_rt, "uint16", out=out, scratch=zbuf), args.rounds, args.calls)
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16")
    rendered = AncshPipeline(K, wa, wn, B, N, dev, render_mesh=mesh, **kw).prepare()
    annotated = AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare()
    torch.cuda.synchronize()

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        gen = (rendered.stream_render_batches(rbatches[k] for _ in range(passes) for k in range(len(rbatches))) if name == "r" else
               annotated.stream_depth_batches(dbatches[k] for _ in range(passes) for k in range(len(dbatches))))
        for _ in gen:
            n += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n          # ms per batch of B frames, steady state over the slots

    for name in "rd":                                         # warm-up: every slot replayed with real input
        leg(name, 1)
    ms = {name: [] for name in "rd"}
    for _ in range(args.rounds):
        for name in "rd":
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    op = float(np.median(op_ms))
    print(json.dumps({"metric": "frames/s: the renderer alone; the rendered stream (r) vs the annotated depth stream fed the same frames from the host (d)",
                      "device": torch.cuda.get_device_name(0), "operator_frames_per_s": round(1e3 * B / op, 1), "operator_ms_per_batch": round(op, 4),
                      "operator_ms_per_batch_rounds": [round(x, 4) for x in op_ms],
                      "stream_frames_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "r_over_d": round(med["r"] / med["d"], 4),
                      "h2d_bytes_per_batch_r": B * (4 * D.GEOM_WORDS + 8 * D.RENDER_WIDTH + 8 * D.SCENE_WIDTH),
                      "h2d_bytes_per_batch_d": B * (4 * D.GEOM_WORDS + 8 * D.SCENE_WIDTH) + 3 * cap,
                      "object_pixels_per_frame": round(float(np.mean(valid)), 1), "crop_pixels_per_frame": args.side * args.side,
                      "triangles": int(mesh[1].shape[0]), "vertices": int(mesh[0].shape[0]),
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(rbatches) * B,
                                "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


if __name__ == "__main__":
    main()
