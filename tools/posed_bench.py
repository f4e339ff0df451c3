"""What building the per-frame tables costs, on the host and on the device: AncshPipeline(..., render_mesh=mesh, kinematics=kin), whose step
builds its render and scene tables from one pose per frame (ancsh_pose_scene_build) and centres its crops (ancsh_render_centre_crops),
against the rendered stream fed tables from depth.pack_render_scene / depth.pack_frame_scene, at tools/render_bench.py's object, frames and
shape (K = 3, 32 x 1024, 10000 / 200 hypotheses, couple=True, synthetic weights, predicted joints).  Measured:
  a: microseconds per frame of the two host packers, one core of this machine (--pack-calls calls each);
  e: the two new entries alone, back to back, on one batch of 32 frames (HIP events around --calls pairs);
  three legs, alternated in one process for --rounds rounds:
    b: the rendered stream, its tables packed BEFORE the clock starts (tools/render_bench.py's leg r);
    c: the same stream, its tables packed inside the loop, one frame at a time: what a user of render_mesh= pays without the new entries;
    d: the posed stream on the same views and joint values (the poses are 32 doubles each, made before the clock; submit_posed's checks
       run inside it).
--instances N (default 1: one object, the single-object entries): N > 1 builds a library of N distinct instances -- boxes of tess - 1, tess and
tess + 1 quads per edge in turn, so their triangle counts are unequal and their mean stays near one object's, each with its own hinge
position -- and mixes them within every batch (frame f of batch b shows instance (f + b) mod N); the streams then go through the *_lib
entries.  --library takes that path for --instances 1 too: the same work through the library's code.  --idle-tess T appends one more instance
of T quads per edge that no frame shows: it only raises Tmax, the size of the raster grid, so every frame launches idle waves up to it --
leg r, the renderer alone on one batch (HIP events around --calls calls), and leg d with and without it give what those waves cost.
--images: what annotated_images=True costs.  The timed legs are then the posed stream three ways, alternated in one process: d as above; j
on a pipeline built with annotated_images=True whose stream does not ask for the images (the step's two more launches and the images'
device-to-host copies are paid, the host never touches them); i on that pipeline with stream_posed_batches(..., annotated_images=True) (the
host also cuts every batch's four image buffers into per-frame arrays); and the option's two launches alone, HIP events around each in an
eager step of the same pipeline (three lead launches of the entry in front of the timed one).
--joint-values: what joint_values=True costs.  The timed legs are then the posed stream two ways, alternated in one process: d as above; v on
a pipeline built with joint_values=True (the step's one more launch, ancsh_joint_values_rec, and a 36-column articulation block to copy out);
and that launch alone on slot 0's buffers, HIP events around --calls back-to-back calls.
Prints one JSON line: a record, not a gate.

    python tools/posed_bench.py [--rounds 3] [--passes 4] [--slots 8] [--frames 320] [--side 128] [--tess 8] [--instances 1] [--library] [--idle-tess 0] [--images | --joint-values]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import articulated_pose_amd  # noqa: E402,F401
from articulated_pose_amd import depth as D  # noqa: E402
from articulated_pose_amd.dataset import identity_rig  # noqa: E402
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402
from render_bench import HI, LO, SCALE, tessellated_box  # noqa: E402

ZERO = np.zeros((3, 3))
PARTS = [[0], [1], [2]]


def projection():
    t, near, far = np.tan(np.radians(20.0)), 0.1, 100.0
    return np.array([[1.0 / t, 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1.0, 0]])


def make_frame(rs):
    """One frame of render_bench's three-link object: (the view matrix, the opening of link 1's hinge)."""
    V = np.eye(4)
    V[:3, :3] = D._rotation_from_rpy(*rs.uniform(-0.5, 0.5, 3))[:3, :3]
    V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
    return V, rs.uniform(0.1, 1.2)


def hinge(i):
    """Where instance i's link 1 hangs: instance 0 is render_bench's object, every further one has its hinge 5 mm further out."""
    return (0.3 + 0.005 * i, 0.02, 0.12)


def host_tables(P, V, opening, side, i=0):
    """The two host packers on the link poses the reference takes from its simulator, for instance i."""
    pos = np.array([[0.0, 0.0, 0.0], hinge(i), [-0.34, -0.03, 0.02]])
    orn = np.array([[0, 0, 0, 1.0], [0, np.sin(opening / 2), 0, np.cos(opening / 2)], [0, 0, np.sin(0.2), np.cos(0.2)]])
    return (D.pack_render_scene(V, P, pos, orn, side, side, depth_scale=SCALE, instance=i),
            D.pack_frame_scene(V, P, pos, orn, ZERO, ZERO, ZERO[:2], PARTS, side, side, depth_scale=SCALE))


def kinematics(P, side, i=0):
    """The same object as a tree: link 1 hinged about y beside link 0, link 2 fixed on the other side, turned 0.4 about z."""
    return D.pack_kinematics(P, side, side, [-1, 0, 0], ["fixed", "revolute", "fixed"], [(0, 0, 0), hinge(i), (-0.34, -0.03, 0.02)],
                             [(0, 0, 0), (0, 0, 0), (0, 0, 0.4)], [(0, 0, 0), (0, 1, 0), (0, 0, 0)], ZERO, ZERO, ZERO[:2], PARTS, depth_scale=SCALE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=4, help="passes over the frames per timed leg")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--side", type=int, default=128, help="the image and the crop: side x side pixels")
    ap.add_argument("--tess", type=int, default=8, help="quads per box edge: 12 tess^2 triangles per link")
    ap.add_argument("--calls", type=int, default=200, help="back-to-back pairs of the two entries between their two events")
    ap.add_argument("--pack-calls", type=int, default=300, help="calls of each host packer for leg a")
    ap.add_argument("--instances", type=int, default=1, help="instances mixed within every batch; above 1: a library through the *_lib entries")
    ap.add_argument("--library", action="store_true", help="take the library's path for --instances 1 too")
    ap.add_argument("--idle-tess", type=int, default=0, help="append an instance of this many quads per edge that no frame shows (a library only)")
    ap.add_argument("--images", action="store_true", help="time the posed stream with and without annotated_images=True (legs d, j, i)")
    ap.add_argument("--joint-values", action="store_true", help="time the posed stream with and without joint_values=True (legs d, v)")
    args = ap.parse_args()
    if args.images and args.joint_values:
        ap.error("--images and --joint-values each replace the timed legs: pass one of them")
    K, B, N, dev = 3, 32, 1024, torch.device("cuda:0")
    rs = np.random.RandomState(0)
    P, side, ninst = projection(), args.side, args.instances
    if not 1 <= ninst <= D.LIBRARY_MAX_INSTANCES or args.tess < 2:
        ap.error("--instances must be in [1, %d] and --tess >= 2" % D.LIBRARY_MAX_INSTANCES)
    library = ninst > 1 or args.library or args.idle_tess > 0
    tess = [args.tess + (i % 3 - 1 if ninst > 1 else 0) for i in range(ninst)]
    meshes = [D.pack_mesh([tessellated_box(LO, HI, t)] * K) for t in tess + [args.idle_tess] * (args.idle_tess > 0)]
    mesh = D.pack_mesh_library(meshes) if library else meshes[0]
    kin = np.stack([kinematics(P, side, i) for i in range(len(meshes))]) if library else kinematics(P, side)
    crops = [(side, side, (0, 0))] * B
    nf, rigs, jf = np.ones(B, np.float32), np.tile(identity_rig(K), (B, 1)), rs.normal(size=(B, 13))
    views, tbatches, pbatches = [], [], []
    for b in range(args.frames // B):
        frames = [make_frame(rs) + ((f + b) % ninst,) for f in range(B)]
        tables = [host_tables(P, V, o, side, i) for V, o, i in frames]
        views.append(frames)
        tbatches.append((crops, nf, dict(render=np.stack([t[0] for t in tables]), scene=np.stack([t[1] for t in tables]), rig=rigs, frame=jf)))
        pbatches.append((crops, nf, dict(pose=np.stack([D.pack_pose([0.0, o, 0.0], V, instance=i) for V, o, i in frames]), rig=rigs, frame=jf)))
    # the device's tables against the host packers', on the last batch
    rt, sc = D.pose_scene_tables(kin, pbatches[-1][2]["pose"], dev)
    parity = max(float(np.abs(rt - tbatches[-1][2]["render"]).max()), float(np.abs(sc - tbatches[-1][2]["scene"]).max()))
    # a: the host packers
    V, o, _ = views[0][0]
    pos = np.array([[0.0, 0.0, 0.0], [0.3, 0.02, 0.12], [-0.34, -0.03, 0.02]])
    orn = np.array([[0, 0, 0, 1.0], [0, np.sin(o / 2), 0, np.cos(o / 2)], [0, 0, np.sin(0.2), np.cos(0.2)]])
    t0 = time.perf_counter()
    for _ in range(args.pack_calls):
        D.pack_render_scene(V, P, pos, orn, side, side, depth_scale=SCALE)
    t1 = time.perf_counter()
    for _ in range(args.pack_calls):
        D.pack_frame_scene(V, P, pos, orn, ZERO, ZERO, ZERO[:2], PARTS, side, side, depth_scale=SCALE)
    t2 = time.perf_counter()
    pack_us = {"pack_render_scene": 1e6 * (t1 - t0) / args.pack_calls, "pack_frame_scene": 1e6 * (t2 - t1) / args.pack_calls}
    # e: the two entries alone
    d_mesh, d_kin, d_pose = D.mesh_to_device(mesh, dev), torch.from_numpy(kin).to(dev), torch.from_numpy(pbatches[-1][2]["pose"]).to(dev)
    geom = np.zeros((B, D.GEOM_WORDS), np.int32)
    cap = D.pack_crop_geometry([c[:2] for c in crops], np.full((B, 2), D.CROP_CENTRE, np.int64), geom)
    h_geom = torch.from_numpy(geom).pin_memory()
    d_geom = h_geom.to(dev)
    out = (torch.zeros((B, D.RENDER_WIDTH), dtype=torch.float64, device=dev), torch.zeros((B, D.SCENE_WIDTH), dtype=torch.float64, device=dev))
    bounds = torch.zeros((B, 4), dtype=torch.int32, device=dev)

    def pair():                                               # every crop asks for its centre again: the second entry does its whole work
        d_geom.copy_(h_geom, non_blocking=True)
        D.pose_scene_build(d_kin, d_pose, out=out)
        D.centre_crop_origins(d_mesh, d_geom, out[0], scratch=bounds)
    for _ in range(20):
        pair()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    op_ms = []
    for _ in range(args.rounds):
        e0.record()
        for _ in range(args.calls):
            pair()
        e1.record()
        torch.cuda.synchronize()
        op_ms.append(e0.elapsed_time(e1) / args.calls)
    # r: the renderer alone, on the tables and origins the pair left behind
    pix, zbuf = (torch.zeros((cap,), dtype=torch.int16, device=dev), torch.zeros((cap,), dtype=torch.uint8, device=dev)), torch.zeros((cap,), dtype=torch.int64, device=dev)
    render_ms = []
    for k in range(args.rounds + 1):
        e0.record()
        for _ in range(args.calls):
            D.render_depth(d_mesh, d_geom, out[0], "uint16", out=pix, scratch=zbuf)
        e1.record()
        torch.cuda.synchronize()
        if k:                                                 # the first round warms up
            render_ms.append(e0.elapsed_time(e1) / args.calls)
    wa, wn = synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    kw = dict(couple=True, slots=args.slots, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
              depth_capacity=cap, depth_dtype="uint16", render_mesh=mesh)
    rendered = None if args.images or args.joint_values else AncshPipeline(K, wa, wn, B, N, dev, **kw).prepare()
    posed = AncshPipeline(K, wa, wn, B, N, dev, kinematics=kin, **kw).prepare()
    imaged = AncshPipeline(K, wa, wn, B, N, dev, kinematics=kin, annotated_images=True, **kw).prepare() if args.images else None
    valued = AncshPipeline(K, wa, wn, B, N, dev, kinematics=kin, joint_values=True, **kw).prepare() if args.joint_values else None
    torch.cuda.synchronize()

    def packed_in_the_loop(passes):
        for _ in range(passes):
            for frames in views:
                tables = [host_tables(P, V, o, side, i) for V, o, i in frames]
                yield crops, nf, dict(render=np.stack([t[0] for t in tables]), scene=np.stack([t[1] for t in tables]), rig=rigs, frame=jf)

    def leg(name, passes):
        t0, n = time.perf_counter(), 0
        poses = (pbatches[k] for _ in range(passes) for k in range(len(pbatches)))
        gen = (rendered.stream_render_batches(tbatches[k] for _ in range(passes) for k in range(len(tbatches))) if name == "b" else
               rendered.stream_render_batches(packed_in_the_loop(passes)) if name == "c" else
               posed.stream_posed_batches(poses) if name == "d" else valued.stream_posed_batches(poses) if name == "v" else imaged.stream_posed_batches(poses, annotated_images=name == "i"))
        for _ in gen:
            n += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n          # ms per batch of B frames, steady state over the slots

    legs = "dji" if args.images else "dv" if args.joint_values else "bcd"
    for name in legs:                                         # warm-up: every slot replayed with real input
        leg(name, 1)
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            ms[name].append(leg(name, args.passes))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    op = float(np.median(op_ms))
    two = {"ancsh_raw_point_labels": [], "ancsh_depth_annotated_images": []}
    if args.images:                                           # the two launches alone: an eager step, events around every ABI call
        from articulated_pose_amd import _lib
        eager = AncshPipeline(K, wa, wn, B, N, dev, kinematics=kin, annotated_images=True, use_graph=False, **dict(kw, slots=1))
        for k in range(args.rounds + 3):
            if k >= 2:                                        # two passes warm up
                _lib.profile_start(lead_for={name: 3 for name in two})
            eager.submit_posed(pbatches[0][0], pbatches[0][1], **pbatches[0][2])
            for name, _, call_ms in (_lib.profile_stop() if k >= 2 else ()):
                if name in two:
                    two[name].append(call_ms)
            eager.retire()
    value_ms = []
    if args.joint_values:                                     # the launch alone, on the buffers slot 0's last replay left behind
        from articulated_pose_amd.pose.joint_values import JOINT_VALUES_WIDTH, joint_values_batch
        sl = valued.slots[0]
        art = sl.out["articulation"][:, :, :12].contiguous()
        wide = torch.empty((B, K, 12 + JOINT_VALUES_WIDTH), dtype=torch.float64, device=dev)
        for k in range(args.rounds + 1):
            e0.record()
            for _ in range(args.calls):
                joint_values_batch(valued.kin, sl.render, sl.scene, sl.rig, sl.header(B)[2], sl.out["record"], art, pose=sl.pose, out=wide)
            e1.record()
            torch.cuda.synchronize()
            if k:                                             # the first round warms up
                value_ms.append(e0.elapsed_time(e1) / args.calls)
    ratios = (dict(v_over_d=round(med["v"] / med["d"], 4), joint_values_ms_per_batch=round(med["v"] - med["d"], 4),
                   joint_values_launch_us=round(1e3 * float(np.median(value_ms)), 2), joint_values_launch_us_rounds=[round(1e3 * x, 2) for x in value_ms],
                   joint_values_d2h_bytes_per_batch=8 * B * K * JOINT_VALUES_WIDTH) if args.joint_values else
              dict(j_over_d=round(med["j"] / med["d"], 4), i_over_d=round(med["i"] / med["d"], 4), images_ms_per_batch=round(med["i"] - med["d"], 4),
                   images_d2h_bytes_per_batch=60 * cap, images_pinned_bytes=60 * cap * args.slots,
                   images_launch_us={k: round(1e3 * float(np.median(v)), 2) for k, v in two.items()},
                   images_launch_us_rounds={k: [round(1e3 * x, 2) for x in v] for k, v in two.items()}) if args.images else
              dict(d_over_b=round(med["d"] / med["b"], 4), d_over_c=round(med["d"] / med["c"], 4)))
    print(json.dumps({"metric": "frames/s: the rendered stream with tables packed before the clock (b) and inside the loop (c) vs the posed stream (d); "
                                "the host packers (a) and the two new entries alone (e); --images: the posed stream (d) vs the same stream built "
                                "with annotated_images=True, not asked for (j) and asked for (i); --joint-values: the posed stream (d) vs the same stream built "
                                "with joint_values=True (v)",
                      "device": torch.cuda.get_device_name(0), "host_pack_us_per_frame": {k: round(v, 1) for k, v in pack_us.items()},
                      "host_pack_frames_per_s_one_core": round(1e6 / sum(pack_us.values()), 1),
                      "entries_us_per_batch": round(1e3 * op, 2), "entries_us_per_batch_rounds": [round(1e3 * x, 2) for x in op_ms],
                      "entries_frames_per_s": round(1e3 * B / op, 1),
                      "render_us_per_batch": round(1e3 * float(np.median(render_ms)), 2), "render_us_per_batch_rounds": [round(1e3 * x, 2) for x in render_ms],
                      "stream_frames_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_batch_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      **ratios,
                      "h2d_bytes_per_batch_b": B * (4 * D.GEOM_WORDS + 8 * D.RENDER_WIDTH + 8 * D.SCENE_WIDTH),
                      "h2d_bytes_per_batch_d": B * (4 * D.GEOM_WORDS + 8 * D.POSE_WIDTH),
                      "max_abs_device_minus_host_tables": parity, "triangles": int(mesh[1].shape[0]), "vertices": int(mesh[0].shape[0]),
                      "instances": ninst, "library": library, "triangles_per_instance": [int(m[1].shape[0]) for m in meshes], "idle_tess": args.idle_tess,
                      "mean_triangles_per_frame": round(float(np.mean([meshes[i][1].shape[0] for fr in views for _, _, i in fr])), 1),
                      "shape": {"K": K, "B": B, "N": N, "niter_a": 10000, "niter_b": 200, "slots": args.slots, "frames": len(tbatches) * B,
                                "side": side, "passes": args.passes, "rounds": args.rounds, "calls": args.calls}}))


if __name__ == "__main__":
    main()
