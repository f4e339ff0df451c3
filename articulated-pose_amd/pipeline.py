"""End-to-end hot path for a batch of depth point clouds on one MI355X:

    ANCSH forward  (joint axes / association heads)        main.py --test --nocs_type=ancsh
    NPCS  forward  (part-NOCS + part masks, the "baseline" network the pose stage reads when
                    USE_BASELINE, evaluation/parallel_ancsh_pose.py:232-237)   main.py --test --nocs_type=npcs
    pose fit       (per-part RANSAC + articulated LM)      evaluation/pose_multi_process.py

The whole step is ~100 asynchronous launches on one HIP stream; `AncshPipeline` captures them once
into a hipGraph and replays it per batch.  With `raw_capacity` set the captured step starts from raw clouds of any size
(sampled on the GPU) and draws a fresh RANSAC sample stream per batch: submit() / retire() / stream_batches().
"""
import collections

import numpy as np
import torch

from .network import Network
from .pose import PoseSolver
from .stream import (ALL_INPUTS, EVERY_INPUT, JOINT_SOURCES, OPTION_FLAGS, SIDE, SIDE_INPUTS, Output, check_built_with, check_joint_source, check_options,  # noqa: F401
                     check_side_inputs, fill_rows, header_layout, label_buffers, pack_results, patch_dense, per_pixel, per_raw_row, pump,
                     refuse_built_frame, refuse_side_inputs, require_side_inputs, side_host, split_item, stage_side_input, take_annotated_images,
                     take_dense, take_images)


def check_hardware_queues(slots):
    """Every batch in flight sits on its own HIP stream; streams share the process's hardware queues, and where there are fewer
    queues than batches in flight a 1.6 ms stage-B kernel of one batch holds back other batches' kernels queued behind it.  The
    HIP runtime reads GPU_MAX_HW_QUEUES once, when it initialises; the host owns that setting and the package never changes it.
    Called by AncshPipeline: warns when the setting (unset: the runtime's default of 4) is below the slot count.  Returns the
    value the host set (None = unset / not an integer)."""
    import os
    import warnings
    raw = os.environ.get("GPU_MAX_HW_QUEUES")
    try:
        cur = int(raw) if raw not in (None, "") else None
    except ValueError:
        warnings.warn("GPU_MAX_HW_QUEUES=%r is not an integer: ignored by this check (the HIP runtime decides what it makes of it)" % raw)
        cur = None
    have = 4 if cur is None else cur
    if have < slots:
        warnings.warn("AncshPipeline(slots=%d) on %d hardware queues (GPU_MAX_HW_QUEUES): batches in flight share hardware queues and "
                      "wait behind each other's long pose kernels" % (slots, have))
    return cur


def f16x2_weight_violations(nets):
    """The weight half of the F16x2 range guard (the kernels check the activations): every kernel the F16x2 path packs -- all rows of
    every layer the split-16 launches run, except layer2/conv0's feature rows 3.. and fa_layer1/conv_0's rows ..1023, which stay f32
    (per-point partial sums, the single-source share) -- against f16's largest value.  nets = [(label, Network)];
    -> [(label:layer, max |w|)] with |w| > 65504 (NaN ignored).  Host-side, no GPU needed."""
    from .pointnet_util import f16_range_violations
    from .weights import layer_table
    kernels = []
    for label, net in nets:
        for full, cin, cout, _bn, _kind in layer_table(net.n_max_parts, net.is_mixed, net.early_split_nocs, net.scope):
            w = net.weights.get(full + "/weights")
            if w is None:
                continue
            w = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w).reshape(-1, np.shape(w)[-1])
            if full.endswith("/layer2/conv0"):
                w = w[:3]
            elif full.endswith("/fa_layer1/conv_0"):
                w = w[1024:]
            kernels.append(("%s:%s" % (label, full), w))
    return f16_range_violations(kernels)


def check_joint_inputs(joint_source, couple, joint_cls, pred):
    """The joint association a load_inputs() call must carry, checked before anything is copied: "gt" needs joint_cls (a label per
    point); "predicted" with couple=False needs pred["index_per_point"] (the ANCSH network's index head, (B, N, C)); "predicted" with
    couple=True reads the head from the step's own forward and needs neither.  ValueError otherwise."""
    check_joint_source(joint_source)
    if joint_source == "gt":
        if joint_cls is None:
            raise ValueError("joint_source='gt' fits the joints from joint_cls: load_inputs(P, joint_cls, ...) needs it")
    elif not couple and (pred is None or pred.get("index_per_point") is None):
        raise ValueError("joint_source='predicted' with couple=False reads the joint association from pred['index_per_point']: "
                         "load_inputs(P, None, pred=...) must include it")


class _Slot(object):
    """Buffers + stream + captured graph of one batch in flight."""

    def __init__(self, B, N, K, device, opts):
        f = dict(dtype=torch.float32, device=device)
        self.record_width, self.art_width = opts.record_width, opts.art_width      # columns of a streamed record row / of a row of the articulation block
        self.P = torch.zeros((B, N, 3), **f)
        self.joint_cls = torch.zeros((B, N), dtype=torch.int32, device=device)
        self.pred_nocs = torch.zeros((B, N, 3 * K), **f)
        self.pred_mask = torch.zeros((B, N, K), **f)
        self.pred_axis = torch.zeros((B, N, 3), **f)
        self.pred_index = None                  # joint_source="predicted", couple=False: the (B, N, C) index head load_inputs() supplies
        self.draws_a = self.draws_b = None      # optional replayed sample streams (see AncshPipeline.load_draws)
        self.stream = torch.cuda.Stream(device=device)
        self.graph = None
        self.out = None
        # range guard (F16x2): the flag words the guarded launches OR into, and the f32 graph of the same step that refits flagged clouds
        self.flags = torch.zeros((B,), dtype=torch.int32, device=device) if opts.range_guard else None
        self.graph32 = None
        self.out32 = None
        self.perm = self.src_rows = self.gt_built = self.frame_built = None
        for inp in EVERY_INPUT:                 # a side input the slot is not built with: no device buffer
            setattr(self, inp.name, None)
        self.bounds = self.reproj_tables = self.reproj_pix = self.refine_bufs = None
        if opts.raw_capacity is not None:
            self._init_stream(B, N, K, device, opts)

    def _init_stream(self, B, N, K, device, opts):
        """Streaming: raw rows + a header (stream.header_layout) on the device, their pinned staging, the side inputs (stream.SIDE_INPUTS)
        with their pinned twins, the streamed outputs with theirs (self.outputs), and the events that say when the staging / the outputs'
        twins may be touched again.  The rows are opts.rows' (stream.ROW_KINDS); with point_ground_truth the sampler leaves its
        permutation in the slot (its perm_out); with build_point_gt what travels in is the 7-column annotated rows (src_rows) the step's
        first launch builds the 18-column rows from, which then have no pinned twin.  depth (raw_capacity = the pixel capacity): the rows
        are unprojected on the device, so they have no pinned twin either."""
        f = dict(dtype=torch.float32, device=device)
        cap, kind, depth, range_guard = opts.raw_capacity, opts.rows, opts.depth_dtype, opts.range_guard
        self.keyed, self.nchan = opts.keyed, kind.nchan
        if opts.point_ground_truth:
            self.perm = torch.zeros((B, N), dtype=torch.int32, device=device)
        self.layout = lay = header_layout(B, self.keyed, bool(depth), opts.label_images or opts.annotated_images)
        self.raw_rows = torch.zeros((cap, self.nchan), **f)
        self.hdr = torch.zeros((lay.words,), dtype=torch.int32, device=device)
        if opts.build_point_gt:
            self.src_rows = torch.zeros((cap, kind.staged), **f)
        self.staged_rows = self.src_rows if opts.build_point_gt else self.raw_rows      # the device buffer submit() copies the clouds into
        self.h_rows = None if depth else torch.zeros((cap, kind.staged), dtype=torch.float32).pin_memory()
        self.h_hdr = torch.zeros((lay.words,), dtype=torch.int32).pin_memory()
        self.h2d_done = torch.cuda.Event()
        self.d2h_done = torch.cuda.Event()
        # dense / label_images: the per-raw-row (dense) or per-row and per-pixel (rowlab, img) labels / values the captured step writes
        # (slot-owned, outside the graph's pool, so a later replay never hands their memory to another tensor) and the f32 graph's own
        # (range guard); rowlab is device only: nobody reads rows.  Their pinned twins cost 4 + 28 bytes per row / pixel of capacity.
        for name, built in (("dense", opts.dense), ("rowlab", opts.label_images or opts.annotated_images), ("img", opts.label_images)):
            setattr(self, name, label_buffers(cap, device) if built else None)
            setattr(self, name + "32", label_buffers(cap, device) if built and range_guard else None)
        # annotated_images: the four per-pixel images of annotated frames (aimg: predicted labels / values, ground-truth labels / values),
        # slot-owned like img; rowlab holds the per-row predictions they are gathered from.  Their pinned twins cost 60 bytes per pixel.
        from .depth import annotated_image_buffers
        self.aimg = annotated_image_buffers(cap, device) if opts.annotated_images else None
        self.aimg32 = annotated_image_buffers(cap, device) if opts.annotated_images and range_guard else None
        hdr = self.h_hdr.numpy()               # host views of the pinned staging (written with numpy, no torch op per cloud)
        self.np_rows = None if depth else self.h_rows.numpy()
        self.np_seed, self.np_off, self.np_nf = hdr[lay.seed].view(np.int64), hdr[lay.off], hdr[lay.nf].view(np.float32)
        self.np_base = hdr[lay.base] if self.keyed else None      # the key block's cloud_base (hdr[3], reserved, stays 0)
        unit = None
        if depth:
            unit = self._init_depth(B, cap, depth, device, annotate=opts.link_counts, rendered=opts.render, sensor=opts.sensor)
        else:
            fill_rows(kind, self.np_rows, K)
            self.np_off[:] = np.arange(B + 1) * (cap // B)
            self.np_nf[:] = 1.0
            self.staged_rows.copy_(self.h_rows)
            self.hdr.copy_(self.h_hdr)
        for inp in opts.inputs:                # sl.gt / sl.h_gt / sl.np_gt and so on: the device buffer, its pinned twin and its numpy view
            host = side_host(inp, B, K, unit)
            setattr(self, "h_" + inp.name, host)
            setattr(self, "np_" + inp.name, host.numpy())
            setattr(self, inp.name, host.to(device))
        if opts.posed:                         # what ancsh_pose_scene_build writes and the renderer and the annotation read, and the crop
            from .depth import RENDER_WIDTH, SCENE_WIDTH         # centring's scratch: slot-owned, never an H2D target
            self.render = torch.zeros((B, RENDER_WIDTH), dtype=torch.float64, device=device)
            self.scene = torch.zeros((B, SCENE_WIDTH), dtype=torch.float64, device=device)
            self.bounds = torch.zeros((B, 4), dtype=torch.int32, device=device)
        if opts.build_gt_pose:                 # what ancsh_gt_pose_build writes behind the sampler and the two error launches read: slot-owned,
            self.gt_built = torch.zeros((B, K, SIDE["gt"].shape(K)[1]), dtype=torch.float64, device=device)      # never an H2D target
            self.frame_built = torch.zeros((B,) + SIDE["frame"].shape(K), dtype=torch.float64, device=device)
        # the predicted frames' tables and the pixel triple the renderer draws them into, two crops per frame; with refine= the loop's buffers
        # (the silhouette term's field: 4 bytes per pixel and part; the coverage term's cover: 8).  Slot-owned, shared with the range guard's
        # f32 graph.
        if opts.reprojection or opts.refine:
            from .pose.reprojection import predicted_frames
            self.reproj_tables, self.reproj_pix = predicted_frames(B, cap, depth, device)
        if opts.refine:
            from .pose.refinement import refine_buffers
            self.refine_bufs = refine_buffers(B, K, device, silhouette=opts.silhouette, joints=opts.refine_joints, pixel_capacity=cap,
                                              coverage=opts.refine_coverage, scale=opts.refine_scale)
        # the streamed outputs, in the order submit copies them out: the record first, right behind the replay.  record and
        # articulation live in the graph's pool (sl.out / sl.out32), the others in slot-owned buffers; the flag words, the depth
        # front end's valid-pixel counts and the annotated frames' valid pixels per link are not refit.
        pinned = lambda dtype, *shape: lambda: (torch.zeros(shape, dtype=dtype).pin_memory(),)
        labels = lambda: label_buffers(cap)
        outs = [Output("record", lambda sl, f32: (sl.pick("out", f32)[opts.record_key],), pinned(torch.float64, B, K, self.record_width),
                       refit=range_guard)]
        if depth:
            outs.append(Output("counts", lambda sl, f32: (sl.counts,), pinned(torch.int32, B)))
            if opts.link_counts:
                outs.append(Output("link_counts", lambda sl, f32: (sl.link_counts,), pinned(torch.int32, B, 16)))
        if opts.articulation:
            outs.append(Output("articulation", lambda sl, f32: (sl.pick("out", f32)["articulation"],), pinned(torch.float64, B, K, self.art_width),
                               refit=range_guard))
        if opts.dense:
            outs.append(Output("dense", lambda sl, f32: sl.pick("dense", f32), labels, refit=range_guard, extent=per_raw_row,
                               take=take_dense, patch=patch_dense))
        if opts.label_images:
            outs.append(Output("label_images", lambda sl, f32: sl.pick("img", f32), labels, refit=range_guard, extent=per_pixel,
                               take=take_images))
        if opts.annotated_images:
            outs.append(Output("annotated_images", lambda sl, f32: sl.pick("aimg", f32), lambda: annotated_image_buffers(cap), refit=range_guard,
                               extent=per_pixel, take=take_annotated_images))
        if range_guard:
            outs.append(Output("flags", lambda sl, f32: (sl.flags,), pinned(torch.int32, B)))
        self.outputs = {o.name: o for o in outs}
        img = self.outputs.get("label_images")
        self.h_img, self.h_img32 = (img.host, img.host32) if img else (None, None)

    def _init_depth(self, B, capacity, depth, device, annotate=False, rendered=False, sensor=False):
        """The depth front end's buffers: the pixel and mask buffers with their pinned staging, the kernel's scratch, the valid-pixel
        counts, and host / device views of the header's geometry, camera and dest blocks.  Until the first submit: B crops of random
        depths in front of a unit camera (a defined, non-degenerate input for prepare()'s passes).
        annotate (annotated frames, ancsh_depth_annotate_stream): the mask buffers carry the link labels -- the same bytes per pixel --, the
        scratch holds 16 counters per chunk, and the slot owns the per-link counts; the header's camera block is not read, the scene
        tables (a side input) carry the camera.  Until the first submit: every pixel labelled 0.
        rendered (render_mesh=, ancsh_render_depth_labels): the step writes the pixel and label buffers itself, so they have no pinned
        staging, and the slot owns the renderer's z-buffer, 8 bytes a pixel.  Until the first submit: the mesh in its model frames in
        front of the unit camera.
        sensor (sensor=, ancsh_depth_sensor_model): a second pixel and label pair (apix, amask), 3 bytes a pixel of capacity (5 with
        float32 depths), which the step's sensor launch writes from the first and the annotation and its inverse read; without a sensor
        the two names are the first pair.
        -> the unit camera's six coefficients and the depth scale (what stream.unit_scene builds the slot's first scenes from)."""
        from .depth import CAM_WORDS, DEPTH_DTYPES, GEOM_WORDS, MAX_CHUNKS, SCENE_MAX_LINKS
        npt, tt, _ = DEPTH_DTYPES[depth]
        self.pix = torch.zeros((capacity,), dtype=tt, device=device)
        self.mask = torch.zeros((capacity,), dtype=torch.uint8, device=device)
        self.h_pix = None if rendered else torch.zeros((capacity,), dtype=tt).pin_memory()
        self.h_mask = None if rendered else torch.zeros((capacity,), dtype=torch.uint8).pin_memory()
        self.zbuf = torch.zeros((capacity,), dtype=torch.int64, device=device) if rendered else None
        self.apix, self.amask = self.pix, self.mask
        if sensor:
            self.apix = torch.zeros((capacity,), dtype=tt, device=device)
            self.amask = torch.full((capacity,), 255, dtype=torch.uint8, device=device)
        self.scratch = torch.zeros((B * MAX_CHUNKS * (SCENE_MAX_LINKS if annotate else 1),), dtype=torch.int32, device=device)
        self.counts = torch.zeros((B,), dtype=torch.int32, device=device)
        lay, hdr = self.layout, self.h_hdr.numpy()
        self.np_pix, self.np_mask = (None, None) if rendered else (self.h_pix.numpy().view(npt), self.h_mask.numpy())
        self.np_geom = hdr[lay.geom].reshape(B, GEOM_WORDS)
        self.np_cam = hdr[lay.cam].view(np.float32).reshape(B, CAM_WORDS)
        self.geom = self.hdr[lay.geom].view(B, GEOM_WORDS)
        self.cam = self.hdr[lay.cam].view(torch.float32).view(B, CAM_WORDS)
        self.np_dest, self.dest = (hdr[lay.dest], self.hdr[lay.dest]) if lay.dest is not None else (None, None)
        rs = np.random.RandomState(0)
        per = capacity // B
        w = max(1, int(np.sqrt(per)))
        h = per // w
        scale = 1.0 / 65535.0 if npt == np.uint16 else 1.0
        if not rendered:
            self.np_pix[:] = rs.randint(32768, 65536, capacity).astype(np.uint16) if npt == np.uint16 else rs.uniform(0.5, 1.0, capacity).astype(np.float32)
            self.np_mask[:] = 0 if annotate else 1
        unit = (1.0 / w, 0.0, -0.5, 0.0, 1.0 / h, -0.5, scale)
        for b in range(B):
            self.np_geom[b] = (b * per, h, w, 0, 0)
            self.np_cam[b] = unit
        self.link_counts = torch.zeros((B, SCENE_MAX_LINKS), dtype=torch.int32, device=device) if annotate else None
        if lay.dest is not None:
            self.np_dest[:] = self.np_geom[:, 0]
        self.np_nf[:] = 1.0
        if not rendered:
            self.pix.copy_(self.h_pix)
            self.mask.copy_(self.h_mask)
        self.hdr.copy_(self.h_hdr)
        return unit

    def pick(self, name, f32=False):
        """Attribute `name` of the step (out, dense, rowlab, img, aimg), or (f32=True) its twin of the range guard's f32 graph."""
        return getattr(self, name + "32" if f32 else name)

    def header(self, B):
        """(seed (1,) int64 -- keyed: the key block (4,) int32 --, offsets (B+1,) int32, norm factors (B,) float32) views of the device
        header."""
        lay, key = self.layout, self.hdr[self.layout.key]
        return key if self.keyed else key.view(torch.int64), self.hdr[lay.off], self.hdr[lay.nf].view(torch.float32)


class AncshPipeline(object):
    """step() runs the next batch through the whole path and returns that batch's outputs.

    couple=True : the pose stage reads the networks' own outputs (production data flow).
    couple=False: the pose stage reads `pred_*` buffers supplied by the caller -- used by the benchmark,
                  where random-init networks (no checkpoint ships with the reference) would hand the
                  fitter degenerate parts; every stage still runs inside the step.
    (Running one batch's own dependency graph on two streams -- [ANCSH net] || [NPCS net -> stage A], joined for stage B --
    was measured and dropped: both networks are matrix-pipe-bound even at 32 clouds, so their kernels time-slice instead of
    overlapping: 4.32 vs 4.45 ms for a lone batch, and 2.17 vs 1.75 ms/step with 16 batches in flight, where the 32 streams
    exceed the hardware queues.  Re-measured in round 3 with the geometry computed first and ONLY the NPCS network on the second
    stream: 17.2 k vs 20.1 k clouds/s at 16 batches in flight, 14.0 k vs 19.3 k at 8 -- two matrix-bound kernels interleaving
    their workgroups lose the XCD-local L2 reuse and each other's instruction-cache; coordinated batching beats concurrency.
    A narrower variant -- both networks' matrix-bound SA launches in order on the slot's stream, only the eleven small latency-bound
    launches of layer3 / fa_layer1 / fa_layer2 of the NPCS network forked to a side stream and joined before the tails (the two
    forwards driven phase by phase, outputs bit-identical) -- gained 1 % for a lone batch (8.58 k vs 8.48 k) and lost 15 % at 16
    batches in flight (17.2 k vs 20.1 k; 14.0 k vs 19.3 k at 8): every fork / join inside a batch costs more than it overlaps.  Likewise stage A || stage B of the fit on two streams -- they only share the partition --
    bought 0.13 ms of a lone batch's 4.29 ms and cost 0.44 ms/step at 16 batches in flight: dropped.)
    slots: batches kept in flight on separate HIP streams (round-robin).  The pose fit is latency-bound
           (a few hundred waves; a degenerate 3-point sample may run MINPACK's full 4200-evaluation budget in
           ONE lane, exactly as scipy does) while the networks are throughput-bound, so overlapping batch i's
           fit with batch i+1's networks keeps the CUs busy; results equal those of slots=1 (to the last bit for equal lm_schedule; slots <= 2 select the eight-lane LM schedule, see below).

    The options (README, "Streaming"; their rules are stream.check_options, every one checked on the host before anything touches the GPU):
    joint_types: None (all revolute) | "revolute" | "prismatic" | K - 1 of them for joints 1..K-1 (PoseSolver).  A prismatic joint is fitted
        with the shared-rotation objective and never reads its joint direction; the per-problem kind array is built once, no launch more.
    joint_source: stage B's joint association.  "gt" = a label per point (load_inputs' joint_cls, or column 3 of a streamed row); "predicted" =
        the argmax of the ANCSH network's index_per_point head, from the step's own forward (couple=True) or load_inputs'
        pred["index_per_point"] (couple=False): a stream then takes (n_raw, 3) xyz clouds.  Same launch count either way.
    lm_schedule: few batches in flight = a latency deployment, so slots <= 2 take the eight-lanes-per-fit schedule unless lm_schedule says
        otherwise (the C ABI's default never depends on slots or batch size).  The schedules agree to ~1e-7, not to the last bit: pass
        "throughput" for bytes equal to a many-slot pipeline.
    tie_window: None = no tie statistics in the step (they cost stage A's finish kernel ~20 us a batch); parallel_ancsh_pose.TIE_WINDOW to get them.
    arithmetic: of the shared-MLP layers.  None = what ANCSH_SA_BF16X3 / ANCSH_SPLIT_SCHEME say (default f32, the graded arithmetic);
        "f32" | "bf16x3" | "f16x2" pins it for this pipeline.
    range_guard (arithmetic="f16x2"): the guarded kernels flag every (cloud, network) with an activation beyond f16's range, and flagged clouds
        are refit by an f32 graph of the same step (streaming: retire() does it; step(): out["range_flags"] + rerun_f32()).
    raw_capacity: None = step() on inputs the caller loads; an int = the streaming pipeline (submit / retire / stream_batches), whose slots
        hold up to raw_capacity raw rows per batch, padding included.  Needs couple=True.
    keyed (streaming): the header leads with a key block (ancsh_stream_key) whose cloud_base submit() writes with the seed; cloud b is sampled
        and fitted as global cloud cloud_base + b, so one captured graph serves a shard at any offset (dist.ShardedPipeline).
    articulation (couple=True, num_points <= ARTICULATION_MAX_N): one more launch (ancsh_articulation_rec) leaves out["articulation"], the
        (B, K, 12) block of part boxes and camera-space joints; retire(articulation=True) returns it.
    joint_states (with articulation): one more launch (ancsh_joint_state_rec) widens that block to (B, K, 20), its 12 columns bit for bit and
        the joint state behind them.  It is still out["articulation"]: no new name in the result tuple.
    The streamed record is the pose record and one block of columns per option below that reports something per part, each written by one
        launch that copies the record so far bit for bit: pose.record.BLOCKS is the one table of the blocks, their order, widths, column
        names and out[...] names, and pipe.record_layout (pose.record.RecordLayout) says where each lies in THIS pipeline's record.
    fit_quality: one more launch behind the fit (ancsh_fit_quality_rec) leaves out["record_wide"], the record's columns bit for bit and the
        fit-quality block behind them.  Works with couple=False too.
    ground_truth (streaming): submit(..., gt=...) brings a (K, 19) block per cloud and one more launch (ancsh_gt_error_rec) leaves
        out["record_gt"], the error block behind the record so far.
    point_ground_truth (streaming, with articulation): the rows are dataset.pack_cloud's 18 columns, submit(..., frame=...) brings part 0's
        ground-truth NAOCS pose per cloud, and the last launch of the articulation group (ancsh_point_gt_rec) leaves out["record_point_gt"]:
        both networks' test losses (coord_regress_loss: "L2" | "L1") and the joint errors, the point-gt block behind the record so far.
    build_point_gt (with point_ground_truth): the stream takes (n_raw, 7) annotated clouds and one rig per cloud (submit(..., rig=...)), and the
        step's first launch (ancsh_point_gt_build) builds the 18-column rows on the device.
    build_gt_pose (with point_ground_truth): one more launch directly behind the sampler (ancsh_gt_pose_build) fits the ground-truth poses
        of step 1 of evaluation.sh from the slot's rows, perm and P into slot-owned tables, which the two error launches read: submit takes
        no frame (ValueError), and of gt (ground_truth=True) only the box extents, columns 13..15 (pose.gt_errors.pack_box_extents; None =
        NaN extents, so only the two IoU columns are NaN).  step() leaves out["gt_pose"] (B, K, 19) and out["gt_frame"] (B, 13).
    dense (streaming): the last launch (ancsh_raw_point_labels) labels every raw row; retire(dense=True) returns (labels, values, offsets).
    depth_capacity, depth_dtype: the depth front end (submit_depth / stream_depth_batches) in raw_capacity's place: a slot holds up to
        depth_capacity pixels of crops and masks, unprojected on the device (ancsh_depth_unproject_stream) in front of the xyz sampler.
        Needs joint_source="predicted"; refuses dense.
    label_images (depth): two more launches carry the row labels back to the pixels; retire(label_images=True) returns per frame an (h, w)
        label image and an (h, w, 7) value image.  32 bytes of pinned memory per pixel of capacity and slot.
    depth_capacity with point_ground_truth and build_point_gt: annotated depth frames -- depth crop, link-label crop and a scene table per
        frame (submit_depth(..., scene=, rig=, frame=)); the step starts with ancsh_depth_annotate_stream, then ancsh_point_gt_build and
        the sampler.  retire(link_counts=True) returns the valid pixels per link.  Refuses label_images: its rows are link-major.
    annotated_images (those annotated frames, rendered and posed ones included): two more launches at the step's end --
        ancsh_raw_point_labels over the slot's 18-column rows, then ancsh_depth_annotated_images, the inverse of the annotation's sort --
        carry every row's prediction and ground truth back to its pixel; retire(annotated_images=True) returns per frame (labels (h, w),
        values (h, w, 7), gt_labels (h, w), gt_values (h, w, 6)).  60 bytes of pinned memory per pixel of capacity and slot (twice that
        with range_guard).
    render_mesh (with those annotated-frame options): depth.pack_mesh's arrays, uploaded once and shared by the slots; the step starts with
        ancsh_render_depth_labels, which renders every frame's depth and label crops into the slot's device buffers in front of
        ancsh_depth_annotate_stream.  submit_render / stream_render_batches take crop geometry and tables only: no pixel crosses PCIe.
    render_mesh = depth.pack_mesh_library's 4 arrays: a library of instances, uploaded once; the frame's instance travels in its table's
        reserved value -- depth.pack_render_scene(..., instance=i) for submit_render, depth.pack_pose(q, view, instance=i) for submit_posed, where
        kinematics is the (ninst, 672) np.stack of the instances' tables -- and the step calls the *_lib entries: the same launch count.
    kinematics (with render_mesh): depth.pack_kinematics' table, uploaded once and shared by the slots; the step starts with
        ancsh_pose_scene_build, which writes the slot's render and scene tables from one pose per frame (depth.pack_pose: joint values and a
        view matrix), and ancsh_render_centre_crops, which centres the crops that ask for it on the projected object, in front of the
        renderer.  submit_posed / stream_posed_batches take crops and poses only: 32 doubles per frame cross PCIe.
    sensor (those annotated frames, submitted, rendered, posed or from a library): depth.pack_sensor's table, uploaded once; one launch,
        ancsh_depth_sensor_model, directly behind the renderer (submitted frames: behind the H2D copy) degrades every frame -- noise, holes,
        edge dropout, disparity steps, keyed by the slot's own seed or key block -- into a second pixel pair of the slot, 3 bytes per pixel
        of capacity (5 with float32), which the annotation and annotated_images read.  Results keep their form; counts, link counts and
        images are the degraded frame's.  A short batch's padding frames take pixels of their own behind the batch's.
    reprojection (with render_mesh, whatever else is built): render-and-compare at the step's end -- ancsh_reproject_scene_build turns the
        record's two poses per part into two render tables per frame, the renderer draws those 2 * B predicted frames into a pixel triple of the
        slot (22 bytes per pixel of capacity, 26 with float32), and ancsh_reproject_compare_rec scores them against the pair the annotation
        read (with sensor=: the degraded one): out["record_reproj"], the reprojection block (pose.reprojection.COLUMN_NAMES: observed pixels, then
        predicted pixels, overlap, IoU and the depth residual's mean |d|, RMS, max and mean per pose) behind the record so far.  Five launches more;
        the result tuple keeps its form.  A short batch's padding frames take pixels of their own, as with a sensor.
    refine (with render_mesh, whatever else is built): pose.refinement.pack_refine's table, uploaded once: render-and-compare ICP at the step's
        end, behind reprojection's three calls when both are on (they share the slot's predicted tables and pixel triple) -- iters + 1 times
        ancsh_reproject_scene_build on the working poses, the renderer and ancsh_refine_pass, then ancsh_refine_rec: 5 (iters + 1) + 1 launches.
        A table of pack_refine(silhouette=...) adds the silhouette term: ancsh_silhouette_field once in front of the loop and
        ancsh_refine_pass_sil in it, 5 (iters + 1) + 2 launches and 4 bytes per pixel of depth_capacity, part and slot; poses shifted across
        the ray come back, and cost_start / cost_best charge pixels that hang over the observed part.
        A table of pack_refine(joints=...) (with kinematics=) adds the joint step: ancsh_refine_joint_step behind every pass solves the
        parts of an object together through its revolute and prismatic joints, 6 (iters + 1) + 1 launches (+ 1 with the silhouette field); the
        slot holds a second (B, K, 2, 18) block and a (B, 2, 8) row per object besides, out["refine_object"] (pose.refinement.OBJ_COLUMNS; not
        streamed).  The best-of is then kept per OBJECT: cost_best <= cost_start holds for out["refine_object"], not for each part's columns,
        whose best_pass and passes_solved are the object's.
        A table of pack_refine(silhouette=..., coverage=...) adds the coverage term: ancsh_coverage_field behind the renderer in every pass
        and ancsh_refine_pass_cov, 6 (iters + 1) + 2 launches (7 (iters + 1) + 2 with the joint step) and 8 bytes more per pixel of
        depth_capacity, part and slot; a part is pulled over observed pixels it leaves bare.  The record's columns are unchanged.
        A table of pack_refine(silhouette=..., coverage=..., scale=...) solves s with R and t: ancsh_refine_pass_scale in
        ancsh_refine_pass_cov's place, the same launches, sums of 48 values; column s of the refinement block is then the refined scale.
        out["record_refined"]: the refinement block (pose.refinement.COLUMN_NAMES: per pose the refined [R | s | t], cost_start, cost_best,
        n_used, best_pass, passes_solved) behind the record so far; pose.refinement.refined_record(record, layout=pipe.record_layout) gives the
        (.., 26) record of the refined poses.  The slot holds two (B, K, 26) working records, the (B, K, 2, 18) best block and the
        (B, K, 2, 32) sums besides.
    joint_values (with kinematics= and articulation): the step's last launch (ancsh_joint_values_rec), behind ancsh_refine_rec when refine= is on,
        inverts ancsh_pose_scene_build's forward kinematics on the part poses: per part and pose the joint value q of the part's bridging joint
        in the kinematic table's own parametrisation, its error against the submitted q, and the angle and gap by which the two sides of the
        joint miss one axis -- for the record's two poses and, with refine=, the two kept refined poses (NaN without).  The 24 columns
        (pose.joint_values.COLUMN_NAMES; named_columns, joint_value_table) ride behind the articulation block's 12 or 20: it is still
        out["articulation"], no new name in the result tuple or the record.  Works with a library.
    In every streaming mode out["record"] stays (B, K, 26); the RECORD that retire / stream_* return is the widest one built,
    out[pipe.record_layout.key], pipe.record_layout.width columns."""

    ninst = None                                # a library's size (render_mesh=depth.pack_mesh_library(...)); None for a single object

    def __init__(self, num_parts, weights_ancsh, weights_npcs, batch_size, num_points, device="cuda:0",
                 inlier_th=0.1, niter_a=10000, niter_b=200, couple=True, use_graph=True, seed=0, slots=1, lm_schedule=None, tie_window=None,
                 arithmetic=None, raw_capacity=None, range_guard=False, keyed=False, articulation=False, dense=False, joint_source="gt",
                 joint_types=None, depth_capacity=None, depth_dtype="uint16", label_images=False, joint_states=False, fit_quality=False,
                 ground_truth=False, point_ground_truth=False, coord_regress_loss="L2", build_point_gt=False, build_gt_pose=False,
                 render_mesh=None, kinematics=None, annotated_images=False, sensor=None, reprojection=False, refine=None, joint_values=False):
        # the options, checked on the host before anything touches the GPU
        from .pose.parallel_ancsh_pose import check_joint_types
        check_joint_types(joint_types, num_parts)
        if arithmetic not in (None, "f32", "bf16x3", "f16x2"):
            raise ValueError("arithmetic must be None, 'f32', 'bf16x3' or 'f16x2'")
        self.opts = o = check_options(batch_size, num_points, couple, inlier_th, raw_capacity, depth_capacity, depth_dtype, keyed, range_guard,
                                      arithmetic, articulation, joint_states, fit_quality, ground_truth, point_ground_truth, build_point_gt, dense,
                                      label_images, joint_source, coord_regress_loss, build_gt_pose, render_mesh, kinematics, annotated_images, sensor,
                                      reprojection, refine, joint_values=joint_values)
        self.refine = o.refine
        self.record_layout = o.layout           # where each block of the streamed record lies (pose.record.RecordLayout)
        for name in OPTION_FLAGS:               # pipe.keyed, pipe.articulation, ...: what the step, the tools and dist.ShardedPipeline read
            setattr(self, name, getattr(o, name))
        self.joint_source, self.arithmetic = joint_source, arithmetic
        self.K, self.B, self.N = num_parts, batch_size, num_points
        self.couple, self.seed = couple, seed
        self.hw_queues = check_hardware_queues(max(1, slots))
        self.device = torch.device(device)
        self.mesh = self.kin = None
        if o.posed:                             # the kinematic table (a library: the stack of them): checked here, uploaded once below and shared by all slots
            from .depth import check_kinematics, check_kinematics_library
            kinematics = check_kinematics_library(kinematics, num_parts) if np.ndim(kinematics) == 2 else check_kinematics(kinematics, num_parts)
        if o.render:                            # the mesh (or the library): checked, then uploaded once and shared by all slots
            from .depth import mesh_to_device
            self.mesh = mesh_to_device(render_mesh, self.device)
            self.ninst = self.mesh.ninst
        if o.posed:
            self.kin = torch.from_numpy(kinematics).to(self.device)
        self.sensor_table = None
        if o.sensor:                            # the sensor table (check_options has checked it): uploaded once and shared by all slots
            from .depth import check_sensor
            self.sensor_table = torch.from_numpy(check_sensor(sensor)).to(self.device)
        self.refine_table, self.refine_iters = None, 0
        if o.refine:                            # the refinement's parameters (check_options has checked them): uploaded once and shared by all slots
            from .pose.refinement import check_refine_table
            table = check_refine_table(refine)
            self.refine_table, self.refine_iters = torch.from_numpy(table).to(self.device), int(table[0])
        # the networks; both layer by layer in grouped launches (paired.py; identical outputs); ANCSH_PAIRED=0: one forward after the other
        self.ancsh = Network(num_parts, weights_ancsh, "ancsh", device)
        self.npcs = Network(num_parts, weights_npcs, "npcs", device)
        if self.range_guard:                    # the weights the F16x2 path packs are checked here, once
            bad = f16x2_weight_violations([("ancsh", self.ancsh), ("npcs", self.npcs)])
            if bad:
                raise ValueError("range_guard: weights beyond f16's range (|w| > 65504) in " +
                                 ", ".join("%s (max |w| = %.6g)" % nb for nb in bad))
        import os
        from .paired import PairedNetworks
        self.paired = PairedNetworks([self.ancsh, self.npcs]) if os.environ.get("ANCSH_PAIRED", "1") != "0" else None
        if self.paired is not None and not self.paired.eligible():
            self.paired = None
        # the solver
        self.solver = PoseSolver(num_parts, inlier_th, niter_a, niter_b, device,
                                 lm_schedule=lm_schedule or ("latency" if max(1, slots) <= 2 else "auto"), tie_window=tie_window,
                                 joint_types=joint_types)
        self.solver.prepare(batch_size)     # the (B * (K - 1)) joint-kind array (None when every joint is revolute): never built inside a captured step
        self.f32_reruns = 0                 # batches retire() refit in f32 (range guard)
        # the slots
        self.slots = [_Slot(batch_size, num_points, num_parts, self.device, o) for _ in range(max(1, slots))]
        self._next = 0
        self._use_graph = use_graph
        self.stream = self.slots[0].stream
        self._prepared = False
        self._inflight = collections.deque()       # (slot, tag, seed, valid clouds) of submitted, unretired batches, oldest first
        self._submitted = 0

    # single-slot conveniences (slot 0)
    @property
    def P(self):
        return self.slots[0].P

    def load_inputs(self, P, joint_cls=None, pred=None, slot=None):
        """P (B, N, 3); joint_cls (B, N) int (joint_source="gt"; ignored when "predicted"); pred: the pose stage's inputs for couple=False
        (nocs_per_point, instance_per_point, joint_axis_per_point and, when "predicted", index_per_point (B, N, C)).  The joint
        association is checked (check_joint_inputs) before anything is copied."""
        check_joint_inputs(self.joint_source, self.couple, joint_cls, pred)
        index = None
        if self.predicted and pred is not None and pred.get("index_per_point") is not None:
            index = torch.as_tensor(pred["index_per_point"])
            if index.dim() != 3 or tuple(index.shape[:2]) != (self.B, self.N):
                raise ValueError("pred['index_per_point'] must be (%d, %d, C), got %s" % (self.B, self.N, tuple(index.shape)))
            if self._prepared and any(sl.pred_index is not None and sl.pred_index.shape != index.shape for sl in self.slots):
                raise ValueError("pred['index_per_point'] changed shape after prepare(): the captured step reads a (B, N, %d) buffer"
                                 % self.slots[0].pred_index.shape[2])
        for sl in (self.slots if slot is None else [self.slots[slot]]):
            sl.P.copy_(torch.as_tensor(P))
            if not self.predicted:
                sl.joint_cls.copy_(torch.as_tensor(np.asarray(joint_cls, np.int32)) if not torch.is_tensor(joint_cls) else joint_cls)
            if pred is not None:
                sl.pred_nocs.copy_(torch.as_tensor(pred["nocs_per_point"]))
                sl.pred_mask.copy_(torch.as_tensor(pred["instance_per_point"]))
                sl.pred_axis.copy_(torch.as_tensor(pred["joint_axis_per_point"]))
            if index is not None:
                if sl.pred_index is None or sl.pred_index.shape != index.shape:
                    sl.pred_index = torch.zeros(tuple(index.shape), dtype=torch.float32, device=self.device)
                sl.pred_index.copy_(index)

    def _check_index_loaded(self):
        """joint_source="predicted" with couple=False: every slot needs the index head load_inputs() supplies -- checked before any GPU
        work of prepare() / step()."""
        if self.predicted and not self.couple and any(sl.pred_index is None for sl in self.slots):
            raise ValueError("joint_source='predicted' with couple=False: no index head loaded -- call load_inputs(P, None, "
                             "pred={..., 'index_per_point': ...}) first")

    def load_draws(self, draws_a, draws_b, slot=None):
        """Replay explicit 3-point sample streams (e.g. numpy's, `pose.parallel_ancsh_pose.draws_from_seed`) instead of the
        on-device generator: draws_a (B,K,niter_a,3), draws_b (B,K-1,niter_b,6) int32.  Call before prepare()."""
        for sl in (self.slots if slot is None else [self.slots[slot]]):
            sl.draws_a = torch.as_tensor(np.ascontiguousarray(draws_a, np.int32)).to(self.device)
            sl.draws_b = None if draws_b is None else torch.as_tensor(np.ascontiguousarray(draws_b, np.int32)).to(self.device)

    def _networks(self, P, geom, arithmetic, flags):
        if self.paired is not None:
            return self.paired.predict(P, geom, arithmetic, flags)          # every backbone layer of both networks in one grouped launch
        return self.ancsh.predict(P, geom, arithmetic, flags, 0), self.npcs.predict(P, geom, arithmetic, flags, 1)

    def _sample(self, sl):
        """The captured step's first launch when streaming: the slot's raw clouds -> its P / joint_cls.  -> the device key: the seed
        (1,) int64, or (keyed) the key block."""
        from . import _lib
        from .dataset import RAW_JCLS_COL, RAW_NCHAN
        seed, off, nf = sl.header(self.B)
        if self.posed:                     # posed objects: the slot's poses -> its render and scene tables, then the centred crops' origins
            from .depth import centre_crop_origins, pose_scene_build
            pose_scene_build(self.kin, sl.pose, out=(sl.render, sl.scene))
            centre_crop_origins(self.mesh, sl.geom, sl.render, scratch=sl.bounds)
        if self.render:                    # rendered frames: the mesh and the slot's render tables -> its depth and label crops, on the device
            from .depth import render_depth
            render_depth(self.mesh, sl.geom, sl.render, self.depth_dtype, out=(sl.pix, sl.mask), scratch=sl.zbuf)
        if self.sensor:                    # a depth sensor's defects: the slot's clean crops -> its second pixel pair, keyed by the slot's own seed
            from .depth import depth_sensor_model
            depth_sensor_model(sl.pix, sl.mask, sl.geom, sl.scene, self.sensor_table, seed, out=(sl.apix, sl.amask))
        if self.link_counts:               # annotated depth frames: the slot's depth and label crops -> its annotated rows, offsets and counts
            from .depth import depth_annotate
            depth_annotate(sl.apix, sl.amask, sl.geom, sl.scene, out=(sl.src_rows, off, sl.counts, sl.link_counts), scratch=sl.scratch)
        if self.build_point_gt:            # the slot's annotated rows and rigs -> its 18-column rows, in front of the unchanged sampler
            from .dataset import point_gt_build
            point_gt_build(sl.src_rows, off, sl.rig, self.K, sl.raw_rows)
        if self.depth_dtype is not None and not self.link_counts:   # the depth front end: the slot's crops -> its rows, offsets and counts, in front of the xyz sampler
            from .depth import depth_unproject
            depth_unproject(sl.pix, sl.mask, sl.geom, sl.cam, out=(sl.raw_rows, off, sl.counts), scratch=sl.scratch)
        if self.predicted:                 # xyz rows: the sampler's xyz twin, same P (no joint_cls: the fit reads the index head)
            _lib.call("ancsh_input_sample_stream_xyz_keyed" if self.keyed else "ancsh_input_sample_stream_xyz", self.B, self.N, sl.nchan,
                      _lib.ptr(sl.raw_rows), self.raw_capacity, _lib.ptr(off), _lib.ptr(nf), _lib.ptr(seed), _lib.ptr(sl.P), _lib.ptr(sl.perm))
            return seed
        # point_ground_truth: the 18-column rows, whose last column is the joint label, and the slot's perm_out
        nchan, jcls_col = (sl.nchan, sl.nchan - 1) if self.point_ground_truth else (RAW_NCHAN, RAW_JCLS_COL)
        _lib.call("ancsh_input_sample_stream_keyed" if self.keyed else "ancsh_input_sample_stream", self.B, self.N, nchan,
                  _lib.ptr(sl.raw_rows), self.raw_capacity, _lib.ptr(off), _lib.ptr(nf), jcls_col, _lib.ptr(seed), _lib.ptr(sl.P),
                  _lib.ptr(sl.joint_cls), _lib.ptr(sl.perm))
        return seed

    def _run(self, sl=None, f32=False):
        """The step on slot sl: in the pipeline's arithmetic, or (f32=True: the range guard's refit) in f32 from the same slot inputs."""
        sl = sl or self.slots[0]
        guard = self.range_guard and not f32
        if guard:
            sl.flags.zero_()                  # the captured step's first node: the guarded launches only OR into the words
        key = self._sample(sl) if self.raw_capacity is not None else None
        seed_dev, key_dev = (None, key) if self.keyed else (key, None)
        gt_in, frame_in = sl.gt, sl.frame
        if self.build_gt_pose:            # directly behind the sampler: both ground-truth pose tables from the slot's rows, perm and P, one launch;
            from .pose.gt_pose import gt_pose_batch      # of the submitted gt only the box extents (columns 13..15) are read, where they lie
            gt_pose_batch(sl.raw_rows, sl.header(self.B)[1], sl.perm, sl.P, None if sl.gt is None else sl.gt[:, :, 13:16],
                          out=(sl.gt_built, sl.frame_built))
            gt_in, frame_in = sl.gt_built if self.ground_truth else None, sl.frame_built
        from . import pointnet_util
        geom = pointnet_util.Geometry()       # FPS / ball query / 3-NN depend only on P: computed once, used by both nets
        # the arithmetic goes down the layer helpers explicitly (None: the module globals); nothing global is changed
        a, n = self._networks(sl.P, geom, "f32" if f32 else self.arithmetic, sl.flags if guard else None)
        if self.couple:
            nocs, mask, axis = n["nocs_per_point"], n["W"], a["joint_axis_per_point"]
            index = a["index_per_point"] if self.predicted else None
        else:
            nocs, mask, axis, index = sl.pred_nocs, sl.pred_mask, sl.pred_axis, sl.pred_index if self.predicted else None
        assoc = dict(joint_index=index) if self.predicted else dict(joint_cls=sl.joint_cls)      # one of them: the solver refuses both
        sol = self.solver.solve(sl.P, nocs, mask, axis, draws_a=sl.draws_a, draws_b=sl.draws_b, seed=self.seed, seed_dev=seed_dev,
                                key_dev=key_dev, fit_quality=self.fit_quality, ground_truth=gt_in, **assoc)
        out = dict(ancsh=a, npcs=n, pose=sol, record=sol["record"])      # (B, K, 26) float64, written by the fit's two finish kernels
        carried = self.record_layout.carried                             # block -> (the out[...] name, the width) of the record its launch copies
        if self.fit_quality:             # behind the fit and the record poison: the fit-quality block, one launch (the solver issued it)
            out["record_wide"] = sol["record_wide"]
        if self.ground_truth:            # behind those: the error block, one launch (the solver issued it)
            out["record_gt"] = sol["record_gt"]
        if self.articulation:            # behind the fit and the record poison: (B, K, 12) float64, one launch
            from .pose.joint_params import articulation_batch
            out["articulation"] = articulation_batch(a, n, sol["record"])
            if self.joint_states:        # one more: the block's 12 columns and the joint state behind them, (B, K, 20) float64
                from .pose.joint_params import joint_state_batch
                out["articulation"] = joint_state_batch(sl.P, n, sol["record"], out["articulation"])
            if self.point_ground_truth:  # the last of the group: the record so far and the point-gt block behind it, one launch
                from .pose.point_gt import point_gt_batch
                out["record_point_gt"] = point_gt_batch(sl.raw_rows, sl.header(self.B)[1], sl.perm, a, n, out["articulation"], frame_in,
                                                        out[carried("point_gt")[0]], self.coord_regress_loss)
        if self.dense or self.label_images or self.annotated_images:      # at most one: a depth pipeline refuses dense=True, annotated frames label_images
            # the last launch: every raw row of the slot's batch (label_images: its unprojected rows; annotated_images: its 18-column rows),
            # into the slot's own (capacity, .) buffers
            from .dataset import raw_point_labels
            _, off, nf = sl.header(self.B)
            rl = raw_point_labels(sl.raw_rows, off, nf, sl.P, n, a, out=sl.pick("dense" if self.dense else "rowlab", f32))
            if self.dense:
                out["dense"] = rl
            elif self.label_images:      # one more launch: the rows back to the pixels they came from
                from .depth import depth_label_images
                out["label_images"] = depth_label_images(sl.pix, sl.mask, sl.geom, sl.dest, off, rl[0], rl[1], out=sl.pick("img", f32),
                                                         scratch=sl.scratch)
            else:                        # one more launch: the rows and their ground truth back through the annotation's link-major sort.
                # (Nothing between the annotation and here writes sl.scratch: its per-chunk histograms are what the inverse ranks with.)
                from .depth import depth_annotated_images
                out["annotated_images"] = depth_annotated_images(sl.apix, sl.amask, sl.geom, sl.scene, sl.dest, off, sl.counts, rl[0], rl[1],
                                                                 sl.raw_rows, out=sl.pick("aimg", f32), scratch=sl.scratch)
        if self.reprojection:            # the step's last three calls, behind the record's poison: the record's poses -> two render tables per
            # frame, the renderer on 2 * B frames, and the predicted pixels against the pair the annotation read -> its block behind the record
            from .pose.reprojection import reprojection_batch
            out["record_reproj"] = reprojection_batch(self.mesh, sl.render, sl.scene, sl.rig, sl.header(self.B)[2], sl.geom,
                                                      (sl.apix, sl.amask), out[carried("reprojection")[0]], self.depth_dtype, sl.reproj_tables,
                                                      sl.reproj_pix)
        if self.refine:                  # the step's last 5 (iters + 1) + 1 launches: the record's poses refined on the pair the annotation read, in
            # the predicted tables and pixel triple reprojection has finished with -> its block behind the record so far
            from .pose.refinement import refine_batch
            out["record_refined"] = refine_batch(self.mesh, sl.render, sl.scene, sl.rig, sl.header(self.B)[2], sl.geom, (sl.apix, sl.amask),
                                                 out[carried("refinement")[0]], self.depth_dtype,
                                                 sl.reproj_tables, sl.reproj_pix, self.refine_table, self.refine_iters, sl.refine_bufs,
                                                 kin=self.kin if self.opts.refine_joints else None)
            if self.opts.refine_joints:  # the joint step's row per (frame, pose): (B, 2, 8) float64, slot-owned, not streamed
                out["refine_object"] = sl.refine_bufs.obj[0]
        if self.opts.joint_values:       # the step's last launch: the joint values q read off the record's two poses per part and, with refine=, the
            # kept refined ones, against the submitted pose table -> the articulation block and the 24 columns behind it, (B, K, art_width)
            from .pose.joint_values import joint_values_batch
            out["articulation"] = joint_values_batch(self.kin, sl.render, sl.scene, sl.rig, sl.header(self.B)[2], sol["record"], out["articulation"],
                                                     pose=sl.pose, refined=sl.refine_bufs.best if self.refine else None)
        if self.build_gt_pose:           # the tables the step built: (B, K, 19) and (B, 13) float64, slot-owned
            out["gt_pose"], out["gt_frame"] = sl.gt_built, sl.frame_built
        if guard:
            out["range_flags"] = sl.flags     # (B,) int32: bit 0 = the ANCSH network, bit 1 = the NPCS network saw |x| > 65504
        return out

    def prepare(self):
        self._check_index_loaded()
        torch.cuda.synchronize(self.device)
        for sl in self.slots:
            with torch.cuda.stream(sl.stream):
                for _ in range(2):
                    sl.out = self._run(sl)
                if self.range_guard:
                    for _ in range(2):
                        sl.out32 = self._run(sl, f32=True)
            sl.stream.synchronize()
            if self._use_graph:
                sl.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(sl.graph, stream=sl.stream):
                    sl.out = self._run(sl)
                if self.range_guard:
                    # the refit: a second graph per slot, captured from the same slot inputs (raw rows + header, or P / joint_cls)
                    sl.graph32 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(sl.graph32, stream=sl.stream):
                        sl.out32 = self._run(sl, f32=True)
        if self._use_graph:
            # first launches of the instantiated graphs (the runtime uploads an executable graph on its first launch), all slots in
            # flight together as in steady state; results are those of the eager passes above
            import os
            for _ in range(int(os.environ.get("ANCSH_PREPARE_REPLAYS", "2"))):
                for sl in self.slots:
                    with torch.cuda.stream(sl.stream):
                        if self.range_guard:
                            self._replay(sl, f32=True)
                        self._replay(sl)
            self.synchronize()
        self._prepared = True
        return self

    def _replay(self, sl, f32=False):
        """The step (f32=True: the range guard's f32 step) on slot sl, enqueued on the current stream: a replay of its captured graph,
        or without one the launches themselves."""
        graph = sl.graph32 if f32 else sl.graph
        if graph is not None:
            graph.replay()
        elif f32:
            sl.out32 = self._run(sl, f32=True)
        else:
            sl.out = self._run(sl)

    def next_slot(self):
        """The slot the next step() will use: its outputs still hold the batch issued len(slots) steps ago (a consumer that must
        block the host for them -- e.g. a host-staged gather -- reads them here, when they have long been complete)."""
        return self.slots[self._next]

    def step(self):
        """Issue the next batch (asynchronous).  Returns (slot, outputs); outputs are valid once slot.stream is synchronised -- and
        only until the slot's NEXT step: a captured step owns its memory pool, so while a replay is in flight an output buffer may hold
        another tensor of the step (the pose record shares its block with the farthest-point indices, which the replay writes first; the
        same holds for out["articulation"], the (B, K, 12) block of articulation=True).
        Whatever the caller enqueued on ITS current stream before calling step() (a clone or a gather of the slot's previous outputs) is
        ordered before the new batch: the slot's stream waits for that stream here.  A consumer on any other stream is the caller's to order."""
        self._check_index_loaded()
        sl = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        cur = torch.cuda.current_stream(self.device)
        if cur != sl.stream and not cur.query():     # an idle caller stream (the throughput loop) costs one query, no event and no barrier packet
            sl.stream.wait_stream(cur)
        with torch.cuda.stream(sl.stream):
            self._replay(sl)
        return sl, sl.out

    def rerun_f32(self, slot):
        """Range guard: replay slot's f32 graph (the same step from the same slot inputs, in f32) on its stream and return its outputs --
        asynchronous, valid once slot.stream is synchronised and until that slot's next step() or rerun_f32().  slot: a _Slot (as step()
        returns it) or its index.  For the clouds whose out["range_flags"] word is non-zero after step()."""
        if not self.range_guard:
            raise RuntimeError("rerun_f32() needs AncshPipeline(..., arithmetic='f16x2', range_guard=True)")
        sl = self.slots[slot] if isinstance(slot, int) else slot
        with torch.cuda.stream(sl.stream):
            self._replay(sl, f32=True)
        return sl.out32

    def synchronize(self):
        for sl in self.slots:
            sl.stream.synchronize()

    # ---- streaming: raw clouds in, pose records out (raw_capacity set) ---------------------------------------------------------
    def submit(self, clouds, norm_factors, seed=None, tag=None, cloud_base=0, gt=None, frame=None, rig=None):
        """Enqueue one batch of raw clouds (asynchronous): clouds = 1..batch_size (n_raw, 4) float32 arrays [x y z joint_cls] of any
        sizes (all of them, plus the padding below, <= raw_capacity rows), norm_factors = one finite float per cloud.
        joint_source="predicted": (n_raw, 3) xyz clouds, or (n_raw, 4) ones whose 4th column is ignored.  A short batch
        is padded with copies of its first cloud, whose records retire() drops.  seed: the generator key of the batch's sampling and
        of its pose fit (stage B uses seed + 1); None = self.seed + 2k for the k-th submitted batch (2k + 1 is its stage B).
        cloud_base (keyed=True only; written into the pinned header with the seed): the global index of the batch's cloud 0 -- cloud b
        is sampled and fitted as global cloud cloud_base + b; (cloud_base + batch_size) * num_parts must stay below 2^20.
        gt (a pipeline built with ground_truth=True; ValueError on any other): the valid clouds' (n_valid, K, 19) ground truth
        (pose.gt_errors.pack_ground_truth); None = all-NaN rows, a batch without ground truth.  Padding clouds get NaN rows.
        A pipeline built with point_ground_truth=True takes (n_raw, 18) clouds (dataset.pack_cloud's rows) whichever the joint source, and
        frame (ValueError on any other pipeline): the valid clouds' (n_valid, 13) ground-truth NAOCS poses of part 0
        (pose.point_gt.pack_joint_frame), staged with the header as gt is; None = NaN rows, which blank the joint columns.
        A pipeline built with build_point_gt=True takes (n_raw, 7) annotated clouds (dataset.pack_annotated_cloud: x y z | cx cy cz | part,
        the part an integer in [0, num_parts)) instead, and rig (ValueError on any other pipeline, and when it is missing on this one): the
        valid clouds' (n_valid, RIG_WIDTH(num_parts)) tables (dataset.pack_joint_rig), staged with the header as frame is; the padding
        clouds of a short batch take the first cloud's.
        A pipeline built with build_gt_pose=True fits the ground-truth poses itself: frame is a ValueError (the device builds it), and of gt
        only columns 13..15, the box extents, are read (pose.gt_errors.pack_box_extents).
        Bad input raises ValueError before anything is enqueued; a full in-flight window (every slot submitted, not retired) raises
        RuntimeError.  Either way the pipeline stays usable."""
        o = self.opts
        if o.raw_capacity is None:
            raise RuntimeError("submit() needs AncshPipeline(..., raw_capacity=<rows>)")
        if o.depth_dtype is not None:
            raise RuntimeError("a pipeline built with depth_capacity takes depth frames: submit_depth()")
        refuse_built_frame(o, frame, "AncshPipeline")
        side = dict(gt=gt, frame=frame, rig=rig)

        def front():
            require_side_inputs(o.inputs, side)
            valid, nf = o.rows.check(clouds, norm_factors, self.K, self.B)
            padded = valid + [valid[0]] * (self.B - len(valid))
            rows = sum(c.shape[0] for c in padded)
            if rows > o.raw_capacity:
                raise ValueError("the batch needs %d raw rows (short batches are padded with their first cloud), raw_capacity is %d"
                                 % (rows, o.raw_capacity))

            def stage(sl):
                np.concatenate(padded, axis=0, out=sl.np_rows[:rows])
                sl.np_off[0] = 0
                np.cumsum([c.shape[0] for c in padded], out=sl.np_off[1:])
                return [(sl.staged_rows[:rows], sl.h_rows[:rows])]
            return len(valid), nf, stage
        self._enqueue(front, seed, tag, cloud_base, **side)

    def submit_depth(self, frames, norm_factors, cameras=None, depth_scale=1.0, seed=None, tag=None, cloud_base=0, gt=None, scene=None,
                     frame=None, rig=None):
        """Enqueue one batch of depth frames (asynchronous; a pipeline built with depth_capacity): frames = 1..batch_size tuples
        (depth_crop (h, w) of the pipeline's depth_dtype, mask_crop (h, w) bool / integer or None = every pixel, (row0, col0) = the crop's
        origin in the full image); norm_factors = one finite float per frame; cameras = one 6-vector of unprojection coefficients
        (depth.unprojection_from_intrinsics / unprojection_from_projmat) or one per frame; depth_scale = one value or one per frame
        (depth unit -> the cloud's unit).  The valid pixels of each crop (mask non-zero and a usable depth) become the frame's cloud on the
        device; a frame without one gives an all-NaN record and count 0.  A short batch is padded with its first frame (whose pixels are
        not copied again -- with sensor=, whose draws follow the frame's index, they are, into pixels of their own), and all crops, padding included, must fit depth_capacity pixels.  seed, tag, cloud_base, gt: as submit().
        A pipeline built with point_ground_truth=True, build_point_gt=True takes annotated frames: the second element of a frame is its
        link-label crop (h, w), an integer array whose values outside [0, nlinks) are not object, and scene = one (240,) float64 table
        (depth.pack_frame_scene) or one per frame carries the camera, the depth scale and every link's map -- cameras stays None and
        depth_scale is not read.  A frame in which a used link has fewer valid pixels than its scene's minimum gives an all-NaN record and
        count 0, like one without a valid pixel.  rig (required) and frame: as submit() takes them.  scene, frame or rig on any other
        pipeline: ValueError.  Bad input
        raises ValueError before anything is enqueued; a full in-flight window raises RuntimeError.  Either way the pipeline stays usable."""
        o = self.opts
        if o.depth_dtype is None:
            raise RuntimeError("submit_depth() needs AncshPipeline(..., depth_capacity=<pixels>)")
        if o.posed:
            raise RuntimeError("a pipeline built with kinematics= builds its frames from poses on the device: submit_posed()")
        if o.render:
            raise RuntimeError("a pipeline built with render_mesh= renders its frames on the device: submit_render()")
        annotated = o.link_counts
        refuse_built_frame(o, frame, "AncshPipeline")
        refuse_side_inputs(o.inputs, dict(scene=scene), "AncshPipeline")

        def front():
            from .depth import check_annotated_frames, check_depth_frames, pack_depth_frames
            if annotated:
                if scene is None or rig is None or cameras is not None:
                    raise ValueError(SIDE["scene"].missing)
                depths, masks, origins, nf, scenes = check_annotated_frames(frames, norm_factors, scene, o.depth_dtype, self.K, self.B)
            else:
                depths, masks, origins, nf, cam = check_depth_frames(frames, norm_factors, cameras, depth_scale, o.depth_dtype, self.B)
            n_valid = len(depths)
            pad = self.B - n_valid if o.sensor else 0     # a sensor's draws follow the frame's index: its padding frames get pixels of their own
            pixels = sum(d.size for d in depths) + pad * depths[0].size
            self._check_depth_capacity(pixels + (self.B - n_valid - pad) * depths[0].size)

            def stage(sl):
                pack_depth_frames(depths + depths[:1] * pad, masks + masks[:1] * pad, list(origins) + [origins[0]] * pad, sl.np_pix, sl.np_mask,
                                  sl.np_geom)
                if not pad:
                    sl.np_geom[n_valid:] = sl.np_geom[0]   # the padding clouds alias the first frame's pixels
                if not annotated:                          # (the scenes of annotated frames carry the camera)
                    sl.np_cam[:n_valid] = cam
                    sl.np_cam[n_valid:] = cam[0]
                self._stage_dest(sl, n_valid)
                return [(sl.pix[:pixels], sl.h_pix[:pixels]), (sl.mask[:pixels], sl.h_mask[:pixels])]
            return n_valid, nf, stage, dict(scene=scenes) if annotated else {}
        self._enqueue(front, seed, tag, cloud_base, gt=gt, frame=frame, rig=rig)

    def submit_render(self, crops, norm_factors, render, scene, rig, gt=None, frame=None, seed=None, tag=None, cloud_base=0):
        """Enqueue one batch of frames the step renders itself (asynchronous; a pipeline built with render_mesh=): crops = 1..batch_size
        tuples (h, w, (row0, col0)) -- the crop of the full image to render and its origin --, norm_factors = one finite float per
        frame, render = one (208,) float64 table (depth.pack_render_scene) or one per frame, scene and rig (both required), gt, frame,
        seed, tag, cloud_base: as submit_depth takes them for annotated frames.  Only the geometry and the tables cross to the device:
        ancsh_render_depth_labels writes the slot's depth and label crops in front of ancsh_depth_annotate_stream.  A short batch is
        padded with its first crop (which the padding frames render again, where it lies; with sensor=: into pixels of their own), and all crops, padding included, must fit
        depth_capacity pixels.  Bad input raises ValueError before anything is enqueued; a full in-flight window raises RuntimeError.
        Either way the pipeline stays usable."""
        o = self.opts
        if not o.render:
            raise RuntimeError("submit_render() needs AncshPipeline(..., %s); depth frames made elsewhere travel through submit_depth()"
                               % SIDE["render"].built_with)
        if o.posed:
            raise RuntimeError("a pipeline built with kinematics= builds the render and scene tables itself: submit_posed()")
        refuse_built_frame(o, frame, "AncshPipeline")

        def front():
            from .depth import check_crops, check_scenes
            if render is None or scene is None or rig is None:
                raise ValueError(SIDE["render"].missing)
            n_valid, nf, padded, stage = self._crop_front(check_crops, crops, norm_factors)
            scenes = check_scenes(scene, n_valid, self.K)
            self._check_depth_capacity(padded)
            return n_valid, nf, stage, dict(scene=scenes)
        self._enqueue(front, seed, tag, cloud_base, render=render, gt=gt, frame=frame, rig=rig)

    def submit_posed(self, crops, norm_factors, pose, rig, gt=None, frame=None, seed=None, tag=None, cloud_base=0):
        """Enqueue one batch of frames the step poses, renders and annotates itself (asynchronous; a pipeline built with render_mesh= and
        kinematics=): crops = 1..batch_size tuples (h, w, (row0, col0)) as submit_render takes them, or (h, w, None) for a crop centred on
        the projected object (ancsh_render_centre_crops; the origin stays on the device -- depth.centre_crops returns it); norm_factors =
        one finite float per frame; pose = one (32,) float64 row (depth.pack_pose: joint values and the view matrix) or one per frame; rig
        (required), gt, frame, seed, tag, cloud_base: as submit_render takes them.  32 doubles per frame cross to the device in place of the
        two tables' 448: ancsh_pose_scene_build writes the slot's render and scene tables in front of the renderer.  A short batch is padded
        with its first crop and pose.  Bad input raises ValueError before anything is enqueued; a full in-flight window raises
        RuntimeError.  Either way the pipeline stays usable."""
        o = self.opts
        if not o.posed:
            raise RuntimeError("submit_posed() needs AncshPipeline(..., %s); this pipeline takes %s()"
                               % (SIDE["pose"].built_with, "submit_render" if o.render else "submit_depth" if o.depth_dtype is not None else "submit"))
        refuse_built_frame(o, frame, "AncshPipeline")

        def front():
            from .depth import check_posed_crops
            if pose is None or rig is None:
                raise ValueError(SIDE["pose"].missing)
            n_valid, nf, padded, stage = self._crop_front(check_posed_crops, crops, norm_factors)
            self._check_depth_capacity(padded)
            return n_valid, nf, stage
        self._enqueue(front, seed, tag, cloud_base, pose=pose, gt=gt, frame=frame, rig=rig)

    def _crop_front(self, check, crops, norm_factors):
        """What submit_render's and submit_posed's front() share: check = depth.check_crops or depth.check_posed_crops -> (valid frames, their
        norm factors, the pixels of the batch with its padding -- for _check_depth_capacity, once the caller's own tables are checked --,
        stage).  The padding frames alias the first frame's pixels: they render the same bytes (posed: from the same pose, to the same origin)."""
        from .depth import check_norm_factors
        shapes, origins = check(crops, self.B)
        n_valid = len(shapes)
        nf = check_norm_factors(norm_factors, n_valid)
        padded = sum(h * w for h, w in shapes) + (self.B - n_valid) * shapes[0][0] * shapes[0][1]

        def stage(sl):
            self._stage_crops(sl, shapes, origins)
            self._stage_dest(sl, n_valid)
            return []
        return n_valid, nf, padded, stage

    def _check_depth_capacity(self, pixels):
        if pixels > self.opts.depth_capacity:
            raise ValueError("the batch needs %d pixels (short batches are padded with their first frame), depth_capacity is %d"
                             % (pixels, self.opts.depth_capacity))

    def _stage_crops(self, sl, shapes, origins):
        """The geometry rows of crops the step renders: a padding frame renders the first crop again where it lies -- or, with a sensor, whose
        draws follow the frame's index, into pixels of its own behind the batch's (the capacity check has counted them either way).  So it
        does with reprojection: a padding frame is fitted under its own key, and its predicted crop is not the first frame's."""
        from .depth import pack_crop_geometry
        n_valid = len(shapes)
        pad = self.B - n_valid if self.opts.sensor or self.opts.reprojection or self.opts.refine else 0
        pack_crop_geometry(shapes + shapes[:1] * pad, list(origins) + [origins[0]] * pad, sl.np_geom)
        if not pad:
            sl.np_geom[n_valid:] = sl.np_geom[0]

    def _stage_dest(self, sl, n_valid):
        """label_images / annotated_images: a valid frame's images lie where its crop does; a padding cloud writes none."""
        if self.opts.label_images or self.opts.annotated_images:
            sl.np_dest[:n_valid] = sl.np_geom[:n_valid, 0]
            sl.np_dest[n_valid:] = -1

    def _enqueue(self, front, seed, tag, cloud_base, **side):
        """What submit() and submit_depth() share.  front() checks the front end's arguments and capacity (ValueError) and returns
        (valid clouds, their norm factors, stage[, side inputs it has checked itself]); stage(sl) fills the slot's pinned staging and
        returns its (device, pinned) copies.  side: the batch's side inputs by name (stream.SIDE_INPUTS).
        Checks in order: the key, front()'s, the ground truth, the frames, the rigs, the in-flight window (RuntimeError); only then prepare().  On the slot's
        stream: the H2D copies (the side inputs' with the header's) with h2d_done right behind them, the step, the outputs' D2H copies (the record's first, right behind the replay: the
        next replay's pool reuses its block, see step()), d2h_done."""
        from .dataset import check_stream_key, seed_bits
        o = self.opts
        if o.keyed:
            cloud_base = check_stream_key(cloud_base, self.B, self.K)
        elif cloud_base != 0:
            raise ValueError("cloud_base needs AncshPipeline(..., keyed=True)")
        n_valid, nf, stage, *checked = front()
        side = check_side_inputs(o.inputs, dict(side, **(checked[0] if checked else {})), n_valid, self.K, "AncshPipeline", self.ninst)
        if len(self._inflight) == len(self.slots):
            raise RuntimeError("all %d slots hold unretired batches: retire() one first" % len(self.slots))
        if not self._prepared:
            self.prepare()
        seed = self.seed + 2 * self._submitted if seed is None else int(seed)
        sl = self.slots[self._next]
        sl.h2d_done.synchronize()                  # the previous batch's copies out of the pinned staging have completed
        sl.np_seed[0] = seed_bits(seed)
        if o.keyed:
            sl.np_base[0] = cloud_base
        copies = stage(sl)
        sl.np_nf[:n_valid] = nf
        sl.np_nf[n_valid:] = nf[0]
        for inp in o.inputs:
            stage_side_input(inp, getattr(sl, "np_" + inp.name), side[inp.name], n_valid)
            copies.append((getattr(sl, inp.name), getattr(sl, "h_" + inp.name)))
        cur = torch.cuda.current_stream(self.device)
        if cur != sl.stream and not cur.query():
            sl.stream.wait_stream(cur)
        with torch.cuda.stream(sl.stream):
            for dev, host in copies + [(sl.hdr, sl.h_hdr)]:
                dev.copy_(host, non_blocking=True)
            sl.h2d_done.record(sl.stream)
            self._replay(sl)
            for out in sl.outputs.values():
                out.copy_out(sl, n_valid)
            sl.d2h_done.record(sl.stream)
        self._next = (self._next + 1) % len(self.slots)
        self._submitted += 1
        self._inflight.append((sl, tag, seed, n_valid))

    def retire(self, flags=False, articulation=False, dense=False, label_images=False, link_counts=False, annotated_images=False):
        """Wait for the oldest submitted batch -> (tag, seed, record): record = its valid clouds' (n_valid, K, 26) float64 pose
        records, a fresh host array (a pipeline built with fit_quality, ground_truth, point_ground_truth, reprojection or refine: the
        (n_valid, K, pipe.record_layout.width) records -- the same 26 columns, then the blocks those options build, in pose.record.BLOCKS'
        order; pipe.record_layout.block(record, name) cuts one out; flagged clouds take every column from the f32 graph).
        Range guard: when a valid cloud's flag word is non-zero, the slot's f32 graph refits the batch
        (its raw rows and header are still in the slot: a slot is reused only after it retires) and the flagged clouds' records are
        the f32 ones (pipe.f32_reruns counts these batches).  flags=True: (tag, seed, record, flag words (n_valid,) int32; zeros
        without the guard).  articulation=True (a pipeline built with articulation=True): + the (n_valid, K, 12) float64 articulation
        block (flagged clouds: the f32 graph's rows, like their records); built with joint_states=True it is the (n_valid, K, 20) block
        whose columns 12..19 hold the joint state.  dense=True (a pipeline built with dense=True): + (labels (R,)
        int32, values (R, 7) float32, offsets (n_valid+1,) int64) as the last element: the valid clouds' R raw rows in submission order,
        cloud c's rows [offsets[c], offsets[c+1]) (raw_point_labels; flagged clouds: the f32 graph's rows).  A pipeline built with
        depth_capacity appends the valid-pixel counts (n_valid,) int32 of the batch's frames as the last element.  label_images=True (a
        pipeline built with label_images=True): + a list with one (labels (h, w) int32, values (h, w, 7) float32) pair per valid frame,
        aligned with the submitted crop, behind the articulation block and in front of the counts: a valid pixel holds its row's label and
        [W of the label | part NOCS | NAOCS] (as dense), every other pixel -1 / NaN (flagged clouds: the f32 graph's images).
        The tuple's order is stream.RESULT_NAMES (stream.unpack_results reads it by name).  link_counts=True (a pipeline of annotated
        depth frames: depth_capacity with point_ground_truth=True, build_point_gt=True): + the (n_valid, 16) int32 valid pixels per link
        of the batch's frames, behind everything else.  annotated_images=True (a pipeline of annotated frames built with
        annotated_images=True): + a list with one (labels (h, w) int32, values (h, w, 7) float32, gt_labels (h, w) int32, gt_values (h, w, 6)
        float32) tuple per valid frame, aligned with the submitted (or rendered) crop, where label_images' pairs would stand: a valid pixel
        holds its row's predicted label and [W of the label | part NOCS | NAOCS], its row's ground-truth part and [part NOCS | NAOCS];
        every other pixel, and every pixel of a frame without rows, -1 / NaN (flagged clouds: the f32 graph's images)."""
        check_built_with(self.opts, "retire", "AncshPipeline", articulation=articulation, dense=dense, label_images=label_images,
                         annotated_images=annotated_images, link_counts=link_counts)
        if not self._inflight:
            raise RuntimeError("retire(): no batch in flight")
        sl, tag, seed, n_valid = self._inflight.popleft()
        sl.d2h_done.synchronize()
        asked = dict(flags=flags, articulation=articulation, dense=dense, label_images=label_images, annotated_images=annotated_images,
                     counts=self.opts.depth_dtype is not None, link_counts=link_counts)
        # the flag words decide the refit whether or not the caller asked for them
        want = [o for o in sl.outputs.values() if o.name in ("record", "flags") or asked.get(o.name)]
        got = {o.name: o.value(sl, n_valid) for o in want}
        got.setdefault("flags", np.zeros((n_valid,), np.int32))
        hit = np.flatnonzero(got["flags"])
        if hit.size:
            refit = [o for o in want if o.host32 is not None]
            self.rerun_f32(sl)
            with torch.cuda.stream(sl.stream):
                for o in refit:
                    o.copy_out(sl, n_valid, f32=True)
            sl.stream.synchronize()
            for o in refit:
                o.patch(got[o.name], o.value(sl, n_valid, f32=True), hit)
            self.f32_reruns += 1
        if self.opts.link_counts:
            # annotated frames: a frame without rows (no valid pixel, or a link below the minimum: the reference skips it) carries no
            # information.  Its pose record and its losses are NaN from the device; ancsh_point_gt_rec's two point counts read 0 there (no
            # sampled point has a part), and are blanked here, so that the whole row is NaN
            got["record"][got["counts"] == 0] = np.nan
        return pack_results(dict(got, tag=tag, seed=seed), **asked)

    def stream_batches(self, batches, flags=False, articulation=False, dense=False):
        """(`stream` is slot 0's HIP stream.)  Generator over submit / retire: batches yields (clouds, norm_factors) or (clouds, norm_factors, tag) (tag defaults to the
        batch's index) -- a pipeline built with ground_truth=True: (clouds, norm_factors, gt) or (clouds, norm_factors, gt, tag), gt as
        submit() takes it; built with point_ground_truth=True: the frame (submit()'s) behind the ground truth, in front of the tag; built with build_point_gt=True: the rig (submit()'s) behind the frame, in front of the tag --; up to len(slots) batches stay in flight; yields (tag, seed, record) in submission order (flags=True: + the
        flag words; articulation=True: + the (n_valid, K, 12) articulation block; dense=True: + (labels, values, offsets) of the raw rows,
        last -- see retire())."""
        check_built_with(self.opts, "stream_batches", "AncshPipeline", articulation=articulation, dense=dense)

        def submit(k, item):
            clouds, norm_factors, side, tag = split_item(item, self.opts.inputs, k)
            self.submit(clouds, norm_factors, tag=tag, **side)
        yield from pump(batches, self._inflight, len(self.slots), submit, lambda: self.retire(flags, articulation, dense))

    def stream_depth_batches(self, batches, cameras=None, depth_scale=1.0, flags=False, articulation=False, label_images=False,
                             link_counts=False, annotated_images=False):
        """stream_batches over submit_depth: batches yields (frames, norm_factors) or (frames, norm_factors, tag) or, with a dict as the
        last item, per-batch overrides of submit_depth's cameras / depth_scale / seed / cloud_base / gt / scene / frame / rig (annotated
        frames travel with their scene and rig there); yields what retire() returns, in
        submission order, the valid-pixel counts last (label_images=True: the per-frame image pairs in front of them; link_counts=True,
        annotated frames: the (n_valid, 16) per-link counts behind them; annotated_images=True, annotated frames: the per-frame image
        4-tuples where label_images' pairs would stand)."""
        check_built_with(self.opts, "stream_depth_batches", "AncshPipeline", articulation=articulation, label_images=label_images,
                         annotated_images=annotated_images)

        def submit(k, item):
            item = tuple(item)
            kw = dict(cameras=cameras, depth_scale=depth_scale)
            if isinstance(item[-1], dict):
                kw.update(item[-1])
                item = item[:-1]
            self.submit_depth(item[0], item[1], tag=item[2] if len(item) > 2 else k, **kw)
        yield from pump(batches, self._inflight, len(self.slots), submit,
                        lambda: self.retire(flags, articulation, label_images=label_images, link_counts=link_counts,
                                            annotated_images=annotated_images))

    def stream_render_batches(self, batches, flags=False, articulation=False, link_counts=False, annotated_images=False):
        """stream_depth_batches over submit_render: batches yields (crops, norm_factors, {render=, scene=, rig=, gt=, frame=, seed=,
        cloud_base=}) or the same with a tag behind the dict (the tag defaults to the batch's index); yields what stream_depth_batches
        yields for the same frames, in submission order: the valid-pixel counts last, link_counts=True: the (n_valid, 16) per-link
        counts behind them; annotated_images=True: the per-frame image 4-tuples in front of the counts."""
        check_built_with(self.opts, "stream_render_batches", "AncshPipeline", articulation=articulation, link_counts=link_counts,
                         annotated_images=annotated_images)

        def submit(k, item):
            item = tuple(item)
            if len(item) < 3 or not isinstance(item[2], dict):
                raise ValueError("a stream_render_batches item is (crops, norm_factors, {render=, scene=, rig=, ...}[, tag])")
            self.submit_render(item[0], item[1], tag=item[3] if len(item) > 3 else k, **item[2])
        yield from pump(batches, self._inflight, len(self.slots), submit,
                        lambda: self.retire(flags, articulation, link_counts=link_counts, annotated_images=annotated_images))

    def stream_posed_batches(self, batches, flags=False, articulation=False, link_counts=False, annotated_images=False):
        """stream_render_batches over submit_posed: batches yields (crops, norm_factors, {pose=, rig=, gt=, frame=, seed=, cloud_base=}) or
        the same with a tag behind the dict (the tag defaults to the batch's index); yields what stream_render_batches yields for the same
        frames."""
        check_built_with(self.opts, "stream_posed_batches", "AncshPipeline", articulation=articulation, link_counts=link_counts,
                         annotated_images=annotated_images)

        def submit(k, item):
            item = tuple(item)
            if len(item) < 3 or not isinstance(item[2], dict):
                raise ValueError("a stream_posed_batches item is (crops, norm_factors, {pose=, rig=, ...}[, tag])")
            self.submit_posed(item[0], item[1], tag=item[3] if len(item) > 3 else k, **item[2])
        yield from pump(batches, self._inflight, len(self.slots), submit,
                        lambda: self.retire(flags, articulation, link_counts=link_counts, annotated_images=annotated_images))
