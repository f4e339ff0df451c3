"""What AncshPipeline's streaming half (submit / submit_depth / retire / stream_*) and dist.ShardedPipeline's share, each written once:
the slot header's layout, the label buffers, the table of streamed outputs, the table of row kinds, the table of side inputs, the one
check of the options both constructors take, the names and order of what retire() returns, the "asked for x but not built with x"
guard, and the submit-when-room / retire-when-full loop.  Host-side plumbing only: nothing here launches a kernel."""
import collections

import numpy as np
import torch

from . import dataset, depth as depth_mod
from .pose import gt_errors, joint_params, joint_values as joint_values_mod, point_gt, quality, refinement as refinement_mod, reprojection as reprojection_mod
from .pose.record import RecordLayout

# ---- the slot header ---------------------------------------------------------------------------------------------------------
# [seed (int64 bits) -- keyed: the 16-byte key block (ancsh_stream_key: seed, cloud_base, reserved) -- | offsets (B+1) int32 |
#  norm factors (B) float32 | depth: geom (B x GEOM_WORDS) int32 | cam (B x CAM_WORDS) float32 | label_images / annotated_images: dest (B) int32]
# The kernels read it through the pointers AncshPipeline._sample passes: the order is theirs, not this module's to change.
HeaderLayout = collections.namedtuple("HeaderLayout", "key seed base off nf geom cam dest words")


def header_layout(B, keyed=False, depth=False, label_images=False):
    """The int32 word ranges (slices; None = not in this header) of a slot header for B clouds, and its length `words`."""
    from .depth import CAM_WORDS, GEOM_WORDS
    at = 4 if keyed else 2
    parts = dict(key=slice(0, at), seed=slice(0, 2), base=slice(2, 3) if keyed else None)
    for name, n in (("off", B + 1), ("nf", B), ("geom", GEOM_WORDS * B if depth else 0), ("cam", CAM_WORDS * B if depth else 0),
                    ("dest", B if depth and label_images else 0)):
        parts[name] = slice(at, at + n) if n else None
        at += n
    return HeaderLayout(words=at, **parts)


def label_buffers(capacity, device=None):
    """(labels (capacity,) int32 filled -1, values (capacity, 7) float32 filled NaN): what ancsh_raw_point_labels and
    ancsh_depth_label_images write per raw row / per pixel.  On `device`, or (None) in pinned host memory."""
    from .dataset import DENSE_VALUES
    pair = (torch.full((capacity,), -1, dtype=torch.int32, device=device),
            torch.full((capacity, DENSE_VALUES), float("nan"), dtype=torch.float32, device=device))
    return pair if device is not None else tuple(t.pin_memory() for t in pair)


# ---- the table of streamed outputs ---------------------------------------------------------------------------------------------
# An output's extent for a batch of n_valid clouds in slot sl (padding clouds follow the valid ones in every buffer): leading rows to copy.
def per_cloud(sl, n_valid):
    return n_valid


def per_raw_row(sl, n_valid):          # the batch's own offsets: a slot's staging is rewritten only after it retires
    return int(sl.np_off[n_valid])


def per_pixel(sl, n_valid):            # the batch's own geometry {start h w row0 col0}, likewise
    return int(sum(int(g[1]) * int(g[2]) for g in sl.np_geom[:n_valid]))


# How retire() turns an output's pinned buffers into the value it returns (fresh host arrays) ...
def take_rows(host, sl, n_valid, n):
    return host[0][:n].numpy().copy()


def take_dense(host, sl, n_valid, n):
    return host[0][:n].numpy().copy(), host[1][:n].numpy().copy(), sl.np_off[:n_valid + 1].astype(np.int64)


def take_images(host, sl, n_valid, n):
    from .depth import cut_label_images
    return cut_label_images(host[0].numpy()[:n], host[1].numpy()[:n], [(int(g[1]), int(g[2])) for g in sl.np_geom[:n_valid]])


def take_annotated_images(host, sl, n_valid, n):
    from .depth import cut_annotated_images
    return cut_annotated_images(*(h.numpy()[:n] for h in host), [(int(g[1]), int(g[2])) for g in sl.np_geom[:n_valid]])


# ... and how the f32 refit's value replaces the flagged clouds' part of it
def patch_items(value, redo, hit):     # indexed by cloud: array rows, or a list of per-frame images
    for c in hit:
        value[c] = redo[c]


def patch_dense(value, redo, hit):     # (labels, values, offsets): cloud c owns rows [offsets[c], offsets[c+1])
    off = value[2]
    for c in hit:
        a, e = off[c], off[c + 1]
        value[0][a:e], value[1][a:e] = redo[0][a:e], redo[1][a:e]


class Output(object):
    """One streamed output of a slot: where the captured step leaves it on the device, its pinned host twin(s), and how a batch's part
    of it is copied out, returned and patched.  source(sl, f32) -> the device tensors behind slot sl's last replay (the f32 graph's for
    f32=True); make_host() -> their pinned twins, one per tensor; refit: the range guard's f32 graph has its own, with their own twins."""

    def __init__(self, name, source, make_host, refit=False, extent=per_cloud, take=take_rows, patch=patch_items):
        self.name, self.source, self.extent, self.take, self.patch = name, source, extent, take, patch
        self.host = make_host()
        self.host32 = make_host() if refit else None

    def copy_out(self, sl, n_valid, f32=False):
        """Enqueue the batch's device -> pinned copies on the current stream."""
        n = self.extent(sl, n_valid)
        for h, d in zip(self.host32 if f32 else self.host, self.source(sl, f32)):
            h[:n].copy_(d[:n], non_blocking=True)

    def value(self, sl, n_valid, f32=False):
        """The batch's value from the pinned twins (once the copies have completed)."""
        return self.take(self.host32 if f32 else self.host, sl, n_valid, self.extent(sl, n_valid))


# ---- the row kinds of a stream -----------------------------------------------------------------------------------------------------
# What a slot's rows are: nchan columns in the slot's raw_rows, `staged` columns in what travels in (annotated rows are built into 18-column
# rows on the device), check(clouds, norm_factors, K, most) -> (clouds, norm factors) or ValueError, and fill(rows, rs, K, n): the columns
# behind x y z of the n random rows a slot holds until its first submit (the draws, in this order, are what prepare() sees).
RowKind = collections.namedtuple("RowKind", "name nchan staged check fill")


def _fill_labelled(rows, rs, K, n):
    rows[:, 3] = rs.randint(0, K, n)


def _fill_point_gt(rows, rs, K, n):
    rows[:, 3] = rs.randint(0, K, n)
    rows[:, 4:dataset.NCHAN - 1] = rs.uniform(0.0, 1.0, (n, dataset.NCHAN - 5))
    rows[:, dataset.NCHAN - 1] = rs.randint(0, K, n)


def _fill_annotated(rows, rs, K, n):
    rows[:, 3:6] = rs.uniform(0.0, 1.0, (n, 3))
    rows[:, 6] = rs.randint(0, K, n)


ROW_KINDS = {k.name: k for k in (
    RowKind("labelled", dataset.RAW_NCHAN, dataset.RAW_NCHAN, lambda c, nf, K, most: dataset.check_raw_clouds(c, nf, most),
            _fill_labelled),                                                                                      # x y z joint_cls
    RowKind("xyz", 3, 3, lambda c, nf, K, most: dataset.check_raw_clouds(c, nf, most, xyz_only=True), lambda rows, rs, K, n: None),
    RowKind("point_gt", dataset.NCHAN, dataset.NCHAN, lambda c, nf, K, most: point_gt.check_point_clouds(c, nf, most), _fill_point_gt),
    RowKind("annotated", dataset.NCHAN, dataset.ANNOTATED_NCHAN, lambda c, nf, K, most: dataset.check_annotated_clouds(c, nf, K, most),
            _fill_annotated))}


def fill_rows(kind, rows, K):
    """The (capacity, kind.staged) rows a slot holds until its first submit: a defined, non-degenerate input for prepare()'s passes."""
    rs = np.random.RandomState(0)
    rows[:, :3] = rs.uniform(-0.5, 0.5, (rows.shape[0], 3))
    kind.fill(rows, rs, K, rows.shape[0])


# ---- the table of side inputs ------------------------------------------------------------------------------------------------------
# What travels in with a batch besides its rows or pixels, one float64 block per cloud, staged in pinned memory and copied with the
# header.  option: the Options flag it is built with, built_with: that option as the refusal spells it; shape(K): a cloud's block;
# fill(K, unit): what a slot holds until its first submit (unit: the unit camera and depth scale of a depth slot's default crops);
# check(value, n, K) -> the (n,) + shape(K) array or ValueError (None: the front end has checked it); pad: what the padding clouds of a
# short batch get, "nan" (and so does a whole batch without the input) or "first" (a copy of the first cloud's); missing: the
# ValueError of a submit without a required input (None: the input is optional).
SideInput = collections.namedtuple("SideInput", "name option built_with shape dtype fill check pad missing")


def unit_scene(K, unit):
    """One link with the identity map behind the camera `unit` = (6 unprojection coefficients, depth scale): rank 0, part 0, M = [I | 0]."""
    s = np.zeros(depth_mod.SCENE_WIDTH)
    s[0:6], s[6], s[7:13], s[13], s[14] = unit[:6], unit[6], unit[:6], 10, 1
    s[depth_mod.SCENE_HEAD + 2:depth_mod.SCENE_HEAD + 14] = np.eye(4)[:3].reshape(12)
    return s


ANNOTATED = "point_ground_truth=True, build_point_gt=True"
SIDE_INPUTS = (             # in the order of their H2D copies; gt, frame, rig is also their order in a stream_batches item
    SideInput("scene", "link_counts", "depth_capacity=<pixels>, " + ANNOTATED, lambda K: (depth_mod.SCENE_WIDTH,), torch.float64, unit_scene,
              None, "first",
              "a pipeline built with " + ANNOTATED + " takes annotated frames: submit_depth(frames, norm_factors, scene=..., rig=...) needs "
              "one depth.pack_frame_scene table and one dataset.pack_joint_rig table per frame, and cameras=None (the scene carries the "
              "camera)"),
    SideInput("gt", "ground_truth", "ground_truth=True", lambda K: (K, gt_errors.GT_WIDTH), torch.float64, lambda K, unit: np.nan,
              gt_errors.check_ground_truth, "nan", None),
    SideInput("frame", "point_ground_truth", "point_ground_truth=True", lambda K: (point_gt.FRAME_WIDTH,), torch.float64, lambda K, unit: np.nan,
              lambda v, n, K: point_gt.check_frames(v, n), "nan", None),
    SideInput("rig", "build_point_gt", ANNOTATED, lambda K: (dataset.RIG_WIDTH(K),), torch.float64, lambda K, unit: dataset.identity_rig(K),
              dataset.check_rigs, "first",
              "a pipeline built with build_point_gt=True builds every cloud's rows from its rig: submit(..., rig=...) needs one "
              "dataset.pack_joint_rig table per cloud"))
SIDE = {inp.name: inp for inp in SIDE_INPUTS}


def unit_render(K, unit):
    """unit_scene's inverse: the pixel map of the camera `unit`, one link with the identity map."""
    r = np.zeros(depth_mod.RENDER_WIDTH)
    r[0], r[2], r[4], r[5] = 1.0 / unit[0], -unit[2] / unit[0], 1.0 / unit[4], -unit[5] / unit[4]
    r[6], r[7], r[8] = unit[6], 1e-6, 1
    r[depth_mod.RENDER_HEAD:depth_mod.RENDER_HEAD + depth_mod.RENDER_LINK] = np.eye(4)[:3].reshape(12)
    return r


# One more row of the table, kept beside it: the render tables of a pipeline that renders its frames itself (render_mesh=).  It is the
# first H2D copy of such a batch (the step's first launch reads it) and, like scene, it travels by name, never by position in an item.
RENDERED = "depth_capacity=<pixels>, " + ANNOTATED + ", render_mesh=<depth.pack_mesh(...)>"
RENDER_INPUT = SideInput("render", "render", RENDERED, lambda K: (depth_mod.RENDER_WIDTH,), torch.float64, unit_render,
                         lambda v, n, K: depth_mod.check_render_tables(v, n), "first",
                         "a pipeline built with render_mesh= renders its frames: submit_render(crops, norm_factors, render=..., scene=..., "
                         "rig=...) needs one depth.pack_render_scene table per frame")
ALL_INPUTS = (RENDER_INPUT,) + SIDE_INPUTS
SIDE[RENDER_INPUT.name] = RENDER_INPUT


def unit_pose(K, unit):
    """Every joint at 0 and the object 1.5 units in front of the camera: a half turn about x and a step back (the render map is -V o W)."""
    p = np.zeros(depth_mod.POSE_WIDTH)
    p[16:28] = [1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.5]
    return p


# And one beside that: the poses of a pipeline that also builds its tables itself (kinematics=).  `render` and `scene` are then no inputs --
# their slot buffers stay and ancsh_pose_scene_build fills them --, and the pose is the batch's first H2D copy.
POSED = RENDERED + ", kinematics=<depth.pack_kinematics(...)>"
POSE_INPUT = SideInput("pose", "posed", POSED, lambda K: (depth_mod.POSE_WIDTH,), torch.float64, unit_pose,
                       lambda v, n, K: depth_mod.check_poses(v, n), "first",
                       "a pipeline built with kinematics= builds its tables from poses: submit_posed(crops, norm_factors, pose=..., rig=...) "
                       "needs one depth.pack_pose row and one dataset.pack_joint_rig table per frame")
EVERY_INPUT = (POSE_INPUT,) + ALL_INPUTS       # whatever a submit may carry by name (ALL_INPUTS and SIDE_INPUTS are pinned by the tests)
SIDE[POSE_INPUT.name] = POSE_INPUT


def side_host(inp, B, K, unit=None, pin=True):
    """The (B,) + shape(K) host staging of side input `inp`, holding its fill; pinned unless pin=False."""
    host = torch.zeros((B,) + inp.shape(K), dtype=inp.dtype)
    host = host.pin_memory() if pin else host
    host.numpy()[:] = inp.fill(K, unit)
    return host


def refuse_side_inputs(built, given, cls):
    """ValueError for the first side input of `given` = {name: value or None} that a `cls` with the side inputs `built` does not take."""
    for inp in EVERY_INPUT:
        if given.get(inp.name) is not None and inp not in built:
            raise ValueError("%s needs %s(..., %s)" % (inp.name, cls, inp.built_with))


def refuse_built_frame(opts, frame, cls):
    """ValueError for a frame handed to a `cls` built with build_gt_pose=True: the captured step fits it on the device."""
    if opts.build_gt_pose and frame is not None:
        raise ValueError("frame: a %s built with build_gt_pose=True takes no frame -- the device builds it (ancsh_gt_pose_build fits "
                         "part 0's ground-truth NAOCS pose from the sampled rows inside the step)" % cls)


def require_side_inputs(built, given):
    """ValueError for the first of the side inputs `built` that a submit must carry and `given` lacks."""
    for inp in built:
        if inp.missing and given.get(inp.name) is None:
            raise ValueError(inp.missing)


LIBRARY_CHECKS = dict(pose=depth_mod.check_poses, render=depth_mod.check_render_tables)   # the tables that carry a library frame's instance


def check_side_inputs(built, given, n, K, cls, ninst=None):
    """Refuse and check, input by input in the table's order -> {name: the checked (n, ...) array, or None} for the side inputs `built`.
    ninst: the pipeline holds a library of ninst instances, and the pose or render tables must each name one of them."""
    out = {}
    for inp in EVERY_INPUT:
        v = given.get(inp.name)
        if v is not None:
            refuse_side_inputs(built, {inp.name: v}, cls)
            if ninst is not None and inp.name in LIBRARY_CHECKS:
                v = LIBRARY_CHECKS[inp.name](v, n, ninst)
            else:
                v = v if inp.check is None else inp.check(v, n, K)
        if inp in built:
            out[inp.name] = v
    return out


def stage_side_input(inp, view, value, n):
    """Fill a slot's (B, ...) staging `view` from a batch's checked value for its n valid clouds, by the input's padding rule."""
    if inp.pad == "nan":           # NaN rows for the padding clouds and for a batch without the input
        view[:] = np.nan
        if value is not None:
            view[:n] = value
    else:                          # a padding cloud is a copy of the first cloud, side input included
        view[:n] = value
        view[n:] = value[0]


def split_item(item, built, k):
    """A stream_batches item (clouds, norm_factors[, one value per side input of `built`, in the table's order][, tag]) ->
    (clouds, norm_factors, {name: value or None}, tag); the tag defaults to k, the batch's index."""
    names = [inp.name for inp in built]
    side = {name: item[2 + i] if len(item) > 2 + i else None for i, name in enumerate(names)}
    return item[0], item[1], side, item[2 + len(names)] if len(item) > 2 + len(names) else k


# ---- the options both constructors take --------------------------------------------------------------------------------------------
JOINT_SOURCES = ("gt", "predicted")


def check_joint_source(joint_source):
    """-> joint_source if it names one of JOINT_SOURCES; ValueError otherwise (before anything touches the GPU)."""
    if joint_source not in JOINT_SOURCES:
        raise ValueError("joint_source must be one of %s, got %r" % (JOINT_SOURCES, joint_source))
    return joint_source


class Options(collections.namedtuple("Options", "raw_capacity depth_capacity depth_dtype keyed predicted range_guard articulation joint_states "
                                     "fit_quality ground_truth point_ground_truth build_point_gt build_gt_pose dense label_images annotated_images link_counts render posed sensor reprojection "
                                     "coord_regress_loss record_width record_key joint_values art_width rows inputs refine_scale refine_coverage refine_joints silhouette refine")):
    __slots__ = ()

    @property
    def layout(self):
        """The streamed record's blocks (pose.record.RecordLayout): record_width and record_key are its width and key."""
        return RecordLayout.of(self)


OPTION_FLAGS = Options._fields[:Options._fields.index("record_width")]      # the flags; the rest is derived from them


def check_options(batch_size=1, num_points=None, couple=True, inlier_th=0.1, raw_capacity=None, depth_capacity=None, depth_dtype="uint16",
                  keyed=False, range_guard=False, arithmetic="f16x2", articulation=False, joint_states=False, fit_quality=False,
                  ground_truth=False, point_ground_truth=False, build_point_gt=False, dense=False, label_images=False, joint_source="gt",
                  coord_regress_loss="L2", build_gt_pose=False, render_mesh=None, kinematics=None, annotated_images=False, sensor=None,
                  reprojection=False, refine=None, joint_values=False):
    """Every rule between the options of AncshPipeline and dist.ShardedPipeline, checked on the host before anything touches the GPU
    (ValueError) -> Options: the flags, the streamed record's width and the name the step leaves it under (pose.record.BLOCKS: the one
    table of the record's blocks; Options.layout says where each lies), the articulation block's
    width, the row kind (a ROW_KINDS entry; None without a stream) and the side inputs a submit takes (SIDE_INPUTS entries).
    raw_capacity in the result is the slots' capacity: depth_capacity's value on a depth pipeline.
    build_gt_pose (with point_ground_truth): the step fits both ground-truth pose tables itself, so `frame` is no side input and of `gt`
    only the box extents (columns 13..15) are read.
    render_mesh (annotated depth frames only): the step renders the frames itself from this mesh (depth.pack_mesh), so `render` is one
    more side input and no pixel travels in.
    kinematics (with render_mesh): the step builds the render and scene tables itself from this table (depth.pack_kinematics) and one pose
    per frame, so `pose` (POSE_INPUT) takes the place of the `render` and `scene` inputs.
    A library: render_mesh = depth.pack_mesh_library's 4 arrays, alone (submit_render: the instance of a frame in render[9]) or with kinematics
    = the (ninst, 672) stack of its instances' tables (submit_posed: in pose[28]); the two counts must agree.
    annotated_images (annotated depth frames only, rendered and posed ones included): the step carries every row's prediction and ground
    truth back to the pixel it came from -- the link-major twin of label_images, which stays refused there.
    sensor (annotated depth frames only, submitted, rendered, posed or from a library): depth.pack_sensor's table; the step degrades every
    frame as that depth sensor would (ancsh_depth_sensor_model) into a second pair of pixel buffers, which the annotation and the images read.
    reprojection (with render_mesh, whatever else is built): the step re-renders the mesh at the fitted poses and compares it with the frame the
    annotation read; the record's reprojection block (pose.reprojection.COLUMN_NAMES), under the name "record_reproj".
    refine (with render_mesh, whatever else is built): pose.refinement.pack_refine's table; the step refines the record's poses on the depth
    frame (render-and-compare ICP); the record's refinement block (pose.refinement.COLUMN_NAMES), under the name "record_refined".
        A table of pack_refine(silhouette=...) turns the silhouette term on (Options.silhouette): one more launch and 4 bytes per pixel and part.
        A table of pack_refine(joints=...) (with kinematics) turns the joint step on (Options.refine_joints): the parts of an object are
        solved together through their joints, one more launch per pass.
        A table of pack_refine(silhouette=..., coverage=...) turns the coverage term on (Options.refine_coverage): one more launch per pass
        (ancsh_coverage_field) and 8 bytes per pixel and part; with joint values it needs kinematics like a pack_refine(joints=...) table.
        A table of pack_refine(silhouette=..., coverage=..., scale=...) turns the scale unknown on (Options.refine_scale): the loop solves
        s with R and t (ancsh_refine_pass_scale in ancsh_refine_pass_cov's place, no further launch), and column s of the refinement block
        is the refined scale.  It is refused together with joint values in the table.
    joint_values (with kinematics and articulation): the step's last launch (ancsh_joint_values_rec) reads the joint values q off the record's
        and, with refine, the kept refined part poses; its 24 columns (pose.joint_values.COLUMN_NAMES) ride behind the articulation block
        (Options.art_width), as the joint states do: no new name in the result tuple or the record."""
    predicted = check_joint_source(joint_source) == "predicted"
    if articulation:
        if not couple:
            raise ValueError("articulation=True reads the networks' heads: it needs couple=True")
        if num_points is not None and not 1 <= int(num_points) <= joint_params.ARTICULATION_MAX_N:
            raise ValueError("articulation=True keeps the joint medians in LDS: num_points must be in [1, %d], got %d"
                             % (joint_params.ARTICULATION_MAX_N, num_points))
    joint_states = joint_params.check_joint_states(joint_states, bool(articulation))
    joint_values = joint_values_mod.check_joint_values(joint_values, kinematics is not None, bool(articulation))
    fit_quality = quality.check_fit_quality(fit_quality, inlier_th)
    if ground_truth and raw_capacity is None and depth_capacity is None:
        raise ValueError("ground_truth=True travels in with a streamed batch (submit / submit_depth): it needs raw_capacity or "
                         "depth_capacity")
    # (depth frames carry no per-point ground truth -- unless build_point_gt=True makes it from link labels and scenes)
    point_ground_truth = point_gt.check_point_ground_truth(point_ground_truth, bool(articulation),
                                                           depth_capacity is not None and not build_point_gt)
    point_gt.check_loss_type(coord_regress_loss)
    if point_ground_truth and raw_capacity is None and depth_capacity is None:
        raise ValueError("point_ground_truth=True travels in with a streamed batch's raw rows (submit): it needs raw_capacity")
    if build_point_gt and not point_ground_truth:
        raise ValueError("build_point_gt=True builds the rows point_ground_truth=True reads: it needs point_ground_truth=True")
    if build_gt_pose and not point_ground_truth:
        raise ValueError("build_gt_pose=True fits the ground-truth poses from the sampled 18-column rows point_ground_truth=True brings: "
                         "it needs point_ground_truth=True")
    if depth_capacity is not None:
        depth_dtype = depth_mod.check_depth_dtype(depth_dtype)
        if raw_capacity is not None:
            raise ValueError("depth_capacity takes raw_capacity's place: pass one of them")
        if not predicted:
            raise ValueError("depth_capacity needs joint_source='predicted': a depth pixel carries no joint label")
        if dense:
            raise ValueError("dense=True labels the raw rows of an xyz stream; with the depth front end its product is a label "
                             "image: pass label_images=True")
        if not int(batch_size) <= int(depth_capacity) < (1 << 30):
            raise ValueError("depth_capacity must be in [batch_size, 2^30) pixels")
        raw_capacity = depth_capacity = int(depth_capacity)
    if label_images and depth_capacity is None:
        raise ValueError("label_images=True carries the labels back to the pixels of depth frames: it needs depth_capacity")
    link_counts = depth_capacity is not None and bool(build_point_gt)      # annotated depth frames
    if link_counts and label_images:
        raise ValueError("label_images=True carries rows back to pixels in pixel order; the rows of annotated depth frames "
                         "(point_ground_truth=True, build_point_gt=True) are link-major: pass one of them (annotated_images=True gives "
                         "such frames their predicted and ground-truth images)")
    if annotated_images and not link_counts:
        raise ValueError("annotated_images=True carries the predictions and the ground truth of annotated depth frames back to their pixels: "
                         "it needs " + ", ".join(["depth_capacity=<pixels>"] * (depth_capacity is None) +
                                                 ["point_ground_truth=True"] * (not point_ground_truth) +
                                                 ["build_point_gt=True"] * (not build_point_gt)))
    if render_mesh is not None and not link_counts:
        raise ValueError("render_mesh renders the annotated depth frames of the step on the device: it needs " + RENDERED.rsplit(", ", 1)[0])
    if kinematics is not None and render_mesh is None:
        raise ValueError("kinematics poses the mesh the step renders: it needs " + RENDERED)
    if kinematics is not None:             # a stack of tables goes with a mesh library of as many instances, one table with one mesh
        nkin = np.shape(kinematics)[0] if np.ndim(kinematics) == 2 else None
        nmesh = max(np.size(render_mesh[3]) - 1, 0) if depth_mod.is_mesh_library(render_mesh) else None
        if nkin != nmesh:
            count = lambda n, one, many: one if n is None else many % n
            raise ValueError("kinematics and render_mesh must hold the same instances: kinematics is %s, render_mesh is %s (a library: "
                             "depth.pack_mesh_library(...) and np.stack of its instances' depth.pack_kinematics tables)"
                             % (count(nkin, "a single table", "a stack of %d tables"),
                                count(nmesh, "a single mesh", "a mesh library of %d instances")))
    if sensor is not None:
        if not link_counts:
            raise ValueError("sensor degrades the annotated depth frames of the step on the device: it needs depth_capacity=<pixels>, " + ANNOTATED)
        depth_mod.check_sensor(sensor)
    reprojection = reprojection_mod.check_reprojection(reprojection, render_mesh is not None)
    refine = refinement_mod.check_refine(refine, render_mesh is not None)
    silhouette = refinement_mod.has_silhouette(refine)                   # the slot then owns the field's planes
    refine_joints = refinement_mod.has_joints(refine)                    # ... and the joint step's two buffers
    refine_coverage = refinement_mod.has_coverage(refine)                # ... and the predicted field's planes
    refine_scale = refinement_mod.has_scale(refine)                      # ... and sums of 48 values; check_refine_table refused it with joints
    if refine_joints and kinematics is None:
        raise ValueError("refine=<pose.refinement.pack_refine(joints=...)> solves an object's parts together through the joints of its "
                         "kinematic table: it needs kinematics=<depth.pack_kinematics(...)> (" + RENDERED + ")")
    refine = refine is not None
    if raw_capacity is not None:
        if not couple:
            raise ValueError("streaming (raw_capacity) feeds the pose fit from the networks: it needs couple=True")
        if not 1 <= int(raw_capacity) < (1 << 30):
            raise ValueError("raw_capacity must be in [1, 2^30) rows")
        raw_capacity = int(raw_capacity)
    if keyed and raw_capacity is None:
        raise ValueError("keyed=True keys the streaming header: it needs raw_capacity")
    if dense and raw_capacity is None:
        raise ValueError("dense=True labels the raw rows of a stream: it needs raw_capacity")
    if range_guard and arithmetic != "f16x2":
        raise ValueError("range_guard=True needs arithmetic='f16x2' (f32 and bf16x3 have f32's range)")
    # the streamed record: the blocks these flags build, in pose.record.BLOCKS' order; its width and the name the step leaves it under
    layout = RecordLayout(fit_quality, ground_truth, point_ground_truth, reprojection, refine)
    rows = None if raw_capacity is None else ROW_KINDS["annotated" if build_point_gt else "point_gt" if point_ground_truth else
                                                       "xyz" if predicted else "labelled"]
    o = Options(raw_capacity, depth_capacity, depth_dtype if depth_capacity is not None else None, bool(keyed), predicted, bool(range_guard),
                bool(articulation), joint_states, fit_quality, bool(ground_truth), point_ground_truth, bool(build_point_gt), bool(build_gt_pose), bool(dense),
                bool(label_images), bool(annotated_images), link_counts, render_mesh is not None, kinematics is not None, sensor is not None, reprojection, coord_regress_loss, layout.width, layout.key, joint_values,
                (20 if joint_states else 12) + (joint_values_mod.JOINT_VALUES_WIDTH if joint_values else 0), rows, (), refine_scale, refine_coverage, refine_joints, silhouette, refine)
    # (build_gt_pose: the frame is fitted on the device -- ancsh_gt_pose_build -- and no longer travels in; gt still does, for its extents)
    # (kinematics: the device builds render and scene too -- ancsh_pose_scene_build -- and the pose travels in, first)
    return o._replace(inputs=((POSE_INPUT,) if o.posed else ()) +
                      tuple(i for i in ALL_INPUTS if raw_capacity is not None and getattr(o, i.option)
                            and not (build_gt_pose and i.name == "frame") and not (o.posed and i.name in ("render", "scene"))))


# ---- what retire() returns ---------------------------------------------------------------------------------------------------
RESULT_ORDER = ("tag", "seed", "record", "flags", "articulation", "dense", "label_images", "counts", "link_counts")
RESULT_ALWAYS = RESULT_ORDER[:3]
# RESULT_ORDER with the annotated frames' images directly behind label_images (a pipeline has one of the two, never both).  RESULT_ORDER
# itself stays the nine names its users have always compared it with; every helper below goes by RESULT_NAMES.
RESULT_NAMES = RESULT_ORDER[:RESULT_ORDER.index("label_images") + 1] + ("annotated_images",) + RESULT_ORDER[RESULT_ORDER.index("label_images") + 1:]
BUILT_WITH = dict(articulation="articulation=True", dense="dense=True", label_images="depth_capacity=<pixels>, label_images=True",
                  annotated_images="depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True, annotated_images=True",
                  link_counts="depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True")


def result_names(**asked):
    """The names of retire()'s tuple, in its order (RESULT_NAMES): tag, seed, record, then those of flags / articulation / dense /
    label_images / annotated_images / counts / link_counts that are asked for (counts: always, on a depth pipeline)."""
    return [k for k in RESULT_NAMES if k in RESULT_ALWAYS or asked.get(k)]


def pack_results(named, **asked):
    return tuple(named[k] for k in result_names(**asked))


def unpack_results(got, **asked):
    """pack_results' inverse: a retired tuple -> {name: value}."""
    return dict(zip(result_names(**asked), got))


def only_asked(**asked):
    """Keywords for a pipeline's retire / stream_batches: only the blocks asked for (a stand-in need not know the others)."""
    return {k: True for k, v in asked.items() if v}


def check_built_with(owner, method, cls, **asked):
    """RuntimeError when `method` is asked for an output that `owner` (a `cls`) was not built with."""
    for name in RESULT_NAMES:
        if asked.get(name) and not getattr(owner, name):
            raise RuntimeError("%s(%s=True) needs %s(..., %s)" % (method, name, cls, BUILT_WITH[name]))


def pump(batches, inflight, window, submit, retire):
    """The streaming loop: submit(k, item) for every item of `batches` while fewer than `window` batches are in `inflight`, retire() the
    oldest first when it is full, and drain at the end; yields what retire() returns, in submission order."""
    for k, item in enumerate(batches):
        if len(inflight) == window:
            yield retire()
        submit(k, item)
    while inflight:
        yield retire()
