"""Render-and-compare ICP of a batch of pose records (ancsh_refine_pass, ancsh_refine_rec, csrc/refinement.hip): the loop that acts on what
pose.reprojection only scores.  Each part's mesh is rendered at its working pose, the rendered surface is compared with the observed depth
pixel by pixel (point-to-plane on same-pixel pairs, truncated at max_dist), one damped Gauss-Newton step moves R and t about the part's
centre, and the result is the evaluated pose of lowest cost -- never worse than the fitted pose on its own measure.  s is carried: the NOCS
scale is the network's, and one view constrains size only weakly.  Point-to-plane on same-pixel pairs does not see the silhouette, and a part
that shows one or two flat faces leaves directions unobservable: the damping leaves those where the fit put them -- unless the table is one of
pack_refine(silhouette=...): then ancsh_silhouette_field finds, once per step, every crop pixel's nearest observed pixel of each part, and
ancsh_refine_pass_sil adds one row per predicted pixel that hangs over the observed part's edge, pulling it back across the ray, and charges
such pixels in the cost.  Each part is refined on its own -- unless the table is one of pack_refine(joints=...) and the object's kinematic
table is at hand: then ancsh_refine_joint_step runs behind every pass, solves the object's parts together through rows that keep each
revolute and prismatic joint's two sides on one axis, and keeps the best-of per object.  The silhouette term is one-sided: an observed pixel
of the part that the prediction leaves bare is only charged.  A table of pack_refine(silhouette=..., coverage=...) adds the other side:
ancsh_coverage_field finds, behind the renderer in every pass, every crop pixel's nearest PREDICTED pixel of each part, and
ancsh_refine_pass_cov adds one row per bare observed pixel that pulls that predicted pixel over it.  With both pixel terms on, a table of
pack_refine(..., scale=...) stops carrying s: the overhang and the gap rows are the two that observe size, ancsh_refine_pass_scale adds every
row's derivative by a relative change of the part's size about its centre, solves 7 x 7 and moves s with R and t, clamped per step and held
to a band about the fitted s."""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib
from .reprojection import _tables

REFINE_WIDTH = 36               # include/ancsh_hip.h, ANCSH_REFINE_WIDTH: the columns behind the carried record row, 18 per pose
REFINE_SUMS, REFINE_PARAMS, MAX_ITERS = 32, 8, 8      # ANCSH_REFINE_SUMS, ANCSH_REFINE_PARAMS, ANCSH_REFINE_MAX_ITERS
REFINE_SIL_SUMS, REFINE_SIL_PARAMS = 36, 16               # ANCSH_REFINE_SIL_SUMS, ANCSH_REFINE_SIL_PARAMS: with the silhouette term
REFINE_JOINT_PARAMS, REFINE_OBJ, JOINT_XI = 24, 8, 48       # ANCSH_REFINE_JOINT_PARAMS, ANCSH_REFINE_OBJ; the debug step's 6 * 8 values: the joint step
REFINE_COV_SUMS, REFINE_COV_PARAMS = 40, 32               # ANCSH_REFINE_COV_SUMS, ANCSH_REFINE_COV_PARAMS: with the coverage term as well
REFINE_SCALE_SUMS, REFINE_SCALE_PARAMS = 48, 48           # ANCSH_REFINE_SCALE_SUMS, ANCSH_REFINE_SCALE_PARAMS: with the scale unknown as well
OBJ_COLUMNS = ("cost_start", "cost_best", "best_pass", "passes_solved", "cost", "joints", "solved", "gap_rms")      # an obj row, per (frame, pose)
FIELD_SENTINEL = -32768                                   # both halves of a field word: the part has no observed pixel in the frame
BEST_WIDTH = REFINE_WIDTH // 2
COL_BASELINE, COL_NONLINEAR = 0, BEST_WIDTH           # counted from the end of the carried row
POSE_COLUMNS = tuple("R%d%d" % (a, k) for a in range(3) for k in range(3)) + ("s", "tx", "ty", "tz", "cost_start", "cost_best", "n_used",
                                                                              "best_pass", "passes_solved")
COLUMN_NAMES = tuple("baseline_" + c for c in POSE_COLUMNS) + tuple("nonlinear_" + c for c in POSE_COLUMNS)
SUMS_COLUMNS = dict(A=slice(0, 21), b=slice(21, 27), rr=27, n_used=28, n_obs=29, cost=30, solved=31)
SIL_SUMS_COLUMNS = dict(SUMS_COLUMNS, mm=32, n_sil=33, n_far=34)
COV_SUMS_COLUMNS = dict(SIL_SUMS_COLUMNS, mm_c=36, n_cov=37, n_cfar=38)
SCALE_SUMS_COLUMNS = dict(COV_SUMS_COLUMNS, A_s=slice(40, 47), b_s=47)
PARAMS_LENGTHS = {"ancsh_refine_pass": (REFINE_PARAMS, REFINE_JOINT_PARAMS), "ancsh_refine_pass_sil": (REFINE_SIL_PARAMS, REFINE_JOINT_PARAMS),
                  "ancsh_refine_pass_cov": (REFINE_COV_PARAMS,), "ancsh_refine_pass_scale": (REFINE_SCALE_PARAMS,),
                  "ancsh_refine_joint_step": (REFINE_JOINT_PARAMS, REFINE_COV_PARAMS)}      # the params table per entry: a longer one holds the shorter ones in front
RefineBuffers = namedtuple("RefineBuffers", "work best sums field state obj xi cover")      # refine_buffers' record; None = a term that is off
BUILT_WITH = "depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True, render_mesh=<depth.pack_mesh(...)>"


def check_refine_table(table):
    """-> table as a fresh (REFINE_PARAMS,) float64 array, (REFINE_SIL_PARAMS,) with the silhouette term or (REFINE_JOINT_PARAMS,) with the
    joint step or (REFINE_COV_PARAMS,) with the coverage term or (REFINE_SCALE_PARAMS,) with the scale unknown (has_silhouette, has_joints,
    has_coverage, has_scale); ValueError unless it is one pack_refine makes."""
    try:
        t = np.array(table, np.float64)
    except (TypeError, ValueError):
        t = np.zeros(0)
    if t.shape not in ((REFINE_PARAMS,), (REFINE_SIL_PARAMS,), (REFINE_JOINT_PARAMS,), (REFINE_COV_PARAMS,), (REFINE_SCALE_PARAMS,)):
        raise ValueError("refine: one (%d,) float64 table (pose.refinement.pack_refine), or (%d,) with silhouette=, got shape %s"
                         % (REFINE_PARAMS, REFINE_SIL_PARAMS, t.shape))
    if t.shape[0] == REFINE_SCALE_PARAMS:
        check_refine_table(_scale_front(t))                              # the coverage table in front, by its own rules and messages
        max_step, max_total = t[32:34].tolist()
        if not (np.isfinite(max_step) and 0.0 < max_step <= 0.5):
            raise ValueError("refine: scale max_step must be finite and in (0, 0.5], got %r" % max_step)
        if not (np.isfinite(max_total) and max_step <= max_total <= 1.0):
            raise ValueError("refine: scale max_total must be finite, >= max_step and <= 1, got %r" % max_total)
        if (t[34:] != 0).any():
            raise ValueError("refine: the reserved values 34..47 must be 0")
        return t
    iters, max_dist, min_cos, damping, max_angle, min_pixels = t[:6].tolist()
    if not (iters == int(iters) if np.isfinite(iters) else False) or not 1 <= iters <= MAX_ITERS:
        raise ValueError("refine: iters must be an integer in [1, %d], got %r" % (MAX_ITERS, iters))
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError("refine: max_dist must be finite and > 0, got %r" % max_dist)
    if not 0.0 <= min_cos <= 1.0:
        raise ValueError("refine: min_cos is a cosine in [0, 1], got %r" % min_cos)
    if not (np.isfinite(damping) and damping >= 0):
        raise ValueError("refine: damping must be finite and >= 0, got %r" % damping)
    if not 0.0 < max_angle <= np.pi / 2:
        raise ValueError("refine: max_angle_deg must be in (0, 90], got %r" % np.degrees(max_angle))
    if not (np.isfinite(min_pixels) and min_pixels == int(min_pixels) and min_pixels >= 1):
        raise ValueError("refine: min_pixels must be an integer >= 1, got %r" % min_pixels)
    if (t[6:REFINE_PARAMS] != 0).any():
        raise ValueError("refine: the reserved values 6..7 must be 0")
    if t.shape[0] == REFINE_COV_PARAMS and not (t[8:REFINE_SIL_PARAMS] != 0).any():
        raise ValueError("refine: coverage needs the silhouette term (its rows are the other side of the overhang rows): pass silhouette= as well")
    if t.shape[0] == REFINE_SIL_PARAMS or (t.shape[0] > REFINE_SIL_PARAMS and (t[8:REFINE_SIL_PARAMS] != 0).any()):
        weight, dist, slack = t[8:11].tolist()
        if not (np.isfinite(weight) and weight > 0):
            raise ValueError("refine: silhouette weight must be finite and > 0, got %r" % weight)
        if not (np.isfinite(dist) and dist > 0):
            raise ValueError("refine: silhouette dist must be finite and > 0, got %r" % dist)
        if not (np.isfinite(slack) and slack >= 0):
            raise ValueError("refine: silhouette slack must be finite and >= 0 pixels, got %r" % slack)
        if (t[11:REFINE_SIL_PARAMS] != 0).any():
            raise ValueError("refine: the reserved values 11..15 must be 0")
    if t.shape[0] == REFINE_JOINT_PARAMS or (t.shape[0] == REFINE_COV_PARAMS and (t[REFINE_SIL_PARAMS:REFINE_JOINT_PARAMS] != 0).any()):
        weight, axis_length = t[16:18].tolist()
        if not (np.isfinite(weight) and weight > 0):
            raise ValueError("refine: joints weight must be finite and > 0, got %r" % weight)
        if not (np.isfinite(axis_length) and axis_length >= 0):
            raise ValueError("refine: joints axis_length must be finite and >= 0, got %r" % axis_length)
        if (t[18:REFINE_JOINT_PARAMS] != 0).any():
            raise ValueError("refine: the reserved values 18..23 must be 0")
    if t.shape[0] == REFINE_COV_PARAMS:
        weight, dist, slack = t[24:27].tolist()
        if not (np.isfinite(weight) and weight > 0):
            raise ValueError("refine: coverage weight must be finite and > 0, got %r" % weight)
        if not (np.isfinite(dist) and dist > 0):
            raise ValueError("refine: coverage dist must be finite and > 0, got %r" % dist)
        if not (np.isfinite(slack) and slack >= 0):
            raise ValueError("refine: coverage slack must be finite and >= 0 pixels, got %r" % slack)
        if (t[27:] != 0).any():
            raise ValueError("refine: the reserved values 27..31 must be 0")
    return t


SCALE_NEEDS = "refine: scale needs the silhouette and coverage terms (their rows are what observes size)"
SCALE_JOINTS = ("refine: scale with joints is not built: scaling an object's parts separately opens its joints, and the joint step's 6 K system "
                "has no scale unknown yet (pass scale= or joints=, not both)")


def _scale_front(t):
    """The first 32 values of a 48-value table, after the two rules that are the scale unknown's own."""
    if not (t[8:REFINE_SIL_PARAMS] != 0).any() or not (t[REFINE_JOINT_PARAMS:REFINE_COV_PARAMS] != 0).any():
        raise ValueError(SCALE_NEEDS)
    if (t[REFINE_SIL_PARAMS:REFINE_JOINT_PARAMS] != 0).any():
        raise ValueError(SCALE_JOINTS)
    return t[:REFINE_COV_PARAMS]


def has_silhouette(table):
    """A checked table: the silhouette term is on iff it holds at least REFINE_SIL_PARAMS values and value 8 (its weight) is > 0."""
    return table is not None and table.shape[0] >= REFINE_SIL_PARAMS and bool(table[8] > 0)


def has_joints(table):
    """A checked table: the joint step is on iff it is the (REFINE_JOINT_PARAMS,) one, or the (REFINE_COV_PARAMS,) one with value 16 (the
    joints' weight) > 0; never with the (REFINE_SCALE_PARAMS,) one."""
    return table is not None and (table.shape[0] == REFINE_JOINT_PARAMS or (table.shape[0] == REFINE_COV_PARAMS and bool(table[16] > 0)))


def has_coverage(table):
    """A checked table: the coverage term is on iff it holds at least REFINE_COV_PARAMS values and value 24 (its weight) is > 0."""
    return table is not None and table.shape[0] >= REFINE_COV_PARAMS and bool(table[24] > 0)


def has_scale(table):
    """A checked table: the scale unknown is on iff it is the (REFINE_SCALE_PARAMS,) one."""
    return table is not None and table.shape[0] == REFINE_SCALE_PARAMS


def pack_refine(iters=3, max_dist=0.1, min_cos=0.1, damping=1e-3, max_angle_deg=10.0, min_pixels=32, silhouette=None, joints=None,
                coverage=None, scale=None):
    """The parameter table ancsh_refine_pass reads, (REFINE_PARAMS,) float64: iters Gauss-Newton passes (1..8; one more pass evaluates the
    last pose); max_dist: a pixel pair further apart than this counts as missed, and a step's translation is clamped to it; min_cos: pixels
    seen at a flatter angle are left out; damping: relative Levenberg damping of the diagonal; max_angle_deg: the clamp of a step's
    rotation; min_pixels: fewer used pixels leave the pose as it is.  Lengths are in the scaled cloud's unit, where an object's diagonal is
    about 1.  The defaults are starting values; nobody has tuned them.
    silhouette = dict(weight=1.0, dist=<cloud units>, slack=1.0), or (weight, dist): the silhouette term, a (REFINE_SIL_PARAMS,) table.  A
    predicted pixel of the part where the camera saw neither the part nor anything nearer is pulled towards the nearest observed pixel of
    the part: weight scales its row against the depth rows; further than dist (at the pixel's depth) it pulls no more and is charged dist^2;
    within slack pixels it is ignored (sensor holes, one pixel of raster disagreement).  min_pixels then counts these rows too.
    joints = dict(weight=1.0, axis_length=0.5), or (weight, axis_length): the joint step (ancsh_refine_joint_step), a (REFINE_JOINT_PARAMS,)
    table: values 0..7 as above, 8..15 the silhouette values (all 0 without the term), 16 weight, 17 axis_length, 18..23 reserved.  Behind
    every pass the parts of an object are solved together: rows that keep each revolute and prismatic joint's two sides on one axis join the
    parts' own normal equations.  weight scales a joint row against a mean part's pixel rows (a residual in cloud units counts weight^2 *
    the parts' mean row count times); axis_length (cloud units) turns the angle between the two sides' axis directions into a length.  It
    needs the object's kinematic table (kinematics=).  These defaults, too, are starting values nobody has tuned.
    coverage = dict(weight=1.0, dist=<cloud units>, slack=1.0), or (weight, dist), with silhouette=: the coverage term, a (REFINE_COV_PARAMS,)
    table: values 0..15 as above, 16..23 the joint step's (all 0 without joints=), 24 weight, 25 dist, 26 slack, 27..31 reserved.  An observed
    pixel of the part that the prediction leaves bare pulls the nearest predicted pixel of the part over it -- the silhouette term's other
    side, with the same three values' meaning; min_pixels counts these rows too.  Nobody has tuned these defaults either.
    scale = dict(max_step=0.05, max_total=0.25), or (max_step, max_total), with silhouette= and coverage= and without joints=: the scale
    unknown (ancsh_refine_pass_scale), a (REFINE_SCALE_PARAMS,) table: values 0..31 as above, 32 max_step, 33 max_total, 34..47 reserved.  s
    is solved with R and t: a step changes it by at most the factor 1 +- max_step (in (0, 0.5]), and the kept s stays within [s_0 / (1 +
    max_total), s_0 (1 + max_total)] of the fitted s_0 (max_step <= max_total <= 1).  The overhang and the gap rows are what observes size;
    depth rows alone cannot tell scale from depth along the ray.  These, too, are starting values nobody has tuned.
    ValueError: check_refine_table's."""
    if scale is not None:
        if silhouette is None or coverage is None:
            raise ValueError(SCALE_NEEDS)
        if joints is not None:
            raise ValueError(SCALE_JOINTS)
        if isinstance(scale, dict) and set(scale) - {"max_step", "max_total"}:
            raise ValueError("refine: scale takes max_step and max_total, got %s" % sorted(scale))
        try:
            if isinstance(scale, dict):
                sc = [float(scale.get("max_step", 0.05)), float(scale.get("max_total", 0.25))]
            else:
                max_step, max_total = scale
                sc = [float(max_step), float(max_total)]
        except (TypeError, ValueError):
            raise ValueError("refine: scale is dict(max_step=, max_total=) or (max_step, max_total), of numbers")
        front = pack_refine(iters, max_dist, min_cos, damping, max_angle_deg, min_pixels, silhouette=silhouette, coverage=coverage).tolist()
        return check_refine_table(front + sc + [0.0] * (REFINE_SCALE_PARAMS - REFINE_COV_PARAMS - len(sc)))
    if coverage is not None:
        if silhouette is None:
            raise ValueError("refine: coverage needs the silhouette term (its rows are the other side of the overhang rows): pass silhouette= as well")
        if isinstance(coverage, dict) and (set(coverage) - {"weight", "dist", "slack"} or "dist" not in coverage):
            raise ValueError("refine: coverage takes weight, dist (required) and slack, got %s" % sorted(coverage))
        try:
            if isinstance(coverage, dict):
                cov = [float(coverage.get("weight", 1.0)), float(coverage["dist"]), float(coverage.get("slack", 1.0))]
            else:
                weight, dist = coverage
                cov = [float(weight), float(dist), 1.0]
        except (TypeError, ValueError):
            raise ValueError("refine: coverage is dict(weight=, dist=, slack=) or (weight, dist), of numbers")
        front = pack_refine(iters, max_dist, min_cos, damping, max_angle_deg, min_pixels, silhouette=silhouette, joints=joints).tolist()
        front = front + [0.0] * (REFINE_JOINT_PARAMS - len(front))
        return check_refine_table(front + cov + [0.0] * (REFINE_COV_PARAMS - REFINE_JOINT_PARAMS - len(cov)))
    try:
        head = [float(iters), float(max_dist), float(min_cos), float(damping), float(np.radians(float(max_angle_deg))), float(min_pixels)]
    except (TypeError, ValueError):
        raise ValueError("refine: iters, max_dist, min_cos, damping, max_angle_deg and min_pixels are numbers")
    head = head + [0.0] * (REFINE_PARAMS - len(head))
    if joints is not None:
        if isinstance(joints, dict) and set(joints) - {"weight", "axis_length"}:
            raise ValueError("refine: joints takes weight and axis_length, got %s" % sorted(joints))
        try:
            if isinstance(joints, dict):
                jt = [float(joints.get("weight", 1.0)), float(joints.get("axis_length", 0.5))]
            else:
                weight, axis_length = joints
                jt = [float(weight), float(axis_length)]
        except (TypeError, ValueError):
            raise ValueError("refine: joints is dict(weight=, axis_length=) or (weight, axis_length), of numbers")
        sil = [0.0] * (REFINE_SIL_PARAMS - REFINE_PARAMS) if silhouette is None else \
            pack_refine(iters, max_dist, min_cos, damping, max_angle_deg, min_pixels, silhouette=silhouette)[REFINE_PARAMS:].tolist()
        return check_refine_table(head + sil + jt + [0.0] * (REFINE_JOINT_PARAMS - REFINE_SIL_PARAMS - len(jt)))
    if silhouette is None:
        return check_refine_table(head)
    if isinstance(silhouette, dict) and (set(silhouette) - {"weight", "dist", "slack"} or "dist" not in silhouette):
        raise ValueError("refine: silhouette takes weight, dist (required) and slack, got %s" % sorted(silhouette))
    try:
        if isinstance(silhouette, dict):
            tail = [float(silhouette.get("weight", 1.0)), float(silhouette["dist"]), float(silhouette.get("slack", 1.0))]
        else:
            weight, dist = silhouette
            tail = [float(weight), float(dist), 1.0]
    except (TypeError, ValueError):
        raise ValueError("refine: silhouette is dict(weight=, dist=, slack=) or (weight, dist), of numbers")
    return check_refine_table(head + tail + [0.0] * (REFINE_SIL_PARAMS - REFINE_PARAMS - len(tail)))


def check_refine(refine, rendered):
    """-> the checked table or None; ValueError (before anything touches the GPU) when it is asked of a pipeline that holds no mesh to render."""
    if refine is None:
        return None
    if not rendered:
        raise ValueError("refine=<pose.refinement.pack_refine(...)> re-renders the object's mesh at the working poses and compares it with the "
                         "frame: it needs render_mesh=<depth.pack_mesh(...)> (" + BUILT_WITH + ")")
    return check_refine_table(refine)


def named_columns(record):
    """The trailing REFINE_WIDTH columns of a column block (..., >= REFINE_WIDTH) -> {name: (...) array}, by COLUMN_NAMES: what the eager
    operators (refine_rec) return.  Of a pipeline's streamed record the block is the last only while nothing is built behind it: cut it out
    first, named_columns(pipe.record_layout.block(record, "refinement"))."""
    if record.shape[-1] < REFINE_WIDTH:
        raise ValueError("expected at least %d trailing columns, got %d" % (REFINE_WIDTH, record.shape[-1]))
    tail = record[..., record.shape[-1] - REFINE_WIDTH:]
    return {name: tail[..., k] for k, name in enumerate(COLUMN_NAMES)}


def refined_record(record, layout=None):
    """A streamed record with the refinement's columns -> (..., 26): the two refined poses in a pose record's own columns, as
    depth.reprojection_frames, pose.gt_errors and the other operators on a record take them.  A copy.  layout (pose.record.RecordLayout,
    a pipeline's record_layout): the block is read where it says; None: it is the record's last, behind at least a pose record."""
    if layout is not None:
        record = layout.check(record)[..., :layout.span("refinement").stop]
    if record.shape[-1] < 26 + REFINE_WIDTH:
        raise ValueError("expected a record of at least %d columns, got %d" % (26 + REFINE_WIDTH, record.shape[-1]))
    tail = record[..., record.shape[-1] - REFINE_WIDTH:]
    cat = np.concatenate if isinstance(record, np.ndarray) else (lambda parts, axis: torch.cat(parts, dim=axis))
    return cat([tail[..., :13], tail[..., BEST_WIDTH:BEST_WIDTH + 13]], -1)


def _f64(name, t, shape):
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s float64 tensor" % (name, tuple(shape)))


def _params(entry, params):
    if params.dtype != torch.float64 or params.dim() != 1 or int(params.shape[0]) not in PARAMS_LENGTHS[entry] or not params.is_contiguous():
        raise ValueError("params must be a contiguous float64 table of %s values (pack_refine) for %s"
                         % (" or ".join(str(n) for n in PARAMS_LENGTHS[entry]), entry))


def refine_buffers(B, K, device, passes=1, silhouette=False, joints=False, pixel_capacity=None, coverage=False, scale=False):
    """What a slot owns for the loop, a RefineBuffers record: work = two (B, K, 26) pose buffers, best (B, K, 2, 18), sums (passes, B, K, 2,
    32 -- 36 with the silhouette term, 40 with the coverage term, 48 with scale=True, which needs coverage=True), float64; silhouette=True: field = field_buffer's planes of pixel_capacity
    pixels; joints=True: state (B, K, 2, 18), obj (passes, B, 2, 8) and the debug output xi (passes, B, 2, 48) -- None with one pass;
    coverage=True (with silhouette=True): cover = field_buffer's planes of 2 * pixel_capacity pixels."""
    if silhouette and pixel_capacity is None:
        raise ValueError("refine_buffers(silhouette=True) allocates the field with the rest: it needs pixel_capacity")
    if coverage and not silhouette:
        raise ValueError("refine_buffers(coverage=True) needs silhouette=True: the coverage term runs with the silhouette term")
    if scale and not coverage:
        raise ValueError("refine_buffers(scale=True) needs coverage=True: the scale unknown runs with both pixel terms")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)
    return RefineBuffers(work=(z(B, K, 26), z(B, K, 26)), best=z(B, K, 2, BEST_WIDTH),
                         sums=z(passes, B, K, 2, REFINE_SCALE_SUMS if scale else REFINE_COV_SUMS if coverage else REFINE_SIL_SUMS if silhouette else REFINE_SUMS),
                         field=field_buffer(K, pixel_capacity, device) if silhouette else None, state=z(B, K, 2, BEST_WIDTH) if joints else None,
                         obj=z(passes, B, 2, REFINE_OBJ) if joints else None, xi=z(passes, B, 2, JOINT_XI) if joints and passes > 1 else None,
                         cover=field_buffer(K, 2 * int(pixel_capacity), device) if coverage else None)


def field_buffer(K, pixel_capacity, device):
    """What a slot owns for the silhouette term: (K, pixel_capacity) int32, one plane per part, 4 bytes per pixel and part."""
    return torch.zeros((K, int(pixel_capacity)), dtype=torch.int32, device=device)


def silhouette_field(obs_depth, obs_labels, geom, scene, K, out=None):
    """ancsh_silhouette_field on device tensors (no host sync): the observed pair (pixel_capacity,), geom (B, 5) int32, scene (B, 240) ->
    field (K, pixel_capacity) int32: per crop pixel and part the offset to the nearest pixel observed for the part, (di & 0xffff) | (dj &
    0xffff) << 16, FIELD_SENTINEL in both halves for a part without one.  Words outside the crops are left as they are."""
    from ..depth import _byte_plane, _depth_plane
    _lib.require_device(obs_depth)
    kind, cap = _depth_plane(obs_depth)
    _byte_plane("labels", obs_labels, cap)
    if not 1 <= int(K) <= 8:
        raise ValueError("K=%d must be in [1, 8]" % K)
    B = _tables(None, scene, None, None, None, geom, int(K))
    if out is None:
        out = field_buffer(K, cap, obs_depth.device)
    if out.dtype != torch.int32 or tuple(out.shape) != (int(K), cap) or not out.is_contiguous():
        raise ValueError("field must be a contiguous (%d, %d) int32 tensor" % (K, cap))
    _lib.require_cuda(obs_labels, geom, scene, out)
    _lib.call("ancsh_silhouette_field", B, int(K), kind, _lib.ptr(obs_depth), _lib.ptr(obs_labels), cap, _lib.ptr(geom), _lib.ptr(scene),
              _lib.ptr(out))
    return out


def coverage_field(pred, geom_out, scene, K, out=None):
    """ancsh_coverage_field on device tensors (no host sync): pred = pose.reprojection.predicted_buffers' triple as the renderer left it (2 *
    pixel_capacity pixels), geom_out (2B, 5) int32 = ancsh_reproject_scene_build's description of the predicted frames, scene (B, 240) ->
    cover (K, 2 * pixel_capacity) int32: silhouette_field's words for the pixels PREDICTED for each part, pose v's half behind v *
    pixel_capacity.  Words outside the crops are left as they are."""
    from ..depth import _byte_plane, _depth_plane
    _lib.require_device(pred[0])
    kind, cap2 = _depth_plane(pred[0])
    _byte_plane("labels", pred[1], cap2)
    if not 1 <= int(K) <= 8:
        raise ValueError("K=%d must be in [1, 8]" % K)
    if cap2 % 2:
        raise ValueError("the predicted pair holds two halves: an even number of pixels, got %d" % cap2)
    B = _tables(None, scene, None, None, None, None, int(K), B=int(scene.shape[0]) if scene.dim() == 2 else 0)
    if geom_out.dtype != torch.int32 or tuple(geom_out.shape) != (2 * B, 5) or not geom_out.is_contiguous():
        raise ValueError("geom_out must be a contiguous (%d, 5) int32 tensor" % (2 * B))
    if out is None:
        out = field_buffer(K, cap2, pred[0].device)
    if out.dtype != torch.int32 or tuple(out.shape) != (int(K), cap2) or not out.is_contiguous():
        raise ValueError("cover must be a contiguous (%d, %d) int32 tensor" % (K, cap2))
    _lib.require_cuda(pred[1], geom_out, scene, out)
    _lib.call("ancsh_coverage_field", B, int(K), kind, _lib.ptr(pred[0]), _lib.ptr(pred[1]), cap2 // 2, _lib.ptr(geom_out), _lib.ptr(scene),
              _lib.ptr(out))
    return out


def refine_pass(mesh, obs_depth, obs_labels, pred, geom, scene, pred_render, norm_factor, params, pass_index, is_last, pose_in, pose_out,
                best, sums, field=None, cover=None, fitted=None):
    """ancsh_refine_pass on device tensors (no host sync, no allocation): mesh = depth.mesh_to_device's; the observed pair (pixel_capacity,);
    pred = pose.reprojection.predicted_buffers' triple as the renderer left it for pred_render (2B, 208), the tables of pose_in (B, K, >= 26);
    params = pack_refine's table on the device.  Writes pose_out (B, K, 26), best (B, K, 2, 18) and sums (B, K, 2, 32); -> pose_out.
    field = silhouette_field's (K, pixel_capacity) planes: ancsh_refine_pass_sil, with a (16,) table and sums (B, K, 2, 36).
    cover = coverage_field's (K, 2 * pixel_capacity) planes of this pass's prediction, with field: ancsh_refine_pass_cov, with a (32,) table
    and sums (B, K, 2, 40).
    fitted = the record the loop started from (B, K, >= 26), with field and cover: ancsh_refine_pass_scale, with a (48,) table and sums (B, K,
    2, 48); a (48,) table needs it."""
    from ..depth import RENDER_WIDTH, _byte_plane, _check_device_mesh, _depth_plane, _pixel_pair, _scratch_size
    _lib.require_device(pose_in)
    verts, tris, tri_link, V, T = _check_device_mesh(mesh)[:5]
    kind, cap = _depth_plane(obs_depth)
    _byte_plane("labels", obs_labels, cap)
    _pixel_pair("the predicted pair", "observed", pred[0], pred[1], obs_depth.dtype, 2 * cap)
    _scratch_size(pred[2], 2 * cap, torch.int64)
    K = int(pose_in.shape[1]) if pose_in.dim() == 3 else 0
    B = _tables(None, scene, None, norm_factor, pose_in, geom, K, name="pose_in")
    ld = int(pose_in.shape[2])
    _f64("pred_render", pred_render, (2 * B, RENDER_WIDTH))
    sil, cov, scl = field is not None, cover is not None, fitted is not None
    if cov and not sil:
        raise ValueError("cover goes with field: the coverage term runs with the silhouette term")
    if scl and not cov:
        raise ValueError("fitted goes with field and cover: the scale unknown runs with both pixel terms")
    if not scl and params.dim() == 1 and int(params.shape[0]) == REFINE_SCALE_PARAMS:
        raise ValueError("a (%d,) table solves s as well: it needs fitted, the record the loop started from" % REFINE_SCALE_PARAMS)
    if scl and (fitted.dtype != torch.float64 or fitted.dim() != 3 or tuple(fitted.shape[:2]) != (B, K) or fitted.shape[2] < 26 or
                not fitted.is_contiguous()):
        raise ValueError("fitted must be a contiguous (%d, %d, >= 26) float64 tensor" % (B, K))
    _params("ancsh_refine_pass_scale" if scl else "ancsh_refine_pass_cov" if cov else "ancsh_refine_pass_sil" if sil else "ancsh_refine_pass", params)
    _f64("pose_out", pose_out, (B, K, 26))
    _f64("best", best, (B, K, 2, BEST_WIDTH))
    _f64("sums", sums, (B, K, 2, REFINE_SCALE_SUMS if scl else REFINE_COV_SUMS if cov else REFINE_SIL_SUMS if sil else REFINE_SUMS))
    if sil and (field.dtype != torch.int32 or tuple(field.shape) != (K, cap) or not field.is_contiguous()):
        raise ValueError("field must be a contiguous (%d, %d) int32 tensor" % (K, cap))
    if cov and (cover.dtype != torch.int32 or tuple(cover.shape) != (K, 2 * cap) or not cover.is_contiguous()):
        raise ValueError("cover must be a contiguous (%d, %d) int32 tensor" % (K, 2 * cap))
    _lib.require_cuda(obs_depth, obs_labels, pred[0], pred[1], pred[2], geom, scene, pred_render, norm_factor, params, pose_out, best, sums, field,
                      cover, fitted)
    head = (B, K, kind, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), int(V), int(T), _lib.ptr(obs_depth), _lib.ptr(obs_labels), cap,
            _lib.ptr(pred[2]), _lib.ptr(pred[0]), _lib.ptr(pred[1]), _lib.ptr(geom), _lib.ptr(scene), _lib.ptr(pred_render), _lib.ptr(norm_factor),
            _lib.ptr(params))
    tail = (int(pass_index), int(bool(is_last)), _lib.ptr(pose_in), ld, _lib.ptr(pose_out), _lib.ptr(best), _lib.ptr(sums))
    if scl:
        _lib.call("ancsh_refine_pass_scale", *head, _lib.ptr(field), _lib.ptr(cover), _lib.ptr(fitted), int(fitted.shape[2]), *tail)
    elif cov:
        _lib.call("ancsh_refine_pass_cov", *head, _lib.ptr(field), _lib.ptr(cover), *tail)
    elif sil:
        _lib.call("ancsh_refine_pass_sil", *head, _lib.ptr(field), *tail)
    else:
        _lib.call("ancsh_refine_pass", *head, *tail)
    return pose_out


def refine_joint_step(kin, scene, pred_render, norm_factor, params, pass_index, is_last, pose_in, sums, pose_out, best, state, obj, xi=None):
    """ancsh_refine_joint_step on device tensors (no host sync, no allocation), directly behind refine_pass of the same pass and on its
    arguments: kin = the object's kinematic table (672,) or a library's (ninst, 672) on the device; params = a pack_refine(joints=...) table
    (24,), or (32,) with joint values; sums (B, K, 2, 32, 36 or 40) what the pass wrote.  Overwrites pose_out (B, K, 26) and best (B, K, 2, 18); state (B, K, 2, 18) and obj
    (B, 2, 8; OBJ_COLUMNS) are its own, written on pass 0 and carried from pass to pass; xi (B, 2, 48) or None: the clamped step.  -> pose_out."""
    from ..depth import KIN_WIDTH, RENDER_WIDTH
    _lib.require_device(pose_in)
    B, K = (int(v) for v in pose_in.shape[:2]) if pose_in.dim() == 3 else (0, 0)
    _tables(None, scene, None, norm_factor, pose_in, None, K, name="pose_in", B=B)
    ld = int(pose_in.shape[2])
    if kin.dtype != torch.float64 or kin.dim() not in (1, 2) or kin.shape[-1] != KIN_WIDTH or kin.shape[0] < 1 or not kin.is_contiguous():
        raise ValueError("kin must be a contiguous (%d,) or (ninst, %d) float64 tensor (depth.pack_kinematics)" % (KIN_WIDTH, KIN_WIDTH))
    ninst = int(kin.shape[0]) if kin.dim() == 2 else 1
    _f64("pred_render", pred_render, (2 * B, RENDER_WIDTH))
    _params("ancsh_refine_joint_step", params)
    if sums.dim() != 4 or sums.shape[3] not in (REFINE_SUMS, REFINE_SIL_SUMS, REFINE_COV_SUMS):
        raise ValueError("sums must be a contiguous (%d, %d, 2, %d, %d or %d) float64 tensor" % (B, K, REFINE_SUMS, REFINE_SIL_SUMS, REFINE_COV_SUMS))
    _f64("sums", sums, (B, K, 2, int(sums.shape[3])))
    _f64("pose_out", pose_out, (B, K, 26))
    _f64("best", best, (B, K, 2, BEST_WIDTH))
    _f64("state", state, (B, K, 2, BEST_WIDTH))
    _f64("obj", obj, (B, 2, REFINE_OBJ))
    if xi is not None:
        _f64("xi", xi, (B, 2, JOINT_XI))
    _lib.require_cuda(kin, scene, pred_render, norm_factor, params, sums, pose_out, best, state, obj, xi)
    _lib.call("ancsh_refine_joint_step", B, K, _lib.ptr(kin), ninst, _lib.ptr(scene), _lib.ptr(pred_render), _lib.ptr(norm_factor),
              _lib.ptr(params), int(pass_index), int(bool(is_last)), _lib.ptr(pose_in), ld, _lib.ptr(sums), int(sums.shape[3]),
              _lib.ptr(pose_out), _lib.ptr(best), _lib.ptr(state), _lib.ptr(obj), _lib.ptr(xi))
    return pose_out


def refine_rec(best, carried, out=None):
    """ancsh_refine_rec on device tensors (no host sync): best (B, K, 2, 18) and the record so far (B, K, ld) float64 -> (B, K, ld + 36): the
    carried row bit for bit and the 36 columns behind it (COLUMN_NAMES)."""
    _lib.require_device(carried)
    if carried.dtype != torch.float64 or carried.dim() != 3 or carried.shape[2] < 26 or not carried.is_contiguous():
        raise ValueError("carried must be a contiguous (B, K, >= 26) float64 tensor")
    B, K, ld = (int(v) for v in carried.shape)
    _f64("best", best, (B, K, 2, BEST_WIDTH))
    if out is None:
        out = torch.empty((B, K, ld + REFINE_WIDTH), dtype=torch.float64, device=carried.device)
    _f64("out", out, (B, K, ld + REFINE_WIDTH))
    _lib.require_cuda(best, out)
    _lib.call("ancsh_refine_rec", B, K, _lib.ptr(best), _lib.ptr(carried), ld, _lib.ptr(out))
    return out


def refine_batch(mesh, render, scene, rig, norm_factor, geom, obs, carried, depth_dtype, tables, pred, params, iters, buffers, kin=None):
    """The captured step's sequence, no host sync and no allocation beyond the output: iters + 1 times ancsh_reproject_scene_build on the
    working poses, the renderer, ancsh_refine_pass; then ancsh_refine_rec -- 5 (iters + 1) + 1 launches.  tables and pred are
    pose.reprojection's slot-owned pair and triple (shared with reprojection=True, whose three calls come first); params = pack_refine's
    table on the device and iters its first value on the host; buffers = refine_buffers'.  sums of `passes` > 1 rows keeps every pass's sums
    (pass p in row p); one row holds the last pass's.  refine_buffers(silhouette=True), with a (16,) table: ancsh_silhouette_field once in
    front of the loop and ancsh_refine_pass_sil in it -- 5 (iters + 1) + 2 launches.  kin = the kinematic table(s) on the device, with a
    (24,) table and refine_buffers(joints=True): ancsh_refine_joint_step behind every pass -- 6 (iters + 1) + 1 launches (+ 1 with the field);
    obj and xi of `passes` > 1 rows keep every pass's (one device copy carries the object's row on).  refine_buffers(coverage=True), with
    a (32,) table: ancsh_coverage_field behind the renderer and ancsh_refine_pass_cov in every pass -- 6 (iters + 1) + 2 launches, 7 (iters +
    1) + 2 with the joint step.  A (48,) table with refine_buffers(scale=True): ancsh_refine_pass_scale in ancsh_refine_pass_cov's place,
    given `carried` as the fitted record -- the coverage loop's 6 (iters + 1) + 2 launches.  -> (B, K, ld + 36) float64."""
    from ..depth import render_depth
    from .reprojection import reproject_scene_build
    work, best, sums, field, state, obj, xi, cover = buffers
    joints, scale = kin is not None, int(params.shape[0]) == REFINE_SCALE_PARAMS
    if scale != (int(sums.shape[-1]) == REFINE_SCALE_SUMS):
        raise ValueError("the scale unknown takes both a (%d,) table and refine_buffers(scale=True)" % REFINE_SCALE_PARAMS)
    if joints != (state is not None):
        raise ValueError("the joint step takes both kin and refine_buffers(joints=True)")
    cap = int(obs[0].shape[0])
    src = carried
    if field is not None:
        silhouette_field(obs[0], obs[1], geom, scene, int(carried.shape[1]), out=field)
    for p in range(iters + 1):
        reproject_scene_build(render, scene, rig, norm_factor, src, geom, cap, out=tables)
        render_depth(mesh, tables[1], tables[0], depth_dtype, out=pred[:2], scratch=pred[2])
        if cover is not None:
            coverage_field(pred, tables[1], scene, int(carried.shape[1]), out=cover)
        dst = work[p % 2]
        refine_pass(mesh, obs[0], obs[1], pred, geom, scene, tables[0], norm_factor, params, p, p == iters, src, dst, best,
                    sums[p if sums.shape[0] > 1 else 0], field=field, cover=cover, fitted=carried if scale else None)
        if joints:
            if p and obj.shape[0] > 1:
                obj[p].copy_(obj[p - 1])
            refine_joint_step(kin, scene, tables[0], norm_factor, params, p, p == iters, src, sums[p if sums.shape[0] > 1 else 0], dst, best,
                              state, obj[p if obj.shape[0] > 1 else 0], None if xi is None else xi[p])
        src = dst
    return refine_rec(best, carried)
