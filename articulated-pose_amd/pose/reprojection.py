"""Render-and-compare of a batch of pose records (ancsh_reproject_scene_build, ancsh_reproject_compare_rec, csrc/reprojection.hip): the
object's own mesh put at the fitted per-part poses, rendered through the frame's camera, and its silhouette and depth compared with the frame
the annotation read -- how well a pose explains the pixels, without ground truth.  Two launches around the renderer's three; a consumer gates
a pose on the 15 columns without copying a pixel back."""
import torch

from .. import _lib
from ..dataset import RIG_WIDTH
from ..depth import GEOM_WORDS, RENDER_WIDTH, SCENE_WIDTH

REPROJECTION_WIDTH = 15         # include/ancsh_hip.h, ANCSH_REPROJECTION_WIDTH: the columns behind the carried record row
# the columns, counted from the end of the carried row: the observed pixels of the part, then seven per pose
COL_OBSERVED, COL_BASELINE, COL_NONLINEAR = 0, 1, 8      # BASELINE / NONLINEAR: + predicted, both, IoU, mean |d|, RMS d, max |d|, mean d
POSE_COLUMNS = ("n_pred", "n_both", "iou", "mean_abs", "rms", "max_abs", "mean_signed")
COLUMN_NAMES = ("n_obs",) + tuple("baseline_" + c for c in POSE_COLUMNS) + tuple("nonlinear_" + c for c in POSE_COLUMNS)
BUILT_WITH = "depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True, render_mesh=<depth.pack_mesh(...)>"


def check_reprojection(reprojection, rendered):
    """-> bool(reprojection); ValueError (before anything touches the GPU) when it is asked of a pipeline that holds no mesh to render."""
    if reprojection and not rendered:
        raise ValueError("reprojection=True re-renders the object's mesh at the fitted poses and compares it with the frame: it needs "
                         "render_mesh=<depth.pack_mesh(...)> (" + BUILT_WITH + ")")
    return bool(reprojection)


def named_columns(columns):
    """The trailing REPROJECTION_WIDTH columns of a column block (..., >= REPROJECTION_WIDTH) -> {name: (...) array}, by COLUMN_NAMES: what
    the eager operators (reproject_compare) return.  Of a pipeline's streamed record the block is the last only while nothing is built
    behind it (refine=): cut it out first, named_columns(pipe.record_layout.block(record, "reprojection"))."""
    if columns.shape[-1] < REPROJECTION_WIDTH:
        raise ValueError("expected at least %d trailing columns, got %d" % (REPROJECTION_WIDTH, columns.shape[-1]))
    tail = columns[..., columns.shape[-1] - REPROJECTION_WIDTH:]
    return {name: tail[..., k] for k, name in enumerate(COLUMN_NAMES)}


def _tables(render, scene, rig, norm_factor, record, geom, K, name="record", B=None):
    """The family's check of device tables (pose.refinement's wrappers call it too): every table that is not None against the frame count B
    (geom's rows unless given) and K, and `record` -- a pose record or a working pose buffer, under its argument's name -- as (B, K, >= 26)."""
    B = (int(geom.shape[0]) if geom.dim() else 0) if B is None else B    # geom's rows; a 0-dim geom fails its shape check below
    for what, t, shape, dtype in (("render", render, (B, RENDER_WIDTH), torch.float64), ("scene", scene, (B, SCENE_WIDTH), torch.float64),
                                  ("rig", rig, (B, RIG_WIDTH(K)) if rig is not None else None, torch.float64),
                                  ("norm_factor", norm_factor, (B,), torch.float32), ("geom", geom, (B, GEOM_WORDS), torch.int32)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s %s tensor" % (what, shape, str(dtype).replace("torch.", "")))
    if record is not None and (record.dtype != torch.float64 or record.dim() != 3 or tuple(record.shape[:2]) != (B, K) or record.shape[2] < 26
                               or not record.is_contiguous()):
        raise ValueError("%s must be a contiguous (%d, %d, >= 26) float64 tensor" % (name, B, K))
    return B


def reproject_scene_build(render, scene, rig, norm_factor, record, geom, pixel_capacity, out=None):
    """ancsh_reproject_scene_build on device tensors (no host sync): the frames' render (B, 208) and scene (B, 240) tables, rigs (B,
    RIG_WIDTH(K)), norm factors (B,) float32, record (B, K, >= 26) float64 and geometry rows (B, 5) int32 in a buffer of pixel_capacity
    pixels -> (render tables (2B, 208) float64, geometry rows (2B, 5) int32) of the predicted frames, row v * B + f; out = the same pair
    preallocated (a captured step passes slot-owned buffers)."""
    _lib.require_device(record)
    K = int(record.shape[1]) if record.dim() == 3 else 0
    B = _tables(render, scene, rig, norm_factor, record, geom, K)
    if out is None:
        out = (torch.zeros((2 * B, RENDER_WIDTH), dtype=torch.float64, device=record.device),
               torch.zeros((2 * B, GEOM_WORDS), dtype=torch.int32, device=record.device))
    render_out, geom_out = out
    if render_out.dtype != torch.float64 or tuple(render_out.shape) != (2 * B, RENDER_WIDTH) or geom_out.dtype != torch.int32 \
            or tuple(geom_out.shape) != (2 * B, GEOM_WORDS) or not (render_out.is_contiguous() and geom_out.is_contiguous()):
        raise ValueError("out must be contiguous (render (%d, %d) float64, geom (%d, %d) int32)" % (2 * B, RENDER_WIDTH, 2 * B, GEOM_WORDS))
    _lib.require_cuda(render, scene, rig, norm_factor, geom, render_out, geom_out)
    _lib.call("ancsh_reproject_scene_build", B, K, _lib.ptr(render), _lib.ptr(scene), _lib.ptr(rig), int(rig.shape[1]), _lib.ptr(norm_factor),
              _lib.ptr(record), int(record.shape[2]), _lib.ptr(geom), int(pixel_capacity), _lib.ptr(render_out), _lib.ptr(geom_out))
    return render_out, geom_out


def reproject_compare(obs_depth, obs_labels, pred_depth, pred_labels, geom, scene, carried, out=None):
    """ancsh_reproject_compare_rec on device tensors (no host sync): the observed pair (pixel_capacity,), the predicted pair (2 *
    pixel_capacity,) the renderer wrote for reproject_scene_build's tables, the frames' geometry rows and scene tables, and the record so far
    (B, K, ld) float64 -> (B, K, ld + 15) float64: the carried row bit for bit and the 15 columns behind it (COLUMN_NAMES)."""
    from ..depth import _byte_plane, _depth_plane, _pixel_pair
    _lib.require_device(carried)
    kind, cap = _depth_plane(obs_depth)
    _byte_plane("labels", obs_labels, cap)
    _pixel_pair("the predicted pair", "observed", pred_depth, pred_labels, obs_depth.dtype, 2 * cap)
    K = int(carried.shape[1]) if carried.dim() == 3 else 0
    B = _tables(None, scene, None, None, carried, geom, K)
    ld = int(carried.shape[2])
    if out is None:
        out = torch.empty((B, K, ld + REPROJECTION_WIDTH), dtype=torch.float64, device=carried.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (B, K, ld + REPROJECTION_WIDTH) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (%d, %d, %d) float64 tensor" % (B, K, ld + REPROJECTION_WIDTH))
    _lib.require_cuda(obs_depth, obs_labels, pred_depth, pred_labels, geom, scene, out)
    _lib.call("ancsh_reproject_compare_rec", B, K, kind, _lib.ptr(obs_depth), _lib.ptr(obs_labels), cap, _lib.ptr(pred_depth),
              _lib.ptr(pred_labels), _lib.ptr(geom), _lib.ptr(scene), _lib.ptr(carried), ld, _lib.ptr(out))
    return out


def predicted_buffers(capacity, depth_dtype, device):
    """The pixel triple the predicted frames are rendered into: (depth (2 * capacity,), labels (2 * capacity,) uint8 filled 255, z-buffer (2 *
    capacity,) int64) -- 22 bytes per pixel of capacity, 26 with float32 depths."""
    from ..depth import DEPTH_DTYPES, NOT_OBJECT, check_depth_dtype
    tt = DEPTH_DTYPES[check_depth_dtype(depth_dtype)][1]
    return (torch.zeros((2 * capacity,), dtype=tt, device=device), torch.full((2 * capacity,), NOT_OBJECT, dtype=torch.uint8, device=device),
            torch.zeros((2 * capacity,), dtype=torch.int64, device=device))


def predicted_frames(B, capacity, depth_dtype, device):
    """What the predicted frames of B observed ones live in, slot-owned and shared by reprojection and refinement: (tables = the pair
    reproject_scene_build writes, render (2B, 208) float64 and geom (2B, 5) int32; pred = predicted_buffers' triple)."""
    tables = (torch.zeros((2 * B, RENDER_WIDTH), dtype=torch.float64, device=device), torch.zeros((2 * B, GEOM_WORDS), dtype=torch.int32, device=device))
    return tables, predicted_buffers(capacity, depth_dtype, device)


def reprojection_batch(mesh, render, scene, rig, norm_factor, geom, obs, carried, depth_dtype, tables, pred):
    """The three calls of the captured step, no host sync and no allocation beyond the output: tables = (render (2B, 208), geom (2B, 5)) and
    pred = predicted_buffers' triple are slot-owned; obs = the (depth, labels) pair the annotation read.  -> (B, K, ld + 15) float64."""
    from ..depth import render_depth
    cap = int(obs[0].shape[0])
    reproject_scene_build(render, scene, rig, norm_factor, carried, geom, cap, out=tables)
    render_depth(mesh, tables[1], tables[0], depth_dtype, out=pred[:2], scratch=pred[2])
    return reproject_compare(obs[0], obs[1], pred[0], pred[1], geom, scene, carried)
