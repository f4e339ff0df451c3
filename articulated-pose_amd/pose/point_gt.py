"""What a streamed batch's per-point ground truth says about it (ancsh_point_gt_rec, csrc/point_gt.hip): the test-time losses of both
networks -- the numbers lib/network.py:257-316 writes to test_loss.txt -- and step 5 of evaluation.sh, each joint's axis angle error and
line-to-line distance in camera space (evaluation/eval_joint_params.py:189-256), in one launch behind the articulation launches, from
18-column raw rows (dataset.pack_cloud) that travel in with the batch and are sampled on the device."""
import numpy as np
import torch

from .. import _lib
from ..dataset import NCHAN

POINT_GT_WIDTH = 21             # include/ancsh_hip.h, ancsh_point_gt_rec: the columns behind the carried row (ld in CARRIED_WIDTHS)
FRAME_WIDTH = 13                # a frame row: [R (9, row-major) | s | t (3)] of the ground-truth NAOCS pose of part 0
# the columns, counted from the block's first (pose.record: RecordLayout.span("point_gt").start): column = ld + PGT_*
PGT_ANGLE_ERR, PGT_DIST_ERR = 0, 1                      # row j >= 1: the errors of joint j
PGT_JOINT_POINT, PGT_JOINT_AXIS = slice(2, 5), slice(5, 8)      # row j >= 1: the ground-truth joint j in camera space
PGT_MIOU, PGT_NPCS_MIOU = 8, 9                          # miou_loss[j] of the ANCSH and of the NPCS network
PGT_PART_POINTS, PGT_JOINT_POINTS = 10, 11              # sampled points with cls_gt == j / joint_cls_gt == j
PGT_NOCS, PGT_GOCS, PGT_HEATMAP, PGT_UNITVEC, PGT_ORIENT = 12, 13, 14, 15, 16      # the cloud's ANCSH losses, on every row
PGT_INDEX = slice(17, 20)                               # the cloud's ANCSH index_loss[0..2], on every row
PGT_NPCS_NOCS = 20                                      # the cloud's NPCS nocs_loss, on every row
POINT_GT_COLUMNS = ("angle_err", "dist_err", "joint_point_x", "joint_point_y", "joint_point_z", "joint_axis_x", "joint_axis_y", "joint_axis_z",
                    "miou_loss", "npcs_miou_loss", "part_points", "joint_points", "nocs_loss", "gocs_loss", "heatmap_loss", "unitvec_loss",
                    "orient_loss", "index_loss_0", "index_loss_1", "index_loss_2", "npcs_nocs_loss")
RAW_COLUMNS = "x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls"
_TYPE_L = {"L2": 0, "L1": 1}


def __getattr__(name):
    """CARRIED_WIDTHS: the widths of the carried row, from the record's table (pose.record, which reads this module's width: hence lazily)."""
    if name == "CARRIED_WIDTHS":
        from .record import CARRIED_WIDTHS
        return CARRIED_WIDTHS
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def check_point_ground_truth(point_ground_truth, articulation, depth=False):
    """-> bool(point_ground_truth); ValueError (before anything touches the GPU) when it is asked for without the articulation block,
    whose predicted joints it compares against, or on a depth pipeline, whose frames carry no per-point ground truth."""
    if point_ground_truth and not articulation:
        raise ValueError("point_ground_truth=True compares against the articulation block's joints: it needs articulation=True")
    if point_ground_truth and depth:
        raise ValueError("point_ground_truth=True reads 18-column raw rows: depth frames (depth_capacity) carry no per-point ground truth "
                         "(build_point_gt=True makes it on the device from link-label crops and scene tables)")
    return bool(point_ground_truth)


def check_loss_type(coord_regress_loss):
    if coord_regress_loss not in _TYPE_L:
        raise ValueError("coord_regress_loss must be 'L2' or 'L1' on the test path (got %r)" % (coord_regress_loss,))
    return coord_regress_loss


def check_point_clouds(clouds, norm_factors, max_clouds=None):
    """dataset.check_raw_clouds for a point-ground-truth stream: 1..max_clouds non-empty (n_raw, 18) arrays (dataset.pack_cloud's rows) and
    one finite norm factor per cloud.  -> (list of contiguous float32 (n_raw, 18) arrays, float32 (B,) norm factors); ValueError, before
    anything touches a device, otherwise."""
    if not isinstance(clouds, (list, tuple)):
        raise ValueError("clouds must be a list of (n_raw, %d) arrays [%s]" % (NCHAN, RAW_COLUMNS))
    if not 1 <= len(clouds) <= (max_clouds or 65535):
        raise ValueError("a batch holds 1..%d clouds, got %d" % (max_clouds or 65535, len(clouds)))
    out = []
    for i, c in enumerate(clouds):
        c = np.asarray(c.cpu().numpy() if torch.is_tensor(c) else c)
        if c.ndim != 2 or c.shape[1] != NCHAN or c.shape[0] == 0:
            raise ValueError("cloud %d: expected a non-empty (n_raw, %d) array [%s] (dataset.pack_cloud), got shape %s"
                             % (i, NCHAN, RAW_COLUMNS, c.shape))
        out.append(np.ascontiguousarray(c, np.float32))
    nf = np.asarray(norm_factors, np.float32).reshape(-1)
    if nf.size != len(out) or not np.isfinite(nf).all():
        raise ValueError("norm_factors: one finite value per cloud (%d clouds, got %s)" % (len(out), nf.tolist()))
    return out, nf


def check_frames(frame, n, name="frame"):
    """-> frame as a C-contiguous (n, 13) float64 numpy array; ValueError naming the entry (before anything touches a device) for anything
    that is not n rows of FRAME_WIDTH real numbers.  NaN is allowed: it marks a cloud without a ground-truth NAOCS pose."""
    try:
        a = np.ascontiguousarray(frame, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be an (n, %d) array of real numbers, got %r" % (name, FRAME_WIDTH, type(frame).__name__))
    if a.shape != (n, FRAME_WIDTH):
        raise ValueError("%s must be (%d, %d) -- one row [R (9) | s | t (3)], the ground-truth NAOCS pose of part 0, per cloud --, got %s"
                         % (name, n, FRAME_WIDTH, a.shape))
    if np.isinf(a).any():
        c, e = np.argwhere(np.isinf(a))[0]
        raise ValueError("%s[%d][%d] is infinite (NaN marks a missing entry)" % (name, c, e))
    return a


def pack_joint_frame(rt_naocs, scale_naocs):
    """The (n, 13) frames of n clouds from the reference's pickle shapes: rt_naocs[f] = gn_gt[...]['rt']['gt'] (K 4 x 4 matrices, part 0's is
    read), scale_naocs[f] = gn_gt[...]['scale']['gt'] (K scalars or 1-vectors, part 0's is read).  A cloud whose entry is None gets a NaN
    row."""
    n = len(rt_naocs)
    if len(scale_naocs) != n:
        raise ValueError("pack_joint_frame: rt_naocs and scale_naocs must hold one entry per frame")
    out = np.full((n, FRAME_WIDTH), np.nan)
    for f in range(n):
        if rt_naocs[f] is None or scale_naocs[f] is None:
            continue
        m = np.asarray(rt_naocs[f][0], np.float64)
        out[f, :9] = m[:3, :3].reshape(9)
        out[f, 9] = float(np.asarray(scale_naocs[f][0], np.float64).reshape(-1)[0])
        out[f, 10:] = m[:3, 3]
    return out


def point_gt_batch(raw_rows, offsets, perm, ancsh_pred, npcs_pred, art, frame, record, coord_regress_loss="L2", debug=False):
    """The per-point ground truth of a batch in ONE launch: raw_rows (capacity, 18) float32 on the device (dataset.pack_cloud's rows),
    offsets (B+1,) int32 (cloud c owns rows [offsets[c], offsets[c+1])), perm (B, N) int32 = the sampler's perm_out; ancsh_pred /
    npcs_pred = the two networks' output dicts (the ANCSH W / nocs / gocs / heatmap / unitvec / joint_axis / index heads, the NPCS W / nocs);
    art = the (B, K, 12) articulation block or the (B, K, 20) joint-state block; frame (B, 13) float64 = pack_joint_frame's rows; record
    (B, K, ld) float64, ld in CARRIED_WIDTHS.  Returns the (B, K, ld + 21) float64 block on the device: row (c, j) = [the input row, bit
    for bit | POINT_GT_COLUMNS] (include/ancsh_hip.h has the definitions and the NaN rules).  debug=True: (block, joint_gt (B, K-1, 6)
    float64 = the ground-truth joints [point | axis] in global NOCS, bit-equal to ancsh_joint_params(axis_mean=1)).  No host
    synchronisation and no allocation beyond the outputs: the captured streaming step calls it."""
    from .record import CARRIED_WIDTHS
    _lib.require_cuda(raw_rows, offsets, perm, art, frame, record)
    check_loss_type(coord_regress_loss)
    dev = record.device
    B, K = record.shape[:2]
    ld = record.shape[2] if record.dim() == 3 else -1
    if record.dtype != torch.float64 or record.dim() != 3 or ld not in CARRIED_WIDTHS or not record.is_contiguous():
        raise ValueError("record must be a contiguous (B, K, ld) float64 tensor, ld in %s" % (CARRIED_WIDTHS,))
    if art.dtype != torch.float64 or art.dim() != 3 or tuple(art.shape[:2]) != (B, K) or art.shape[2] not in (12, 20) or not art.is_contiguous():
        raise ValueError("art must be a contiguous (B, K, 12) or (B, K, 20) float64 tensor")
    if frame.dtype != torch.float64 or tuple(frame.shape) != (B, FRAME_WIDTH) or not frame.is_contiguous():
        raise ValueError("frame must be a contiguous (B, %d) float64 tensor" % FRAME_WIDTH)
    if raw_rows.dtype != torch.float32 or raw_rows.dim() != 2 or raw_rows.shape[1] != NCHAN or not raw_rows.is_contiguous():
        raise ValueError("raw_rows must be a contiguous (capacity, %d) float32 tensor [%s]" % (NCHAN, RAW_COLUMNS))
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (B + 1,) or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous (B+1,) int32 tensor")
    if perm.dtype != torch.int32 or perm.dim() != 2 or perm.shape[0] != B or not perm.is_contiguous():
        raise ValueError("perm must be a contiguous (B, N) int32 tensor")
    N = perm.shape[1]
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    heads = [f32(ancsh_pred[k]) for k in ("W", "nocs_per_point", "gocs_per_point", "heatmap_per_point", "unitvec_per_point",
                                          "joint_axis_per_point", "index_per_point")] + [f32(npcs_pred["W"]), f32(npcs_pred["nocs_per_point"])]
    G, JC = heads[2].shape[-1], heads[6].shape[-1]
    for t, ch in zip(heads, (K, 3 * K, G, 1, 3, 3, JC, K, 3 * K)):
        if t.numel() != B * N * ch:
            raise ValueError("a head of shape %s where (%d, %d, %d) is expected" % (tuple(t.shape), B, N, ch))
    wide = torch.empty((B, K, ld + POINT_GT_WIDTH), dtype=torch.float64, device=dev)
    joint_gt = torch.empty((B, max(K - 1, 0), 6), dtype=torch.float64, device=dev) if debug else None
    _lib.call("ancsh_point_gt_rec", B, N, K, NCHAN, _lib.ptr(raw_rows), int(raw_rows.shape[0]), _lib.ptr(offsets), _lib.ptr(perm), G, JC,
              *[_lib.ptr(t) for t in heads], _lib.ptr(art), art.shape[2], _lib.ptr(frame), _lib.ptr(record), ld,
              _TYPE_L[coord_regress_loss], _lib.ptr(wide), _lib.ptr(joint_gt if K > 1 else None))
    return (wide, joint_gt) if debug else wide


def stream_point_tables(rows, num_parts, is_mixed=True, pred_joint=True, early_split=True, pred_joint_ind=True, network="ancsh", layout=None):
    """The closing lines of eval_joint_params.py (:262-269) and the test_loss.txt line (lib/network.py:228-243) from accumulated streamed
    rows of a point-ground-truth pipeline (AncshPipeline(..., point_ground_truth=True)): rows (F, K, ld + 21) float64, one frame per
    leading index, as retire / stream_batches return them.  -> (joint lines, loss line):
      * joint lines: the shapes line, then per joint k the 'joint k with mean angle error ... degrees, mean dist ...' line and the bare
        pair under it; a NaN error counts as 0 (:264-265) and a line is the mean absolute error over the frames;
      * loss line: every loss's mean over the frames, then loss.collect_losses and loss.format_loss_result.  network="npcs": the NPCS
        network's line (its nocs and mIoU losses; it has no joint heads).
    layout (pose.record.RecordLayout, a pipeline's record_layout): rows are that pipeline's records, whatever else it was built with, and
    the block is read where the layout says; None: the block is the rows' last."""
    from ..loss import collect_losses, format_loss_result
    from .record import CARRIED_WIDTHS
    rows = np.asarray(rows, np.float64)
    if layout is not None:
        rows = layout.check(rows, "rows")[..., :layout.span("point_gt").stop]
    if rows.ndim != 3 or rows.shape[1] != num_parts or rows.shape[2] - POINT_GT_WIDTH not in CARRIED_WIDTHS:
        raise ValueError("rows must be (frames, %d, ld + %d) streamed point-ground-truth rows, ld in %s, got %s"
                         % (num_parts, POINT_GT_WIDTH, CARRIED_WIDTHS, rows.shape))
    if network not in ("ancsh", "npcs"):
        raise ValueError("network must be 'ancsh' or 'npcs', got %r" % (network,))
    ld = rows.shape[2] - POINT_GT_WIDTH
    r = np.nan_to_num(rows[:, 1:, ld + PGT_ANGLE_ERR], nan=0.0)
    t = np.nan_to_num(rows[:, 1:, ld + PGT_DIST_ERR], nan=0.0)
    lines = ["%s %s %s" % (r.shape, t.shape, num_parts)]
    for k in range(num_parts - 1):
        ra, ta = np.mean(np.abs(r[:, k])), np.mean(np.abs(t[:, k]))
        lines.append('joint {} with mean angle error {} degrees, mean dist {}'.format(k, ra, ta))
        lines.append("%s %s" % (ra, ta))
    col = lambda c: torch.from_numpy(np.ascontiguousarray(rows[:, 0, ld + c]))
    if network == "npcs":
        ld_ = {"nocs_loss": col(PGT_NPCS_NOCS), "miou_loss": torch.from_numpy(np.ascontiguousarray(rows[:, :, ld + PGT_NPCS_MIOU]))}
        flags = dict(is_mixed=False, pred_joint=False, pred_joint_ind=False)
        return lines, format_loss_result(collect_losses(ld_, **flags), early_split=early_split, **flags)
    ld_ = {"nocs_loss": col(PGT_NOCS), "miou_loss": torch.from_numpy(np.ascontiguousarray(rows[:, :, ld + PGT_MIOU])),
           "heatmap_loss": col(PGT_HEATMAP), "unitvec_loss": col(PGT_UNITVEC), "orient_loss": col(PGT_ORIENT),
           "index_loss": torch.from_numpy(np.ascontiguousarray(rows[:, 0, ld + PGT_INDEX.start:ld + PGT_INDEX.stop]))}
    if is_mixed:
        ld_["gocs_loss"] = col(PGT_GOCS)
    losses = collect_losses(ld_, is_mixed, pred_joint, pred_joint_ind)
    return lines, format_loss_result(losses, is_mixed, pred_joint, early_split, pred_joint_ind)
