"""Errors of a batch of pose records against ground truth (ancsh_gt_error_rec, csrc/gt_errors.hip): what the reference's offline
evaluation reports per frame and part -- rpy_err / xyz_err / scale_err of both poses (evaluation/parallel_ancsh_pose.py, the end of
solver_ransac_nonlinear), the 3-D IoU of the amodal boxes (compute_miou.py:150-229) and the relative rotation / translation error per
joint (eval_pose_err.py:279-338) -- in one launch behind the fit, from ground truth that travels in with the batch."""
import numpy as np
import torch

from .. import _lib

GT_WIDTH = 19                   # include/ancsh_hip.h, ancsh_gt_error_rec: a ground-truth row
GT_ERROR_WIDTH = 12             # the error columns behind the carried row: the record or the fit-quality wide record (pose.record)
GT_NRES = 50                    # the reference's iou_3d grid (lib/d3_utils.py:55)
# columns of a ground-truth row
GT_R, GT_S, GT_T, GT_EXTENT, GT_T_NAOCS = slice(0, 9), 9, slice(10, 13), slice(13, 16), slice(16, 19)
# the error columns, counted from the block's first (pose.record: RecordLayout.span("gt_errors").start): column = ld + ERR_*
ERR_RPY, ERR_XYZ, ERR_SCALE, ERR_IOU, ERR_REL_ROT = 0, 1, 2, 3, 4                          # the baseline pose (record columns 0..12)
ERR_NL_RPY, ERR_NL_XYZ, ERR_NL_SCALE, ERR_NL_IOU, ERR_NL_REL_ROT = 5, 6, 7, 8, 9           # the nonlinear pose (13..25)
ERR_NL_REL_TRANS = 10           # nonlinear pose: |(t_naocs_j - t_naocs_0) - (dynam_j - canon_j) R_0[:, 0]|
ERR_POINTS = 11                 # points of predicted NPCS part j
ERR_OF_KEY = {"baseline": ERR_RPY, "nonlinear": ERR_NL_RPY}      # where a key's five columns start


def check_ground_truth(gt, n, K, name="gt"):
    """-> gt as a C-contiguous (n, K, 19) float64 numpy array; ValueError naming the entry (before anything touches a device) for
    anything that is not n x K rows of GT_WIDTH real numbers.  NaN is allowed: it marks what a frame has no ground truth for."""
    try:
        a = np.ascontiguousarray(gt, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be an (n, K, %d) array of real numbers, got %r" % (name, GT_WIDTH, type(gt).__name__))
    if a.shape != (n, K, GT_WIDTH):
        raise ValueError("%s must be (%d, %d, %d) -- one row [R_gt (9) | s_gt | t_gt (3) | box extent (3) | t_naocs (3)] per cloud and "
                         "part --, got %s" % (name, n, K, GT_WIDTH, a.shape))
    if np.isinf(a).any():
        c, j, e = np.argwhere(np.isinf(a))[0]
        raise ValueError("%s[%d][%d][%d] is infinite (NaN marks a missing entry)" % (name, c, j, e))
    return a


def pack_ground_truth(rt, scale, box_extent, rt_naocs=None):
    """The (n, K, 19) ground truth of n frames from the reference's pickle shapes: rt[f] = pn_gt[...]['rt']['gt'] (K 4 x 4 matrices),
    scale[f] = pn_gt[...]['scale']['gt'] (K scalars or 1-vectors), box_extent[f] = bbox3d_all[instance] (K corner tables, entry j =
    [[min corner], [max corner]]: the extent is [j][1][0] - [j][0][0], compute_miou.py) or a (K, 3) array of extents, rt_naocs[f] =
    gn_gt[...]['rt']['gt'] (only its translations are read); None: columns 16..18 are NaN and so is the relative translation error.
    A frame whose rt / scale / box_extent is None gets all-NaN rows."""
    n = len(rt)
    if len(scale) != n or len(box_extent) != n or (rt_naocs is not None and len(rt_naocs) != n):
        raise ValueError("pack_ground_truth: rt, scale, box_extent (and rt_naocs) must hold one entry per frame")
    K = next((len(r) for r in rt if r is not None), 0)
    out = np.full((n, K, GT_WIDTH), np.nan)
    for f in range(n):
        if rt[f] is None or scale[f] is None or box_extent[f] is None:
            continue
        if len(rt[f]) != K or len(scale[f]) != K or len(box_extent[f]) != K:
            raise ValueError("pack_ground_truth: frame %d does not hold %d parts" % (f, K))
        for j in range(K):
            m = np.asarray(rt[f][j], np.float64)
            out[f, j, GT_R] = m[:3, :3].reshape(9)
            out[f, j, GT_S] = float(np.asarray(scale[f][j], np.float64).reshape(-1)[0])
            out[f, j, GT_T] = m[:3, 3]
            e = np.asarray(box_extent[f][j], np.float64)
            out[f, j, GT_EXTENT] = e if e.shape == (3,) else np.asarray(box_extent[f][j][1][0], np.float64) - np.asarray(box_extent[f][j][0][0], np.float64)
            if rt_naocs is not None and rt_naocs[f] is not None:
                out[f, j, GT_T_NAOCS] = np.asarray(rt_naocs[f][j], np.float64)[:3, 3]
    return out


def pack_box_extents(box_extent):
    """The (n, K, 19) ground truth of n frames that holds the part boxes only: NaN everywhere except columns 13..15, which are
    pack_ground_truth's for the same box_extent (box_extent[f] = K corner tables or a (K, 3) array of extents; None: a NaN frame).  What a
    pipeline built with build_gt_pose=True reads of its gt: the poses are fitted on the device."""
    n = len(box_extent)
    K = next((len(e) for e in box_extent if e is not None), 0)
    out = np.full((n, K, GT_WIDTH), np.nan)
    for f in range(n):
        if box_extent[f] is None:
            continue
        if len(box_extent[f]) != K:
            raise ValueError("pack_box_extents: frame %d does not hold %d parts" % (f, K))
        for j in range(K):
            e = np.asarray(box_extent[f][j], np.float64)
            out[f, j, GT_EXTENT] = e if e.shape == (3,) else np.asarray(box_extent[f][j][1][0], np.float64) - np.asarray(box_extent[f][j][0][0], np.float64)
    return out


def gt_error_batch(P, npcs_nocs, npcs_mask, record, gt, nres=GT_NRES):
    """The errors of a batch in ONE launch: P (B, N, C >= 3) float32 sampled points, npcs_nocs (B, N, 3K) and npcs_mask (B, N, K) float32:
    the heads the record was fitted on, record (B, K, ld) float64 -- the record or the fit-quality wide record --, gt (B, K, 19) float64
    on the device.  Returns the (B, K, ld + 12) float64 block on the device: row (c, j) = [the input row, bit for bit | rpy_err, xyz_err,
    scale_err, 3-D IoU, relative rotation error of the baseline pose | the same five of the nonlinear pose | its relative translation
    error | points of part j] (include/ancsh_hip.h has the definitions and the NaN rules).  No host synchronisation and no allocation
    beyond the output: the captured streaming step calls it."""
    from .record import carried_widths
    _lib.require_cuda(record, gt, P, npcs_nocs, npcs_mask)
    B, K = record.shape[:2]
    ld = record.shape[2] if record.dim() == 3 else -1
    if record.dtype != torch.float64 or record.dim() != 3 or ld not in carried_widths("gt_errors") or not record.is_contiguous():
        raise ValueError("record must be a contiguous (B, K, ld) float64 tensor, ld in %s" % (carried_widths("gt_errors"),))
    if gt.dtype != torch.float64 or tuple(gt.shape) != (B, K, GT_WIDTH) or not gt.is_contiguous():
        raise ValueError("gt must be a contiguous (B, K, %d) float64 tensor" % GT_WIDTH)
    N = P.shape[1] if P.dim() == 3 else -1
    for name, t, shape in (("npcs_nocs", npcs_nocs, (B, N, 3 * K)), ("npcs_mask", npcs_mask, (B, N, K))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s float32 tensor" % (name, shape))
    if P.dtype != torch.float32 or P.dim() != 3 or P.shape[0] != B or P.shape[2] < 3 or not P.is_contiguous():
        raise ValueError("P must be a contiguous (B, N, >= 3) float32 tensor")
    if not 2 <= int(nres) <= 64:
        raise ValueError("nres must be in [2, 64], got %r" % (nres,))
    wide = torch.empty((B, K, ld + GT_ERROR_WIDTH), dtype=torch.float64, device=record.device)
    _lib.call("ancsh_gt_error_rec", B, N, K, int(nres), _lib.ptr(P), P.shape[2], _lib.ptr(npcs_nocs), _lib.ptr(npcs_mask), _lib.ptr(record),
              ld, _lib.ptr(gt), _lib.ptr(wide))
    return wide
