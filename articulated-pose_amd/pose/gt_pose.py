"""The ground-truth poses of a streamed batch (ancsh_gt_pose_build, csrc/gt_pose.hip): step 1 of evaluation.sh -- per part, the Umeyama
fit between the sampled points' ground-truth part NOCS / NAOCS and the sampled points (evaluation/compute_gt_pose.py:80-89, run with --nocs
ANCSH and with --nocs NAOCS) -- in one launch directly behind the sampler, from the 18-column raw rows (dataset.pack_cloud), the sampler's
permutation and the sampled P.  It writes the (B, K, 19) table ancsh_gt_error_rec reads and the (B, 13) table ancsh_point_gt_rec reads."""
import torch

from .. import _lib
from ..dataset import NCHAN
from .gt_errors import GT_WIDTH
from .point_gt import FRAME_WIDTH, RAW_COLUMNS


def gt_pose_batch(raw_rows, offsets, perm, P, extent=None, num_parts=None, out=None):
    """Both ground-truth pose tables of a batch in ONE launch: raw_rows (capacity, 18) float32 on the device (dataset.pack_cloud's rows),
    offsets (B+1,) int32 (cloud c owns rows [offsets[c], offsets[c+1])), perm (B, N) int32 = the sampler's perm_out, P (B, N, C >= 3)
    float32 = the sampled points the networks read; extent: None (NaN extents) or a (B, K, 3) float64 tensor whose last dimension is
    dense -- a view such as gt[:, :, 13:16] of a (B, K, 19) table is read where it lies.  Returns (gt (B, K, 19), frame (B, 13)) float64 on
    the device: gt rows are [R (9) | s | t (3) of the part-NOCS fit | the extent row, bit for bit | t of the NAOCS fit], frame rows [R (9) |
    s | t (3)] of part 0's NAOCS fit (include/ancsh_hip.h has the definitions and the NaN rules).  K is extent's, out[0]'s or num_parts
    (at least one of them must say it, and they must agree).  out = (gt, frame): write into these contiguous tensors instead (either may be
    None to skip it).  No host synchronisation and no allocation beyond the outputs: the captured streaming step calls it."""
    _lib.require_cuda(raw_rows, offsets, perm, P, extent, *(out or ()))
    if raw_rows.dtype != torch.float32 or raw_rows.dim() != 2 or raw_rows.shape[1] != NCHAN or not raw_rows.is_contiguous():
        raise ValueError("raw_rows must be a contiguous (capacity, %d) float32 tensor [%s]" % (NCHAN, RAW_COLUMNS))
    if perm.dtype != torch.int32 or perm.dim() != 2 or not perm.is_contiguous():
        raise ValueError("perm must be a contiguous (B, N) int32 tensor")
    B, N = perm.shape
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (B + 1,) or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous (B+1,) int32 tensor")
    if P.dtype != torch.float32 or P.dim() != 3 or tuple(P.shape[:2]) != (B, N) or P.shape[2] < 3 or not P.is_contiguous():
        raise ValueError("P must be a contiguous (B, N, >= 3) float32 tensor")
    K, ld_extent = (None if num_parts is None else int(num_parts)), None
    if extent is not None:
        if extent.dtype != torch.float64 or extent.dim() != 3 or extent.shape[0] != B or extent.shape[2] != 3:
            raise ValueError("extent must be a (B, K, 3) float64 tensor")
        if K is not None and extent.shape[1] != K:
            raise ValueError("extent holds %d parts, num_parts is %d" % (extent.shape[1], K))
        K = extent.shape[1]
        # row (c, j) lies at (c * K + j) * ld_extent: a dense last dimension and clouds K rows apart (a dimension of one has no stride to check)
        ld_extent = extent.stride(1) if K > 1 else extent.stride(0) if B > 1 else 3
        if extent.stride(2) != 1 or ld_extent < 3 or (B > 1 and extent.stride(0) != K * ld_extent):
            raise ValueError("extent must be contiguous or a column slice of a contiguous (B, K, W) table, got strides %s"
                             % (tuple(extent.stride()),))
    if out is None:
        if K is None:
            raise ValueError("gt_pose_batch needs the part count: pass extent, out or num_parts")
        gt = torch.empty((B, K, GT_WIDTH), dtype=torch.float64, device=raw_rows.device)
        frame = torch.empty((B, FRAME_WIDTH), dtype=torch.float64, device=raw_rows.device)
    else:
        gt, frame = out
        if gt is None and frame is None:
            raise ValueError("out = (gt, frame): at least one of them must be a tensor")
        if gt is not None:
            if gt.dtype != torch.float64 or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != GT_WIDTH or not gt.is_contiguous() \
                    or (K is not None and gt.shape[1] != K):
                raise ValueError("out[0] must be a contiguous (B, K, %d) float64 tensor" % GT_WIDTH)
            K = gt.shape[1]
        if frame is not None and (frame.dtype != torch.float64 or tuple(frame.shape) != (B, FRAME_WIDTH) or not frame.is_contiguous()):
            raise ValueError("out[1] must be a contiguous (B, %d) float64 tensor" % FRAME_WIDTH)
        if K is None:
            raise ValueError("gt_pose_batch needs the part count: pass extent, out[0] or num_parts")
    _lib.call("ancsh_gt_pose_build", B, N, K, NCHAN, _lib.ptr(raw_rows), int(raw_rows.shape[0]), _lib.ptr(offsets), _lib.ptr(perm), _lib.ptr(P),
              P.shape[2], _lib.ptr(extent), ld_extent or 0, _lib.ptr(gt), _lib.ptr(frame))
    return gt, frame
