"""Fit quality of a batch of pose records (ancsh_fit_quality_rec, csrc/fit_quality.hip): what the reference prints per part and drops
(evaluation/parallel_ancsh_pose.py:273, 311, 322) -- the consensus the RANSAC winners reached -- and what its verifiers say about the
poses the record actually holds: the residual norm of every point of the part under the refit baseline pose and under the nonlinear pose,
as inliers, mean, RMS, median and max.  One launch behind the fit; a consumer gates a pose on it without copying a point back."""
import math

import torch

from .. import _lib

FIT_QUALITY_WIDTH = 39          # include/ancsh_hip.h, ancsh_fit_quality_rec: the record's 26 columns + 13 of quality
FIT_QUALITY_MAX_N = 8192        # ANCSH_FIT_QUALITY_MAX_N: a longer part gets NaN statistics (and its true point count)
# columns of the wide record behind the 26 of the record
COL_POINTS, COL_CONSENSUS_A, COL_BASELINE, COL_SCORE_B, COL_NONLINEAR = 26, 27, 28, 33, 34       # BASELINE / NONLINEAR: + inliers, mean, RMS, median, max


def check_fit_quality(fit_quality, inlier_th):
    """-> bool(fit_quality); ValueError (before anything touches the GPU) when it is asked for with a threshold the verifier's test
    rho < inlier_th cannot use: not a finite number above 0."""
    if fit_quality and not (isinstance(inlier_th, (int, float)) and math.isfinite(inlier_th) and inlier_th > 0):
        raise ValueError("fit_quality=True counts the points with a residual below inlier_th: it must be finite and > 0, got %r" % (inlier_th,))
    return bool(fit_quality)


def fit_quality_batch(sol, inlier_th):
    """The fit quality of a PoseSolver.solve() result in ONE launch: sol["off"], sol["_src"], sol["_tgt"] (the packed rows both fit stages
    read), sol["record"] (B, K, 26) float64 as it stands (after the poison), sol["best_a"] and sol.get("score_b").  Returns the (B, K, 39)
    float64 block on the device: row (c, j) = [record row (26, bit for bit) | points of the part | stage A's consensus count | baseline
    pose: inliers at inlier_th, mean, RMS, median, max residual | stage B's score | nonlinear pose: the same five] (include/ancsh_hip.h has
    the NaN rules).  No host synchronisation and no allocation beyond the output: the captured streaming step calls it."""
    record, off, src, tgt = sol["record"], sol["off"], sol["_src"], sol["_tgt"]
    best_a, score_b = sol.get("best_a"), sol.get("score_b")
    _lib.require_cuda(record, off, src, tgt, best_a, score_b)
    check_fit_quality(True, inlier_th)
    B, K = record.shape[:2]
    if record.dtype != torch.float64 or tuple(record.shape) != (B, K, 26) or not record.is_contiguous():
        raise ValueError("record must be a contiguous (B, K, 26) float64 tensor")
    if off.dtype != torch.int32 or off.numel() != B * K + 1 or not off.is_contiguous():
        raise ValueError("off must be a contiguous int32 tensor of B * K + 1 = %d entries" % (B * K + 1))
    for name, t in (("_src", src), ("_tgt", tgt)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous (rows, 3) float32 tensor" % name)
    if best_a is not None and (best_a.dtype != torch.int32 or best_a.numel() != 2 * B * K or not best_a.is_contiguous()):
        raise ValueError("best_a must be a contiguous (B, K, 2) int32 tensor")
    if score_b is not None and (score_b.dtype != torch.float64 or score_b.numel() != B * (K - 1) or not score_b.is_contiguous()):
        raise ValueError("score_b must be a contiguous (B, K - 1) float64 tensor")
    wide = torch.empty((B, K, FIT_QUALITY_WIDTH), dtype=torch.float64, device=record.device)
    _lib.call("ancsh_fit_quality_rec", B, K, _lib.ptr(off), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(record), float(inlier_th),
              _lib.ptr(best_a), _lib.ptr(score_b), _lib.ptr(wide))
    return wide
