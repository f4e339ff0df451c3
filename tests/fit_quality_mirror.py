"""numpy mirror of ancsh_fit_quality_rec (include/ancsh_hip.h): the verifier's residual norm of every point of a part
(evaluation/parallel_ancsh_pose.py:51-52, 189-192, the matmul written out) under the two poses of a record row, and its inliers, mean, RMS,
median and max.  Test helper only: float64, elementwise (numpy never fuses a multiply into an add), one part at a time."""
import numpy as np

WIDTH = 39
MAX_N = 8192


def residual_norms(src, tgt, pose):
    """src, tgt (n, 3) float32 (the point's part-NOCS triple, the sampled point), pose (13,) float64 [R row-major | s | t] -> rho (n,) float64:
    y_c = (R_c0 x_0 + R_c1 x_1) + R_c2 x_2;  r_c = (tgt_c - s y_c) - t_c;  rho = sqrt((r_0^2 + r_1^2) + r_2^2)."""
    x, g, m = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64), np.asarray(pose, np.float64)
    r = []
    for c in range(3):
        y = (m[3 * c] * x[:, 0] + m[3 * c + 1] * x[:, 1]) + m[3 * c + 2] * x[:, 2]
        r.append((g[:, c] - m[9] * y) - m[10 + c])
    return np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])


def five(rho, inlier_th):
    """[inliers, mean, RMS, median, max] of a part's norms (n >= 1)."""
    return np.array([np.sum(rho < inlier_th), np.mean(rho), np.sqrt(np.mean(rho * rho)), np.median(rho), np.max(rho)], np.float64)


def fit_quality_reference(off, src, tgt, record, inlier_th, best_a=None, score_b=None):
    """off (B*K+1,), src / tgt (rows, 3) float32, record (B, K, 26) float64, best_a (B*K, 2) int or None, score_b (B*(K-1),) float64 or None
    -> (B, K, 39) float64."""
    record = np.asarray(record, np.float64)
    B, K = record.shape[:2]
    off = np.asarray(off, np.int64)
    wide = np.full((B, K, WIDTH), np.nan)
    wide[:, :, :26].view(np.uint64)[...] = record.view(np.uint64)
    for c in range(B):
        for j in range(K):
            p = c * K + j
            a, n = off[p], off[p + 1] - off[p]
            wide[c, j, 26] = n
            if best_a is not None:
                wide[c, j, 27] = np.asarray(best_a).reshape(-1, 2)[p, 1]
            if score_b is not None and K > 1:
                wide[c, j, 33] = np.asarray(score_b, np.float64).reshape(-1)[c * (K - 1) + max(j - 1, 0)]
            if not 1 <= n <= MAX_N:
                continue
            for q, col in ((0, 28), (1, 34)):
                pose = record[c, j, 13 * q:13 * q + 13]
                if not np.isnan(pose).any():
                    wide[c, j, col:col + 5] = five(residual_norms(src[a:a + n], tgt[a:a + n], pose), inlier_th)
    return wide


def partition(P, nocs, mask):
    """ancsh_pose_partition on the host: labels = argmax(mask) (first maximum), every cloud's points grouped by label in ascending point
    order; -> (off (B*K+1,) int32, src (B*N, 3), tgt (B*N, 3) float32)."""
    P, nocs, mask = np.asarray(P, np.float32), np.asarray(nocs, np.float32), np.asarray(mask, np.float32)
    B, N, K = mask.shape
    off, src, tgt = [0], [], []
    for c in range(B):
        lab = np.argmax(mask[c], 1)
        for j in range(K):
            idx = np.flatnonzero(lab == j)
            src.append(nocs[c, idx, 3 * j:3 * j + 3])
            tgt.append(P[c, idx, :3])
            off.append(off[-1] + len(idx))
    return np.asarray(off, np.int32), np.concatenate(src), np.concatenate(tgt)
