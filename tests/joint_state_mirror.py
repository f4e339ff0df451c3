"""numpy mirror of ancsh_joint_state_rec (include/ancsh_hip.h), written from the pred-side expressions of pose/evaluation.py -- `_frames` /
`boundaries` (scale_pred, dynam, canon: :201-212) and `relative_errors` (R_0^T R_j, t_j - t_0, dynam - canon: :215-246) -- plus the column
definitions of the joint state.  Test helper only: one cloud at a time, float64 unless the expression it mirrors is float32."""
import numpy as np

WIDTH = 20


def relative_pose(R, t):
    """R (K, 3, 3), t (K, 3) float64 -> (Rrel (K-1, 3, 3) = R_0^T R_j, t_j - t_0 (K-1, 3)): relative_errors' r_diff_pred and its
    NAOCS t_diff_pred."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    # Rrel[j][a][c] = sum_k R_0[k][a] R_j[k][c], the three products rounded one by one and added in k order: elementwise numpy, which
    # never fuses a multiply into an add (np.matmul hands 3 x 3 float64 to a BLAS that does, and lands an ulp away)
    A, Bm = R[0].T[None, :, None, :], np.swapaxes(R[1:], -1, -2)[:, None, :, :]
    return (A[..., 0] * Bm[..., 0] + A[..., 1] * Bm[..., 1]) + A[..., 2] * Bm[..., 2], t[1:] - t[:1]


def rotation_angle(Rrel):
    """(c, v, angle in degrees): c = (tr Rrel - 1) / 2 = the cosine, v = the antisymmetric part = axis * sine, angle = atan2(|v|, c)."""
    Rrel = np.asarray(Rrel, np.float64)
    c = (np.trace(Rrel) - 1.0) / 2.0
    v = 0.5 * np.array([Rrel[2, 1] - Rrel[1, 2], Rrel[0, 2] - Rrel[2, 0], Rrel[1, 0] - Rrel[0, 1]])
    return c, v, np.degrees(np.arctan2(np.sqrt(v @ v), c))


def part_extents(P, nocs, mask, R0, t0):
    """One cloud: (scale_pred (K, 3) float32, dynam (K,) float64, count (K,)) as ancsh_part_extents defines them (compute_miou.py:196-208,
    eval_pose_err.py:253-268): the part of a point is the first maximum of its mask row; scale_pred = 2 max |nocs_j - 0.5|; dynam = the min
    of the x coordinate in part 0's frame, the pose rounded to float32 like compose_rt, the products in float64."""
    P, nocs, mask = np.asarray(P, np.float32), np.asarray(nocs, np.float32), np.asarray(mask, np.float32)
    K = mask.shape[1]
    lab = np.argmax(mask, 1)
    r = np.asarray(R0, np.float64).astype(np.float32).astype(np.float64)
    t = np.asarray(t0, np.float64).astype(np.float32).astype(np.float64)
    m30 = np.float64(np.float32(-(t[0] * r[0, 0] + t[1] * r[1, 0] + t[2] * r[2, 0])))
    x = ((P[:, 0].astype(np.float64) * r[0, 0] + P[:, 1].astype(np.float64) * r[1, 0]) + P[:, 2].astype(np.float64) * r[2, 0]) + m30
    scale, dynam, count = np.full((K, 3), np.nan, np.float32), np.full(K, np.nan), np.zeros(K, np.int64)
    for j in range(K):
        sel = lab == j
        count[j] = sel.sum()
        if count[j]:
            scale[j] = np.float32(2) * np.abs(nocs[sel, 3 * j:3 * j + 3] - np.float32(0.5)).max(0)
            dynam[j] = x[sel].min()
    return scale, dynam, count


def joint_state_reference(P, npcs_nocs, npcs_mask, record, art):
    """P (B, N, >= 3), npcs_nocs (B, N, 3K), npcs_mask (B, N, K) float32; record (B, K, 26), art (B, K, 12) float64 -> (B, K, 20) float64."""
    record, art = np.asarray(record, np.float64), np.asarray(art, np.float64)
    B, K = record.shape[:2]
    wide = np.full((B, K, WIDTH), np.nan)
    wide[:, :, :12] = art
    for b in range(B):
        R, t = record[b, :, 13:22].reshape(K, 3, 3), record[b, :, 23:26]
        scale, dynam, count = part_extents(np.asarray(P)[b, :, :3], npcs_nocs[b], npcs_mask[b], R[0], t[0])
        canon = -scale[:, 0] / np.float32(2) + np.float32(0.5)                      # float32 (evaluation.py:208)
        wide[b, :, 19] = count
        nan_pose = np.isnan(record[b, :, 13:26]).any(1)
        dead = nan_pose | nan_pose[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            wide[b, :, 18] = np.where(dead, np.nan, dynam - canon.astype(np.float64))     # (evaluation.py:233)
            Rrel, dt = relative_pose(R, t)
            for j in range(1, K):
                if dead[j]:
                    continue
                c, v, wide[b, j, 12] = rotation_angle(Rrel[j - 1])
                u = art[b, j, 9:12] / np.sqrt(art[b, j, 9:12] @ art[b, j, 9:12])
                wide[b, j, 13] = np.degrees(np.arctan2(v @ (R[0].T @ u), c))
                wide[b, j, 14:17] = dt[j - 1]
                wide[b, j, 17] = dt[j - 1] @ u
    return wide
