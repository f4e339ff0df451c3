"""numpy mirror of ancsh_gt_error_rec (include/ancsh_hip.h), operation by operation: the evaluation's rpy_err / xyz_err / scale_err, the
3-D IoU of the amodal boxes and the relative rotation / translation errors of a record row against a ground-truth row.  Test helper
only: float64, elementwise (numpy never fuses a multiply into an add), one cloud and one part at a time; the part pass (scale_pred,
dynam, count) is joint_state_mirror's."""
import numpy as np

from joint_state_mirror import part_extents

GT_WIDTH = 19
WIDTH = 12
SIGNS = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]], np.float64)


def rot_diff_degree(A, B):
    """A, B (9,) row-major: tr(A B^T) = (d_0 + d_1) + d_2, d_a = (A_a0 B_a0 + A_a1 B_a1) + A_a2 B_a2; arccos((tr - 1) / 2) mod 2 pi, in
    degrees.  No clamp: a trace above 3 gives NaN."""
    A, B = np.asarray(A, np.float64).reshape(9), np.asarray(B, np.float64).reshape(9)
    d = [(A[3 * a] * B[3 * a] + A[3 * a + 1] * B[3 * a + 1]) + A[3 * a + 2] * B[3 * a + 2] for a in range(3)]
    tr = (d[0] + d[1]) + d[2]
    with np.errstate(invalid="ignore"):
        return np.fmod(np.arccos((tr - 1.0) / 2.0), 2.0 * np.pi) / np.pi * 180.0


def relative(A, B):
    """(A^T B)_ac = (A_0a B_0c + A_1a B_1c) + A_2a B_2c, (9,) row-major."""
    A, B = np.asarray(A, np.float64).reshape(9), np.asarray(B, np.float64).reshape(9)
    return np.array([(A[a] * B[c] + A[3 + a] * B[3 + c]) + A[6 + a] * B[6 + c] for a in range(3) for c in range(3)])


def corners(extent, s, R, t):
    """get_3d_bbox(extent, shift = 1/2) * s through . R^T + t: (8, 3), reference's corner order."""
    extent, R, t = np.asarray(extent, np.float64), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)
    bb = (SIGNS * (extent / 2.0) + 0.5) * s
    return np.stack([((R[3 * e] * bb[:, 0] + R[3 * e + 1] * bb[:, 1]) + R[3 * e + 2] * bb[:, 2]) + t[e] for e in range(3)], axis=1)


def _frame(bb):
    o = bb[4]
    u = [bb[5] - o, bb[7] - o, bb[0] - o]
    return o, u, [(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] for v in u]


def grid(b1, b2, nres):
    """numpy.linspace's coordinates over the joint bounds: arange * step + start, the last one exactly stop; -> 3 arrays (nres,)."""
    both = np.concatenate([b1, b2], 0)
    lo, hi = both.min(0), both.max(0)
    out = []
    for c in range(3):
        x = np.arange(nres, dtype=np.float64) * ((hi[c] - lo[c]) / (nres - 1)) + lo[c]
        x[-1] = hi[c]
        out.append(x)
    return out


def projections(bb, xs, ys, zs):
    """The three projections of every grid point on the box's edges, (3, nres, nres, nres), and the edges' squared lengths."""
    o, u, d = _frame(bb)
    ux, uy, uz = (xs - o[0])[:, None, None], (ys - o[1])[None, :, None], (zs - o[2])[None, None, :]
    return np.stack([(ux * v[0] + uy * v[1]) + uz * v[2] for v in u]), d


def iou_counts(b1, b2, nres=50, return_clearance=False):
    """(intersection, union) of two (8, 3) corner tables on the nres^3 grid; return_clearance: + the smallest distance of a projection
    from the face it is tested against, in units of the edge length (how far the counts are from depending on a rounding)."""
    xs, ys, zs = grid(b1, b2, nres)
    ins, clear = [], np.inf
    for bb in (b1, b2):
        p, d = projections(bb, xs, ys, zs)
        ins.append(np.all([(p[k] > 0.0) & (p[k] < d[k]) for k in range(3)], axis=0))
        for k in range(3):
            clear = min(clear, np.abs(p[k]).min() / np.sqrt(d[k]), np.abs(p[k] - d[k]).min() / np.sqrt(d[k]))
    I, U = int((ins[0] & ins[1]).sum()), int((ins[0] | ins[1]).sum())
    return (I, U, clear) if return_clearance else (I, U)


def gt_error_reference(P, npcs_nocs, npcs_mask, record, gt, nres=50, return_counts=False):
    """P (B, N, >= 3), npcs_nocs (B, N, 3K), npcs_mask (B, N, K) float32; record (B, K, ld) float64, ld = 26 or 39; gt (B, K, 19) float64
    -> (B, K, ld + 12) float64 (return_counts: + {(c, j, q): (intersection, union, clearance)} of the pairs it counted)."""
    record, gt = np.ascontiguousarray(record, np.float64), np.asarray(gt, np.float64)
    B, K, ld = record.shape
    wide = np.full((B, K, ld + WIDTH), np.nan)
    wide[:, :, :ld].view(np.uint64)[...] = record.view(np.uint64)
    counts = {}
    for c in range(B):
        scale, dynam, count = part_extents(np.asarray(P)[c, :, :3], npcs_nocs[c], npcs_mask[c], record[c, 0, 13:22].reshape(3, 3), record[c, 0, 23:26])
        canon = -scale[:, 0] / np.float32(2) + np.float32(0.5)                  # float32
        for j in range(K):
            g, g0 = gt[c, j], gt[c, 0]
            wide[c, j, ld + 11] = count[j]
            for q in range(2):
                m, m0 = record[c, j, 13 * q:13 * q + 13], record[c, 0, 13 * q:13 * q + 13]
                e = wide[c, j, ld + 5 * q:ld + 5 * q + 5]
                dead, dead0 = np.isnan(m).any(), np.isnan(m0).any()
                if not dead:
                    e[0] = rot_diff_degree(m[:9], g[:9])
                    dt = m[10:13] - g[10:13]
                    e[1] = np.sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2])
                    e[2] = np.abs(m[9] - g[9])
                if not dead and not np.isnan(g[:16]).any() and count[j] > 0:
                    b_gt = corners(g[13:16], g[9], g[:9], g[10:13])
                    b_pr = corners(scale[j].astype(np.float64), m[9], m[:9].astype(np.float32).astype(np.float64),
                                   m[10:13].astype(np.float32).astype(np.float64))
                    I, U, clear = iou_counts(b_gt, b_pr, nres, True)
                    counts[(c, j, q)] = (I, U, clear)
                    e[3] = 1.0 if U == 0 else I / U
                rel = j > 0 and not dead and not dead0
                if rel:
                    e[4] = rot_diff_degree(relative(g0[:9], g[:9]), relative(m0[:9], m[:9]))
                if q == 1 and rel:
                    with np.errstate(invalid="ignore"):
                        d = dynam[j] - np.float64(canon[j])
                        v = (g[16:19] - g0[16:19]) - d * m0[[0, 3, 6]]
                        wide[c, j, ld + 10] = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (wide, counts) if return_counts else wide
