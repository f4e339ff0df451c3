"""numpy statement of ancsh_reproject_scene_build and ancsh_reproject_compare_rec (include/ancsh_hip.h): the predicted frames' render tables
from a pose record, one scalar float64 operation at a time in the written order, and the pixel comparison with exact integer sums (uint16) or
math.fsum (float32: the entry adds in a fixed order, so it agrees with the exact sum to rounding, not to the last bit).  exact_record builds
the record that undoes a frame's own maps in closed form.  Validated on its own in tests/test_reprojection_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import pose_scene_mirror as PM

RENDER_WIDTH, RENDER_HEAD, RENDER_LINK = 208, 16, 12
SCENE_WIDTH, SCENE_HEAD, SCENE_LINK, MAX_LINKS = 240, 16, 14, 16
RIG_ROT, RIG_HEAD, WIDTH = 4, 22, 15
f64 = np.float64


def rig_part(rig, j, K):
    w = 15 + 9 * K
    return rig[RIG_HEAD + j * w:RIG_HEAD + (j + 1) * w]


def link_parts(sc, K):
    """The part of every link as both entries read it: -1 for a link beyond nlinks, without a rank, or whose part is outside [0, K)."""
    nl = int(sc[14]) if 1.0 <= sc[14] <= MAX_LINKS else 0
    out = np.full(MAX_LINKS, -1, np.int64)
    for l in range(nl):
        rank, part = sc[SCENE_HEAD + SCENE_LINK * l], sc[SCENE_HEAD + SCENE_LINK * l + 1]
        if 0.0 <= rank < MAX_LINKS and 0.0 <= part < K:
            out[l] = int(part)
    return out, nl


def nocs_map(rig, j, K):
    """Q (3, 4): canonical coordinates -> part NOCS of part j, ancsh_point_gt_build's nocs_p as a map."""
    pt = rig_part(rig, j, K)
    o = [f64(f64(f64(f64(f64(0.0 - pt[a]) - pt[3 + a]) * pt[6 + a]) + 0.5) - pt[9 + a]) for a in range(3)]
    Q = np.zeros((3, 4))
    if rig[3] != 0.0:
        Rr = rig[RIG_ROT:RIG_ROT + 9].reshape(3, 3)
        for a in range(3):
            for k in range(3):
                Q[a, k] = f64(Rr[a, k] * pt[6 + k])
            Q[a, 3] = f64(f64(f64(f64(Rr[a, 0] * f64(o[0] - 0.5)) + f64(Rr[a, 1] * f64(o[1] - 0.5))) + f64(Rr[a, 2] * f64(o[2] - 0.5))) + 0.5)
    else:
        for a in range(3):
            Q[a, a], Q[a, 3] = pt[6 + a], o[a]
    return Q


def predicted_map(rt, sc, rig, nf, pose, l, j, K):
    """Link l of part j under the 13-value pose -> its (3, 4) render map, steps 1..5 of the header."""
    R = rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)].reshape(3, 4)
    M = sc[SCENE_HEAD + SCENE_LINK * l + 2:SCENE_HEAD + SCENE_LINK * (l + 1)].reshape(3, 4)
    N = PM.compose(M, R)
    P = np.zeros((3, 4))
    for a in range(3):
        for k in range(3):
            P[a, k] = f64(pose[9] * pose[3 * a + k])
        P[a, 3] = pose[10 + a]
    T2 = PM.compose(P, PM.compose(nocs_map(rig, j, K), N))
    out = np.zeros((3, 4))
    for a in range(3):
        for k in range(4):
            v = f64(T2[a, k] / nf)
            out[a, k] = -v if a == 1 else v
    return out


def scene_tables(render, scene, rig, norm_factor, record, geom, pixel_capacity):
    """The entry on its own arguments -> (render_out (2n, 208) float64, geom_out (2n, 5) int32)."""
    render, scene, rig = np.asarray(render, f64), np.asarray(scene, f64), np.asarray(rig, f64)
    record, geom = np.asarray(record, f64), np.asarray(geom, np.int64).reshape(-1, 5)
    n, K = record.shape[:2]
    out, gout = np.zeros((2 * n, RENDER_WIDTH)), np.zeros((2 * n, 5), np.int64)
    for v in range(2):
        for f in range(n):
            row = v * n + f
            out[row, :RENDER_HEAD] = render[f, :RENDER_HEAD]
            gout[row] = geom[f]
            if geom[f, 0] >= 0:
                gout[row, 0] = min(int(geom[f, 0]) + v * int(pixel_capacity), 0x7fffffff)
            parts, nl = link_parts(scene[f], K)
            nf = f64(np.float32(norm_factor[f]))
            for l in range(nl):
                j = parts[l]
                pose = record[f, max(j, 0), 13 * v:13 * v + 13]
                at = RENDER_HEAD + RENDER_LINK * l
                if j < 0 or not np.isfinite(pose).all() or not np.isfinite(nf) or nf == 0.0:
                    out[row, at:at + RENDER_LINK] = np.nan
                else:
                    out[row, at:at + RENDER_LINK] = predicted_map(render[f], scene[f], rig[f], nf, pose, l, j, K).reshape(12)
    return out, gout.astype(np.int32)


def usable(d):
    d = np.asarray(d)
    if d.dtype == np.uint16:
        return d != 0
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def part_image(depth, labels, parts):
    """(h, w) int: the part of every pixel by the entry's rule, -1 where the pixel belongs to none."""
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab < MAX_LINKS) & usable(depth)
    return np.where(ok, parts[np.where(lab < MAX_LINKS, lab, 0)], -1)


def pose_columns(obs, pred, sc, j, K):
    """(n_obs, the seven columns of one pose) for part j: obs and pred are (depth, labels) crops; exact counts, exact integer sums for
    uint16, math.fsum for float32; pose validity is the caller's."""
    parts, _ = link_parts(sc, K)
    o, p = part_image(obs[0], obs[1], parts) == j, part_image(pred[0], pred[1], parts) == j
    both = o & p
    n_obs, n_pred, n_both = int(o.sum()), int(p.sum()), int(both.sum())
    uni = n_obs + n_pred - n_both
    nan = float("nan")
    cols = [float(n_pred), float(n_both), n_both / uni if uni > 0 else nan, nan, nan, nan, nan]
    if n_both:
        scale = f64(sc[6])
        if np.asarray(obs[0]).dtype == np.uint16:
            dq = [int(a) - int(b) for a, b in zip(np.asarray(pred[0])[both].tolist(), np.asarray(obs[0])[both].tolist())]
            s1, s, s2, mx = sum(abs(v) for v in dq), sum(dq), sum(v * v for v in dq), max(abs(v) for v in dq)
            nb = f64(n_both)
            cols[3:] = [f64(f64(f64(s1) * scale) / nb), f64(np.sqrt(f64(f64(s2) / nb)) * scale), f64(f64(mx) * scale), f64(f64(f64(s) * scale) / nb)]
        else:
            d = [f64(f64(f64(a) - f64(b)) * scale) for a, b in zip(np.asarray(pred[0])[both], np.asarray(obs[0])[both])]
            cols[3:] = [math.fsum(abs(v) for v in d) / n_both, math.sqrt(math.fsum(f64(v * v) for v in d) / n_both), max(abs(v) for v in d),
                        math.fsum(d) / n_both]
    return n_obs, cols


def compare(obs_frames, pred_frames, scene, carried):
    """obs_frames: per frame (depth, labels) crops; pred_frames: per frame ((depth, labels) baseline, (depth, labels) nonlinear); scene (n,
    240); carried (n, K, ld) -> wide (n, K, ld + 15)."""
    carried = np.asarray(carried, f64)
    n, K, ld = carried.shape
    wide = np.full((n, K, ld + WIDTH), np.nan)
    wide[:, :, :ld] = carried
    for f in range(n):
        for j in range(K):
            ok = [np.isfinite(carried[f, j, 13 * v:13 * v + 13]).all() for v in range(2)]
            for v in range(2):
                n_obs, cols = pose_columns(obs_frames[f], pred_frames[f][v], scene[f], j, K)
                if ok[0] or ok[1]:
                    wide[f, j, ld] = n_obs
                if ok[v]:
                    wide[f, j, ld + 1 + 7 * v:ld + 8 + 7 * v] = cols
    return wide


# ---- the record that undoes a frame's own maps, in closed form ------------------------------------------------------------------------------------
def _hom(A):
    return np.vstack([np.asarray(A, f64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def exact_pose(rt, rig, nf, canon, l, j, K):
    """The pose [R (9) | s | t (3)] of part j under which link l's predicted map is its own render map: nf * D * R_l * N_l^-1 * Q_j^-1 with the
    inverses in closed form -- N_l = [Rc | offset] (`canon`, the kinematic table's own) inverts to [Rc^T | -Rc^T offset], Q_j to (Rr^T (n - 0.5)
    + 0.5 - o) / factor -- and s = nf / factor, which needs one factor for all three axes."""
    pt = rig_part(rig, j, K)
    fac = pt[6]
    assert pt[6] == pt[7] == pt[8], "an exact similarity needs an isotropic NOCS factor"
    o = np.array([((0.0 - pt[a]) - pt[3 + a]) * fac + 0.5 - pt[9 + a] for a in range(3)])
    Rr = rig[RIG_ROT:RIG_ROT + 9].reshape(3, 3) if rig[3] != 0.0 else np.eye(3)
    unrot = _hom(np.concatenate([Rr.T, (0.5 - Rr.T @ np.full(3, 0.5))[:, None]], 1))
    unscale = _hom(np.concatenate([np.eye(3) / fac, (-o / fac)[:, None]], 1))
    Rc, off = canon[0], canon[1]
    Ninv = _hom(np.concatenate([Rc.T, (-Rc.T @ off)[:, None]], 1))
    D = np.diag([1.0, -1.0, 1.0, 1.0])
    Rl = _hom(rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)])
    factors = (Rl, Ninv, unscale, unrot)
    pose4 = float(nf) * (D @ Rl @ Ninv @ unscale @ unrot)
    s = float(nf) / fac
    return np.concatenate([(pose4[:3, :3] / s).reshape(9), [s], pose4[:3, 3]]), factors


def exact_record(render, scene, rig, norm_factor, kin, K):
    """(n, K, 26): for every part, exact_pose through the part's link of lowest rank, in both pose slots; NaN rows for a part without a link."""
    n = len(render)
    rec = np.full((n, K, 26), np.nan)
    for f in range(n):
        parts, nl = link_parts(scene[f], K)
        for j in range(K):
            links = [l for l in range(nl) if parts[l] == j]
            if links:
                l = min(links, key=lambda i: scene[f][SCENE_HEAD + SCENE_LINK * i])
                k = kin[PM.KIN_HEAD + PM.KIN_LINK * l:PM.KIN_HEAD + PM.KIN_LINK * (l + 1)]
                pose, _ = exact_pose(render[f], rig[f], f64(np.float32(norm_factor[f])), (k[19:28].reshape(3, 3), k[28:31]), l, j, K)
                rec[f, j, :13] = rec[f, j, 13:] = pose
    return rec
