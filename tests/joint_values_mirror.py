"""Python statement of ancsh_joint_values_rec (include/ancsh_hip.h): the joint values q read off the part poses, one float64 operation at a
time in the header's order.  The link maps are ancsh_reproject_scene_build's mirror's (reprojection_mirror.scene_tables), the part of a link its
link_parts.  Validated on its own in tests/test_joint_values_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import pose_scene_mirror as PM
import reprojection_mirror as RP

WIDTH, HEAD, COLS, GROUPS = 24, 4, 5, 4
NAN = float("nan")
PI, TWO_PI = 3.14159265358979323846, 6.28318530717958647692


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def sigma(M):
    s = 0.0
    for a in range(3):
        for k in range(3):
            s = s + M[a][k] * M[a][k]
    return math.sqrt(s / 3.0)


def instance(value, ninst):
    return int(value) if 0.0 <= value < ninst and float(int(value)) == value else -1


def bridging_joint(kin_i, sc, j, K):
    """(l, kind, p, b) of part j's bridging joint in a scene table under the instance's kinematic table, or None."""
    parts, nl = RP.link_parts(sc, K)
    for l in range(1, nl):
        if parts[l] != j:
            continue
        pd, kd = float(kin_i[PM.KIN_HEAD + PM.KIN_LINK * l + 2]), float(kin_i[PM.KIN_HEAD + PM.KIN_LINK * l + 3])
        if kd not in (1.0, 2.0):
            continue
        if not (0.0 <= pd < l and float(int(pd)) == pd):
            continue
        b = int(parts[int(pd)])
        if b < 0 or b == j:
            continue
        return l, kd, int(pd), b
    return None


def group_columns(Bl, Bp, kl, kd, q_true):
    """The five columns of one pose group from the child's and the parent's (3, 4) maps (lists of Python floats) and the link's 40 kin values."""
    Ml, Mp = [r[:3] for r in Bl], [r[:3] for r in Bp]
    tl, tp = [r[3] for r in Bl], [r[3] for r in Bp]
    sl, sp = sigma(Ml), sigma(Mp)
    ss = sp * sl
    Rt = [[kl[4 + 4 * a + k] for k in range(3)] for a in range(3)]
    org, a = [kl[4 + 4 * i + 3] for i in range(3)], [kl[16], kl[17], kl[18]]
    with np.errstate(all="ignore"):
        div = lambda x, y: float(np.float64(x) / np.float64(y))          # IEEE division: a zero or NaN divisor gives inf / NaN, no exception
        E = [[div((Mp[0][i] * Ml[0][k] + Mp[1][i] * Ml[1][k]) + Mp[2][i] * Ml[2][k], ss) for k in range(3)] for i in range(3)]
        G = [[(Rt[0][i] * E[0][k] + Rt[1][i] * E[1][k]) + Rt[2][i] * E[2][k] for k in range(3)] for i in range(3)]
        v = [(G[2][1] - G[1][2]) / 2.0, (G[0][2] - G[2][0]) / 2.0, (G[1][0] - G[0][1]) / 2.0]
        c = (((G[0][0] + G[1][1]) + G[2][2]) - 1.0) / 2.0
        d = [tl[i] - (dot(Mp[i], org) + tp[i]) for i in range(3)]
        ra = [dot(Rt[i], a) for i in range(3)]
        w = [dot(Mp[i], ra) for i in range(3)]
        ww = dot(w, w)
        ln = math.sqrt(ww) if ww >= 0.0 else NAN
        if not all(math.isfinite(x) and x != 0.0 for x in (sl, sp, ln)):
            return [NAN] * COLS
        u = [w[i] / ln for i in range(3)]
        if kd == 1.0:
            Ga = [dot(G[i], a) for i in range(3)]
            x = [a[1] * Ga[2] - a[2] * Ga[1], a[2] * Ga[0] - a[0] * Ga[2], a[0] * Ga[1] - a[1] * Ga[0]]
            q = math.atan2(dot(a, v), c)
            off = math.atan2(math.sqrt(dot(x, x)), dot(a, Ga))
            gap = math.sqrt(dot(d, d))
        else:
            q = dot(d, u)
            off = math.atan2(math.sqrt(dot(v, v)), c)
            r = [d[i] - q * u[i] for i in range(3)]
            gap = math.sqrt(dot(r, r))
        err = q - q_true
        if kd == 1.0:
            if err > PI:
                err = err - TWO_PI
            elif err < -PI:
                err = err + TWO_PI
    return [q, err, off, gap, sl / sp]


def joint_values(kin, render, scene, rig, norm_factor, record, art, pose=None, refined=None):
    """The entry on its own arguments -> wide (n, K, art's width + 24)."""
    kin = np.asarray(kin, np.float64).reshape(-1, PM.KIN_WIDTH)
    render, scene, rig = np.asarray(render, np.float64), np.asarray(scene, np.float64), np.asarray(rig, np.float64)
    record, art = np.asarray(record, np.float64), np.asarray(art, np.float64)
    n, K, ld = art.shape
    wide = np.full((n, K, ld + WIDTH), np.nan)
    wide.view(np.uint64)[:, :, :ld] = np.ascontiguousarray(art).view(np.uint64)      # bit for bit, NaN payloads included
    geom = np.zeros((n, 5), np.int32)
    groups = [record[:, :, :13], record[:, :, 13:26]]
    if refined is not None:
        refined = np.asarray(refined, np.float64)
        groups += [refined[:, :, 0, :13], refined[:, :, 1, :13]]
    # ancsh_reproject_scene_build's maps of every link under its own part's pose, per group: tables[g][f] (208,)
    tables = []
    for g in range(0, len(groups), 2):
        t, _ = RP.scene_tables(render, scene, rig, norm_factor, np.concatenate([groups[g], groups[g + 1]], 2), geom, 0)
        tables += [t[:n], t[n:]]
    link = lambda t, l: [[float(x) for x in t[RP.RENDER_HEAD + RP.RENDER_LINK * l + 4 * a:RP.RENDER_HEAD + RP.RENDER_LINK * l + 4 * a + 4]] for a in range(3)]
    for f in range(n):
        nf = float(np.float32(norm_factor[f]))
        inst = instance(float(render[f, 9]), len(kin))
        if inst < 0 or not math.isfinite(nf) or nf == 0.0:
            continue
        for j in range(K):
            found = bridging_joint(kin[inst], scene[f], j, K)
            if found is None:
                continue
            l, kd, p, b = found
            kl = [float(x) for x in kin[inst, PM.KIN_HEAD + PM.KIN_LINK * l:PM.KIN_HEAD + PM.KIN_LINK * (l + 1)]]
            q_true = float(pose[f][l]) if pose is not None else NAN
            row = wide[f, j, ld:]
            row[:HEAD] = [l, kd, b, q_true]
            for g in range(len(groups)):
                if np.isfinite(groups[g][f, j]).all() and np.isfinite(groups[g][f, b]).all():
                    row[HEAD + COLS * g:HEAD + COLS * (g + 1)] = group_columns(link(tables[g][f], l), link(tables[g][f], p), kl, kd, q_true)
    return wide
