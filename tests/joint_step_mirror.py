"""Python-float statement of ancsh_refine_joint_step (include/ancsh_hip.h): the joint step of render-and-compare ICP one scalar float64 operation
at a time in the written order (a Python float is an IEEE double, math.sqrt is correctly rounded), so that on the entry's own inputs -- the
pass's sums, the predicted render tables, the poses the pass read -- it gives xi, pose_out, best, state and obj byte for byte.  The quaternion
update is refinement_mirror's.  Validated on its own in tests/test_refine_joints_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import refinement_mirror as RF
from reprojection_mirror import link_parts

PARAMS, OBJ, XI, BEST = 24, 8, 48, 18
KIN_WIDTH, KIN_HEAD, KIN_LINK = 672, 32, 40
RENDER_HEAD, RENDER_LINK = 16, 12
NAN = float("nan")
dot = RF.dot


def link_map(rt, l):
    return [float(v) for v in rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)]]


def point(R, x, nf):
    m = [((R[4 * b] * x[0] + R[4 * b + 1] * x[1]) + R[4 * b + 2] * x[2]) + R[4 * b + 3] for b in range(3)]
    return RF.cloud(m[0], m[1], m[2], nf)


def direction(R, d):
    """-> (normalise(F R d), whether its length is finite and > 0)."""
    m = [(R[4 * b] * d[0] + R[4 * b + 1] * d[1]) + R[4 * b + 2] * d[2] for b in range(3)]
    m[1] = -m[1]
    n2 = dot(m, m)
    ln = math.sqrt(n2) if n2 >= 0.0 else NAN
    if not (ln > 0.0 and math.isfinite(ln)):
        return [NAN] * 3, False                                            # the joint is not active: the values are never used
    return [v / ln for v in m], True


def rows(e, h, r, sc, ident):
    """Three rows: (G (3 x 12): [-[sc e]x | ident I] for the child's part, [[sc h]x | -ident I] for the parent's; r0 = sc r)."""
    ea, ha = [sc * v for v in e], [sc * v for v in h]
    G = [[0.0, ea[2], -ea[1]], [-ea[2], 0.0, ea[0]], [ea[1], -ea[0], 0.0]]
    Gb = [[0.0, -ha[2], ha[1]], [ha[2], 0.0, -ha[0]], [-ha[1], ha[0], 0.0]]
    out = []
    for a in range(3):
        out.append(G[a] + [ident if a == k else 0.0 for k in range(3)] + Gb[a] + [-ident if a == k else 0.0 for k in range(3)])
    return out, [sc * v for v in r]


def rotate_T(T, d):
    return [(T[4 * i] * d[0] + T[4 * i + 1] * d[1]) + T[4 * i + 2] * d[2] for i in range(3)]


def joints(kin, sc, rt, nf, live, centres, K, axis_len, frozen=None):
    """The active joints of one (frame, pose), l ascending: dicts l, p, kind, a, b (the child's and the parent's part), G (6 or 9 rows of
    12), r0, and x_c, x_p, u_c, u_p.  frozen = {link: u_p}: a prismatic joint's projection is built from this direction, not from the
    tables' (the rows are linearised with u_p held fixed: finite differences of the residual hold it fixed too)."""
    parts, nl = link_parts(sc, K)
    kin = np.asarray(kin, np.float64).reshape(-1, KIN_WIDTH)
    iv = float(rt[9])
    if not (0.0 <= iv < len(kin) and float(int(iv)) == iv):
        return []
    tab = kin[int(iv)]
    out = []
    for l in range(1, nl):
        kl = [float(v) for v in tab[KIN_HEAD + KIN_LINK * l:KIN_HEAD + KIN_LINK * (l + 1)]]
        pd, kd = kl[2], kl[3]
        if not (0.0 <= pd < l and float(int(pd)) == pd) or kd not in (1.0, 2.0):
            continue
        p = int(pd)
        a, b = parts[l], parts[p]
        if a < 0 or b < 0 or a == b or not (live[a] and live[b]):
            continue
        Rl, Rp, T, ax = link_map(rt, l), link_map(rt, p), kl[4:16], kl[16:19]
        xc, xp = point(Rl, [0.0, 0.0, 0.0], nf), point(Rp, [T[3], T[7], T[11]], nf)
        uc, ok1 = direction(Rl, ax)
        up, ok2 = direction(Rp, rotate_T(T, ax))
        ok = ok1 and ok2
        ca, cb = centres[a], centres[b]
        e, h = [xc[i] - ca[i] for i in range(3)], [xp[i] - cb[i] for i in range(3)]
        r, du = [xc[i] - xp[i] for i in range(3)], [uc[i] - up[i] for i in range(3)]
        G, r0 = rows(e, h, r, 1.0, 1.0)
        Gd, rd = rows(uc, up, du, axis_len, 0.0)
        G, r0 = G + Gd, r0 + rd
        if kd == 2.0:
            uf = up if frozen is None else frozen[l]
            P = [[(1.0 if i == k else 0.0) - uf[i] * uf[k] for k in range(3)] for i in range(3)]
            top = [[(P[i][0] * G[0][c] + P[i][1] * G[1][c]) + P[i][2] * G[2][c] for c in range(12)] for i in range(3)]
            r0[:3] = [(P[i][0] * r0[0] + P[i][1] * r0[1]) + P[i][2] * r0[2] for i in range(3)]
            G[:3] = top
            a0, a1, a2 = abs(ax[0]), abs(ax[1]), abs(ax[2])
            k = (2 if a2 < a1 else 1) if a1 < a0 else (2 if a2 < a0 else 0)
            ek = [1.0 if k == i else 0.0 for i in range(3)]
            bx = [ax[1] * ek[2] - ax[2] * ek[1], ax[2] * ek[0] - ax[0] * ek[2], ax[0] * ek[1] - ax[1] * ek[0]]
            bl = math.sqrt(dot(bx, bx))
            ok = ok and bl > 0.0 and math.isfinite(bl)
            if not ok:
                continue
            bx = [v / bl for v in bx]
            vc, ok3 = direction(Rl, bx)
            vp, ok4 = direction(Rp, rotate_T(T, bx))
            ok = ok and ok3 and ok4
            Gv, rv = rows(vc, vp, [vc[i] - vp[i] for i in range(3)], axis_len, 0.0)
            G, r0 = G + Gv, r0 + rv
        if not (ok and all(math.isfinite(v) for v in r0)):
            continue
        out.append(dict(l=l, p=p, kind=int(kd), a=a, b=b, G=G, r0=r0, xc=xc, xp=xp, uc=uc, up=up))
    return out


def solve(H, g):
    """Cholesky in the entry's order -> (ok, xi)."""
    n = len(g)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        for i in range(j, n):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                if not (s > 0.0 and math.isfinite(s)):
                    return False, None
                L[j][j] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y, xi = [0.0] * n, [0.0] * n
    for i in range(n):
        s = 0.0 - g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(n - 1, i, -1):
            s = s - L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    if not all(math.isfinite(v) for v in xi):
        return False, None
    return True, xi


def system(J, sums, live, nrows, K, params, w2n):
    """(H (6K x 6K), g): the parts' damped blocks and the joints' rows, in the entry's order of addition."""
    n, damping, min_pixels = 6 * K, float(params[3]), float(params[5])
    H, g = [[0.0] * n for _ in range(n)], [0.0] * n
    for j in range(K):
        S = [float(v) for v in sums[j]]
        use = live[j] and nrows[j] >= min_pixels
        for a in range(6):
            for b in range(6):
                lo, hi = min(a, b), max(a, b)
                h = 1.0 if a == b else 0.0
                if live[j]:
                    h = S[6 * lo - (lo * (lo - 1)) // 2 + (hi - lo)] if use else 0.0
                    if a == b:
                        h = h + (damping * h + 1e-12)
                H[6 * j + a][6 * j + b] = h
            g[6 * j + a] = S[21 + a] if use else 0.0
    for jt in J:
        col = [6 * jt["a"] + p for p in range(6)] + [6 * jt["b"] + p for p in range(6)]
        G, r0 = jt["G"], jt["r0"]
        for p in range(12):
            for q in range(12):
                t = 0.0
                for r in range(len(G)):
                    t = t + G[r][p] * G[r][q]
                H[col[p]][col[q]] = H[col[p]][col[q]] + w2n * t
            t = 0.0
            for r in range(len(G)):
                t = t + G[r][p] * r0[r]
            g[col[p]] = g[col[p]] + w2n * t
    return H, g


def joint_step(kin, sc, rt, nf, params, pass_index, is_last, poses, sums, pose_out, state, obj):
    """One (frame, pose): poses (K, 13) the pass read, sums (K, 32 or 36) and pose_out (K, 13) what it wrote; state (K, 18) and obj (8,) are
    updated in place.  -> (xi (48,), pose_out (K, 13), best (K, 18), the active joints)."""
    K = len(poses)
    nf = float(nf)
    max_dist, max_angle, min_pixels, weight, axis_len = (float(params[k]) for k in (1, 4, 5, 16, 17))
    poses = [[float(v) for v in p] for p in poses]
    sums = np.asarray(sums, np.float64)
    live = [RF.pose_ok(p, nf) for p in poses]
    centres = [RF.centre(p) if live[j] else None for j, p in enumerate(poses)]
    nrows = [(float(sums[j][28]) + float(sums[j][33]) if sums.shape[1] == 36 else float(sums[j][28])) if live[j] else 0.0 for j in range(K)]
    nsum = ncount = 0.0
    for j in range(K):
        if live[j] and nrows[j] >= min_pixels:
            nsum, ncount = nsum + nrows[j], ncount + 1.0
    has_nbar = ncount > 0.0
    w2n = (weight * weight) * (nsum / ncount) if has_nbar else 0.0
    J = joints(kin, sc, rt, nf, live, centres, K, axis_len)
    njoints, sumr, gap = float(len(J)), 0.0, 0.0
    for jt in J:
        rr = 0.0
        for v in jt["r0"]:
            rr = rr + v * v
        sumr, gap = sumr + rr, gap + dot(jt["r0"], jt["r0"])
    num = den = moved = 0.0
    for j in range(K):
        if not live[j]:
            continue
        if sums[j][29] > 0.0:
            num, den = num + float(sums[j][30]) * float(sums[j][29]), den + float(sums[j][29])
        if sums[j][31] == 1.0:
            moved = 1.0
    coupled = njoints > 0.0 and has_nbar
    if coupled:
        num = num + w2n * sumr
    Cobj = num / den if den > 0.0 else NAN
    out = np.array(pose_out, np.float64).reshape(K, 13).copy()
    xi_out, solved = [0.0] * XI, False
    if coupled and not is_last:
        H, g = system(J, sums, live, nrows, K, params, w2n)
        solved, xi = solve(H, g)
        if solved:
            f = 1.0
            for j in range(K):
                if not live[j]:
                    continue
                wn, dn = math.sqrt(dot(xi[6 * j:], xi[6 * j:])), math.sqrt(dot(xi[6 * j + 3:], xi[6 * j + 3:]))
                if wn > max_angle and max_angle / wn < f:
                    f = max_angle / wn
                if dn > max_dist and max_dist / dn < f:
                    f = max_dist / dn
            if f < 1.0:
                xi = [v * f for v in xi]
            xi_out[:6 * K] = xi
            for j in range(K):
                if live[j]:
                    out[j] = pose_step(xi[6 * j:6 * j + 6], poses[j], centres[j])
    if solved:
        moved = 1.0
    first = pass_index == 0
    cost_start, cost_best = (Cobj, Cobj) if first else (float(obj[0]), float(obj[1]))
    take = first or Cobj < cost_best
    best_pass = float(pass_index) if take else float(obj[2])
    passes_solved = (0.0 if first else float(obj[3])) + moved
    obj[:] = [cost_start, Cobj if take else cost_best, best_pass, passes_solved, Cobj, njoints, 1.0 if solved else 0.0,
              math.sqrt(gap / njoints) if njoints > 0.0 else NAN]
    best = np.full((K, BEST), np.nan)
    for j in range(K):
        if take:
            state[j, :13] = poses[j]
            if first:
                state[j, 13] = sums[j][30] if live[j] else NAN
            state[j, 14] = sums[j][30] if live[j] else NAN
            state[j, 15] = sums[j][28] if live[j] else NAN
        state[j, 16], state[j, 17] = best_pass, passes_solved
        if live[j]:
            best[j] = state[j]
    return np.array(xi_out), out, best, J


def pose_step(xi, pose, c):
    """refinement_mirror.solve_update's tail: the quaternion of w, the pose turned about c and moved by dt."""
    hx, hy, hz = xi[0] / 2.0, xi[1] / 2.0, xi[2] / 2.0
    qn = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    w, x, yq, z = 1.0 / qn, hx / qn, hy / qn, hz / qn
    dR = [1.0 - 2.0 * (yq * yq + z * z), 2.0 * (x * yq - w * z), 2.0 * (x * z + w * yq),
          2.0 * (x * yq + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (yq * z - w * x),
          2.0 * (x * z - w * yq), 2.0 * (yq * z + w * x), 1.0 - 2.0 * (x * x + yq * yq)]
    out = [0.0] * 13
    for a in range(3):
        for k in range(3):
            out[3 * a + k] = (dR[3 * a] * pose[k] + dR[3 * a + 1] * pose[3 + k]) + dR[3 * a + 2] * pose[6 + k]
    out[9] = pose[9]
    u = [pose[10] - c[0], pose[11] - c[1], pose[12] - c[2]]
    for a in range(3):
        out[10 + a] = (dot(dR[3 * a:3 * a + 3], u) + c[a]) + xi[3 + a]
    return out


def step_batch(kin, scene, tables, norm_factor, params, pass_index, is_last, pose_in, sums, pose_out, state, obj):
    """The launch: pose_in (n, K, >= 26), sums (n, K, 2, 32 or 36), pose_out (n, K, 26) as the pass wrote it, tables (2n, 208); state (n, K, 2,
    18) and obj (n, 2, 8) updated in place -> (xi (n, 2, 48), pose_out (n, K, 26), best (n, K, 2, 18))."""
    pose_in, pose_out = np.asarray(pose_in, np.float64), np.array(pose_out, np.float64)
    n, K = pose_in.shape[:2]
    xi, best = np.zeros((n, 2, XI)), np.full((n, K, 2, BEST), np.nan)
    for f in range(n):
        nf = float(np.float32(norm_factor[f]))
        for v in range(2):
            st = state[f, :, v].copy()
            x, po, b, _ = joint_step(kin, scene[f], tables[v * n + f], nf, params, pass_index, is_last, pose_in[f, :, 13 * v:13 * v + 13],
                                     sums[f, :, v], pose_out[f, :, 13 * v:13 * v + 13], st, obj[f, v])
            state[f, :, v] = st
            xi[f, v], pose_out[f, :, 13 * v:13 * v + 13], best[f, :, v] = x, po, b
    return xi, pose_out, best


def residuals(J):
    """Every joint's rows, stacked: (r0 (rows,), G (rows, 6 K) needs K: use stacked(J, K))."""
    return np.concatenate([np.asarray(jt["r0"]) for jt in J]) if J else np.zeros(0)


def stacked(J, K):
    """-> (r0 (rows,), G (rows, 6 K)) of all joints, the 12 columns of each spread to its two parts' places."""
    r0, G = residuals(J), np.zeros((sum(len(jt["G"]) for jt in J), 6 * K))
    at = 0
    for jt in J:
        g = np.asarray(jt["G"])
        G[at:at + len(g), 6 * jt["a"]:6 * jt["a"] + 6] = g[:, :6]
        G[at:at + len(g), 6 * jt["b"]:6 * jt["b"] + 6] = g[:, 6:]
        at += len(g)
    return r0, G


def hinge_gaps(kin, scene, tables, norm_factor, record, K):
    """|x_c - x_p| per (frame, pose, active joint) at the poses `record` (n, K, >= 26) whose predicted tables are `tables` (2n, 208):
    -> list over frames of list over poses of {link: gap}."""
    record = np.asarray(record, np.float64)
    n, out = len(record), []
    for f in range(n):
        nf, per = float(np.float32(norm_factor[f])), []
        for v in range(2):
            poses = [[float(x) for x in record[f, j, 13 * v:13 * v + 13]] for j in range(K)]
            live = [RF.pose_ok(p, nf) for p in poses]
            centres = [RF.centre(p) if live[j] else None for j, p in enumerate(poses)]
            J = joints(kin, scene[f], tables[v * n + f], nf, live, centres, K, 0.0)
            per.append({jt["l"]: math.sqrt(sum((jt["xc"][i] - jt["xp"][i]) ** 2 for i in range(3))) for jt in J})
        out.append(per)
    return out


def refine(mesh, kin, render, scene, rigs, norm_factor, record, geom, frames, params):
    """The whole loop with the joint step behind every pass, on refinement_mirror.refine's arguments and the kinematic table(s) -> (columns
    (n, K, 36), obj (iters + 1, n, 2, 8), poses (iters + 2, n, K, 26), sums (iters + 1, n, K, 2, 32))."""
    import reprojection_mirror as RP
    record = np.asarray(record, np.float64)
    n, K = record.shape[:2]
    iters = int(params[0])
    cap = int(max(g[0] + g[1] * g[2] for g in geom)) + 1
    pass_best, state, obj = np.full((n, K, 2, BEST), np.nan), np.full((n, K, 2, BEST), np.nan), np.zeros((n, 2, OBJ))
    work, poses, objs, all_sums, best = record[:, :, :26].copy(), [record[:, :, :26].copy()], [], [], None
    for p in range(iters + 1):
        S, _ = RF.evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params)
        out = RF.step(S, work, pass_best, p, p == iters, params)
        tables, _ = RP.scene_tables(render, scene, rigs, norm_factor, work, geom, cap)
        _, work, best = step_batch(kin, scene, tables, norm_factor, params, p, p == iters, work, S, out, state, obj)
        poses.append(work.copy())
        objs.append(obj.copy())
        all_sums.append(S)
    return best.reshape(n, K, 2 * BEST), np.stack(objs), np.stack(poses), np.stack(all_sums)
