"""numpy / Python-float statement of ancsh_refine_pass and ancsh_refine_rec (include/ancsh_hip.h): render-and-compare ICP one scalar float64
operation at a time, in the written order (a Python float is an IEEE double, math.sqrt is correctly rounded).  The pixel sums are accumulated
in plain pixel order -- the entry adds in its fixed thread / wave order, so its sums agree to the summation-order bound pass_sums also
returns, not to the last bit --; the solve, the clamp, the quaternion and the update follow the kernel's order exactly, so solve_update on the
entry's own sums gives its pose_out byte for byte.  The frames come from render_mirror, the tables from reprojection_mirror.  Validated on its
own in tests/test_refinement_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import render_mirror as RM
import reprojection_mirror as RP

WIDTH, BEST, SUMS, NACC = 36, 18, 32, 30
EPS = 2.0 ** -52
NAN = float("nan")


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cloud(x, y, z, nf):
    return [nf * x, nf * (-y), nf * z]


def centre(pose):
    return [pose[9] * ((pose[3 * a] * 0.5 + pose[3 * a + 1] * 0.5) + pose[3 * a + 2] * 0.5) + pose[10 + a] for a in range(3)]


def pose_ok(pose, nf):
    return bool(np.isfinite(np.asarray(pose, np.float64)).all()) and math.isfinite(nf) and nf != 0.0


def pass_sums(mesh, obs, pred, origin, sc, rt, nf, pose, j, K, params):
    """One (frame, part, pose): obs = (depth, labels) crop, pred = (depth, labels, keys) crop of the pose's predicted frame, rt its render table
    (208) -> (S (30,): A (21) | b (6) | sum r^2 | n_used | n_obs in plain pixel order, M (30,): the sums of the terms' magnitudes)."""
    verts, tris, tri_link = np.asarray(mesh[0], np.float32).reshape(-1, 3), np.asarray(mesh[1], np.int64).reshape(-1, 3), np.asarray(mesh[2], np.int64)
    parts, _ = RP.link_parts(sc, K)
    o_img, p_img = RP.part_image(obs[0], obs[1], parts) == j, RP.part_image(pred[0], pred[1], parts) == j
    pose = [float(v) for v in pose]
    max_dist, min_cos = float(params[1]), float(params[2])
    c = centre(pose)
    S, M = [0.0] * NACC, [0.0] * NACC
    S[29] = M[29] = float(o_img.sum())
    scale = float(sc[6])
    C = [float(v) for v in sc[7:13]]
    row0, col0 = origin
    for i, jj in zip(*np.nonzero(o_img & p_img)):
        key = int(pred[2][i, jj])
        t = key & 0xFFFFFFFF
        if t >= len(tris):
            continue
        idx, l = tris[t], int(tri_link[t])
        if not 0 <= l < 16 or (idx < 0).any() or (idx >= len(verts)).any():
            continue
        row, col = float(row0 + int(i)), float(col0 + int(jj))
        su, sv = (C[0] * col + C[1] * row) + C[2], (C[3] * col + C[4] * row) + C[5]
        zo = float(obs[0][i, jj]) * scale
        zp = float(np.array([key >> 32], np.uint32).view(np.float32)[0])
        q, p = cloud(zo * su, zo * sv, zo, nf), cloud(zp * su, zp * sv, zp, nf)
        R = [float(v) for v in rt[16 + 12 * l:28 + 12 * l]]
        vt = []
        for k in range(3):
            v0, v1, v2 = (float(v) for v in verts[idx[k]])
            m = [((R[4 * b] * v0 + R[4 * b + 1] * v1) + R[4 * b + 2] * v2) + R[4 * b + 3] for b in range(3)]
            vt.append(cloud(m[0], m[1], m[2], nf))
        e1, e2 = [vt[1][b] - vt[0][b] for b in range(3)], [vt[2][b] - vt[0][b] for b in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        if not all(math.isfinite(v) for v in n):
            continue
        nn2 = dot(n, n)
        if not math.isfinite(nn2):
            continue
        ln = math.sqrt(nn2)
        if not ln > 0.0:
            continue
        n = [v / ln for v in n]
        nq = dot(n, q)
        if nq > 0.0:
            n, nq = [-v for v in n], -nq
        d = [p[b] - q[b] for b in range(3)]
        if not math.sqrt(dot(d, d)) <= max_dist:
            continue
        if not abs(nq) / math.sqrt(dot(q, q)) >= min_cos:
            continue
        r = dot(n, d)
        pc = [p[b] - c[b] for b in range(3)]
        J = [pc[1] * n[2] - pc[2] * n[1], pc[2] * n[0] - pc[0] * n[2], pc[0] * n[1] - pc[1] * n[0], n[0], n[1], n[2]]
        terms = [J[x] * J[y] for x in range(6) for y in range(x, 6)] + [J[x] * r for x in range(6)] + [r * r, 1.0]
        for k, v in enumerate(terms):
            S[k] += v
            M[k] += abs(v)
    return np.array(S), np.array(M)


def sum_bound(S, M):
    """The summation-order bound of every float sum: 4 n eps sum |term|, n the pixels used (the counts are exact: bound 0)."""
    b = 4.0 * S[28] * EPS * M
    b[28:] = 0.0
    return b


def cost(S, params):
    max_dist = float(params[1])
    n_used, n_obs = float(S[28]), float(S[29])
    return (float(S[27]) + (max_dist * max_dist) * (n_obs - n_used)) / n_obs if n_obs != 0.0 else NAN


def solve_update(S, pose, params):
    """The entry's thread 0 on the sums S (>= 27 values: A | b) and the 13-value pose -> (solved, pose_out (13,)), byte for byte."""
    S, pose = [float(v) for v in S], [float(v) for v in pose]
    damping, max_angle, max_dist = float(params[3]), float(params[4]), float(params[1])
    c = centre(pose)
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = S[at]
            at += 1
    for k in range(6):
        A[k][k] = A[k][k] + (damping * A[k][k] + 1e-12)
    L = [[0.0] * 6 for _ in range(6)]
    ok = True
    for i in range(6):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                ok = ok and s > 0.0 and math.isfinite(s)
                L[i][i] = math.sqrt(s) if s >= 0.0 else NAN
            else:
                L[i][j] = s / L[j][j] if L[j][j] != 0.0 else NAN
    if not ok:
        return False, np.array(pose)
    y, xi = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = 0.0 - S[21 + i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    if not all(math.isfinite(v) for v in xi):
        return False, np.array(pose)
    wn, dn = math.sqrt(dot(xi, xi)), math.sqrt(dot(xi[3:], xi[3:]))
    if wn > max_angle or dn > max_dist:
        f = 1.0
        if wn > max_angle:
            f = max_angle / wn
        if dn > max_dist and max_dist / dn < f:
            f = max_dist / dn
        xi = [v * f for v in xi]
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
    return True, np.array(out)


def best_update(best, pass_index, pose, C, n_used):
    """The running best row (18,) after a pass's evaluation; passes_solved is the caller's (after the solve)."""
    if pass_index == 0 or C < best[14]:
        best[:13] = pose
        if pass_index == 0:
            best[13] = C
        best[14], best[15], best[16] = C, n_used, float(pass_index)


def evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params):
    """One pass's sums at the working poses `work` (n, K, >= 26) -> (sums (n, K, 2, 32): the 30 sums and C, NaN for a pose that is not usable,
    solved left 0; bounds (n, K, 2, 30): the summation-order bounds)."""
    work = np.asarray(work, np.float64)
    n, K = work.shape[:2]
    sums, bounds = np.full((n, K, 2, SUMS), np.nan), np.zeros((n, K, 2, NACC))
    sums[..., 31] = 0.0
    cap = int(max(g[0] + g[1] * g[2] for g in geom)) + 1
    np_dtype = np.dtype(np.asarray(frames[0][0]).dtype)
    tables, _ = RP.scene_tables(render, scene, rigs, norm_factor, work, geom, cap)
    for f, g in enumerate(geom):
        nf = float(np.float32(norm_factor[f]))
        for v in range(2):
            rt = tables[v * n + f]
            pred = None
            for j in range(K):
                pose = work[f, j, 13 * v:13 * v + 13]
                if not pose_ok(pose, nf):
                    continue
                if pred is None:
                    pred = RM.render_crop(mesh[0], mesh[1], mesh[2], int(g[1]), int(g[2]), int(g[3]), int(g[4]), rt, np_dtype)
                S, M = pass_sums(mesh, frames[f][:2], pred, (int(g[3]), int(g[4])), scene[f], rt, nf, pose, j, K, params)
                sums[f, j, v, :NACC], sums[f, j, v, 30] = S, cost(S, params)
                bounds[f, j, v] = sum_bound(S, M)
    return sums, bounds


def step(sums, work, best, pass_index, is_last, params):
    """Thread 0 of every workgroup on a pass's sums (n, K, 2, 32; solved is written here): the best rows (n, K, 2, 18) updated in place ->
    the poses the pass writes (n, K, 26).  Fed the entry's own sums it reproduces the entry's best and pose_out byte for byte."""
    work = np.asarray(work, np.float64)
    n, K = work.shape[:2]
    new = work[:, :, :26].copy()
    for f in range(n):
        for j in range(K):
            for v in range(2):
                S, pose = sums[f, j, v], work[f, j, 13 * v:13 * v + 13]
                if np.isnan(S[29]):                                       # the pose was not usable: NaN in the best row, the pose as it came
                    best[f, j, v] = np.nan
                    continue
                solved = 0.0 if pass_index == 0 else best[f, j, v, 17]
                best_update(best[f, j, v], pass_index, pose, S[30], S[28])
                ok = False
                if not is_last and S[28] >= params[5]:
                    ok, out = solve_update(S, pose, params)
                    if ok:
                        new[f, j, 13 * v:13 * v + 13] = out
                S[31] = 1.0 if ok else 0.0
                best[f, j, v, 17] = solved + 1.0 if ok else solved
    return new


def refine(mesh, render, scene, rigs, norm_factor, record, geom, frames, dtype, params):
    """The whole loop on frames_problem's arguments (frames: per frame (depth, labels, origin) observed crops) -> (columns (n, K, 36), sums
    (iters + 1, n, K, 2, 32), bounds (iters + 1, n, K, 2, 30): each pass's summation-order bounds, poses (iters + 2, n, K, 26): the working
    poses each pass read and, last, what the last pass wrote)."""
    record = np.asarray(record, np.float64)
    n, K = record.shape[:2]
    iters = int(params[0])
    best = np.full((n, K, 2, BEST), np.nan)
    work = record[:, :, :26].copy()
    sums, bounds, poses = [], [], [work.copy()]
    for p in range(iters + 1):
        S, Bd = evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params)
        work = step(S, work, best, p, p == iters, params)
        sums.append(S)
        bounds.append(Bd)
        poses.append(work.copy())
    return best.reshape(n, K, WIDTH), np.stack(sums), np.stack(bounds), np.stack(poses)
