"""numpy / Python-float statement of ancsh_refine_pass_scale (include/ancsh_hip.h), on top of coverage_mirror: columns 0..39 of a sums row are
that mirror's own functions' (refinement_mirror.pass_sums, silhouette_mirror.sil_sums, coverage_mirror.cov_sums and cost), and the scale
column's eight sums -- A_0s .. A_5s, A_ss, b_s -- are added here, one scalar float64 operation at a time: rows() walks the three kinds of
pixels again and yields every row's (J, Js, r); evaluate checks that walk against the three functions' A and b byte for byte on every call.
solve_update is the entry's thread 0 (7 x 7 Cholesky, both clamps, the similarity update) in the written order, so step on the entry's own
sums gives its pose_out byte for byte.  Validated on its own in tests/test_refine_scale_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import coverage_mirror as CM
import refinement_mirror as RF
import render_mirror as RM
import reprojection_mirror as RP
import silhouette_mirror as SM

SUMS, NACC, PARAMS = 48, 44, 48
SENTINEL = SM.SENTINEL
EPS, NAN = RF.EPS, RF.NAN
upper = CM._upper


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------------
def _pixel_row(weight, g, m, pc):
    """An overhang or a gap row from its unit direction g, length m and lever pc -> (J, Js, r)."""
    J = [weight * (pc[1] * g[2] - pc[2] * g[1]), weight * (pc[2] * g[0] - pc[0] * g[2]), weight * (pc[0] * g[1] - pc[1] * g[0]),
         weight * g[0], weight * g[1], weight * g[2]]
    return J, weight * RF.dot(g, pc), weight * m


def rows(kind, mesh, obs, pred, fld, cov, origin, sc, rt, nf, pose, j, K, params):
    """The rows of one kind ("depth", "overhang", "gap") of one (frame, part, pose) in plain pixel order, by the three entries' rules -> a
    generator of (J (6), Js, r): Js = the row's derivative by sigma, dot(n, pc), weight dot(g, pc) or weight_c dot(g, pc)."""
    parts, _ = RP.link_parts(sc, K)
    o_img, p_img = RP.part_image(obs[0], obs[1], parts), RP.part_image(pred[0], pred[1], parts)
    pose = [float(v) for v in pose]
    c = RF.centre(pose)
    scale = float(sc[6])
    C = [float(v) for v in sc[7:13]]
    row0, col0 = origin
    ray = lambda row, col: ((C[0] * col + C[1] * row) + C[2], (C[3] * col + C[4] * row) + C[5])
    if kind == "depth":
        verts, tris = np.asarray(mesh[0], np.float32).reshape(-1, 3), np.asarray(mesh[1], np.int64).reshape(-1, 3)
        tri_link = np.asarray(mesh[2], np.int64)
        max_dist, min_cos = float(params[1]), float(params[2])
        for i, jj in zip(*np.nonzero((o_img == j) & (p_img == j))):
            key = int(pred[2][i, jj])
            t = key & 0xFFFFFFFF
            if t >= len(tris):
                continue
            idx, l = tris[t], int(tri_link[t])
            if not 0 <= l < 16 or (idx < 0).any() or (idx >= len(verts)).any():
                continue
            su, sv = ray(float(row0 + int(i)), float(col0 + int(jj)))
            zo, zp = float(obs[0][i, jj]) * scale, upper(key)
            q, p = RF.cloud(zo * su, zo * sv, zo, nf), RF.cloud(zp * su, zp * sv, zp, nf)
            R = [float(v) for v in rt[16 + 12 * l:28 + 12 * l]]
            vt = []
            for k in range(3):
                v0, v1, v2 = (float(v) for v in verts[idx[k]])
                m = [((R[4 * b] * v0 + R[4 * b + 1] * v1) + R[4 * b + 2] * v2) + R[4 * b + 3] for b in range(3)]
                vt.append(RF.cloud(m[0], m[1], m[2], nf))
            e1, e2 = [vt[1][b] - vt[0][b] for b in range(3)], [vt[2][b] - vt[0][b] for b in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            nn2 = RF.dot(n, n)
            if not math.isfinite(nn2) or not math.sqrt(nn2) > 0.0:
                continue
            ln = math.sqrt(nn2)
            n = [v / ln for v in n]
            nq = RF.dot(n, q)
            if nq > 0.0:
                n, nq = [-v for v in n], -nq
            d = [p[b] - q[b] for b in range(3)]
            if not math.sqrt(RF.dot(d, d)) <= max_dist or not abs(nq) / math.sqrt(RF.dot(q, q)) >= min_cos:
                continue
            pc = [p[b] - c[b] for b in range(3)]
            yield [pc[1] * n[2] - pc[2] * n[1], pc[2] * n[0] - pc[0] * n[2], pc[0] * n[1] - pc[1] * n[0], n[0], n[1], n[2]], RF.dot(n, pc), RF.dot(n, d)
    elif kind == "overhang":
        weight, dist, slack = float(params[8]), float(params[9]), float(params[10])
        for i, jj in zip(*np.nonzero((p_img == j) & (o_img != j))):
            zp = upper(pred[2][i, jj])
            if o_img[i, jj] >= 0 and not float(obs[0][i, jj]) * scale > zp:
                continue
            di, dj = int(fld[i, jj, 0]), int(fld[i, jj, 1])
            if di == SENTINEL or float(di * di + dj * dj) <= slack * slack:
                continue
            su, sv = ray(float(row0 + int(i)), float(col0 + int(jj)))
            su2, sv2 = ray(float(row0 + int(i) + di), float(col0 + int(jj) + dj))
            p, p2 = RF.cloud(zp * su, zp * sv, zp, nf), RF.cloud(zp * su2, zp * sv2, zp, nf)
            dv = [p[0] - p2[0], p[1] - p2[1], p[2] - p2[2]]
            m = math.sqrt(RF.dot(dv, dv))
            if not m > 0.0 or m > dist:
                continue
            yield _pixel_row(weight, [dv[0] / m, dv[1] / m, dv[2] / m], m, [p[b] - c[b] for b in range(3)])
    else:
        weight, dist, slack = float(params[24]), float(params[25]), float(params[26])
        for i, jj in zip(*np.nonzero((o_img == j) & (p_img != j))):
            if p_img[i, jj] >= 0 and not upper(pred[2][i, jj]) > float(obs[0][i, jj]) * scale:
                continue
            di, dj = int(cov[i, jj, 0]), int(cov[i, jj, 1])
            if di == SENTINEL or float(di * di + dj * dj) <= slack * slack:
                continue
            z2 = upper(pred[2][int(i) + di, int(jj) + dj])
            su, sv = ray(float(row0 + int(i)), float(col0 + int(jj)))
            su2, sv2 = ray(float(row0 + int(i) + di), float(col0 + int(jj) + dj))
            pn, pt = RF.cloud(z2 * su2, z2 * sv2, z2, nf), RF.cloud(z2 * su, z2 * sv, z2, nf)
            dv = [pn[0] - pt[0], pn[1] - pt[1], pn[2] - pt[2]]
            m = math.sqrt(RF.dot(dv, dv))
            if not m > 0.0 or m > dist:
                continue
            yield _pixel_row(weight, [dv[0] / m, dv[1] / m, dv[2] / m], m, [pn[b] - c[b] for b in range(3)])


def row_sums(rows_):
    """(J, Js, r) rows in order -> (S (35,), M (35,)): [A (21) | b (6) | A_0s .. A_5s | A_ss | b_s] and the sums of the terms' magnitudes."""
    S, M = [0.0] * 35, [0.0] * 35
    for J, Js, r in rows_:
        terms = [J[x] * J[y] for x in range(6) for y in range(x, 6)] + [J[x] * r for x in range(6)] + [J[x] * Js for x in range(6)] + [Js * Js, Js * r]
        for k, v in enumerate(terms):
            S[k] += v
            M[k] += abs(v)
    return np.array(S), np.array(M)


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------------
def usable(pose, nf, s0):
    return RF.pose_ok(pose, nf) and math.isfinite(float(s0)) and float(s0) > 0.0


def evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, fitted, fields=None):
    """One pass's sums at the working poses -> (sums (n, K, 2, 48): coverage_mirror's 40 | A_0s .. A_5s | A_ss | b_s, NaN (solved, [35] and
    [39] 0) for a pose that is not usable or whose fitted s is not finite and > 0; bounds (n, K, 2, 48): 4 (rows + 1) eps magnitude, 0 for
    the counts and the values the entry computes from the sums).  The three kinds are summed apart and added (depth + overhang) + gap, as
    coverage_mirror adds A and b."""
    work, fitted = np.asarray(work, np.float64), np.asarray(fitted, np.float64)
    n, K = work.shape[:2]
    sums, bounds = np.full((n, K, 2, SUMS), np.nan), np.zeros((n, K, 2, SUMS))
    sums[..., 31] = sums[..., 35] = sums[..., 39] = 0.0
    cap = int(max(g[0] + g[1] * g[2] for g in geom)) + 1
    np_dtype = np.dtype(np.asarray(frames[0][0]).dtype)
    tables, _ = RP.scene_tables(render, scene, rigs, norm_factor, work, geom, cap)
    fields = SM.field(frames, scene, K) if fields is None else fields
    for f, g in enumerate(geom):
        nf = float(np.float32(norm_factor[f]))
        for v in range(2):
            rt = tables[v * n + f]
            pred = cov = None
            for j in range(K):
                pose = work[f, j, 13 * v:13 * v + 13]
                if not usable(pose, nf, fitted[f, j, 13 * v + 9]):
                    continue
                if pred is None:
                    pred = RM.render_crop(mesh[0], mesh[1], mesh[2], int(g[1]), int(g[2]), int(g[3]), int(g[4]), rt, np_dtype)
                    cov = CM.cover_of(pred, scene[f], K)
                origin, obs = (int(g[3]), int(g[4])), frames[f][:2]
                Sd, Md = RF.pass_sums(mesh, obs, pred, origin, scene[f], rt, nf, pose, j, K, params)
                Ss, Ms = SM.sil_sums(obs, pred, fields[f][j], origin, scene[f], nf, pose, j, K, params)
                Sc, Mc = CM.cov_sums(obs, pred, cov[j], origin, scene[f], nf, pose, j, K, params)
                mine = [row_sums(rows(kind, mesh, obs, pred, fields[f][j], cov[j], origin, scene[f], rt, nf, pose, j, K, params))
                        for kind in ("depth", "overhang", "gap")]
                for (S, _), theirs in zip(mine, (Sd, Ss, Sc)):              # the walk above found the three functions' rows, term for term
                    assert S[:27].tobytes() == np.asarray(theirs[:27]).tobytes()
                row, mag = np.zeros(SUMS), np.zeros(SUMS)
                row[:30], mag[:30] = Sd, Md
                row[:27] += Ss[:27]
                mag[:27] += Ms[:27]
                row[:27] += Sc[:27]
                mag[:27] += Mc[:27]
                row[32:35], mag[32] = Ss[30:33], Ms[30]
                row[36:39], mag[36] = Sc[33:36], Mc[33]
                row[40:], mag[40:] = (mine[0][0][27:] + mine[1][0][27:]) + mine[2][0][27:], (mine[0][1][27:] + mine[1][1][27:]) + mine[2][1][27:]
                row[30] = CM.cost(row, params)
                sums[f, j, v] = row
                b = 4.0 * (((row[28] + row[33]) + row[37]) + 1.0) * EPS * mag
                b[28:32] = b[33:36] = b[37:40] = 0.0
                bounds[f, j, v] = b
    return sums, bounds


# ---- thread 0 ---------------------------------------------------------------------------------------------------------------------------------
def solve7(S, params):
    """The 7 x 7 damped Cholesky solve on a 48-value sums row, in the entry's order -> (ok, xi (7) before any clamp)."""
    S = [float(v) for v in S]
    damping = float(params[3])
    A = [[0.0] * 7 for _ in range(7)]
    at = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = S[at]
            at += 1
    for a in range(6):
        A[a][6] = A[6][a] = S[40 + a]
    A[6][6] = S[46]
    rhs = S[21:27] + [S[47]]
    for k in range(7):
        A[k][k] = A[k][k] + (damping * A[k][k] + 1e-12)
    L = [[0.0] * 7 for _ in range(7)]
    ok = True
    for i in range(7):
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
        return False, [NAN] * 7
    y, xi = [0.0] * 7, [0.0] * 7
    for i in range(7):
        s = 0.0 - rhs[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(6, -1, -1):
        s = y[i]
        for k in range(i + 1, 7):
            s = s - L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    return all(math.isfinite(v) for v in xi), xi


def clamp(xi, s, s0, params):
    """Both clamps on the solved step: one factor for all seven values, then sigma alone held to s0's band -> xi (7)."""
    max_dist, max_angle, max_step, max_total = float(params[1]), float(params[4]), float(params[32]), float(params[33])
    xi = list(xi)
    wn, dn, sn = math.sqrt(RF.dot(xi, xi)), math.sqrt(RF.dot(xi[3:6], xi[3:6])), abs(xi[6])
    if wn > max_angle or dn > max_dist or sn > max_step:
        f = 1.0
        if wn > max_angle:
            f = max_angle / wn
        if dn > max_dist and max_dist / dn < f:
            f = max_dist / dn
        if sn > max_step and max_step / sn < f:
            f = max_step / sn
        xi = [v * f for v in xi]
    lo, hi, grown = s0 / (1.0 + max_total), s0 * (1.0 + max_total), s * (1.0 + xi[6])
    if grown > hi:
        xi[6] = hi / s - 1.0
    elif grown < lo:
        xi[6] = lo / s - 1.0
    return xi


def update(xi, pose):
    """The similarity update about the pose's centre: R' = dR R, s' = s (1 + sigma), t' = ((1 + sigma) dR (t - c) + c) + d -> (13,)."""
    pose = [float(v) for v in pose]
    c = RF.centre(pose)
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
    grow = 1.0 + xi[6]
    out[9] = pose[9] * grow
    u = [pose[10] - c[0], pose[11] - c[1], pose[12] - c[2]]
    for a in range(3):
        out[10 + a] = (grow * RF.dot(dR[3 * a:3 * a + 3], u) + c[a]) + xi[3 + a]
    return np.array(out)


def solve_update(S, pose, s0, params):
    """The entry's thread 0 on the 48-value sums row -> (solved, pose_out (13,)), byte for byte."""
    pose = [float(v) for v in pose]
    ok, xi = solve7(S, params)
    if not ok:
        return False, np.array(pose)
    if not pose[9] > 0.0:                                                # a working s that is not > 0 fails the solve (the entry divides by it first)
        return False, np.array(pose)
    xi = clamp(xi, pose[9], float(s0), params)
    kept = pose[9] * (1.0 + xi[6])
    if not (math.isfinite(kept) and kept > 0.0):
        return False, np.array(pose)
    return True, update(xi, pose)


def step(sums, work, best, fitted, pass_index, is_last, params):
    """coverage_mirror.step with the 7 x 7 solve: the best rows updated in place -> the poses the pass writes (n, K, 26)."""
    work = np.asarray(work, np.float64)
    n, K = work.shape[:2]
    new = work[:, :, :26].copy()
    for f in range(n):
        for j in range(K):
            for v in range(2):
                S, pose = sums[f, j, v], work[f, j, 13 * v:13 * v + 13]
                if np.isnan(S[29]):
                    best[f, j, v] = np.nan
                    continue
                solved = 0.0 if pass_index == 0 else best[f, j, v, 17]
                RF.best_update(best[f, j, v], pass_index, pose, S[30], S[28])
                ok = False
                if not is_last and (S[28] + S[33]) + S[37] >= params[5]:
                    ok, out = solve_update(S, pose, fitted[f, j, 13 * v + 9], params)
                    if ok:
                        new[f, j, 13 * v:13 * v + 13] = out
                S[31] = 1.0 if ok else 0.0
                best[f, j, v, 17] = solved + 1.0 if ok else solved
    return new


def refine(mesh, render, scene, rigs, norm_factor, record, geom, frames, dtype, params):
    """The whole loop with a 48-value table -> (columns (n, K, 36), sums (iters + 1, n, K, 2, 48), bounds, poses (iters + 2, n, K, 26))."""
    record = np.asarray(record, np.float64)
    n, K = record.shape[:2]
    iters = int(params[0])
    best = np.full((n, K, 2, RF.BEST), np.nan)
    work = record[:, :, :26].copy()
    fields = SM.field(frames, scene, K)
    sums, bounds, poses = [], [], [work.copy()]
    for p in range(iters + 1):
        S, Bd = evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, record, fields)
        work = step(S, work, best, record, p, p == iters, params)
        sums.append(S)
        bounds.append(Bd)
        poses.append(work.copy())
    return best.reshape(n, K, RF.WIDTH), np.stack(sums), np.stack(bounds), np.stack(poses)


# ---- the scale perturbation and its measure (shared by the CPU and the GPU test) -------------------------------------------------------------
def scaled_record(rec, factor):
    """Every part of the record scaled about its centre, the centre kept: s' = f s, t' = c + f (t - c), f alternating factor, 1 / factor
    over (frame, part, pose) -> (record, f (n, K, 2))."""
    out, fs = rec.copy(), np.ones(rec.shape[:2] + (2,))
    for f in range(rec.shape[0]):
        for j in range(rec.shape[1]):
            for v in range(2):
                pose = rec[f, j, 13 * v:13 * v + 13]
                if not np.isfinite(pose).all():
                    continue
                fac = factor if (f + j + v) % 2 == 0 else 1.0 / factor
                c = np.array(RF.centre([float(x) for x in pose]))
                out[f, j, 13 * v + 9] = fac * pose[9]
                out[f, j, 13 * v + 10:13 * v + 13] = c + fac * (pose[10:13] - c)
                fs[f, j, v] = fac
    return out, fs


def rho(exact, start, kept):
    """|log(s_kept / s_true)| / |log(s_start / s_true)| per (frame, part, pose): exactly 1 = the scale as it came, 0 = the true scale."""
    s_true, s_start, s_kept = exact[..., [9, 22]], start[..., [9, 22]], kept[..., [9, 22]]
    return np.abs(np.log(s_kept / s_true)) / np.abs(np.log(s_start / s_true))
