"""numpy / Python-float statement of ancsh_coverage_field and ancsh_refine_pass_cov (include/ancsh_hip.h), on top of silhouette_mirror: the
predicted field is silhouette_mirror.field_of_mask of (predicted part image == j), the depth rows are refinement_mirror.pass_sums, the
overhang rows silhouette_mirror.sil_sums, and the GAP pixels -- observed for the part, not predicted for it -- add their rows here, one scalar
float64 operation at a time in the written order.  The solve, the clamp and the update are refinement_mirror.solve_update, so step on the
entry's own sums gives its pose_out byte for byte.  Validated on its own in tests/test_coverage_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import refinement_mirror as RF
import render_mirror as RM
import reprojection_mirror as RP
import silhouette_mirror as SM

SUMS, NACC, PARAMS = 40, 36, 32
SENTINEL = SM.SENTINEL
EPS, NAN = RF.EPS, RF.NAN


def _upper(key):
    """The float32 in a z-buffer key's upper half, as a Python float."""
    return float(np.array([int(key) >> 32], np.uint32).view(np.float32)[0])


# ---- the predicted field ----------------------------------------------------------------------------------------------------------------------
def cover_of(pred, sc, K):
    """One predicted crop (depth, labels, ...) under scene row sc -> (K, h, w, 2) int16: per part the offset to the nearest PREDICTED pixel."""
    img = RP.part_image(pred[0], pred[1], RP.link_parts(sc, K)[0])
    return np.stack([SM.field_of_mask(img == j) for j in range(K)])


def cover_flat(pred_frames, scene, geom_out, K, cap, fill=0):
    """The entry's buffer: (K, 2 * cap) int32, silhouette_mirror.field_flat's words at a crop's pixels, `fill` everywhere else.  pred_frames:
    the 2 n predicted crops (depth, labels, ...), row v * n + f, None for a row without a crop; scene (n, 240): frame row v * n + f reads
    scene row f; geom_out (2 n, 5): a crop's start lies in the predicted buffers of 2 * cap pixels."""
    n = len(scene)
    out = np.full((K, 2 * cap), fill, np.int32)
    for r, (fr, g) in enumerate(zip(pred_frames, geom_out)):
        if fr is None:
            continue
        s, h, w = int(g[0]), int(g[1]), int(g[2])
        out[:, s:s + h * w] = np.ascontiguousarray(cover_of(fr, scene[r % n], K).astype("<i2")).view("<i4").reshape(K, h * w)
    return out


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------------
def cov_sums(obs, pred, cov, origin, sc, nf, pose, j, K, params):
    """The gap pixels of one (frame, part, pose) in plain pixel order -> (S (36,), M (36,)): their rows' share of A and b in 0..26, and [33]
    sum m_c^2, [34] n_cov, [35] n_cfar.  cov = cover_of(pred, sc, K)[j]."""
    parts, _ = RP.link_parts(sc, K)
    o_img, p_img = RP.part_image(obs[0], obs[1], parts), RP.part_image(pred[0], pred[1], parts)
    pose = [float(v) for v in pose]
    weight, dist, slack = float(params[24]), float(params[25]), float(params[26])
    c = RF.centre(pose)
    S, M = [0.0] * NACC, [0.0] * NACC
    scale = float(sc[6])
    C = [float(v) for v in sc[7:13]]
    row0, col0 = origin
    for i, jj in zip(*np.nonzero((o_img == j) & (p_img != j))):
        zo = float(obs[0][i, jj]) * scale
        if p_img[i, jj] >= 0 and not _upper(pred[2][i, jj]) > zo:          # the prediction puts another part in front
            continue
        di, dj = int(cov[i, jj, 0]), int(cov[i, jj, 1])
        if di == SENTINEL:
            continue
        if float(di * di + dj * dj) <= slack * slack:
            continue
        z2 = _upper(pred[2][int(i) + di, int(jj) + dj])
        row, col = float(row0 + int(i)), float(col0 + int(jj))
        row2, col2 = float(row0 + int(i) + di), float(col0 + int(jj) + dj)
        su, sv = (C[0] * col + C[1] * row) + C[2], (C[3] * col + C[4] * row) + C[5]
        su2, sv2 = (C[0] * col2 + C[1] * row2) + C[2], (C[3] * col2 + C[4] * row2) + C[5]
        pn, pt = RF.cloud(z2 * su2, z2 * sv2, z2, nf), RF.cloud(z2 * su, z2 * sv, z2, nf)
        dv = [pn[0] - pt[0], pn[1] - pt[1], pn[2] - pt[2]]
        m = math.sqrt(RF.dot(dv, dv))
        if not m > 0.0:
            continue
        if m > dist:
            S[35] += 1.0
            continue
        g = [dv[0] / m, dv[1] / m, dv[2] / m]
        r = weight * m
        pc = [pn[b] - c[b] for b in range(3)]
        J = [weight * (pc[1] * g[2] - pc[2] * g[1]), weight * (pc[2] * g[0] - pc[0] * g[2]), weight * (pc[0] * g[1] - pc[1] * g[0]),
             weight * g[0], weight * g[1], weight * g[2]]
        terms = [J[x] * J[y] for x in range(6) for y in range(x, 6)] + [J[x] * r for x in range(6)]
        for k, v in enumerate(terms):
            S[k] += v
            M[k] += abs(v)
        S[33] += m * m
        M[33] += m * m
        S[34] += 1.0
    return np.array(S), np.array(M)


def cost(S, params):
    """The 40-value sums row -> C: ancsh_refine_pass_sil's numerator, the coverage's share added last."""
    max_dist, weight, dist, weight_c, dist_c = float(params[1]), float(params[8]), float(params[9]), float(params[24]), float(params[25])
    n_used, n_obs = float(S[28]), float(S[29])
    if n_obs == 0.0:
        return NAN
    num = (float(S[27]) + (max_dist * max_dist) * (n_obs - n_used)) + (weight * weight) * (float(S[32]) + (dist * dist) * float(S[34]))
    return (num + (weight_c * weight_c) * (float(S[36]) + (dist_c * dist_c) * float(S[38]))) / n_obs


def evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, fields=None):
    """One pass's sums at the working poses -> (sums (n, K, 2, 40): silhouette_mirror's 36 with the coverage rows in A and b | sum m_c^2 |
    n_cov | n_cfar | 0, NaN (solved, [35] and [39] 0) for a pose that is not usable; bounds (n, K, 2, 40): the summation-order bounds 4 (rows +
    1) eps magnitude, 0 for the counts and the values the entry computes from the sums)."""
    work = np.asarray(work, np.float64)
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
                if not RF.pose_ok(pose, nf):
                    continue
                if pred is None:
                    pred = RM.render_crop(mesh[0], mesh[1], mesh[2], int(g[1]), int(g[2]), int(g[3]), int(g[4]), rt, np_dtype)
                    cov = cover_of(pred, scene[f], K)
                origin = (int(g[3]), int(g[4]))
                Sd, Md = RF.pass_sums(mesh, frames[f][:2], pred, origin, scene[f], rt, nf, pose, j, K, params)
                Ss, Ms = SM.sil_sums(frames[f][:2], pred, fields[f][j], origin, scene[f], nf, pose, j, K, params)
                Sc, Mc = cov_sums(frames[f][:2], pred, cov[j], origin, scene[f], nf, pose, j, K, params)
                row, mag = np.zeros(SUMS), np.zeros(SUMS)
                row[:30], mag[:30] = Sd, Md
                row[:27] += Ss[:27]
                mag[:27] += Ms[:27]
                row[:27] += Sc[:27]
                mag[:27] += Mc[:27]
                row[32:35], mag[32] = Ss[30:33], Ms[30]
                row[36:39], mag[36] = Sc[33:36], Mc[33]
                row[30] = cost(row, params)
                sums[f, j, v] = row
                b = 4.0 * (((row[28] + row[33]) + row[37]) + 1.0) * EPS * mag
                b[28:32] = b[33:36] = b[37:] = 0.0
                bounds[f, j, v] = b
    return sums, bounds


def step(sums, work, best, pass_index, is_last, params):
    """Thread 0 of every workgroup on a pass's sums (n, K, 2, 40; solved is written here): the best rows updated in place -> the poses the
    pass writes (n, K, 26).  Fed the entry's own sums it reproduces the entry's best and pose_out byte for byte."""
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
                    ok, out = RF.solve_update(S, pose, params)
                    if ok:
                        new[f, j, 13 * v:13 * v + 13] = out
                S[31] = 1.0 if ok else 0.0
                best[f, j, v, 17] = solved + 1.0 if ok else solved
    return new


def refine(mesh, render, scene, rigs, norm_factor, record, geom, frames, dtype, params):
    """The whole loop with a 32-value table -> (columns (n, K, 36), sums (iters + 1, n, K, 2, 40), bounds, poses (iters + 2, n, K, 26))."""
    record = np.asarray(record, np.float64)
    n, K = record.shape[:2]
    iters = int(params[0])
    best = np.full((n, K, 2, RF.BEST), np.nan)
    work = record[:, :, :26].copy()
    fields = SM.field(frames, scene, K)
    sums, bounds, poses = [], [], [work.copy()]
    for p in range(iters + 1):
        S, Bd = evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, fields)
        work = step(S, work, best, p, p == iters, params)
        sums.append(S)
        bounds.append(Bd)
        poses.append(work.copy())
    return best.reshape(n, K, RF.WIDTH), np.stack(sums), np.stack(bounds), np.stack(poses)


# ---- the joint step on 40-wide sums -----------------------------------------------------------------------------------------------------------
def joint_sums(sums):
    """(..., 40) -> (..., 36) for joint_step_mirror, which counts n_j = sums[28] + sums[33] of a 36-wide row: [33] carries n_sil + n_cov, so
    n_j = (sums[28] + sums[33]) + sums[37] by the new rule (counts are integers: the grouping changes no byte).  Nothing else of 32.. is read."""
    out = np.array(sums[..., :36], np.float64)
    out[..., 33] = sums[..., 33] + sums[..., 37]
    return out
