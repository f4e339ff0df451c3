"""numpy / Python-float statement of ancsh_silhouette_field and ancsh_refine_pass_sil (include/ancsh_hip.h): the nearest observed pixel of every
crop pixel and part as a brute-force search under the tie rule (squared pixel distance in integers, then the lower row, then the lower column),
and render-and-compare ICP with the silhouette term, by importing and extending refinement_mirror: the depth rows are refinement_mirror's own
pass_sums, the overhang pixels add their rows here, one scalar float64 operation at a time in the written order; the solve, the clamp and the
update are refinement_mirror.solve_update, so step on the entry's own sums gives its pose_out byte for byte.  Validated on its own in
tests/test_silhouette_cpu.py.  Test infrastructure only."""
import math

import numpy as np

import refinement_mirror as RF
import render_mirror as RM
import reprojection_mirror as RP

SUMS, NACC, PARAMS = 36, 33, 16
SENTINEL = -32768
EPS, NAN = RF.EPS, RF.NAN


# ---- the field --------------------------------------------------------------------------------------------------------------------------------
def field_of_mask(mask):
    """(h, w) bool: the observed pixels of one part -> (h, w, 2) int16 [di, dj], the offset to the nearest observed pixel; SENTINEL in both
    when there is none (or the crop is taller or wider than 32767 pixels).  Brute force: every pixel against every observed pixel."""
    h, w = mask.shape
    out = np.full((h, w, 2), SENTINEL, np.int16)
    rows, cols = np.nonzero(mask)                                        # row-major: ascending (row, col)
    if len(rows) == 0 or h > 32767 or w > 32767:
        return out
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    for i in range(h):
        d2 = (rows[None, :] - i) ** 2 + (cols[None, :] - np.arange(w, dtype=np.int64)[:, None]) ** 2       # (w, n)
        at = np.argmin(d2, axis=1)                                       # the first minimum: the lowest (row, col) among equals
        out[i, :, 0], out[i, :, 1] = rows[at] - i, cols[at] - np.arange(w)
    return out


def field(frames, scene, K):
    """Per frame (depth, labels, origin) -> a list of (K, h, w, 2) int16 fields, OBSERVED by ancsh_reproject_compare_rec's rule."""
    out = []
    for (d, l, _), sc in zip(frames, scene):
        img = RP.part_image(d, l, RP.link_parts(sc, K)[0])
        out.append(np.stack([field_of_mask(img == j) for j in range(K)]))
    return out


def field_flat(frames, scene, geom, K, cap, fill=0):
    """The entry's buffer: (K, cap) int32, word = (di & 0xffff) | (dj & 0xffff) << 16 at a crop's pixels, `fill` everywhere else."""
    out = np.full((K, cap), fill, np.int32)
    for fld, g in zip(field(frames, scene, K), geom):
        s, h, w = int(g[0]), int(g[1]), int(g[2])
        words = np.ascontiguousarray(fld.astype("<i2")).view("<i4").reshape(K, h * w)
        out[:, s:s + h * w] = words
    return out


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------------
def sil_sums(obs, pred, fld, origin, sc, nf, pose, j, K, params):
    """The overhang pixels of one (frame, part, pose) in plain pixel order -> (S (33,), M (33,)): their rows' share of A and b in 0..26, and
    [30] sum m^2, [31] n_sil, [32] n_far (27..29 stay 0: the depth rows' own)."""
    parts, _ = RP.link_parts(sc, K)
    o_img, p_img = RP.part_image(obs[0], obs[1], parts), RP.part_image(pred[0], pred[1], parts)
    pose = [float(v) for v in pose]
    weight, dist, slack = float(params[8]), float(params[9]), float(params[10])
    c = RF.centre(pose)
    S, M = [0.0] * NACC, [0.0] * NACC
    scale = float(sc[6])
    C = [float(v) for v in sc[7:13]]
    row0, col0 = origin
    for i, jj in zip(*np.nonzero((p_img == j) & (o_img != j))):
        key = int(pred[2][i, jj])
        zp = float(np.array([key >> 32], np.uint32).view(np.float32)[0])
        if o_img[i, jj] >= 0 and not float(obs[0][i, jj]) * scale > zp:   # another part in front of the prediction: an occlusion
            continue
        di, dj = int(fld[i, jj, 0]), int(fld[i, jj, 1])
        if di == SENTINEL:
            continue
        if float(di * di + dj * dj) <= slack * slack:
            continue
        row, col = float(row0 + int(i)), float(col0 + int(jj))
        row2, col2 = float(row0 + int(i) + di), float(col0 + int(jj) + dj)
        su, sv = (C[0] * col + C[1] * row) + C[2], (C[3] * col + C[4] * row) + C[5]
        su2, sv2 = (C[0] * col2 + C[1] * row2) + C[2], (C[3] * col2 + C[4] * row2) + C[5]
        p, p2 = RF.cloud(zp * su, zp * sv, zp, nf), RF.cloud(zp * su2, zp * sv2, zp, nf)
        dv = [p[0] - p2[0], p[1] - p2[1], p[2] - p2[2]]
        m = math.sqrt(RF.dot(dv, dv))
        if not m > 0.0:
            continue
        if m > dist:
            S[32] += 1.0
            continue
        g = [dv[0] / m, dv[1] / m, dv[2] / m]
        r = weight * m
        pc = [p[b] - c[b] for b in range(3)]
        J = [weight * (pc[1] * g[2] - pc[2] * g[1]), weight * (pc[2] * g[0] - pc[0] * g[2]), weight * (pc[0] * g[1] - pc[1] * g[0]),
             weight * g[0], weight * g[1], weight * g[2]]
        terms = [J[x] * J[y] for x in range(6) for y in range(x, 6)] + [J[x] * r for x in range(6)]
        for k, v in enumerate(terms):
            S[k] += v
            M[k] += abs(v)
        S[30] += m * m
        M[30] += m * m
        S[31] += 1.0
    return np.array(S), np.array(M)


def cost(S, params):
    """The 36-value sums row -> C."""
    max_dist, weight, dist = float(params[1]), float(params[8]), float(params[9])
    n_used, n_obs = float(S[28]), float(S[29])
    if n_obs == 0.0:
        return NAN
    return ((float(S[27]) + (max_dist * max_dist) * (n_obs - n_used)) + (weight * weight) * (float(S[32]) + (dist * dist) * float(S[34]))) / n_obs


def evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, fields=None):
    """One pass's sums at the working poses -> (sums (n, K, 2, 36): A | b with the silhouette rows | sum r^2 | n_used | n_obs | C | solved = 0
    | sum m^2 | n_sil | n_far | 0, NaN (solved and [35] 0) for a pose that is not usable; bounds (n, K, 2, 36): the summation-order bounds, 0
    for the counts and the values the entry computes from the sums)."""
    work = np.asarray(work, np.float64)
    n, K = work.shape[:2]
    sums, bounds = np.full((n, K, 2, SUMS), np.nan), np.zeros((n, K, 2, SUMS))
    sums[..., 31] = sums[..., 35] = 0.0
    cap = int(max(g[0] + g[1] * g[2] for g in geom)) + 1
    np_dtype = np.dtype(np.asarray(frames[0][0]).dtype)
    tables, _ = RP.scene_tables(render, scene, rigs, norm_factor, work, geom, cap)
    fields = field(frames, scene, K) if fields is None else fields
    for f, g in enumerate(geom):
        nf = float(np.float32(norm_factor[f]))
        for v in range(2):
            rt = tables[v * n + f]
            pred = None
            for j in range(K):
                pose = work[f, j, 13 * v:13 * v + 13]
                if not RF.pose_ok(pose, nf):
                    continue
                if pred is None:
                    pred = RM.render_crop(mesh[0], mesh[1], mesh[2], int(g[1]), int(g[2]), int(g[3]), int(g[4]), rt, np_dtype)
                origin = (int(g[3]), int(g[4]))
                Sd, Md = RF.pass_sums(mesh, frames[f][:2], pred, origin, scene[f], rt, nf, pose, j, K, params)
                Ss, Ms = sil_sums(frames[f][:2], pred, fields[f][j], origin, scene[f], nf, pose, j, K, params)
                row, mag = np.zeros(SUMS), np.zeros(SUMS)
                row[:30], mag[:30] = Sd, Md
                row[:27] += Ss[:27]
                mag[:27] += Ms[:27]
                row[32:35], mag[32] = Ss[30:33], Ms[30]
                row[30] = cost(row, params)
                sums[f, j, v] = row
                b = 4.0 * (row[28] + row[33] + 1.0) * EPS * mag
                b[28:32] = b[33:] = 0.0
                bounds[f, j, v] = b
    return sums, bounds


def step(sums, work, best, pass_index, is_last, params):
    """Thread 0 of every workgroup on a pass's sums (n, K, 2, 36; solved is written here): the best rows updated in place -> the poses the
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
                if not is_last and S[28] + S[33] >= params[5]:
                    ok, out = RF.solve_update(S, pose, params)
                    if ok:
                        new[f, j, 13 * v:13 * v + 13] = out
                S[31] = 1.0 if ok else 0.0
                best[f, j, v, 17] = solved + 1.0 if ok else solved
    return new


def refine(mesh, render, scene, rigs, norm_factor, record, geom, frames, dtype, params):
    """The whole loop with a 16-value table -> (columns (n, K, 36), sums (iters + 1, n, K, 2, 36), bounds, poses (iters + 2, n, K, 26))."""
    record = np.asarray(record, np.float64)
    n, K = record.shape[:2]
    iters = int(params[0])
    best = np.full((n, K, 2, RF.BEST), np.nan)
    work = record[:, :, :26].copy()
    fields = field(frames, scene, K)
    sums, bounds, poses = [], [], [work.copy()]
    for p in range(iters + 1):
        S, Bd = evaluate(mesh, render, scene, rigs, norm_factor, work, geom, frames, params, fields)
        work = step(S, work, best, p, p == iters, params)
        sums.append(S)
        bounds.append(Bd)
        poses.append(work.copy())
    return best.reshape(n, K, RF.WIDTH), np.stack(sums), np.stack(bounds), np.stack(poses)


# ---- the lateral perturbation and its measure (shared by the CPU and the GPU test) -----------------------------------------------------------
def lateral_record(rec, cen, shift, phase=0.3):
    """Every pose of the record moved by `shift` perpendicular to its part's centroid ray, no tilt: along cos(th) e + sin(th) (ray x e) with
    test_refinement_cpu.perturbed_record's e and th."""
    out = rec.copy()
    for f in range(rec.shape[0]):
        for j in range(rec.shape[1]):
            for v in range(2):
                c = cen[f, j]
                if not (np.isfinite(rec[f, j, 13 * v:13 * v + 13]).all() and np.isfinite(c).all()):
                    continue
                ray = c / np.linalg.norm(c)
                e = np.cross(ray, [0.0, 1.0, 0.0])
                e /= np.linalg.norm(e)
                th = phase + 1.3 * (2 * j + v) + 0.7 * f
                out[f, j, 13 * v + 10:13 * v + 13] += shift * (np.cos(th) * e + np.sin(th) * np.cross(ray, e))
    return out


def lateral_errors(exact, refined, cen):
    """(n, K, 2): how far each refined pose carries its part's observed centroid from where the exact pose has it, across the centroid's ray."""
    n, K = exact.shape[:2]
    out = np.full((n, K, 2), np.nan)
    for f in range(n):
        for j in range(K):
            for v in range(2):
                a, b, c = exact[f, j, 13 * v:13 * v + 13], refined[f, j, 13 * v:13 * v + 13], cen[f, j]
                ray = c / np.linalg.norm(c)
                x = (b[9] / a[9]) * (b[:9].reshape(3, 3) @ a[:9].reshape(3, 3).T @ (c - a[10:13])) + b[10:13]
                d = x - c
                out[f, j, v] = np.linalg.norm(d - (d @ ray) * ray)
    return out
