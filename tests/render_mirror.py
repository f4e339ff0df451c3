"""numpy statement of ancsh_render_depth_labels (include/ancsh_hip.h): int64 coverage on 1/256-pixel fixed point, float64 depth in the
written order, the minimum z-buffer key, the resolve -- byte for byte what the kernels write.  Validated on its own, against analytic
ray-box distances, in tests/test_render_cpu.py.  Test infrastructure only."""
import numpy as np

RENDER_WIDTH, RENDER_HEAD, RENDER_LINK, MAX_LINKS = 208, 16, 12, 16
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FIXED_LIMIT = float(1 << 25)
NOT_OBJECT = 255


def frame_links(rt):
    """The links a frame's table renders: 0 (an all-background frame) unless nlinks is in 1..16 and z_min > 0."""
    with np.errstate(invalid="ignore"):
        return int(rt[8]) if rt[8] >= 1.0 and rt[8] <= MAX_LINKS and rt[7] > 0.0 else 0


def project(verts, R, rt):
    """(n, 3) float32 model points of a link with the map R (3, 4) -> (X, Y int64 fixed point, 1 / z, ok), in the written order."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = [((R[a, 0] * v[:, 0] + R[a, 1] * v[:, 1]) + R[a, 2] * v[:, 2]) + R[a, 3] for a in range(3)]
        z = q[2]
        s, t = q[0] / z, q[1] / z
        col, row = (rt[0] * s + rt[1] * t) + rt[2], (rt[3] * s + rt[4] * t) + rt[5]
        X, Y = np.rint(256.0 * col), np.rint(256.0 * row)
        ok = (z >= rt[7]) & (z < np.inf) & (np.abs(X) < FIXED_LIMIT) & (np.abs(Y) < FIXED_LIMIT)
        iz = 1.0 / z
        return np.where(ok, X, 0).astype(np.int64), np.where(ok, Y, 0).astype(np.int64), iz, ok


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def raster_keys(verts, tris, tri_link, h, w, row0, col0, rt, depth64=None):
    """The z-buffer of one crop, (h, w) uint64: per pixel the minimum of (bits of (float32) d) << 32 | triangle index over the triangles
    that cover its sample point (row0 + i, col0 + j); EMPTY where none does.  depth64: an (h, w) float64 array that receives the winner's d
    before its rounding to float32 (for the mirror's own validation)."""
    verts, tris, tri_link = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(tri_link, np.int64)
    keys = np.full((h, w), EMPTY, np.uint64)
    nl = frame_links(rt)
    if nl == 0:
        return keys
    for t, (idx, l) in enumerate(zip(tris, tri_link)):
        if not 0 <= l < nl or (idx < 0).any() or (idx >= len(verts)).any():
            continue
        R = np.asarray(rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)], np.float64).reshape(3, 4)
        X, Y, iz, ok = project(verts[idx], R, rt)
        if not ok.all():
            continue
        X, Y = [int(v) for v in X], [int(v) for v in Y]                  # Python integers: exact whatever the size
        area2 = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
        if area2 == 0:
            continue
        c_lo, c_hi = max(-((-min(X)) // 256), col0), min(max(X) // 256, col0 + w - 1)
        r_lo, r_hi = max(-((-min(Y)) // 256), row0), min(max(Y) // 256, row0 + h - 1)
        if c_lo > c_hi or r_lo > r_hi:
            continue
        r, c = np.meshgrid(np.arange(r_lo, r_hi + 1, dtype=np.int64), np.arange(c_lo, c_hi + 1, dtype=np.int64), indexing="ij")
        px, py = 256 * c, 256 * r
        ea, eb, ec = edge(X[1], Y[1], X[2], Y[2], px, py), edge(X[2], Y[2], X[0], Y[0], px, py), edge(X[0], Y[0], X[1], Y[1], px, py)
        assert max(np.abs(ea).max(), np.abs(eb).max(), np.abs(ec).max(), abs(area2)) < (1 << 53)
        inside = ((ea >= 0) & (eb >= 0) & (ec >= 0)) if area2 > 0 else ((ea <= 0) & (eb <= 0) & (ec <= 0))
        if not inside.any():
            continue
        ea, eb, ec, r, c = ea[inside], eb[inside], ec[inside], r[inside], c[inside]
        with np.errstate(all="ignore"):
            la, lb, lc = ea.astype(np.float64) / float(area2), eb.astype(np.float64) / float(area2), ec.astype(np.float64) / float(area2)
            invz = (la * iz[0] + lb * iz[1]) + lc * iz[2]
            d64 = 1.0 / invz
            d = d64.astype(np.float32)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        better = key < keys[r - row0, c - col0]
        keys[(r - row0)[better], (c - col0)[better]] = key[better]
        if depth64 is not None:
            depth64[(r - row0)[better], (c - col0)[better]] = d64[better]
    return keys


def resolve(keys, tri_link, depth_scale, dtype):
    """A crop's keys -> (depth (h, w) of `dtype`, labels (h, w) uint8)."""
    tri_link = np.asarray(tri_link, np.int64)
    hit = keys != EMPTY
    t = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit &= t < len(tri_link)
    df = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = df / np.float64(depth_scale)
        if np.dtype(dtype) == np.uint16:
            q = np.rint(v)
            keep = hit & (q >= 1.0) & (q <= 65535.0)
            depth = np.where(keep, q, 0.0).astype(np.uint16)
        else:
            q = v.astype(np.float32)
            keep = hit & (q > 0) & (q < np.inf)
            depth = np.where(keep, q, np.float32(0)).astype(np.float32)
    labels = np.where(keep, tri_link[np.where(hit, t, 0)] if len(tri_link) else 0, NOT_OBJECT).astype(np.uint8)
    return depth, labels


def render_crop(verts, tris, tri_link, h, w, row0, col0, rt, dtype):
    """One frame's crop -> (depth (h, w), labels (h, w) uint8, keys (h, w) uint64)."""
    rt = np.asarray(rt, np.float64)
    keys = raster_keys(verts, tris, tri_link, h, w, row0, col0, rt)
    return resolve(keys, tri_link, rt[6], dtype) + (keys,)


def render_flat(verts, tris, tri_link, geom, render, pixel_capacity, dtype, depth_fill, label_fill):
    """The operator on its own arguments -> (depth (pixel_capacity,), labels (pixel_capacity,)): every pixel of every crop inside the
    buffers written, the others holding the fills.  Crops are written in frame order (frames that share pixels must be equal)."""
    depth, labels = np.full(pixel_capacity, depth_fill, dtype), np.full(pixel_capacity, label_fill, np.uint8)
    for f, g in enumerate(np.asarray(geom, np.int64)):
        start, h, w, row0, col0 = (int(v) for v in g)
        if start < 0 or h < 1 or w < 1 or h * w > pixel_capacity - start:
            continue
        d, l, _ = render_crop(verts, tris, tri_link, h, w, row0, col0, render[f], dtype)
        depth[start:start + h * w], labels[start:start + h * w] = d.reshape(-1), l.reshape(-1)
    return depth, labels
