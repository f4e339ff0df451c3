"""A numpy mirror of ancsh_depth_sensor_model (include/ancsh_hip.h): the draws are Python integers, the arithmetic is float64 in the written
order, one pixel at a time.  Test infrastructure: slow, plain, and validated on its own in tests/test_depth_sensor_cpu.py."""
import numpy as np

SENSOR_WIDTH, SCENE_WIDTH, BACKGROUND = 16, 240, 255
MASK64 = (1 << 64) - 1
TAG = 0xE000000000000000
SQRT3 = np.float64(1.7320508075688772)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def draw(seed, g, p, k):
    """r_k of pixel p of global frame g."""
    return splitmix64((int(seed) & MASK64) ^ splitmix64(TAG | (int(g) << 36) | (int(p) << 4) | k))


def uniform(r):
    return np.float64(r >> 11) * np.float64(2.0 ** -53)


def usable(d):
    """The stored depth value is usable: uint16 >= 1, float32 finite and > 0."""
    return bool(d >= 1) if d.dtype == np.uint16 else bool(np.isfinite(d) and d > 0)


def sensor_crop(depth, labels, depth_scale, sensor, seed, g):
    """One crop: depth (h, w) uint16 / float32, labels (h, w) uint8 -> (depth, labels) of the degraded frame, fresh arrays."""
    t = np.asarray(sensor, np.float64)
    a0, a1, a2, z0, p_hole, p_edge, edge_rel, qd, steps, z_near, z_far = (np.float64(v) for v in t[:11])
    scale = np.float64(depth_scale)
    h, w = depth.shape
    out_d, out_l = depth.copy(), labels.copy()
    surface = np.array([[labels[i, j] != BACKGROUND and usable(depth[i, j]) for j in range(w)] for i in range(h)], bool).reshape(h, w)
    with np.errstate(all="ignore"):
        zc = depth.astype(np.float64) * scale                             # the clean depths, (double)stored * depth_scale
        for i in range(h):
            for j in range(w):
                if not surface[i, j]:
                    continue                                                # copied verbatim
                p, z = i * w + j, zc[i, j]
                keep = bool(z_near <= z and z <= z_far)
                if keep:
                    keep = not uniform(draw(seed, g, p, 0)) < p_hole
                if keep and p_edge > 0:
                    edge = False
                    for ni, nj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                        if 0 <= ni < h and 0 <= nj < w:
                            if not surface[ni, nj] or np.abs(zc[ni, nj] - z) > edge_rel * z:
                                edge = True
                    if edge:
                        keep = not uniform(draw(seed, g, p, 1)) < p_edge
                if keep:
                    r2, r3 = draw(seed, g, p, 2), draw(seed, g, p, 3)
                    S = (r2 >> 32) + (r2 & 0xFFFFFFFF) + (r3 >> 32) + (r3 & 0xFFFFFFFF)
                    n = (np.float64(S) * np.float64(2.0 ** -32) - np.float64(2.0)) * SQRT3
                    dz = z - z0
                    sigma = (a0 + a1 * dz) + a2 * (dz * dz)
                    z1 = z + sigma * n
                    z2 = z1
                    if qd > 0:
                        dq = np.rint((qd / z1) * steps) / steps
                        if dq > 0:
                            z2 = qd / dq
                        else:
                            keep = False
                    if keep and np.float64(z2).tobytes() != np.float64(z).tobytes():
                        v = z2 / scale
                        if depth.dtype == np.uint16:
                            q = np.rint(v)
                            keep = bool(q >= 1 and q <= 65535)
                            if keep:
                                out_d[i, j] = int(q)
                        else:
                            f = np.float32(v)
                            keep = bool(np.isfinite(f) and f > 0)
                            if keep:
                                out_d[i, j] = f
                if not keep:
                    out_d[i, j], out_l[i, j] = 0, BACKGROUND
    return out_d, out_l


def sensor_flat(depth, labels, geom, scenes, sensor, seed, base=0, fill=0, label_fill=BACKGROUND):
    """The entry on flat pixel buffers: depth (cap,), labels (cap,) uint8, geom (n, 5) {start h w row0 col0}, scenes (n, 240) -> (depth_out,
    labels_out) (cap,), prefilled with fill / label_fill where no crop lies.  A frame with h < 1, w < 1 or a crop outside the buffer writes
    nothing."""
    cap = depth.shape[0]
    out_d, out_l = np.full(cap, fill, depth.dtype), np.full(cap, label_fill, np.uint8)
    for f, (start, h, w, _r0, _c0) in enumerate(np.asarray(geom).reshape(-1, 5).tolist()):
        if start < 0 or h < 1 or w < 1 or h * w > cap - start:
            continue
        d, l = sensor_crop(depth[start:start + h * w].reshape(h, w), labels[start:start + h * w].reshape(h, w),
                           np.asarray(scenes, np.float64).reshape(-1, SCENE_WIDTH)[f, 6], sensor, seed, base + f)
        out_d[start:start + h * w], out_l[start:start + h * w] = d.reshape(-1), l.reshape(-1)
    return out_d, out_l


def sensor_frame_list(frames, scenes, sensor, seed, base=0):
    """depth.sensor_frames on the host: [(depth (h, w), labels (h, w) uint8, origin)] -> the same form."""
    scenes = np.asarray(scenes, np.float64)
    scenes = np.broadcast_to(scenes, (len(frames), SCENE_WIDTH)) if scenes.ndim == 1 else scenes
    return [sensor_crop(np.asarray(d), np.asarray(l, np.uint8), scenes[f, 6], sensor, seed, base + f) + (org,)
            for f, (d, l, org) in enumerate(frames)]
