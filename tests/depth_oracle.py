"""numpy float32 restatement of ancsh_depth_unproject_stream (include/ancsh_hip.h): the validity rule, the row-major order, the NaN row
of a cloud without a valid pixel, offsets and counts -- bit for bit what the kernels write.  Test infrastructure only."""
import numpy as np

GEOM_WORDS, CAM_WORDS = 5, 7


def fmaf(a, b, c):
    """round_f32(a * b + c) with ONE rounding, for float32 arrays.  a * b is exact in float64 (48 bits); the float64 sum is rounded to odd
    (TwoSum gives its error exactly), after which the rounding to float32 equals that of the exact sum (53 >= 2 * 24 + 2 bits)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a * b
        t = s + c
        bb = t - s
        e = (s - (t - bb)) + (c - bb)
        fix = np.isfinite(t) & (e != 0) & ((t.view(np.int64) & 1) == 0)
        t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
        return t.astype(np.float32)


def valid_pixels(depth, mask):
    """(h, w) bool: the mask byte is non-zero (or no mask) and the depth is d != 0 (uint16) / d > 0 and d < +inf (float32)."""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        ok = d != 0
    else:
        assert d.dtype == np.float32, d.dtype
        with np.errstate(invalid="ignore"):
            ok = (d > 0) & (d < np.inf)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def unproject_crop(depth, mask, origin, cam):
    """One crop -> (count, 3) float32 rows in np.where order.  cam: 7 float32 {A00 A01 A02 A10 A11 A12 depth_scale}."""
    cam = np.asarray(cam, np.float32)
    i, j = np.where(valid_pixels(depth, mask))
    d = np.asarray(depth)[i, j]
    row, col = (origin[0] + i).astype(np.float32), (origin[1] + j).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        z = d.astype(np.float32) * cam[6]
        gx = fmaf(cam[1], row, fmaf(cam[0], col, cam[2]))
        gy = fmaf(cam[4], row, fmaf(cam[3], col, cam[5]))
        return np.stack([z * gx, z * gy, z], axis=1).astype(np.float32)


def unproject_flat(pix, mask, geom, cam, capacity=None, fill=0.0):
    """The operator on its own arguments: pix (pixel_capacity,), mask (pixel_capacity,) uint8 or None, geom (B, 5) int32, cam (B, 7)
    float32 -> (rows (capacity, 3) float32 -- `fill` where nothing is written --, offsets (B+1,) int32, counts (B,) int32)."""
    pix, geom, cam = np.asarray(pix), np.asarray(geom, np.int32), np.asarray(cam, np.float32)
    capacity = pix.shape[0] if capacity is None else capacity
    rows = np.full((capacity, 3), fill, np.float32)
    B = geom.shape[0]
    offsets, counts = np.zeros(B + 1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        start, h, w, r0, c0 = (int(v) for v in geom[b])
        if start < 0 or h < 1 or w < 1 or start + h * w > pix.shape[0]:
            pts = np.zeros((0, 3), np.float32)
        else:
            m = None if mask is None else mask[start:start + h * w].reshape(h, w)
            pts = unproject_crop(pix[start:start + h * w].reshape(h, w), m, (r0, c0), cam[b])
        counts[b] = len(pts)
        if len(pts) == 0:
            pts = np.full((1, 3), np.nan, np.float32)
        o = int(offsets[b])
        offsets[b + 1] = o + len(pts)
        rows[o:o + len(pts)] = pts
    return rows, offsets, counts


def unproject_frames(frames, cameras, depth_scale):
    """Frames as AncshPipeline.submit_depth takes them -> (clouds: list of (max(count, 1), 3) float32, counts (n,) int32)."""
    n = len(frames)
    cam = np.broadcast_to(np.asarray(cameras, np.float64), (n, 6))
    sc = np.broadcast_to(np.asarray(depth_scale, np.float64).reshape(-1), (n,))
    cam = np.concatenate([cam, sc[:, None]], 1).astype(np.float32)
    clouds, counts = [], []
    for k, (d, m, org) in enumerate(frames):
        pts = unproject_crop(d, m, org, cam[k])
        counts.append(len(pts))
        clouds.append(pts if len(pts) else np.full((1, 3), np.nan, np.float32))
    return clouds, np.asarray(counts, np.int32)
