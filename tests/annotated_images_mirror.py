"""The numpy restatement of ancsh_depth_annotated_images (include/ancsh_hip.h) that its CPU and GPU tests share: the pixel -> row map of an
annotated frame -- for each used link in rank order, np.where(label == link and the depth is valid) in row-major order, concatenated, which
is the order ancsh_depth_annotate_stream's stable counting sort gives the rows -- and the gather of what lies per row back onto the crop."""
import numpy as np

from test_depth_annotate_cpu import valid_depth

NAN_BITS = 0x7fc00000
SCENE_HEAD, SCENE_LINK, MAX_LINKS = 16, 14, 16


def link_order(scene):
    """The used links of a scene table in rank order."""
    nl = int(scene[14])
    ranks = [(int(scene[SCENE_HEAD + SCENE_LINK * l]), l) for l in range(nl) if scene[SCENE_HEAD + SCENE_LINK * l] >= 0]
    return [l for _, l in sorted(ranks)]


def pixel_rows(depth, label, scene):
    """One frame: depth (h, w), label (h, w) link bytes, scene (240,) -> (rows (h, w) int64: the index of every valid pixel's row among the
    frame's rows, -1 for a pixel without one; the frame's row count).  A frame in which a used link has fewer valid pixels than scene[13]
    has no rows at all."""
    ok = valid_depth(depth)
    rows = np.full(depth.shape, -1, np.int64)
    at = 0
    for link in link_order(scene):
        i, j = np.where((label == link) & ok)                            # row-major
        if len(i) < scene[13]:
            return np.full(depth.shape, -1, np.int64), 0
        rows[i, j] = at + np.arange(len(i))
        at += len(i)
    return rows, at


def frame_images(rows, first, labels, values, gt_rows, capacity):
    """Gather: rows (h, w) from pixel_rows, first = the frame's first row (offsets[b]) -> (labels (h, w) int32, values (h, w, 7) float32,
    gt_labels (h, w) int32, gt_values (h, w, 6) float32); a pixel without a row, or whose row lies at or beyond capacity, reads -1 / the
    NaN of NAN_BITS."""
    h, w = rows.shape
    r = np.where(rows >= 0, rows + first, -1)
    on = (r >= 0) & (r < capacity)
    il, igl = np.full((h, w), -1, np.int32), np.full((h, w), -1, np.int32)
    iv = np.full((h, w, 7), NAN_BITS, np.uint32).view(np.float32)
    igv = np.full((h, w, 6), NAN_BITS, np.uint32).view(np.float32)
    src = r[on]
    il[on], iv[on] = labels[src], values[src]
    part = gt_rows[src, 3]
    with np.errstate(invalid="ignore"):
        igl[on] = np.where(np.isfinite(part), part, -1).astype(np.int32)
    igv[on] = gt_rows[src, 4:10]
    return il, iv, igl, igv


def batch_offsets(pix, lab, geom, scenes):
    """(counts (B,), offsets (B + 1,), per-cloud pixel_rows or None for a crop the entry refuses) of a batch laid out in flat buffers."""
    cnt, maps = np.zeros(geom.shape[0], np.int64), []
    for b, (start, h, w) in enumerate(geom[:, :3].tolist()):
        if start < 0 or h < 1 or w < 1 or start + h * w > pix.shape[0]:
            maps.append(None)
            continue
        rows, cnt[b] = pixel_rows(pix[start:start + h * w].reshape(h, w), lab[start:start + h * w].reshape(h, w), scenes[b])
        maps.append(rows)
    return cnt, np.concatenate([[0], np.cumsum(np.maximum(cnt, 1))]), maps


def expected(pix, lab, geom, scenes, dest, labels, values, gt_rows, capacity, icap, fill):
    """The contract over a whole batch: four image buffers of icap elements prefilled with `fill` = (label, value) sentinels, every crop
    with dest >= 0 that fits written in full, nothing else touched.  -> (img_labels, img_values, img_gt_labels, img_gt_values, offsets, counts)."""
    cnt, off, maps = batch_offsets(pix, lab, geom, scenes)
    out = [np.full(icap, fill[0], np.int32), np.full((icap, 7), fill[1], np.float32), np.full(icap, fill[0], np.int32),
           np.full((icap, 6), fill[1], np.float32)]
    for b, rows in enumerate(maps):
        d0 = int(dest[b])
        if rows is None or d0 < 0 or d0 + rows.size > icap:
            continue
        for buf, img in zip(out, frame_images(rows, off[b], labels, values, gt_rows, capacity)):
            buf[d0:d0 + rows.size] = img.reshape((rows.size,) + img.shape[2:])
    return out + [off, cnt]
