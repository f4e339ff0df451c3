"""The depth front end of the streaming pipeline: what a depth camera delivers -- a depth image, an object mask, a camera matrix -- turned
into camera-space clouds on the GPU (ancsh_depth_unproject_stream, include/ancsh_hip.h; reference: tools/preprocess_data.py:259-298).

A frame is (depth_crop (h, w), mask_crop (h, w) or None, (row0, col0)): a crop of the depth image around the object, the object's mask in
it, and the crop's origin in the full image.  A camera is six unprojection coefficients (A00 A01 A02 A10 A11 A12): the valid pixel in
image row `row`, column `col` with depth d becomes z = d * depth_scale, x = z * (A00 col + A01 row + A02), y = z * (A10 col + A11 row + A12).
The helpers below compute them in float64; they are cast to float32 once, when a batch is submitted.

The second half of the module annotates rendered frames (ancsh_depth_annotate_stream; reference: tools/preprocess_data.py:226-348): a frame
is then (depth_crop, link-label crop, (row0, col0)) and travels with one float64 scene table (pack_frame_scene) that holds the camera and
every link's camera-to-URDF map; the device makes the 7-column annotated rows [x y z | cx cy cz | part] dataset.point_gt_build reads.

The third renders such frames on the GPU (ancsh_render_depth_labels; reference: tools/render_synthetic.py:180-225, on the host): the
triangle meshes of an object's links (pack_mesh) and one float64 render table per frame (pack_render_scene: the inverse of the scene
table's camera model and link maps) go in, depth crops and link-label crops come out where the annotation reads them.

The fourth builds both tables on the GPU (ancsh_pose_scene_build; reference: pybullet's forward kinematics in
tools/render_synthetic.py:140-158, 206-217, on the host): an object's kinematic table (pack_kinematics), uploaded once, and one pose per
frame (pack_pose: joint values and a view matrix) go in; and centres crops on the projected object (ancsh_render_centre_crops).

The last three take a LIBRARY of object instances in place of one object (the *_lib entries; reference: tools/render_synthetic.py:52, one
render_data call per instance): pack_mesh_library concatenates the instances' meshes, the kinematics is the (ninst, 672) stack of their
tables, and a frame names its instance in its own table (pack_pose / pack_render_scene, instance=).

Between the renderer and the annotation stands an optional depth sensor (ancsh_depth_sensor_model; the reference has none: pybullet's depth
is clean): one table per pipeline (pack_sensor) of range-dependent noise, holes, dropout at depth discontinuities and disparity steps turns
the clean crops into the frames a real camera would deliver, in a second pair of pixel buffers.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib

# name -> (numpy dtype, torch dtype of the device buffer -- uint16 pixels travel as their int16 bits --, the ABI's depth_type)
DEPTH_DTYPES = {"uint16": (np.uint16, torch.int16, 0), "float32": (np.float32, torch.float32, 1)}
GEOM_WORDS, CAM_WORDS, MAX_CHUNKS = 5, 7, 64       # per cloud: int32 {start h w row0 col0}, float32 {A00..A12 depth_scale}; scratch ints per cloud


def check_depth_dtype(depth_dtype):
    """-> the canonical name ("uint16" | "float32") of a depth dtype given as a name or a numpy dtype; ValueError otherwise."""
    try:
        name = np.dtype(depth_dtype).name
    except TypeError:
        name = None
    if name not in DEPTH_DTYPES:
        raise ValueError("depth_dtype must be 'uint16' or 'float32', got %r" % (depth_dtype,))
    return name


def unprojection_from_intrinsics(fx, fy, cx, cy):
    """Pinhole intrinsics (pixels) -> (A00, A01, A02, A10, A11, A12) float64 = (1/fx, 0, -cx/fx, 0, 1/fy, -cy/fy):
    x = z (col - cx) / fx, y = z (row - cy) / fy."""
    fx, fy, cx, cy = (float(v) for v in (fx, fy, cx, cy))
    return np.array([1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy], np.float64)


def unprojection_from_projmat(projMat, height, width):
    """The reference's convention (tools/preprocess_data.py:271-296) -> (A00 .. A12) float64.  projMat: the (4, 4) projection matrix in
    the `.reshape(4, 4).T` form the reference uses (:229).  There u = col * 2 / W - 1, v1 = row * 2 / H - 1, M = pinv(projMat[:2, :2].T)
    and cloud_cam_real[:, :2] = -d * [u + P02, v1 + P12] @ M with d as the third column; collecting the terms in col and row gives the
    six coefficients."""
    P = np.asarray(projMat, np.float64)
    if P.shape != (4, 4):
        raise ValueError("projMat must be (4, 4), got %s" % (P.shape,))
    H, W = float(height), float(width)
    M = np.linalg.pinv(P[:2, :2].T)
    p02, p12 = P[0, 2], P[1, 2]
    return np.array([-2.0 * M[0, 0] / W, -2.0 * M[1, 0] / H, -((p02 - 1.0) * M[0, 0] + (p12 - 1.0) * M[1, 0]),
                     -2.0 * M[0, 1] / W, -2.0 * M[1, 1] / H, -((p02 - 1.0) * M[0, 1] + (p12 - 1.0) * M[1, 1])], np.float64)


def check_norm_factors(norm_factors, n):
    """-> the norm factors of n frames as a (n,) float32 array; ValueError unless there is one finite value per frame."""
    nf = np.asarray(norm_factors, np.float32).reshape(-1)
    if nf.size != n or not np.isfinite(nf).all():
        raise ValueError("norm_factors: one finite value per frame (%d frames, got %s)" % (n, nf.tolist()))
    return nf


def _per_frame(tables, n, width):
    """One (width,) float64 table, repeated for each of n frames, or whatever array `tables` is: its caller refuses any shape but (n, width)
    in its own words (and what is no array at all as shape (0,))."""
    try:
        a = np.asarray(tables, np.float64)
    except (TypeError, ValueError):
        a = np.zeros(0)
    return np.broadcast_to(a, (n, width)) if a.shape == (width,) else a


def check_depth_frames(frames, norm_factors, cameras, depth_scale, depth_dtype, max_clouds=None):
    """Validate a batch of depth frames before anything is enqueued.  frames: 1..max_clouds tuples (depth_crop (h, w) of dtype
    depth_dtype, mask_crop (h, w) or None, (row0, col0)); norm_factors: one finite value per frame; cameras: one 6-vector or one per
    frame; depth_scale: one finite value or one per frame.  -> (depth crops (contiguous), masks (contiguous uint8 0/1, or None), origins
    (n, 2) int32, norm factors (n,) float32, cam (n, 7) float32 = the six coefficients and the scale); ValueError otherwise."""
    name = check_depth_dtype(depth_dtype)
    npt = DEPTH_DTYPES[name][0]
    if not isinstance(frames, (list, tuple)):
        raise ValueError("frames must be a list of (depth_crop, mask_crop or None, (row0, col0)) tuples")
    if not 1 <= len(frames) <= (max_clouds or 65535):
        raise ValueError("a batch holds 1..%d frames, got %d" % (max_clouds or 65535, len(frames)))
    depths, masks, origins = [], [], []
    for i, fr in enumerate(frames):
        if not isinstance(fr, (list, tuple)) or len(fr) != 3:
            raise ValueError("frame %d: expected (depth_crop, mask_crop or None, (row0, col0))" % i)
        d, m, org = fr
        d = np.asarray(d.cpu().numpy() if torch.is_tensor(d) else d)
        if d.dtype != npt:
            raise ValueError("frame %d: the depth crop is %s, the pipeline streams %s (no silent conversion)" % (i, d.dtype, name))
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 1:
            raise ValueError("frame %d: expected a non-empty (h, w) depth crop, got shape %s" % (i, d.shape))
        if m is not None:
            m = np.asarray(m.cpu().numpy() if torch.is_tensor(m) else m)
            if m.shape != d.shape:
                raise ValueError("frame %d: the mask is %s, the depth crop %s" % (i, m.shape, d.shape))
            if m.dtype != np.bool_ and not np.issubdtype(m.dtype, np.integer):
                raise ValueError("frame %d: the mask must be boolean or integer (non-zero = object), got %s" % (i, m.dtype))
            m = np.ascontiguousarray(m != 0).view(np.uint8)
        try:
            r0, c0 = (int(v) for v in org)
            if (r0, c0) != tuple(org) or not (abs(r0) < (1 << 24) and abs(c0) < (1 << 24)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("frame %d: the crop origin must be an integer pair (row0, col0) below 2^24, got %r" % (i, org))
        if r0 + d.shape[0] > (1 << 24) or c0 + d.shape[1] > (1 << 24):
            raise ValueError("frame %d: image rows / columns must stay below 2^24 (exact as float32)" % i)
        depths.append(np.ascontiguousarray(d))
        masks.append(m)
        origins.append((r0, c0))
    n = len(depths)
    nf = check_norm_factors(norm_factors, n)
    cam64 = _per_frame(cameras, n, 6)
    if cam64.shape != (n, 6) or not np.isfinite(cam64).all():
        raise ValueError("cameras: one finite 6-vector (A00 A01 A02 A10 A11 A12), or one per frame (%d frames)" % n)
    try:
        sc = np.asarray(depth_scale, np.float64).reshape(-1)
    except (TypeError, ValueError):
        sc = np.zeros(0)
    if sc.size == 1:
        sc = np.repeat(sc, n)
    if sc.size != n or not np.isfinite(sc).all():
        raise ValueError("depth_scale: one finite value, or one per frame (%d frames)" % n)
    with np.errstate(over="ignore"):
        cam = np.concatenate([cam64, sc[:, None]], axis=1).astype(np.float32)
    if not np.isfinite(cam).all():
        raise ValueError("cameras / depth_scale: not finite in float32")
    return depths, masks, np.asarray(origins, np.int32).reshape(n, 2), nf, cam


def pack_depth_frames(depths, masks, origins, pix, mask, geom, first=0):
    """Write validated frames (check_depth_frames) into host staging: pix / mask (flat pixel buffers; a frame without a mask gets ones),
    geom (n, 5) int32 rows {start, h, w, row0, col0}, frame k's crop at pixel `first` + the pixels of the frames before it.  -> the pixel
    after the last crop."""
    a = int(first)
    for k, (d, m) in enumerate(zip(depths, masks)):
        h, w = d.shape
        pix[a:a + h * w] = d.reshape(-1)
        if m is None:
            mask[a:a + h * w] = 1
        else:
            mask[a:a + h * w] = m.reshape(-1)
        geom[k] = (a, h, w, origins[k][0], origins[k][1])
        a += h * w
    return a


# ---- what the device wrappers below check before a launch: one function and one message template per kind of buffer.  A wrapper calls them
# in the order its arguments are refused in; what only one wrapper takes (a sensor table, a mesh) it checks itself ---------------------------
_DEPTH_KINDS = {torch.float32: 1, torch.int16: 0}                       # a depth tensor's dtype -> the ABI's depth_type
if hasattr(torch, "uint16"):
    _DEPTH_KINDS[torch.uint16] = 0


def _depth_plane(depth, name=None):
    """-> (depth_type, pixel_capacity) of a flat depth tensor; name: the one depth dtype ("uint16" | "float32") the caller takes."""
    kind = _DEPTH_KINDS.get(depth.dtype)
    if kind is None or (name is not None and kind != DEPTH_DTYPES[name][2]) or depth.dim() != 1 or not depth.is_contiguous():
        raise ValueError("depth must be a contiguous 1-d %s tensor" % (name or "uint16 or float32"))
    return kind, int(depth.shape[0])


def _byte_plane(name, t, cap_px, none=None):
    """The byte beside every depth pixel, a mask or the link labels.  none: what the wrapper makes of None -- "every pixel": it passes (a
    mask); "refused": the ValueError of any other bad plane; by default the wrapper does not look for it."""
    if t is None and none == "every pixel":
        return
    if (t is None and none == "refused") or t.dtype != torch.uint8 or tuple(t.shape) != (cap_px,) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous (%d,) uint8 tensor" % (name, cap_px))


def _pixel_pair(what, whose, depth, labels, dtype, n):
    """A second (depth, labels) pair of n pixels beside the one the wrapper reads."""
    if depth.dtype != dtype or tuple(depth.shape) != (n,) or labels.dtype != torch.uint8 or tuple(labels.shape) != (n,) \
            or not (depth.is_contiguous() and labels.is_contiguous()):
        raise ValueError("%s must be contiguous (depth (%d,) of the %s dtype, labels (%d,) uint8)" % (what, n, whose, n))


_CAM_TABLE = ("cam", CAM_WORDS, torch.float32)                          # _geom_table's kinds; _SCENE_TABLE and _RENDER_TABLE below


def _geom_table(geom, table=None, kind=None):
    """-> B, the frames of the geometry rows (B, 5) int32 and, with kind = (name, width, dtype), of the per-frame table beside them."""
    B = int(geom.shape[0])
    ok = geom.dtype == torch.int32 and tuple(geom.shape) == (B, GEOM_WORDS)
    if kind is not None:
        name, width, dtype = kind
        ok = ok and table.dtype == dtype and tuple(table.shape) == (B, width)
    if not (ok and geom.is_contiguous() and (kind is None or table.is_contiguous())):
        raise ValueError("geom must be (B, 5) int32%s, contiguous"
                         % ("" if kind is None else " and %s (B, %d) %s" % (name, width, str(dtype).replace("torch.", ""))))
    return B


def _int_vector(name, t, n):
    if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous (%d,) int32 tensor" % (name, n))


def _labelled(labels, values, columns):
    """-> n when labels is (n,) int32 and values (n, columns) float32, both contiguous; -1 otherwise."""
    n = int(labels.shape[0]) if labels.dim() == 1 else -1
    if labels.dtype != torch.int32 or values.dtype != torch.float32 or n < 0 or tuple(values.shape) != (n, columns) \
            or not (labels.is_contiguous() and values.is_contiguous()):
        return -1
    return n


def _row_pair(names, labels, values):
    """-> the row capacity of a (labels (capacity,) int32, values (capacity, 7) float32) pair, named as the wrapper's arguments are."""
    cap = _labelled(labels, values, LABEL_VALUES)
    if cap < 0:
        raise ValueError("%s must be (capacity,) int32 and %s (capacity, %d) float32, contiguous" % (names[0], names[1], LABEL_VALUES))
    return cap


def _image_pair(img_labels, img_values):
    """-> the image capacity of out = (img_labels (n,) int32, img_values (n, 7) float32)."""
    icap = _labelled(img_labels, img_values, LABEL_VALUES)
    if icap < 0:
        raise ValueError("out must be contiguous (img_labels (n,) int32, img_values (n, %d) float32)" % LABEL_VALUES)
    return icap


def _scratch_given(scratch, n, wrapper):
    """The scratch tensor an earlier wrapper filled: >= n int32, and never None."""
    if scratch is None or scratch.dtype != torch.int32 or scratch.numel() < n or not scratch.is_contiguous():
        raise ValueError("scratch must be the (>= %d,) int32 tensor %s() was given" % (n, wrapper))


def _scratch_size(scratch, n, dtype=torch.int32):
    """A caller's own working memory: >= n elements of dtype."""
    if scratch.dtype != dtype or scratch.numel() < n or not scratch.is_contiguous():
        raise ValueError("scratch must be a contiguous %s tensor of >= %d elements" % (str(dtype).replace("torch.", ""), n))


def depth_unproject(depth, mask, geom, cam, capacity=None, out=None, scratch=None):
    """ancsh_depth_unproject_stream on device tensors (no host sync): depth (pixel_capacity,) uint16 / float32, mask (pixel_capacity,)
    uint8 or None, geom (B, 5) int32, cam (B, 7) float32.  -> (rows (capacity, 3) float32, offsets (B+1,) int32, counts (B,) int32);
    out = the same triple preallocated (a captured step passes slot-owned buffers); rows beyond offsets[B] keep what they held (fresh:
    zeros)."""
    _lib.require_device(depth)
    dev = depth.device
    kind, cap_px = _depth_plane(depth)
    _byte_plane("mask", mask, cap_px, none="every pixel")
    B = _geom_table(geom, cam, _CAM_TABLE)
    if out is None:
        capacity = cap_px if capacity is None else int(capacity)
        out = (torch.zeros((capacity, 3), dtype=torch.float32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev),
               torch.zeros((B,), dtype=torch.int32, device=dev))
    rows, offsets, counts = out
    if scratch is None:
        scratch = torch.empty((max(1, B) * MAX_CHUNKS,), dtype=torch.int32, device=dev)
    _lib.call("ancsh_depth_unproject_stream", B, kind, _lib.ptr(depth), _lib.ptr(mask), cap_px, _lib.ptr(geom), _lib.ptr(cam),
              _lib.ptr(rows), int(rows.shape[0]), _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(scratch))
    return rows, offsets, counts


LABEL_VALUES = 7        # per pixel, as per raw row: [W of the label | part NOCS (3) | NAOCS (3)] (dataset.DENSE_VALUES)
LABEL_NAN_BITS = 0x7fc00000     # ANCSH_LABEL_NAN_BITS: the float32 NaN of a pixel without a row


def depth_label_images(depth, mask, geom, dest, offsets, labels, values, out=None, scratch=None):
    """ancsh_depth_label_images on device tensors (no host sync): the per-row labels (capacity,) int32 / values (capacity, 7) float32 of
    ancsh_raw_point_labels back on the pixel grid.  depth, mask, geom: what depth_unproject() was given; offsets (B+1,) int32 and scratch:
    what it wrote (pass the SAME scratch tensor to both calls: it carries the per-chunk counts); dest (B,) int32: where cloud b's h * w
    image starts in the image buffers, < 0 = the cloud writes nothing.  -> (img_labels (image_capacity,) int32, img_values
    (image_capacity, 7) float32); out = the same pair preallocated (a captured step passes slot-owned buffers), else pixel_capacity
    elements prefilled with -1 / NaN.  A pixel without a row reads -1 / NaN; elements of no cloud's image keep what they held."""
    _lib.require_device(depth)
    dev = depth.device
    kind, cap_px = _depth_plane(depth)
    _byte_plane("mask", mask, cap_px, none="every pixel")
    B = _geom_table(geom)
    _int_vector("dest", dest, B)
    _int_vector("offsets", offsets, B + 1)
    cap = _row_pair(("labels", "values"), labels, values)
    _scratch_given(scratch, B * MAX_CHUNKS, "depth_unproject")
    if out is None:
        out = (torch.full((cap_px,), -1, dtype=torch.int32, device=dev),
               torch.full((cap_px, LABEL_VALUES), float("nan"), dtype=torch.float32, device=dev))
    img_labels, img_values = out
    icap = _image_pair(img_labels, img_values)
    _lib.require_device(geom, dest, offsets, labels, values, scratch, img_labels, img_values, *(() if mask is None else (mask,)))
    _lib.call("ancsh_depth_label_images", B, kind, _lib.ptr(depth), _lib.ptr(mask), cap_px, _lib.ptr(geom), _lib.ptr(offsets),
              _lib.ptr(scratch), _lib.ptr(labels), _lib.ptr(values), cap, _lib.ptr(dest), _lib.ptr(img_labels), _lib.ptr(img_values), icap)
    return img_labels, img_values


def cut_label_images(labels, values, shapes, first=0):
    """One batch's flat host image buffers -> its per-frame images (pure numpy): labels (>= n,) int32, values (>= n, 7) float32, shapes =
    the frames' (h, w) in submission order, frame k's image at element `first` + the pixels of the frames before it (pack_depth_frames'
    layout).  -> [(labels (h, w) int32, values (h, w, 7) float32)], fresh arrays."""
    labels, values = np.asarray(labels), np.asarray(values)
    if labels.dtype != np.int32 or labels.ndim != 1 or values.dtype != np.float32 or values.shape != (labels.shape[0], LABEL_VALUES):
        raise ValueError("expected labels (n,) int32 and values (n, %d) float32" % LABEL_VALUES)
    out, a = [], int(first)
    for k, hw in enumerate(shapes):
        h, w = (int(v) for v in hw)
        if h < 1 or w < 1:
            raise ValueError("frame %d: expected a non-empty (h, w), got %r" % (k, tuple(hw)))
        if a < 0 or a + h * w > labels.shape[0]:
            raise ValueError("frame %d: pixels [%d, %d) lie outside the %d-pixel buffers" % (k, a, a + h * w, labels.shape[0]))
        out.append((labels[a:a + h * w].reshape(h, w).copy(), values[a:a + h * w].reshape(h, w, LABEL_VALUES).copy()))
        a += h * w
    return out


def unproject_depth_batch(frames, cameras, depth_scale, depth_dtype, device="cuda:0"):
    """Eager wrapper: a batch of depth frames -> (clouds: list of (count, 3) float32 arrays in row-major pixel order -- a frame without a
    valid pixel gives one NaN row --, counts (n,) int32).  One host sync; the streaming pipeline (AncshPipeline.submit_depth) has none."""
    dev = _lib.cuda_device(device)
    depths, masks, origins, _, cam = check_depth_frames(frames, np.ones(len(frames)) if isinstance(frames, (list, tuple)) else None,
                                                        cameras, depth_scale, depth_dtype)
    _, _, (d_pix, d_mask, d_geom) = _stage_frames(depths, masks, origins, check_depth_dtype(depth_dtype), dev, fill=0)
    rows, off, cnt = depth_unproject(d_pix, d_mask, d_geom, torch.from_numpy(cam).to(dev))
    rows, off, cnt = rows.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    return [rows[off[b]:off[b + 1]].copy() for b in range(len(depths))], cnt


def _stage_frames(depths, planes, origins, name, dev, fill):
    """What the eager wrappers stage of validated frames -> (geom (n, 5) int32 on the host, the batch's pixels, (depth, byte plane, geom) on
    `dev`): pack_depth_frames' layout from pixel 0, uint16 depths as their int16 bits, `fill` in the byte plane of no frame."""
    total = sum(d.size for d in depths)
    pix, plane, geom = np.zeros(total, DEPTH_DTYPES[name][0]), np.full(total, fill, np.uint8), np.zeros((len(depths), GEOM_WORDS), np.int32)
    pack_depth_frames(depths, planes, origins, pix, plane, geom)
    up = lambda a: torch.from_numpy(a).to(dev)
    return geom, total, (up(pix.view(np.int16) if name == "uint16" else pix), up(plane), up(geom))


def _cut_frames(depth, labels, geom, name, first=0):
    """Flat host (depth, labels) buffers -> the frames [(depth_crop (h, w) of the dtype `name`, label_crop (h, w), (row0, col0))] of the
    geometry rows, frame k's crop at element `first` + its start; fresh arrays."""
    depth = depth.view(np.uint16) if name == "uint16" else depth
    cut = lambda a, g: a[first + g[0]:first + g[0] + g[1] * g[2]].reshape(g[1], g[2]).copy()
    return [(cut(depth, g), cut(labels, g), (int(g[3]), int(g[4]))) for g in geom]


# ---- annotated depth frames: depth + link labels -> the 7-column rows ancsh_point_gt_build reads (ancsh_depth_annotate_stream) -----------
SCENE_WIDTH, SCENE_MAX_LINKS, SCENE_HEAD, SCENE_LINK = 240, 16, 16, 14      # include/ancsh_hip.h, ANCSH_SCENE_*
NOT_OBJECT = 255                    # the label byte of a pixel of no link
_SCENE_TABLE = ("scene", SCENE_WIDTH, torch.float64)


def coord_unprojection_from_projmat(projMat, height, width):
    """The six coefficients (C00 .. C12) float64 of the reference's OTHER camera point, cloud_cam (tools/preprocess_data.py:271-291), from
    which it computes a pixel's canonical coordinates: as unprojection_from_projmat, with the image row flipped -- v = (H - row) * 2 / H -
    1 in place of v1 = row * 2 / H - 1.  The reference writes (512 - row) for its 512-row images: H here."""
    P = np.asarray(projMat, np.float64)
    if P.shape != (4, 4):
        raise ValueError("projMat must be (4, 4), got %s" % (P.shape,))
    H, W = float(height), float(width)
    M = np.linalg.pinv(P[:2, :2].T)
    p02, p12 = P[0, 2], P[1, 2]
    return np.array([-2.0 * M[0, 0] / W, 2.0 * M[1, 0] / H, -((p02 - 1.0) * M[0, 0] + (p12 + 1.0) * M[1, 0]),
                     -2.0 * M[0, 1] / W, 2.0 * M[1, 1] / H, -((p02 - 1.0) * M[0, 1] + (p12 + 1.0) * M[1, 1])], np.float64)


def _rotation_from_quaternion(w, x, y, z):
    """(4, 4) homogeneous rotation of the quaternion w + xi + yj + zk, normalised first (a zero quaternion: the identity)."""
    n = w * w + x * x + y * y + z * z
    T = np.eye(4)
    if n < 4.0 * np.finfo(np.float64).eps:
        return T
    s = 2.0 / n
    T[:3, :3] = [[1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]]
    return T


def _rotation_from_rpy(roll, pitch, yaw):
    """(4, 4) homogeneous rotation of static-axes x-y-z Euler angles ('sxyz'): Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[cp * cy, sr * sp * cy - cr * sy, cr * sp * cy + sr * sy],
                 [cp * sy, sr * sp * sy + cr * cy, cr * sp * sy - sr * cy],
                 [-sp, sr * cp, cr * cp]]
    return T


# what pack_frame_scene, pack_render_scene and pack_kinematics each need of the reference's conventions (tools/preprocess_data.py)
def _link_poses(link_world_pos, link_world_orn):
    """-> (pos (L, 3), orn (L, 4) [x y z w], L) float64 of 1..16 links' world poses."""
    pos, orn = np.asarray(link_world_pos, np.float64), np.asarray(link_world_orn, np.float64)
    L = pos.shape[0] if pos.ndim == 2 else 0
    if not 1 <= L <= SCENE_MAX_LINKS or pos.shape != (L, 3) or orn.shape != (L, 4):
        raise ValueError("link_world_pos must be (L, 3) and link_world_orn (L, 4) [x y z w] for 1..%d links, got %s and %s"
                         % (SCENE_MAX_LINKS, pos.shape, orn.shape))
    return pos, orn, L


def _cam2world(V):
    """pinv(viewMat.T) with its first three rows negated (:302-303)."""
    cam2world = np.linalg.pinv(V.T)
    cam2world[:3, :] = -cam2world[:3, :]
    return cam2world


def _model2world(orn, pos):
    """A link's (4, 4) world pose from its quaternion [x y z w] -- w goes first (:247-252) -- and position."""
    model2world = _rotation_from_quaternion(orn[3], orn[0], orn[1], orn[2])
    model2world[:3, 3] = pos
    return model2world


def _link_ranks(parts_map, L):
    """{link: (its position in the flattened parts_map, its group's index)}; ValueError unless the map names links of [0, L), each once."""
    flat = [(int(link), j) for j, group in enumerate(parts_map) for link in group]
    if len(set(l for l, _ in flat)) != len(flat) or any(not 0 <= l < L for l, _ in flat):
        raise ValueError("parts_map must name each of its links once, all in [0, %d): got %r" % (L, parts_map))
    return {l: (r, j) for r, (l, j) in enumerate(flat)}


def _canonical_offset(l, L, urdf_link_xyz, urdf_joint_xyz):
    """The translation of link l's canonical -> URDF map (:239-242): -urdf_link_xyz[l], but link 1 of a two-link object takes the joint's."""
    if l == 1 and L == 2:
        joint = np.asarray(urdf_joint_xyz, np.float64)
        if joint.ndim != 2 or joint.shape[0] < 1 or joint.shape[1] != 3:
            raise ValueError("urdf_joint_xyz must be (>= 1, 3) for a two-link object, got %s" % (joint.shape,))
        return joint[0]
    return -urdf_link_xyz[l]


def _inverse_pixel_map(C):
    """The six coefficients (row-major 2 x 3) of the inverse of coord_unprojection_from_projmat's affine pixel -> (s, t) map C."""
    A = np.array([[C[0], C[1]], [C[3], C[4]]])
    Ainv = np.linalg.inv(A)
    shift = -(Ainv @ np.array([C[2], C[5]]))
    return np.array([Ainv[0, 0], Ainv[0, 1], shift[0], Ainv[1, 0], Ainv[1, 1], shift[1]])


def pack_frame_scene(viewMat, projMat, link_world_pos, link_world_orn, urdf_link_xyz, urdf_link_rpy, urdf_joint_xyz, parts_map, height,
                     width, depth_scale=1.0, min_link_pixels=10):
    """One frame's scene table (SCENE_WIDTH,) float64 for ancsh_depth_annotate_stream (include/ancsh_hip.h has its layout), from what
    tools/preprocess_data.py:226-320 reads: viewMat / projMat (4, 4) in the `.reshape(4, 4).T` form of :228-229; every link's world pose
    link_world_pos (L, 3) and link_world_orn (L, 4) quaternions [x y z w] (:231-236 -- the reference sets link 0's to 0 / [0 0 0 1] and
    rounds the others to float32: the values are used as given); the URDF link frames urdf_link_xyz / urdf_link_rpy (L, 3) and joint
    origins urdf_joint_xyz (:238-243, the `link == 1 and num_parts == 2` rule included: with two links, link 1's offset is
    urdf_joint_xyz[0], every other one -urdf_link_xyz[link]); parts_map = the groups of links that make a part (lib/dataset.py:475-485): a
    link's rank is its position in the flattened map, its part the group's index, a link in no group is not used; height, width of the
    full image.  Per link the chain of :298-320 -- pinv(viewMat.T) with its first three rows negated, pinv(parts_model2world[l].T), the
    first three coordinates made homogeneous again, my_canon2urdf_mat.T -- is composed in float64 into one 3 x 4 map M of (x', y', z, 1)."""
    V, P = np.asarray(viewMat, np.float64), np.asarray(projMat, np.float64)
    if V.shape != (4, 4):
        raise ValueError("viewMat must be (4, 4), got %s" % (V.shape,))
    pos, orn, L = _link_poses(link_world_pos, link_world_orn)
    xyz, rpy = np.asarray(urdf_link_xyz, np.float64), np.asarray(urdf_link_rpy, np.float64)
    if xyz.shape != (L, 3) or rpy.shape != (L, 3):
        raise ValueError("urdf_link_xyz and urdf_link_rpy must be (%d, 3), got %s and %s" % (L, xyz.shape, rpy.shape))
    scene = np.zeros(SCENE_WIDTH)
    scene[0:6] = unprojection_from_projmat(P, height, width)
    scene[6] = float(depth_scale)
    scene[7:13] = coord_unprojection_from_projmat(P, height, width)
    scene[13], scene[14] = float(min_link_pixels), L
    rank = _link_ranks(parts_map, L)
    cam2world = _cam2world(V)
    for l in range(L):
        at = SCENE_HEAD + SCENE_LINK * l
        scene[at], scene[at + 1] = rank.get(l, (-1, 0))
        model2world = _model2world(orn[l], pos[l])
        offset = _canonical_offset(l, L, xyz, urdf_joint_xyz)
        canon2urdf = _rotation_from_rpy(*rpy[l])                        # :313-318
        canon2urdf[:3, 3] = offset
        # row vectors: p @ cam2world @ pinv(model2world.T) -> its first three coordinates and a one -> @ canon2urdf.T (:304-305, :319-320)
        G = cam2world @ np.linalg.pinv(model2world.T)
        M = (G[:, :3] @ canon2urdf.T[:3, :3]).T                         # (3, 4): M[a][i] multiplies coordinate i of (x', y', z, 1)
        M[:, 3] += canon2urdf[:3, 3]
        scene[at + 2:at + 14] = M.reshape(12)
    return scene


def check_scenes(scenes, n, K):
    """-> scenes as a C-contiguous (n, SCENE_WIDTH) float64 array (one table is repeated for every frame); ValueError (before anything
    touches a device) unless every table is finite, holds 1..16 links, the ranks of its used links are a permutation of 0 .. used - 1 and
    their parts lie in [0, K)."""
    a = _per_frame(scenes, n, SCENE_WIDTH)
    if a.shape != (n, SCENE_WIDTH):
        raise ValueError("scenes: one (%d,) table (depth.pack_frame_scene), or one per frame (%d frames), got shape %s"
                         % (SCENE_WIDTH, n, a.shape))
    a = np.ascontiguousarray(a)
    if not np.isfinite(a).all():
        raise ValueError("scenes: every value must be finite")
    for i, s in enumerate(a):
        nl = s[14]
        if nl != np.floor(nl) or not 1 <= nl <= SCENE_MAX_LINKS:
            raise ValueError("scene %d: nlinks must be an integer in [1, %d], got %r" % (i, SCENE_MAX_LINKS, float(nl)))
        if s[13] < 0 or s[15] != 0:
            raise ValueError("scene %d: min_link_pixels must be >= 0 and the reserved value 0" % i)
        links = s[SCENE_HEAD:SCENE_HEAD + SCENE_LINK * int(nl)].reshape(int(nl), SCENE_LINK)
        used = links[links[:, 0] != -1]
        if sorted(used[:, 0].tolist()) != list(range(len(used))):
            raise ValueError("scene %d: the ranks of the used links must be a permutation of 0 .. %d (-1 = not used), got %s"
                             % (i, len(used) - 1, links[:, 0].tolist()))
        if not ((used[:, 1] >= 0) & (used[:, 1] < K) & (used[:, 1] == np.floor(used[:, 1]))).all():
            raise ValueError("scene %d: the part of a used link must be an integer in [0, %d), got %s" % (i, K, used[:, 1].tolist()))
    return a


def check_annotated_frames(frames, norm_factors, scenes, depth_dtype, K, max_clouds=None):
    """Validate a batch of annotated depth frames before anything is enqueued.  frames: 1..max_clouds tuples (depth_crop (h, w) of dtype
    depth_dtype, label_crop (h, w) of an integer dtype -- a pixel's link index; a value outside [0, nlinks) of the frame's scene is not
    object --, (row0, col0)); norm_factors: one finite value per frame; scenes: one depth.pack_frame_scene table or one per frame.
    -> (depth crops (contiguous), label crops (contiguous uint8, NOT_OBJECT = 255 outside [0, nlinks)), origins (n, 2) int32, norm factors
    (n,) float32, scenes (n, SCENE_WIDTH) float64); ValueError otherwise."""
    if isinstance(frames, (list, tuple)):
        for i, fr in enumerate(frames):
            if isinstance(fr, (list, tuple)) and len(fr) == 3:
                lab = fr[1]
                lab = None if lab is None else np.asarray(lab.cpu().numpy() if torch.is_tensor(lab) else lab)
                if lab is None or not np.issubdtype(lab.dtype, np.integer):
                    raise ValueError("frame %d: the label crop must be an integer array of link indices, got %s"
                                     % (i, "None" if lab is None else lab.dtype))
    # the crops, origins and norm factors: the depth front end's own checks (a unit camera stands in for the scenes')
    depths, _, origins, nf, _ = check_depth_frames(frames, norm_factors, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 1.0, depth_dtype, max_clouds)
    scenes = check_scenes(scenes, len(depths), K)
    labels = []
    for fr, s in zip(frames, scenes):
        lab = np.asarray(fr[1].cpu().numpy() if torch.is_tensor(fr[1]) else fr[1])
        labels.append(np.ascontiguousarray(np.where((lab >= 0) & (lab < int(s[14])), lab, NOT_OBJECT).astype(np.uint8)))
    return depths, labels, origins, nf, scenes


def depth_annotate(depth, labels, geom, scene, capacity=None, out=None, scratch=None):
    """ancsh_depth_annotate_stream on device tensors (no host sync): depth (pixel_capacity,) uint16 / float32, labels (pixel_capacity,)
    uint8, geom (B, 5) int32, scene (B, SCENE_WIDTH) float64.  -> (rows (capacity, 7) float32, offsets (B+1,) int32, counts (B,) int32,
    link_counts (B, 16) int32); out = the same four preallocated (a captured step passes slot-owned buffers); rows beyond offsets[B] keep
    what they held (fresh: zeros)."""
    _lib.require_device(depth)
    dev = depth.device
    kind, cap_px = _depth_plane(depth)
    _byte_plane("labels", labels, cap_px, none="refused")
    B = _geom_table(geom, scene, _SCENE_TABLE)
    if out is None:
        capacity = cap_px if capacity is None else int(capacity)
        out = (torch.zeros((capacity, 7), dtype=torch.float32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev),
               torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B, SCENE_MAX_LINKS), dtype=torch.int32, device=dev))
    rows, offsets, counts, link_counts = out
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 7 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous (capacity, 7) float32 tensor")
    if link_counts.dtype != torch.int32 or tuple(link_counts.shape) != (B, SCENE_MAX_LINKS) or not link_counts.is_contiguous():
        raise ValueError("link_counts must be a contiguous (B, %d) int32 tensor" % SCENE_MAX_LINKS)
    if scratch is None:
        scratch = torch.empty((max(1, B) * MAX_CHUNKS * SCENE_MAX_LINKS,), dtype=torch.int32, device=dev)
    else:
        _scratch_size(scratch, B * MAX_CHUNKS * SCENE_MAX_LINKS)
    _lib.require_cuda(labels, geom, scene, rows, offsets, counts, link_counts, scratch)
    _lib.call("ancsh_depth_annotate_stream", B, kind, _lib.ptr(depth), _lib.ptr(labels), cap_px, _lib.ptr(geom),
              _lib.ptr(scene), _lib.ptr(rows), int(rows.shape[0]), _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(link_counts),
              _lib.ptr(scratch))
    return rows, offsets, counts, link_counts


def annotate_depth_batch(frames, scenes, depth_dtype, K, device="cuda:0"):
    """Eager wrapper, next to unproject_depth_batch: a batch of annotated depth frames (check_annotated_frames) -> (rows7 (offsets[n], 7)
    float32 [x y z | cx cy cz | part], offsets (n + 1,) int32, counts (n,) int32, link_counts (n, 16) int32) as numpy arrays: frame b's
    rows are rows7[offsets[b]:offsets[b] + counts[b]], link-major in parts_map's order as dataset.pack_annotated_cloud packs them; a frame
    without rows (no valid pixel, or a used link below the scene's minimum) owns one NaN row and counts 0.  One host sync; the streaming
    pipeline (AncshPipeline.submit_depth with scene=) has none."""
    dev = _lib.cuda_device(device)
    depths, labels, origins, _, scenes = check_annotated_frames(frames, np.ones(len(frames)) if isinstance(frames, (list, tuple)) else None,
                                                                scenes, depth_dtype, K)
    _, total, (d_pix, d_lab, d_geom) = _stage_frames(depths, labels, origins, check_depth_dtype(depth_dtype), dev, NOT_OBJECT)
    rows, off, cnt, lc = depth_annotate(d_pix, d_lab, d_geom, torch.from_numpy(scenes).to(dev), capacity=total + len(depths))
    off = off.cpu().numpy()
    return rows[:int(off[-1])].cpu().numpy(), off, cnt.cpu().numpy(), lc.cpu().numpy()


# ---- a depth sensor's defects on the crops of annotated frames: noise, holes, edge dropout, disparity steps (ancsh_depth_sensor_model) ---
SENSOR_WIDTH = 16       # include/ancsh_hip.h, ANCSH_SENSOR_WIDTH


def check_sensor(table):
    """-> table as a fresh (SENSOR_WIDTH,) float64 array; ValueError unless it is one the device entry is meant for: sigma's coefficients
    a0 a1 a2 and edge_rel finite and >= 0, z0 finite, p_hole and p_edge in [0, 1], qd finite and >= 0, steps finite and >= 1, z_near finite,
    z_near <= z_far (z_far may be +inf), the reserved values 0."""
    try:
        t = np.array(table, np.float64)
    except (TypeError, ValueError):
        t = np.zeros(0)
    if t.shape != (SENSOR_WIDTH,):
        raise ValueError("sensor: one (%d,) float64 table (depth.pack_sensor), got shape %s" % (SENSOR_WIDTH, t.shape))
    a0, a1, a2, z0, p_hole, p_edge, edge_rel, qd, steps, z_near, z_far = t[:11].tolist()
    for name, v in (("sigma a0", a0), ("sigma a1", a1), ("sigma a2", a2), ("edge_rel", edge_rel), ("disparity qd", qd)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("sensor: %s must be finite and >= 0, got %r" % (name, v))
    if not np.isfinite(z0):
        raise ValueError("sensor: z0 must be finite, got %r" % z0)
    for name, v in (("p_hole", p_hole), ("p_edge", p_edge)):
        if not 0.0 <= v <= 1.0:
            raise ValueError("sensor: %s is a probability in [0, 1], got %r" % (name, v))
    if not (np.isfinite(steps) and steps >= 1):
        raise ValueError("sensor: disparity steps per pixel must be finite and >= 1, got %r" % steps)
    if not (np.isfinite(z_near) and z_near <= z_far):
        raise ValueError("sensor: z_range needs a finite z_near <= z_far (z_far may be inf), got (%r, %r)" % (z_near, z_far))
    if (t[11:] != 0).any():
        raise ValueError("sensor: the reserved values 11..15 must be 0")
    return t


def pack_sensor(sigma=(0.0, 0.0, 0.0), z0=0.0, p_hole=0.0, p_edge=0.0, edge_rel=0.05, disparity=None, z_range=(0.0, float("inf"))):
    """The sensor table ancsh_depth_sensor_model reads, (SENSOR_WIDTH,) float64 (include/ancsh_hip.h): sigma = (a0, a1, a2), the noise's
    standard deviation sigma(z) = a0 + a1 (z - z0) + a2 (z - z0)^2 in the cloud's length unit; p_hole: the share of surface pixels that
    drop out; p_edge: the share of pixels at a depth discontinuity (a neighbour that is no surface, or |z_n - z| > edge_rel * z) that drop
    out; disparity = None or (qd, steps): depth quantised to 1 / steps of a pixel of disparity, qd = focal length x baseline in length
    units x pixels; z_range = (z_near, z_far): what the sensor sees at all.  The defaults are the identity.  ValueError: check_sensor's."""
    try:
        a0, a1, a2 = (float(v) for v in sigma)
        qd, steps = (0.0, 1.0) if disparity is None else (float(v) for v in disparity)
        z_near, z_far = (float(v) for v in z_range)
        head = [a0, a1, a2, float(z0), float(p_hole), float(p_edge), float(edge_rel), qd, steps, z_near, z_far]
    except (TypeError, ValueError):
        raise ValueError("sensor: sigma = (a0, a1, a2), disparity = None or (qd, steps), z_range = (z_near, z_far), the others numbers")
    return check_sensor(head + [0.0] * (SENSOR_WIDTH - len(head)))


def depth_sensor_model(depth, labels, geom, scene, sensor, seed_or_key, out=None):
    """ancsh_depth_sensor_model on device tensors (no host sync): depth (pixel_capacity,) uint16 / float32 and labels (pixel_capacity,) uint8,
    the clean crops; geom (B, 5) int32; scene (B, SCENE_WIDTH) float64 (only depth_scale is read); sensor (SENSOR_WIDTH,) float64 on the
    device (check_sensor's table); seed_or_key: the device seed (1,) int64, or the key block (4,) int32 (ancsh_depth_sensor_model_keyed).
    -> (depth, labels) of the degraded frame; out = the same pair preallocated (a captured step passes slot-owned buffers), never the input
    pair; else pixel_capacity pixels of depth 0 / label 255.  Every pixel of every crop is written, the others keep what they held."""
    _lib.require_device(depth)
    dev = depth.device
    kind, cap_px = _depth_plane(depth)
    _byte_plane("labels", labels, cap_px, none="refused")
    B = _geom_table(geom, scene, _SCENE_TABLE)
    if sensor.dtype != torch.float64 or tuple(sensor.shape) != (SENSOR_WIDTH,) or not sensor.is_contiguous():
        raise ValueError("sensor must be a contiguous (%d,) float64 tensor (depth.pack_sensor's table)" % SENSOR_WIDTH)
    keyed = seed_or_key.dtype == torch.int32
    if not ((keyed and tuple(seed_or_key.shape) == (4,)) or (seed_or_key.dtype == torch.int64 and tuple(seed_or_key.shape) == (1,))) \
            or not seed_or_key.is_contiguous():
        raise ValueError("seed_or_key must be the device seed (1,) int64 or the key block (4,) int32")
    if out is None:
        out = (torch.zeros((cap_px,), dtype=depth.dtype, device=dev), torch.full((cap_px,), NOT_OBJECT, dtype=torch.uint8, device=dev))
    depth_out, labels_out = out
    _pixel_pair("out", "input's", depth_out, labels_out, depth.dtype, cap_px)
    _lib.require_cuda(labels, geom, scene, sensor, seed_or_key, depth_out, labels_out)
    _lib.call("ancsh_depth_sensor_model_keyed" if keyed else "ancsh_depth_sensor_model", B, kind, _lib.ptr(depth), _lib.ptr(labels),
              cap_px, _lib.ptr(geom), _lib.ptr(scene), _lib.ptr(sensor), _lib.ptr(seed_or_key), _lib.ptr(depth_out), _lib.ptr(labels_out))
    return depth_out, labels_out


def sensor_frames(frames, scenes, sensor, depth_dtype, seed=0, cloud_base=0, device="cuda:0"):
    """Eager wrapper: the annotated frames render_depth_frames returns and annotate_depth_batch takes -- (depth_crop (h, w) of depth_dtype,
    label_crop (h, w), (row0, col0)) -- with one scene table or one per frame (depth_scale is read), the sensor table (pack_sensor), the
    generator seed and the global index of frame 0 -> frames of the same form as the sensor would deliver them: a dropped pixel reads depth
    0 and label 255.  Frame f is keyed as frame cloud_base + f: the frames a streaming pipeline built with sensor= makes of the same batch
    with the same seed and base.  One host sync; the pipeline has none."""
    from .dataset import stream_key_words
    dev = _lib.cuda_device(device)
    table = check_sensor(sensor)
    name = check_depth_dtype(depth_dtype)
    depths, labels, origins, _, scenes = check_annotated_frames(frames, np.ones(len(frames)) if isinstance(frames, (list, tuple)) else None,
                                                                scenes, depth_dtype, SCENE_MAX_LINKS)
    cloud_base = int(cloud_base)
    if not 0 <= cloud_base or cloud_base + len(depths) >= (1 << 20):
        raise ValueError("cloud_base %d with %d frames: the global frame index must stay in [0, 2^20)" % (cloud_base, len(depths)))
    geom, _, (d_pix, d_lab, d_geom) = _stage_frames(depths, labels, origins, name, dev, NOT_OBJECT)
    t = lambda a: torch.from_numpy(a).to(dev)
    depth, labels = depth_sensor_model(d_pix, d_lab, d_geom, t(scenes), t(table), t(stream_key_words(seed, cloud_base)))
    return _cut_frames(depth.cpu().numpy(), labels.cpu().numpy(), geom, name)


# ---- annotated frames, back on the pixel grid: predicted and true part / NOCS images (ancsh_depth_annotated_images) ----------------------
GT_IMAGE_VALUES = 6    # per pixel of the ground-truth value image: [part NOCS (3) | NAOCS (3)], columns 4..9 of an 18-column row


def annotated_image_buffers(capacity, device=None):
    """(labels (capacity,) int32 -1, values (capacity, 7) float32 NaN, gt_labels (capacity,) int32 -1, gt_values (capacity, 6) float32 NaN):
    what ancsh_depth_annotated_images writes per pixel, 60 bytes a pixel.  On `device`, or (None) in pinned host memory."""
    four = (torch.full((capacity,), -1, dtype=torch.int32, device=device),
            torch.full((capacity, LABEL_VALUES), float("nan"), dtype=torch.float32, device=device),
            torch.full((capacity,), -1, dtype=torch.int32, device=device),
            torch.full((capacity, GT_IMAGE_VALUES), float("nan"), dtype=torch.float32, device=device))
    return four if device is not None else tuple(t.pin_memory() for t in four)


def depth_annotated_images(depth, labels, geom, scene, dest, offsets, counts, row_labels, row_values, gt_rows, out=None, scratch=None):
    """ancsh_depth_annotated_images on device tensors (no host sync): the inverse of depth_annotate()'s sort.  depth, labels (the link-label
    bytes), geom, scene: what depth_annotate() was given; offsets (B+1,) int32, counts (B,) int32 and scratch: what it wrote (pass the SAME
    scratch tensor to both calls: it carries the per-chunk histograms); row_labels (capacity,) int32 / row_values (capacity, 7) float32: per
    row, as dataset.raw_point_labels writes them; gt_rows (capacity, >= 10) float32: dataset.point_gt_build's 18-column rows; dest (B,)
    int32: where cloud b's h * w images start in the image buffers, < 0 = the cloud writes nothing.  -> (img_labels (image_capacity,)
    int32, img_values (image_capacity, 7) float32, img_gt_labels (image_capacity,) int32, img_gt_values (image_capacity, 6) float32); out =
    the same four preallocated (a captured step passes slot-owned buffers), else pixel_capacity elements prefilled with -1 / NaN.  A pixel
    without a row reads -1 / NaN in all four; elements of no cloud's image keep what they held."""
    _lib.require_device(depth)
    dev = depth.device
    kind, cap_px = _depth_plane(depth)
    _byte_plane("labels", labels, cap_px, none="refused")
    B = _geom_table(geom, scene, _SCENE_TABLE)
    _int_vector("dest", dest, B)
    _int_vector("offsets", offsets, B + 1)
    _int_vector("counts", counts, B)
    cap = _row_pair(("row_labels", "row_values"), row_labels, row_values)
    if gt_rows.dtype != torch.float32 or gt_rows.dim() != 2 or gt_rows.shape[0] != cap or gt_rows.shape[1] < 10 or not gt_rows.is_contiguous():
        raise ValueError("gt_rows must be a contiguous (%d, >= 10) float32 tensor (dataset.point_gt_build's rows)" % cap)
    _scratch_given(scratch, B * MAX_CHUNKS * SCENE_MAX_LINKS, "depth_annotate")
    if out is None:
        out = annotated_image_buffers(cap_px, dev)
    img_labels, img_values, img_gt_labels, img_gt_values = out
    icap = int(img_labels.shape[0]) if img_labels.dim() == 1 else -1
    if img_labels.dtype != torch.int32 or img_gt_labels.dtype != torch.int32 or img_values.dtype != torch.float32 \
            or img_gt_values.dtype != torch.float32 or icap < 0 or tuple(img_gt_labels.shape) != (icap,) \
            or tuple(img_values.shape) != (icap, LABEL_VALUES) or tuple(img_gt_values.shape) != (icap, GT_IMAGE_VALUES) \
            or not all(t.is_contiguous() for t in out):
        raise ValueError("out must be contiguous (img_labels (n,) int32, img_values (n, %d) float32, img_gt_labels (n,) int32, img_gt_values "
                         "(n, %d) float32)" % (LABEL_VALUES, GT_IMAGE_VALUES))
    _lib.require_cuda(labels, geom, scene, dest, offsets, counts, row_labels, row_values, gt_rows, scratch, *out)
    _lib.call("ancsh_depth_annotated_images", B, kind, _lib.ptr(depth), _lib.ptr(labels), cap_px, _lib.ptr(geom), _lib.ptr(scene),
              _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(scratch), _lib.ptr(row_labels), _lib.ptr(row_values), _lib.ptr(gt_rows),
              int(gt_rows.shape[1]), cap, _lib.ptr(dest), _lib.ptr(img_labels), _lib.ptr(img_values), _lib.ptr(img_gt_labels),
              _lib.ptr(img_gt_values), icap)
    return img_labels, img_values, img_gt_labels, img_gt_values


def cut_annotated_images(labels, values, gt_labels, gt_values, shapes, first=0):
    """cut_label_images for the four image buffers of annotated frames (pure numpy): labels, gt_labels (>= n,) int32, values (>= n, 7) and
    gt_values (>= n, 6) float32, shapes = the frames' (h, w) in submission order.  -> [(labels (h, w) int32, values (h, w, 7) float32,
    gt_labels (h, w) int32, gt_values (h, w, 6) float32)], fresh arrays."""
    gt_labels, gt_values = np.asarray(gt_labels), np.asarray(gt_values)
    pred = cut_label_images(labels, values, shapes, first)
    if gt_labels.dtype != np.int32 or gt_labels.shape != np.shape(labels) or gt_values.dtype != np.float32 \
            or gt_values.shape != (gt_labels.shape[0], GT_IMAGE_VALUES):
        raise ValueError("expected gt_labels (n,) int32 and gt_values (n, %d) float32 beside labels (n,)" % GT_IMAGE_VALUES)
    out, a = [], int(first)
    for (il, iv), (h, w) in zip(pred, ((int(s[0]), int(s[1])) for s in shapes)):
        out.append((il, iv, gt_labels[a:a + h * w].reshape(h, w).copy(), gt_values[a:a + h * w].reshape(h, w, GT_IMAGE_VALUES).copy()))
        a += h * w
    return out


def annotated_frame_images(frames, scenes, rigs, depth_dtype, K, norm_factors=None, P=None, npcs_pred=None, ancsh_pred=None, device="cuda:0"):
    """Eager wrapper, next to annotate_depth_batch: a batch of annotated depth frames (check_annotated_frames) and one dataset.pack_joint_rig
    table per frame -> per frame (labels (h, w) int32, values (h, w, 7) float32, gt_labels (h, w) int32, gt_values (h, w, 6) float32), aligned
    with the frame's crop: at a valid pixel the ground-truth part and [part NOCS | NAOCS] of its 18-column row (dataset.point_gt_build) and
    what dataset.raw_point_labels gives that row from the sampled points P (B, N, 3), the norm factors and the two networks' heads
    (npcs_pred, ancsh_pred); every other pixel -1 / NaN, and so every pixel of a frame without rows.  P = None: no predictions, labels and
    values are -1 / NaN everywhere.  One host sync; the streaming pipeline (annotated_images=True) has none."""
    from .dataset import DENSE_VALUES, NCHAN, check_rigs, point_gt_build, raw_point_labels
    dev = _lib.cuda_device(device)
    n = len(frames) if isinstance(frames, (list, tuple)) else 0
    depths, labels, origins, nf, scenes = check_annotated_frames(frames, np.ones(n) if norm_factors is None else norm_factors, scenes,
                                                                 depth_dtype, K)
    rigs = check_rigs(rigs, len(depths), K)
    _, total, (d_pix, d_lab, d_geom) = _stage_frames(depths, labels, origins, check_depth_dtype(depth_dtype), dev, NOT_OBJECT)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_scene = t(scenes)
    cap = total + len(depths)
    scratch = torch.empty((len(depths) * MAX_CHUNKS * SCENE_MAX_LINKS,), dtype=torch.int32, device=dev)
    rows7, off, cnt, _ = depth_annotate(d_pix, d_lab, d_geom, d_scene, capacity=cap, scratch=scratch)
    rows18 = point_gt_build(rows7, off, t(rigs), K, torch.zeros((cap, NCHAN), dtype=torch.float32, device=dev))
    if P is None:
        rl = (torch.full((cap,), -1, dtype=torch.int32, device=dev), torch.full((cap, DENSE_VALUES), float("nan"), dtype=torch.float32, device=dev))
    else:
        rl = raw_point_labels(rows18, off, nf, torch.as_tensor(P).to(dev), npcs_pred, ancsh_pred)
    out = depth_annotated_images(d_pix, d_lab, d_geom, d_scene, d_geom[:, 0].contiguous(), off, cnt, rl[0], rl[1], rows18, scratch=scratch)
    return cut_annotated_images(*(o.cpu().numpy() for o in out), [d.shape for d in depths])


# ---- rendered frames: articulated triangle meshes -> the depth and link-label crops above (ancsh_render_depth_labels) --------------------
RENDER_WIDTH, RENDER_HEAD, RENDER_LINK = 208, 16, 12            # include/ancsh_hip.h, ANCSH_RENDER_*
_RENDER_TABLE = ("render", RENDER_WIDTH, torch.float64)


def pack_mesh(links):
    """The mesh of an articulated object for ancsh_render_depth_labels.  links: per link one (vertices (v, 3), faces (f, 3)) pair -- the
    vertices in the link's model frame, the frame its world pose places (tools/render_synthetic.py loads one mesh per link) -- or None for
    a link without geometry; at most 16 links.  -> (verts (V, 3) float32, tris (T, 3) int32 -- indices into verts --, tri_link (T,) int32),
    contiguous; ValueError on a non-finite vertex, a face index out of range or more than 16 links."""
    if not isinstance(links, (list, tuple)) or len(links) > SCENE_MAX_LINKS:
        raise ValueError("links: a list of at most %d (vertices, faces) pairs or None, one per link" % SCENE_MAX_LINKS)
    verts, tris, tri_link, base = [], [], [], 0
    for l, link in enumerate(links):
        if link is None:
            continue
        try:
            v, f = link
            v, f = np.asarray(v, np.float64), np.asarray(f)
        except (TypeError, ValueError):
            raise ValueError("link %d: expected (vertices (v, 3), faces (f, 3)) or None" % l)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or (f.size and not np.issubdtype(f.dtype, np.integer)):
            raise ValueError("link %d: expected vertices (v, 3) and integer faces (f, 3), got %s and %s %s" % (l, v.shape, f.dtype, f.shape))
        with np.errstate(over="ignore"):
            v32 = v.astype(np.float32)
        if not np.isfinite(v32).all():
            raise ValueError("link %d: every vertex must be finite in float32" % l)
        if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
            raise ValueError("link %d: a face names a vertex outside [0, %d)" % (l, v.shape[0]))
        verts.append(v32)
        tris.append(f.astype(np.int64) + base)
        tri_link.append(np.full(f.shape[0], l, np.int32))
        base += v.shape[0]
    cat = lambda parts, shape, dtype: np.ascontiguousarray(np.concatenate(parts).astype(dtype)) if parts else np.zeros(shape, dtype)
    verts, tris, tri_link = cat(verts, (0, 3), np.float32), cat(tris, (0, 3), np.int32), cat(tri_link, (0,), np.int32)
    if verts.shape[0] >= (1 << 24) or tris.shape[0] >= (1 << 24):
        raise ValueError("a mesh holds fewer than 2^24 vertices and triangles, got %d and %d" % (verts.shape[0], tris.shape[0]))
    return verts, tris, tri_link


LIBRARY_MAX_INSTANCES = 4096                                            # include/ancsh_hip.h, ANCSH_LIBRARY_MAX_INSTANCES


def pack_mesh_library(meshes):
    """A library of object instances for the *_lib entries (include/ancsh_hip.h): meshes = 1..4096 pack_mesh results, or link lists as
    pack_mesh takes them.  -> (verts (V, 3) float32, tris (T, 3) int32 with GLOBAL vertex indices -- each instance's base added --, tri_link
    (T,) int32, tri_off (ninst + 1,) int32: instance i owns triangles [tri_off[i], tri_off[i + 1])), contiguous.  ValueError when a face
    names a vertex outside its own instance, for more than 4096 instances or 2^24 or more vertices or triangles in all (found from the
    shapes, before anything is concatenated)."""
    if not isinstance(meshes, (list, tuple)) or not 1 <= len(meshes) <= LIBRARY_MAX_INSTANCES:
        raise ValueError("a mesh library holds 1..%d instances (depth.pack_mesh results or link lists), got %s"
                         % (LIBRARY_MAX_INSTANCES, len(meshes) if isinstance(meshes, (list, tuple)) else type(meshes).__name__))
    packed = []
    for i, m in enumerate(meshes):
        is_packed = isinstance(m, tuple) and len(m) == 3 and all(isinstance(a, np.ndarray) for a in m) and m[0].ndim == 2 and m[2].ndim == 1
        try:
            v, t, tl = m if is_packed else pack_mesh(m)
        except ValueError as e:
            raise ValueError("instance %d: %s" % (i, e))
        if v.ndim != 2 or v.shape[1:] != (3,) or t.ndim != 2 or t.shape[1:] != (3,) or tl.shape != (t.shape[0],):
            raise ValueError("instance %d: expected depth.pack_mesh's (verts (V, 3), tris (T, 3), tri_link (T,)), got shapes %s, %s, %s"
                             % (i, v.shape, t.shape, tl.shape))
        packed.append((v, t, tl))
    V, T = sum(v.shape[0] for v, _, _ in packed), sum(t.shape[0] for _, t, _ in packed)
    if V >= (1 << 24) or T >= (1 << 24):
        raise ValueError("a mesh library holds fewer than 2^24 vertices and triangles in all, got %d and %d" % (V, T))
    verts, tris, tri_link, tri_off, base = [], [], [], [0], 0
    for i, (v, t, tl) in enumerate(packed):
        if t.size and (t.min() < 0 or t.max() >= v.shape[0]):
            raise ValueError("instance %d: a face names a vertex outside its own instance's [0, %d)" % (i, v.shape[0]))
        if tl.size and (tl.min() < 0 or tl.max() >= SCENE_MAX_LINKS):
            raise ValueError("instance %d: a triangle's link must be in [0, %d)" % (i, SCENE_MAX_LINKS))
        verts.append(np.asarray(v, np.float32))
        tris.append(t.astype(np.int64) + base)
        tri_link.append(np.asarray(tl, np.int32))
        base += v.shape[0]
        tri_off.append(tri_off[-1] + t.shape[0])
    cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate(parts).astype(dtype))
    return cat(verts, np.float32).reshape(-1, 3), cat(tris, np.int32).reshape(-1, 3), cat(tri_link, np.int32), np.asarray(tri_off, np.int32)


def pack_render_scene(viewMat, projMat, link_world_pos, link_world_orn, height, width, depth_scale=1.0, z_min=1e-6, instance=0):
    """One frame's render table (RENDER_WIDTH,) float64 for ancsh_render_depth_labels (include/ancsh_hip.h has its layout), from
    pack_frame_scene's arguments with its conventions: the inverse of what that table makes ancsh_depth_annotate_stream do.  P is the
    inverse of the affine pixel -> (s, t) map of coord_unprojection_from_projmat(projMat, height, width); R_l is the inverse of the 4 x 4
    G_l = cam2world @ pinv(model2world_l.T) pack_frame_scene composes for row vectors, stored in column form: R_l (v, 1) is the camera
    point (x', y', z) of model point v, and M_l of the frame's scene applied to it is canon2urdf_l v.  instance: the frame's instance of a
    mesh library (pack_mesh_library), an integer in [0, 4096), written to the table's value 9; 0 for a single mesh."""
    V, Pm = np.asarray(viewMat, np.float64), np.asarray(projMat, np.float64)
    if V.shape != (4, 4):
        raise ValueError("viewMat must be (4, 4), got %s" % (V.shape,))
    pos, orn, L = _link_poses(link_world_pos, link_world_orn)
    depth_scale, z_min = float(depth_scale), float(z_min)
    if not (np.isfinite(depth_scale) and depth_scale > 0 and np.isfinite(z_min) and z_min > 0):
        raise ValueError("depth_scale and z_min must be finite and > 0, got %r and %r" % (depth_scale, z_min))
    pixel_map = _inverse_pixel_map(coord_unprojection_from_projmat(Pm, height, width))
    table = np.zeros(RENDER_WIDTH)
    table[0:6] = pixel_map
    table[6], table[7], table[8], table[9] = depth_scale, z_min, L, _instance_value(instance)
    cam2world = _cam2world(V)
    for l in range(L):
        G = cam2world @ np.linalg.pinv(_model2world(orn[l], pos[l]).T)
        table[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)] = np.linalg.inv(G).T[:3].reshape(12)
    if not np.isfinite(table).all():
        raise ValueError("the camera or a link pose is singular: the render table is not finite")
    return table


def _instance_value(instance):
    """pack_pose's / pack_render_scene's instance argument -> the float64 the table carries; ValueError unless an integer in [0, 4096)."""
    try:
        ok = int(instance) == instance and 0 <= instance < LIBRARY_MAX_INSTANCES
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("instance must be an integer in [0, %d), got %r" % (LIBRARY_MAX_INSTANCES, instance))
    return float(int(instance))


def _check_instances(what, values, ninst):
    """ValueError naming the first frame of `what` whose instance value is no integer in [0, ninst) (NaN fails every comparison)."""
    if not (isinstance(ninst, (int, np.integer)) and 1 <= ninst <= LIBRARY_MAX_INSTANCES):
        raise ValueError("ninst: a library holds 1..%d instances, got %r" % (LIBRARY_MAX_INSTANCES, ninst))
    for i, v in enumerate(values):
        if not (v >= 0 and v < ninst and v == np.floor(v)):
            raise ValueError("%s %d: the instance must be an integer in [0, %d), the library's size, got %r" % (what, i, ninst, float(v)))


def check_render_tables(render, n, ninst=None):
    """-> render as a C-contiguous (n, RENDER_WIDTH) float64 array (one table is repeated for every frame); ValueError unless every table is
    finite with depth_scale > 0, z_min > 0, an integer nlinks in 1..16 and zero reserved values.  ninst: the tables go with a mesh library of
    ninst instances, and value 9 must name one of them (None: a single mesh, value 9 is reserved and 0)."""
    a = _per_frame(render, n, RENDER_WIDTH)
    if a.shape != (n, RENDER_WIDTH):
        raise ValueError("render must be (%d, %d): one depth.pack_render_scene table, or one per frame, got shape %s" % (n, RENDER_WIDTH, a.shape))
    a = np.ascontiguousarray(a)
    if ninst is not None:
        _check_instances("render table", a[:, 9], ninst)
    if not np.isfinite(a).all():
        raise ValueError("render: every value must be finite")
    first = 9 if ninst is None else 10                                  # value 9: reserved for a single mesh, the instance of a library
    for i, t in enumerate(a):
        if not (t[6] > 0 and t[7] > 0) or t[8] != np.floor(t[8]) or not 1 <= t[8] <= SCENE_MAX_LINKS or (t[first:RENDER_HEAD] != 0).any():
            raise ValueError("render table %d: depth_scale and z_min must be > 0, nlinks an integer in [1, %d] and the reserved values 0"
                             % (i, SCENE_MAX_LINKS))
    return a


def check_crops(crops, max_frames=None):
    """-> (shapes [(h, w)], origins (n, 2) int32) of 1..max_frames crops (h, w, (row0, col0)) to render; ValueError otherwise (the limits
    are check_depth_frames')."""
    if not isinstance(crops, (list, tuple)) or not 1 <= len(crops) <= (max_frames or 65535):
        raise ValueError("crops: a list of 1..%d (h, w, (row0, col0)) tuples" % (max_frames or 65535))
    shapes, origins = [], []
    for i, c in enumerate(crops):
        try:
            h, w, (r0, c0) = c
            ok = all(int(v) == v for v in (h, w, r0, c0)) and h >= 1 and w >= 1 and abs(r0) < (1 << 24) and abs(c0) < (1 << 24) \
                and r0 + h <= (1 << 24) and c0 + w <= (1 << 24) and h * w < (1 << 30)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("crop %d: expected (h, w, (row0, col0)), integers, h and w >= 1, image rows / columns below 2^24, got %r" % (i, c))
        shapes.append((int(h), int(w)))
        origins.append((int(r0), int(c0)))
    return shapes, np.asarray(origins, np.int32).reshape(len(shapes), 2)


def pack_crop_geometry(shapes, origins, geom, first=0):
    """pack_depth_frames' geometry rows for crops that have no pixels yet: geom (n, 5) int32 {start, h, w, row0, col0}, crop k at pixel
    `first` + the pixels of the crops before it.  -> the pixel after the last crop."""
    a = int(first)
    for k, (h, w) in enumerate(shapes):
        geom[k] = (a, h, w, origins[k][0], origins[k][1])
        a += h * w
    return a


class DeviceMesh(tuple):
    """mesh_to_device's result: the 5-tuple (verts, tris, tri_link, V, T) the operators have always taken.  A mesh library carries three more
    attributes: tri_off, the (ninst + 1,) int32 device tensor; host_tri_off, its host copy; Tmax, the largest instance's triangle count, which
    sizes the raster grid without a device read.  A single mesh has tri_off = None and ninst = None."""
    tri_off = host_tri_off = ninst = None
    Tmax = 0


def is_mesh_library(mesh):
    """True for pack_mesh_library's 4-tuple and for its mesh_to_device form."""
    return (isinstance(mesh, DeviceMesh) and mesh.tri_off is not None) or (not isinstance(mesh, DeviceMesh) and isinstance(mesh, (list, tuple))
                                                                         and len(mesh) == 4)


def mesh_to_device(mesh, device):
    """pack_mesh's arrays on the device, as render_depth takes them: (verts, tris, tri_link, V, T); an empty array still owns one element of
    memory (the entry refuses null pointers).  pack_mesh_library's 4-tuple gives a library (DeviceMesh: the same 5-tuple with tri_off, a host
    copy of it, ninst and Tmax beside it); tri_off must be non-decreasing from 0 to T over 1..4096 instances."""
    if not isinstance(mesh, (list, tuple)) or len(mesh) not in (3, 4):
        raise ValueError("a mesh is depth.pack_mesh's 3 arrays or depth.pack_mesh_library's 4")
    verts, tris, tri_link = mesh[:3]
    verts, tris, tri_link = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32), np.ascontiguousarray(tri_link, np.int32)
    if verts.ndim != 2 or verts.shape[1] != 3 or tris.ndim != 2 or tris.shape[1] != 3 or tri_link.shape != (tris.shape[0],):
        raise ValueError("a mesh is depth.pack_mesh's (verts (V, 3), tris (T, 3), tri_link (T,)), got shapes %s, %s, %s"
                         % (verts.shape, tris.shape, tri_link.shape))
    V, T = verts.shape[0], tris.shape[0]
    if T and (tris.min() < 0 or tris.max() >= V or tri_link.min() < 0 or tri_link.max() >= SCENE_MAX_LINKS):
        raise ValueError("a mesh's triangles name vertices in [0, %d) and links in [0, %d)" % (V, SCENE_MAX_LINKS))
    up = lambda a, shape: torch.from_numpy(a if a.size else np.zeros(shape, a.dtype)).to(device)
    out = DeviceMesh((up(verts, (1, 3)), up(tris, (1, 3)), up(tri_link, (1,)), V, T))
    if len(mesh) == 4:
        off = np.asarray(mesh[3])
        if off.ndim != 1 or not 2 <= off.shape[0] <= LIBRARY_MAX_INSTANCES + 1 or not np.issubdtype(off.dtype, np.integer) or off[0] != 0 \
                or off[-1] != T or (np.diff(off) < 0).any():
            raise ValueError("a mesh library's tri_off is (ninst + 1,) integers for 1..%d instances, non-decreasing from 0 to T = %d, got %s"
                             % (LIBRARY_MAX_INSTANCES, T, off.tolist() if off.size <= 16 else off.shape))
        if V >= (1 << 24) or T >= (1 << 24):
            raise ValueError("a mesh library holds fewer than 2^24 vertices and triangles in all, got %d and %d" % (V, T))
        out.host_tri_off = np.ascontiguousarray(off, np.int32)
        out.tri_off = torch.from_numpy(out.host_tri_off.copy()).to(device)
        out.ninst, out.Tmax = off.shape[0] - 1, int(np.diff(off).max())
    return out


def _check_device_mesh(mesh):
    """The checks render_depth and centre_crop_origins share -> (verts, tris, tri_link, V, T, tri_off or None, ninst, Tmax)."""
    verts, tris, tri_link, V, T = mesh
    _lib.require_device(verts)
    if verts.dtype != torch.float32 or tris.dtype != torch.int32 or tri_link.dtype != torch.int32 or verts.numel() < 3 * max(V, 1) \
            or tris.numel() < 3 * max(T, 1) or tri_link.numel() < max(T, 1) or not (verts.is_contiguous() and tris.is_contiguous() and tri_link.is_contiguous()):
        raise ValueError("mesh must be depth.mesh_to_device's (verts float32, tris int32, tri_link int32, V, T), contiguous")
    tri_off = getattr(mesh, "tri_off", None)
    if tri_off is None:
        return verts, tris, tri_link, V, T, None, None, 0
    ninst, Tmax = int(mesh.ninst), int(mesh.Tmax)
    if tri_off.dtype != torch.int32 or tuple(tri_off.shape) != (ninst + 1,) or not tri_off.is_contiguous() or not tri_off.is_cuda:
        raise ValueError("a mesh library's tri_off must be depth.mesh_to_device's (ninst + 1,) int32 device tensor")
    return verts, tris, tri_link, V, T, tri_off, ninst, Tmax


def render_depth(mesh, geom, render, depth_dtype, out=None, scratch=None, pixel_capacity=None):
    """ancsh_render_depth_labels on device tensors (no host sync): mesh = mesh_to_device's (verts, tris, tri_link, V, T), geom (B, 5) int32,
    render (B, RENDER_WIDTH) float64.  A mesh library (mesh_to_device of pack_mesh_library's arrays) goes through
    ancsh_render_depth_labels_lib: frame b draws the instance its table's value 9 names.  -> (depth (pixel_capacity,) int16 bits of uint16 / float32, labels (pixel_capacity,) uint8); out =
    the same pair preallocated (a captured step passes slot-owned buffers), else pixel_capacity pixels of depth 0 / label 255; scratch: the
    (pixel_capacity,) int64 z-buffer.  Every pixel of every crop is written, the others keep what they held."""
    name = check_depth_dtype(depth_dtype)
    tt = DEPTH_DTYPES[name][1]
    verts, tris, tri_link, V, T, tri_off, ninst, Tmax = _check_device_mesh(mesh)
    dev = verts.device
    B = _geom_table(geom, render, _RENDER_TABLE)
    if out is None:
        if pixel_capacity is None:
            raise ValueError("render_depth needs out=(depth, labels) or pixel_capacity")
        out = (torch.zeros((int(pixel_capacity),), dtype=tt, device=dev), torch.full((int(pixel_capacity),), NOT_OBJECT, dtype=torch.uint8, device=dev))
    depth, labels = out
    kind, cap_px = _depth_plane(depth, name)
    _byte_plane("labels", labels, cap_px)
    if scratch is None:
        scratch = torch.empty((max(1, cap_px),), dtype=torch.int64, device=dev)
    else:
        _scratch_size(scratch, cap_px, torch.int64)
    _lib.require_cuda(tris, tri_link, geom, render, depth, labels, scratch)
    if tri_off is not None:                # a library: the instance of a frame is its table's value 9
        _lib.call("ancsh_render_depth_labels_lib", B, kind, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), int(V), int(T), _lib.ptr(tri_off),
                  ninst, Tmax, _lib.ptr(geom), _lib.ptr(render), _lib.ptr(depth), _lib.ptr(labels), _lib.ptr(scratch), cap_px)
        return depth, labels
    _lib.call("ancsh_render_depth_labels", B, kind, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), int(V), int(T), _lib.ptr(geom),
              _lib.ptr(render), _lib.ptr(depth), _lib.ptr(labels), _lib.ptr(scratch), cap_px)
    return depth, labels


def render_depth_frames(mesh, render_scenes, crops, depth_dtype, device="cuda:0"):
    """Eager wrapper: mesh = pack_mesh's arrays (or pack_mesh_library's: each table's value 9 names its frame's instance), render_scenes =
    one pack_render_scene table or one per crop, crops = a list of (h, w, (row0, col0)) -> a list of (depth_crop (h, w) of depth_dtype, label_crop (h, w) uint8, (row0, col0)): exactly the frames
    AncshPipeline.submit_depth(..., scene=, rig=) and annotate_depth_batch take.  One host sync; the streaming pipeline
    (AncshPipeline.submit_render) has none, and no pixel of it ever reaches the host."""
    dev = _lib.cuda_device(device)
    name = check_depth_dtype(depth_dtype)
    shapes, origins = check_crops(crops)
    d_mesh = mesh_to_device(mesh, dev)
    tables = check_render_tables(render_scenes, len(shapes), d_mesh.ninst)
    geom = np.zeros((len(shapes), GEOM_WORDS), np.int32)
    total = pack_crop_geometry(shapes, origins, geom)
    depth, labels = render_depth(d_mesh, torch.from_numpy(geom).to(dev), torch.from_numpy(tables).to(dev), name,
                                 pixel_capacity=total)
    return _cut_frames(depth.cpu().numpy(), labels.cpu().numpy(), geom, name)


_CompareFront = namedtuple("_CompareFront", "dev name mesh rec geom total tensors tables pred")


def _compare_front(mesh, render_tables, scenes, rigs, norm_factors, record, frames, depth_dtype, device):
    """The common opening of the two eager render-and-compare operators: their host arguments checked and staged.  tensors = what
    reprojection_batch and refine_batch take between the mesh and the dtype name; (tables, pred) = pose.reprojection.predicted_frames'."""
    from .dataset import check_rigs
    from .pose.reprojection import predicted_frames
    dev = _lib.cuda_device(device)
    name = check_depth_dtype(depth_dtype)
    rec = np.ascontiguousarray(record, np.float64)
    if rec.ndim != 3 or rec.shape[2] < 26 or not 1 <= rec.shape[1] <= 8:
        raise ValueError("record must be (n, K, >= 26) float64 with 1 <= K <= 8, got shape %s" % (rec.shape,))
    n, K = rec.shape[:2]
    depths, labels, origins, nf, scenes = check_annotated_frames(frames, norm_factors, scenes, depth_dtype, K)
    if len(depths) != n:
        raise ValueError("record holds %d frames, frames %d" % (n, len(depths)))
    d_mesh = mesh_to_device(mesh, dev)
    tables, rigs = check_render_tables(render_tables, n, d_mesh.ninst), check_rigs(rigs, n, K)
    geom, total, (d_pix, d_lab, d_geom) = _stage_frames(depths, labels, origins, name, dev, NOT_OBJECT)
    t = lambda a: torch.from_numpy(a).to(dev)
    return _CompareFront(dev, name, d_mesh, rec, geom, total, (t(tables), t(scenes), t(rigs), t(nf), d_geom, (d_pix, d_lab), t(rec)),
                         *predicted_frames(n, total, name, dev))


def reprojection_frames(mesh, render_tables, scenes, rigs, norm_factors, record, frames, depth_dtype, device="cuda:0"):
    """Eager render-and-compare, the operator outside the pipeline: mesh = pack_mesh's arrays (or pack_mesh_library's), render_tables and
    scenes = the frames' own tables (one of each, or one per frame), rigs = one dataset.pack_joint_rig table per frame, norm_factors = one
    finite value per frame, record = the frames' (n, K, >= 26) float64 pose records (columns 0..12 the baseline pose, 13..25 the nonlinear
    one), frames = the observed frames as render_depth_frames returns and sensor_frames degrades them: (depth_crop (h, w) of depth_dtype,
    label_crop (h, w), (row0, col0)).  -> (columns (n, K, 15) float64, pose.reprojection.COLUMN_NAMES; predicted: per frame ((depth, labels)
    under the baseline pose, (depth, labels) under the nonlinear pose), crops of the frame's own shape and origin -- the object where the fit
    put it).  The three calls of the streamed step (ancsh_reproject_scene_build, the renderer on 2 n frames, ancsh_reproject_compare_rec) on
    the same tables: a pipeline built with reprojection=True streams the same bytes.  One host sync; the pipeline has none."""
    from .pose.reprojection import REPROJECTION_WIDTH, reprojection_batch
    F = _compare_front(mesh, render_tables, scenes, rigs, norm_factors, record, frames, depth_dtype, device)
    rec, geom, total, name, pred = F.rec, F.geom, F.total, F.name, F.pred
    wide = reprojection_batch(F.mesh, *F.tensors, name, F.tables, pred)
    columns = wide[:, :, rec.shape[2]:].cpu().numpy()
    assert columns.shape == rec.shape[:2] + (REPROJECTION_WIDTH,)
    depth, plab = pred[0].cpu().numpy(), pred[1].cpu().numpy()
    views = [_cut_frames(depth, plab, geom, name, first=v * total) for v in (0, 1)]       # view v's crops lie `total` pixels further on
    return columns, [tuple(view[:2] for view in frame) for frame in zip(*views)]


def refine_frames(mesh, render_tables, scenes, rigs, norm_factors, record, frames, depth_dtype, refine, debug=False, device="cuda:0",
                  kinematics=None):
    """Eager render-and-compare ICP, the operator outside the pipeline: reprojection_frames' arguments and refine = pose.refinement.pack_refine's
    table.  Every part's two poses are refined on the observed depth: iters + 1 times ancsh_reproject_scene_build on the working poses, the
    renderer on 2 n frames and ancsh_refine_pass, then ancsh_refine_rec.  -> columns (n, K, 36) float64, pose.refinement.COLUMN_NAMES: per
    pose [R (9) | s | t (3) | cost_start | cost_best | n_used | best_pass | passes_solved]; pose.refinement.refined_record of the record with
    these columns behind it is the (n, K, 26) record of the refined poses.  debug=True: (columns, sums (iters + 1, n, K, 2, 32)), what every
    pass added up.  A table of pack_refine(silhouette=...) runs the loop with the silhouette term (ancsh_silhouette_field once, then
    ancsh_refine_pass_sil): the debug sums are then (iters + 1, n, K, 2, 36); with coverage= as well (ancsh_coverage_field behind the renderer
    in every pass, ancsh_refine_pass_cov) they are (iters + 1, n, K, 2, 40); with scale= as well (ancsh_refine_pass_scale in that entry's
    place: s is solved with R and t) they are (iters + 1, n, K, 2, 48) and column s of the result is the refined scale.  A table of pack_refine(joints=...) needs kinematics = the
    object's pack_kinematics table (a library: the stack of its instances'): ancsh_refine_joint_step runs behind every pass, the best-of is
    kept per object, and debug=True returns (columns, sums, obj (iters + 1, n, 2, 8)): every pass's object rows,
    pose.refinement.OBJ_COLUMNS.  A pipeline built with refine= streams the same bytes.  One host sync; the pipeline has none."""
    from .pose.refinement import REFINE_WIDTH, check_refine_table, has_coverage, has_joints, has_scale, has_silhouette, refine_batch, \
        refine_buffers
    table = check_refine_table(refine)
    iters = int(table[0])
    if has_joints(table) and kinematics is None:
        raise ValueError("refine=<pose.refinement.pack_refine(joints=...)> solves an object's parts together through the joints of its "
                         "kinematic table: it needs kinematics=<depth.pack_kinematics(...)>")
    F = _compare_front(mesh, render_tables, scenes, rigs, norm_factors, record, frames, depth_dtype, device)
    rec, d_mesh, dev, kin = F.rec, F.mesh, F.dev, None
    n, K = rec.shape[:2]
    if has_joints(table):
        kin = check_kinematics_library(kinematics, K) if np.ndim(kinematics) == 2 else check_kinematics(kinematics, K)
        if (kin.shape[0] if kin.ndim == 2 else None) != (d_mesh.ninst if is_mesh_library(mesh) else None):
            raise ValueError("kinematics and mesh must hold the same instances (a library: the np.stack of its instances' tables)")
    t = lambda a: torch.from_numpy(a).to(dev)
    buffers = refine_buffers(n, K, dev, passes=iters + 1 if debug else 1, silhouette=has_silhouette(table), joints=kin is not None,
                             pixel_capacity=F.total, coverage=has_coverage(table), scale=has_scale(table))
    wide = refine_batch(d_mesh, *F.tensors, F.name, F.tables, F.pred, t(table), iters, buffers, kin=None if kin is None else t(kin))
    columns = wide[:, :, rec.shape[2]:].cpu().numpy()
    assert columns.shape == (n, K, REFINE_WIDTH)
    if not debug:
        return columns
    return (columns, buffers.sums.cpu().numpy()) + ((buffers.obj.cpu().numpy(),) if kin is not None else ())


# ---- posed objects: a kinematic table and joint values + a view per frame -> both tables above (ancsh_pose_scene_build), and crops centred
# on the projected object (ancsh_render_centre_crops) ---------------------------------------------------------------------------------------
KIN_WIDTH, KIN_HEAD, KIN_LINK, POSE_WIDTH = 672, 32, 40, 32             # include/ancsh_hip.h, ANCSH_KIN_* and ANCSH_POSE_WIDTH
CROP_CENTRE = -(1 << 31)                                                # ANCSH_CROP_CENTRE: row0 = col0 = this asks for a centred crop
JOINT_KINDS = {"fixed": 0, "revolute": 1, "prismatic": 2}
_RIGID_TOL = 1e-9


def _compose(A, B):
    """C = A o B of 3 x 4 rigid maps in the contract's order (include/ancsh_hip.h, ancsh_pose_scene_build)."""
    C = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            v = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
            C[i, j] = v + A[i, 3] if j == 3 else v
    return C


def _joint_motion(kind, a, q):
    """J(q) (3, 4) of a joint of `kind` about / along the unit axis a, in the contract's order."""
    J = np.eye(4)[:3].copy()
    if kind == 1:
        s, c = np.sin(q), np.cos(q)
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        for i in range(3):
            for j in range(3):
                J[i, j] = (c * (1.0 if i == j else 0.0) + s * Kx[i, j]) + ((1.0 - c) * a[i]) * a[j]
    elif kind == 2:
        J[:, 3] = q * a
    return J


def _kin_links(kin):
    """(nlinks, the (nlinks, KIN_LINK) view of a kinematic table's links)."""
    L = int(kin[14])
    return L, kin[KIN_HEAD:KIN_HEAD + KIN_LINK * L].reshape(L, KIN_LINK)


def _is_rotation(R):
    return np.isfinite(R).all() and np.abs(R @ R.T - np.eye(3)).max() <= _RIGID_TOL and np.linalg.det(R) > 0


def pack_kinematics(projMat, height, width, parents, joint_kinds, joint_xyz, joint_rpy, joint_axis, urdf_link_xyz, urdf_link_rpy,
                    urdf_joint_xyz, parts_map, depth_scale=1.0, z_min=1e-6, min_link_pixels=10, base=None):
    """An object's kinematic table (KIN_WIDTH,) float64 for ancsh_pose_scene_build (include/ancsh_hip.h has its layout): the camera of
    pack_frame_scene and pack_render_scene (projMat, height, width, depth_scale, z_min, min_link_pixels), the tree -- parents (L,): -1 for
    link 0, the only root, otherwise < l; joint_kinds (L,): "fixed" | "revolute" | "prismatic" or 0 | 1 | 2; joint_xyz, joint_rpy (L, 3): the
    URDF origin of the joint that carries link l, from the parent link's frame to link l's at q = 0; joint_axis (L, 3): its axis in link l's
    frame, normalised here (link 0's three rows are not read) -- and what pack_frame_scene reads per link: urdf_link_xyz, urdf_link_rpy,
    urdf_joint_xyz (the `link == 1 and L == 2` offset rule included) and parts_map.  base: link 0's world pose, (4, 4) or (3, 4) rigid; None =
    the identity, the reference's.  ValueError for a zero axis on a moving joint, a parent that is not < l, more than 16 links, a
    non-finite value."""
    P = np.asarray(projMat, np.float64)
    parents = np.asarray(parents).reshape(-1)
    L = parents.shape[0]
    if not 1 <= L <= SCENE_MAX_LINKS:
        raise ValueError("an object has 1..%d links, got %d" % (SCENE_MAX_LINKS, L))
    if parents[0] != -1 or any(not (0 <= parents[l] < l and int(parents[l]) == parents[l]) for l in range(1, L)):
        raise ValueError("parents: -1 for link 0, the only root; every other link's parent is an integer in [0, l), got %s" % (parents.tolist(),))
    try:
        kinds = [JOINT_KINDS[k] if isinstance(k, str) else int(k) for k in joint_kinds]
    except (KeyError, TypeError, ValueError):
        kinds = []
    if len(kinds) != L or any(k not in (0, 1, 2) for k in kinds):
        raise ValueError("joint_kinds: one of %s (or 0 | 1 | 2) per link, got %r" % (sorted(JOINT_KINDS), joint_kinds))
    jx, jr, ja = (np.asarray(v, np.float64) for v in (joint_xyz, joint_rpy, joint_axis))
    xyz, rpy = np.asarray(urdf_link_xyz, np.float64), np.asarray(urdf_link_rpy, np.float64)
    for name, v in (("joint_xyz", jx), ("joint_rpy", jr), ("joint_axis", ja), ("urdf_link_xyz", xyz), ("urdf_link_rpy", rpy)):
        if v.shape != (L, 3):
            raise ValueError("%s must be (%d, 3), got %s" % (name, L, v.shape))
        if not np.isfinite(v[1:] if name.startswith("joint_") else v).all():
            raise ValueError("%s: every value must be finite" % name)
    depth_scale, z_min = float(depth_scale), float(z_min)
    if not (np.isfinite(depth_scale) and depth_scale > 0 and np.isfinite(z_min) and z_min > 0):
        raise ValueError("depth_scale and z_min must be finite and > 0, got %r and %r" % (depth_scale, z_min))
    kin = np.zeros(KIN_WIDTH)
    kin[0:6] = unprojection_from_projmat(P, height, width)
    kin[6] = depth_scale
    C = kin[7:13] = coord_unprojection_from_projmat(P, height, width)
    kin[13], kin[14] = float(min_link_pixels), L
    kin[16:22] = _inverse_pixel_map(C)                                  # pack_render_scene's pixel map
    kin[22] = z_min
    rank = _link_ranks(parts_map, L)
    if base is None:
        T0 = np.eye(4)[:3]
    else:
        T0 = np.asarray(base, np.float64)
        if T0.shape not in ((4, 4), (3, 4)) or not np.isfinite(T0).all() or not _is_rotation(T0[:3, :3]) \
                or (T0.shape == (4, 4) and not np.array_equal(T0[3], [0, 0, 0, 1])):
            raise ValueError("base: link 0's world pose must be a rigid (4, 4) or (3, 4) matrix")
        T0 = T0[:3]
    for l in range(L):
        k = kin[KIN_HEAD + KIN_LINK * l:KIN_HEAD + KIN_LINK * (l + 1)]
        k[0], k[1] = rank.get(l, (-1, 0))
        k[2], k[3] = parents[l], kinds[l] if l else 0
        if l == 0:
            k[4:16] = T0.reshape(12)
        else:
            T = _rotation_from_rpy(*jr[l])
            T[:3, 3] = jx[l]
            k[4:16] = T[:3].reshape(12)
            n = np.linalg.norm(ja[l])
            if kinds[l] != 0:
                if not (np.isfinite(n) and n > 0):
                    raise ValueError("link %d: a %s joint needs a non-zero, finite axis, got %s"
                                     % (l, "revolute" if kinds[l] == 1 else "prismatic", ja[l].tolist()))
                k[16:19] = ja[l] / n
        offset = _canonical_offset(l, L, xyz, urdf_joint_xyz)           # pack_frame_scene's rule
        k[19:28] = _rotation_from_rpy(*rpy[l])[:3, :3].reshape(9)
        k[28:31] = offset
    if not np.isfinite(kin).all():
        raise ValueError("the camera, a joint origin or a link frame is not finite: the kinematic table is not finite")
    return kin


def check_kinematics(kin, K=None):
    """-> kin as a C-contiguous (KIN_WIDTH,) float64 array; ValueError unless it is finite, holds 1..16 links with parents < l (link 0: -1),
    joint kinds in {0, 1, 2}, unit axes on moving joints and rotations in T_l and Rc_l (all to 1e-9), depth_scale and z_min > 0, zero
    reserved values and zero links beyond nlinks; K: the ranks and parts are check_scenes' too."""
    try:
        a = np.ascontiguousarray(np.asarray(kin, np.float64))
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.shape != (KIN_WIDTH,):
        raise ValueError("kinematics: one (%d,) table (depth.pack_kinematics), got shape %s" % (KIN_WIDTH, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("kinematics: every value must be finite")
    nl = a[14]
    if nl != np.floor(nl) or not 1 <= nl <= SCENE_MAX_LINKS:
        raise ValueError("kinematics: nlinks must be an integer in [1, %d], got %r" % (SCENE_MAX_LINKS, float(nl)))
    if not (a[6] > 0 and a[22] > 0 and a[13] >= 0) or a[15] != 0 or (a[23:KIN_HEAD] != 0).any():
        raise ValueError("kinematics: depth_scale and z_min must be > 0, min_link_pixels >= 0 and the reserved values 0")
    L, links = _kin_links(a)
    if (a[KIN_HEAD + KIN_LINK * L:] != 0).any() or (links[:, 31:] != 0).any():
        raise ValueError("kinematics: links beyond nlinks and reserved values must be 0")
    for l, k in enumerate(links):
        if k[2] != (-1 if l == 0 else np.floor(k[2])) or (l and not 0 <= k[2] < l):
            raise ValueError("kinematics: link %d's parent must be %s, got %r" % (l, "-1" if l == 0 else "an integer in [0, %d)" % l, float(k[2])))
        if k[3] not in (0.0, 1.0, 2.0):
            raise ValueError("kinematics: link %d's joint kind must be 0, 1 or 2, got %r" % (l, float(k[3])))
        if l and k[3] != 0 and abs(np.linalg.norm(k[16:19]) - 1.0) > _RIGID_TOL:
            raise ValueError("kinematics: link %d's joint axis must be a unit vector, got %s" % (l, k[16:19].tolist()))
        if not _is_rotation(k[4:16].reshape(3, 4)[:, :3]) or not _is_rotation(k[19:28].reshape(3, 3)):
            raise ValueError("kinematics: link %d's T_l and Rc_l must hold rotations" % l)
    if K is not None:
        used = links[links[:, 0] != -1]
        if sorted(used[:, 0].tolist()) != list(range(len(used))) or not ((used[:, 1] >= 0) & (used[:, 1] < K) & (used[:, 1] == np.floor(used[:, 1]))).all():
            raise ValueError("kinematics: the ranks of the used links must be a permutation of 0 .. %d (-1 = not used) and their parts integers "
                             "in [0, %d), got %s and %s" % (len(used) - 1, K, links[:, 0].tolist(), links[:, 1].tolist()))
    return a


def check_kinematics_library(kin, K=None):
    """-> a library's kinematics as a C-contiguous (ninst, KIN_WIDTH) float64 array: np.stack of 1..4096 pack_kinematics tables, each of
    which passes check_kinematics (the ValueError names the instance).  All instances share K parts; their link counts may differ."""
    try:
        a = np.ascontiguousarray(np.asarray(kin, np.float64))
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.ndim != 2 or a.shape[1] != KIN_WIDTH or not 1 <= a.shape[0] <= LIBRARY_MAX_INSTANCES:
        raise ValueError("kinematics of a library: (ninst, %d) for 1..%d instances (np.stack of depth.pack_kinematics tables), got shape %s"
                         % (KIN_WIDTH, LIBRARY_MAX_INSTANCES, a.shape))
    for i, row in enumerate(a):
        try:
            check_kinematics(row, K)
        except ValueError as e:
            raise ValueError("instance %d: %s" % (i, e))
    return a


def pack_pose(q, viewMat, instance=0):
    """One frame's pose (POSE_WIDTH,) float64 for ancsh_pose_scene_build: q = up to 16 joint values, link l's at position l (link 0's and
    those of fixed joints are not read), viewMat = the (4, 4) view matrix in the `.reshape(4, 4).T` form of tools/preprocess_data.py:228
    (world -> eye), which must be rigid.  instance: the frame's instance of a library (pack_mesh_library and a stack of kinematic tables), an
    integer in [0, 4096), written to value 28; 0 for a single object.  ValueError otherwise (check_poses' rules)."""
    q = np.asarray(q, np.float64).reshape(-1)
    V = np.asarray(viewMat, np.float64)
    if q.shape[0] > SCENE_MAX_LINKS:
        raise ValueError("q holds one joint value per link, at most %d, got %d" % (SCENE_MAX_LINKS, q.shape[0]))
    if V.shape != (4, 4) or not np.array_equal(V[3], [0, 0, 0, 1]):
        raise ValueError("viewMat must be a rigid (4, 4) matrix with the last row (0, 0, 0, 1)")
    pose = np.zeros(POSE_WIDTH)
    pose[:q.shape[0]] = q
    pose[16:28] = V[:3].reshape(12)
    pose[28] = _instance_value(instance)
    return check_poses(pose, 1, LIBRARY_MAX_INSTANCES)[0]


def check_poses(pose, n, ninst=None):
    """-> pose as a C-contiguous (n, POSE_WIDTH) float64 array (one pose is repeated for every frame); ValueError unless every pose is
    finite, its view's rotation orthonormal to 1e-9 (and proper) and its reserved values 0.  ninst: the poses go with a library of ninst
    instances, and value 28 must name one of them (None: a single object, value 28 is reserved and 0)."""
    a = _per_frame(pose, n, POSE_WIDTH)
    if a.shape != (n, POSE_WIDTH):
        raise ValueError("pose must be (%d, %d): one depth.pack_pose row, or one per frame, got shape %s" % (n, POSE_WIDTH, a.shape))
    a = np.ascontiguousarray(a)
    first = 28 if ninst is None else 29                                 # value 28: reserved for a single object, the instance of a library
    if ninst is not None:
        _check_instances("pose", a[:, 28], ninst)
    if not np.isfinite(a).all():
        raise ValueError("pose: every value must be finite")
    for i, p in enumerate(a):
        if (p[first:] != 0).any() or not _is_rotation(p[16:28].reshape(3, 4)[:, :3]):
            raise ValueError("pose %d: the view matrix must be rigid (its rotation orthonormal to 1e-9) and the reserved values 0" % i)
    return a


def forward_kinematics(kin, q):
    """Every link's world pose (L, 4, 4) float64 of the object `kin` (pack_kinematics) at the joint values q (link l's at position l), in
    ancsh_pose_scene_build's own order: X_l = T_l o J_l(q_l), composed from each link upwards to the root.  Plain numpy."""
    kin = check_kinematics(kin)
    L, links = _kin_links(kin)
    qq = np.zeros(SCENE_MAX_LINKS)
    q = np.asarray(q, np.float64).reshape(-1)
    qq[:min(q.shape[0], SCENE_MAX_LINKS)] = q[:SCENE_MAX_LINKS]
    X = [_compose(k[4:16].reshape(3, 4), _joint_motion(int(k[3]) if l else 0, k[16:19], qq[l])) for l, k in enumerate(links)]
    out = np.tile(np.eye(4), (L, 1, 1))
    for l in range(L):
        W, p = X[l], int(links[l, 2])
        while p >= 0:
            W, p = _compose(X[p], W), int(links[p, 2])
        out[l, :3] = W
    return out


def pose_scene_build(kin, pose, out=None):
    """ancsh_pose_scene_build on device tensors (no host sync): kin (KIN_WIDTH,) float64, pose (B, POSE_WIDTH) float64 -> (render (B,
    RENDER_WIDTH), scene (B, SCENE_WIDTH)) float64; out = the same pair preallocated (a captured step passes slot-owned buffers).  kin (ninst,
    KIN_WIDTH), a library's stack, goes through ancsh_pose_scene_build_lib: frame b reads the table its pose's value 28 names."""
    _lib.require_device(kin)
    B = int(pose.shape[0])
    library = kin.dim() == 2               # a library's stack of tables: the instance of a frame is its pose's value 28
    if kin.dtype != torch.float64 or (tuple(kin.shape) != (KIN_WIDTH,) and not (library and kin.shape[1] == KIN_WIDTH and 1 <= kin.shape[0] <= LIBRARY_MAX_INSTANCES)) \
            or pose.dtype != torch.float64 or tuple(pose.shape) != (B, POSE_WIDTH) or not (kin.is_contiguous() and pose.is_contiguous()):
        raise ValueError("kin must be (%d,) float64 -- a library: (ninst, %d) -- and pose (B, %d) float64, contiguous" % (KIN_WIDTH, KIN_WIDTH, POSE_WIDTH))
    if out is None:
        out = (torch.empty((B, RENDER_WIDTH), dtype=torch.float64, device=kin.device), torch.empty((B, SCENE_WIDTH), dtype=torch.float64, device=kin.device))
    render, scene = out
    if render.dtype != torch.float64 or tuple(render.shape) != (B, RENDER_WIDTH) or scene.dtype != torch.float64 or tuple(scene.shape) != (B, SCENE_WIDTH) \
            or not (render.is_contiguous() and scene.is_contiguous()):
        raise ValueError("out must be (render (B, %d), scene (B, %d)) float64, contiguous" % (RENDER_WIDTH, SCENE_WIDTH))
    _lib.require_cuda(pose, render, scene)
    if library:
        _lib.call("ancsh_pose_scene_build_lib", B, _lib.ptr(kin), int(kin.shape[0]), _lib.ptr(pose), _lib.ptr(render), _lib.ptr(scene))
        return render, scene
    _lib.call("ancsh_pose_scene_build", B, _lib.ptr(kin), _lib.ptr(pose), _lib.ptr(render), _lib.ptr(scene))
    return render, scene


def pose_scene_tables(kin, poses, device="cuda:0"):
    """Eager wrapper: kin = one pack_kinematics table (or a library's (ninst, 672) stack: each pose's value 28 names its instance), poses =
    one pack_pose row or (n, 32) of them -> (render (n, 208), scene (n, 240))
    float64 numpy arrays read back from ancsh_pose_scene_build: what submit_render and render_depth_frames take.  One host sync."""
    dev = _lib.cuda_device(device)
    library = np.ndim(kin) == 2
    kin = check_kinematics_library(kin) if library else check_kinematics(kin)
    p = np.asarray(poses, np.float64)
    poses = check_poses(p, 1 if p.ndim == 1 else p.shape[0], kin.shape[0] if library else None)
    render, scene = pose_scene_build(torch.from_numpy(kin).to(dev), torch.from_numpy(poses).to(dev))
    return render.cpu().numpy(), scene.cpu().numpy()


def centre_crop_origins(mesh, geom, render, scratch=None):
    """ancsh_render_centre_crops on device tensors (no host sync): mesh = mesh_to_device's, geom (B, 5) int32, render (B, RENDER_WIDTH)
    float64; the rows of geom whose row0 and col0 both hold CROP_CENTRE get the origin that centres their crop on the projected object, in
    place.  scratch: (B, 4) int32 of working memory.  -> geom.  A mesh library goes through ancsh_render_centre_crops_lib."""
    verts, tris, tri_link, V, T, tri_off, ninst, _ = _check_device_mesh(mesh)
    B = _geom_table(geom, render, _RENDER_TABLE)
    if scratch is None:
        scratch = torch.empty((max(1, B), 4), dtype=torch.int32, device=verts.device)
    else:
        _scratch_size(scratch, 4 * B)
    _lib.require_cuda(tris, tri_link, geom, render, scratch)
    if tri_off is not None:                # a library: the block of a frame strides over its instance's triangles only
        _lib.call("ancsh_render_centre_crops_lib", B, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), int(V), int(T), _lib.ptr(tri_off), ninst,
                  _lib.ptr(render), _lib.ptr(geom), _lib.ptr(scratch))
        return geom
    _lib.call("ancsh_render_centre_crops", B, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), int(V), int(T), _lib.ptr(render),
              _lib.ptr(geom), _lib.ptr(scratch))
    return geom


def check_posed_crops(crops, max_frames=None):
    """check_crops for crops whose origin may be None = centred on the projected object -> (shapes, origins (n, 2) int32, CROP_CENTRE in
    both places of a centred crop)."""
    if not isinstance(crops, (list, tuple)):
        raise ValueError("crops: a list of (h, w, (row0, col0) or None) tuples")
    centred = [isinstance(c, (list, tuple)) and len(c) == 3 and c[2] is None for c in crops]
    shapes, origins = check_crops([(c[0], c[1], (0, 0)) if m else c for c, m in zip(crops, centred)], max_frames)
    origins[np.asarray(centred, bool)] = CROP_CENTRE
    return shapes, origins


def centre_crops(mesh, render_tables, sizes, device="cuda:0"):
    """Eager wrapper: mesh = pack_mesh's arrays (or pack_mesh_library's), render_tables = one render table or one per crop, sizes = a list of (h, w) -> the (n, 2)
    int32 origins (row0, col0) that centre each h x w crop on its frame's projected object (ancsh_render_centre_crops; (0, 0) where nothing
    projects): what submit_render's crops take.  One host sync."""
    dev = _lib.cuda_device(device)
    shapes, origins = check_posed_crops([(h, w, None) for h, w in sizes])
    d_mesh = mesh_to_device(mesh, dev)
    tables = check_render_tables(render_tables, len(shapes), d_mesh.ninst)
    geom = np.zeros((len(shapes), GEOM_WORDS), np.int32)
    pack_crop_geometry(shapes, origins, geom)
    d_geom = torch.from_numpy(geom).to(dev)
    centre_crop_origins(d_mesh, d_geom, torch.from_numpy(tables).to(dev))
    return d_geom.cpu().numpy()[:, 3:5].copy()
