"""The depth front end of the streaming pipeline: what a depth camera delivers -- a depth image, an object mask, a camera matrix -- turned
into camera-space clouds on the GPU (ancsh_depth_unproject_stream, include/ancsh_hip.h; reference: tools/preprocess_data.py:259-298).

A frame is (depth_crop (h, w), mask_crop (h, w) or None, (row0, col0)): a crop of the depth image around the object, the object's mask in
it, and the crop's origin in the full image.  A camera is six unprojection coefficients (A00 A01 A02 A10 A11 A12): the valid pixel in
image row `row`, column `col` with depth d becomes z = d * depth_scale, x = z * (A00 col + A01 row + A02), y = z * (A10 col + A11 row + A12).
The helpers below compute them in float64; they are cast to float32 once, when a batch is submitted.
"""
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
    nf = np.asarray(norm_factors, np.float32).reshape(-1)
    if nf.size != n or not np.isfinite(nf).all():
        raise ValueError("norm_factors: one finite value per frame (%d frames, got %s)" % (n, nf.tolist()))
    try:
        cam64 = np.asarray(cameras, np.float64)
    except (TypeError, ValueError):
        cam64 = np.zeros(0)
    if cam64.shape == (6,):
        cam64 = np.broadcast_to(cam64, (n, 6))
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


def depth_unproject(depth, mask, geom, cam, capacity=None, out=None, scratch=None):
    """ancsh_depth_unproject_stream on device tensors (no host sync): depth (pixel_capacity,) uint16 / float32, mask (pixel_capacity,)
    uint8 or None, geom (B, 5) int32, cam (B, 7) float32.  -> (rows (capacity, 3) float32, offsets (B+1,) int32, counts (B,) int32);
    out = the same triple preallocated (a captured step passes slot-owned buffers); rows beyond offsets[B] keep what they held (fresh:
    zeros)."""
    if not depth.is_cuda:
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    dev = depth.device
    kinds = {torch.float32: 1, torch.int16: 0}
    if hasattr(torch, "uint16"):
        kinds[torch.uint16] = 0
    if depth.dtype not in kinds or depth.dim() != 1 or not depth.is_contiguous():
        raise ValueError("depth must be a contiguous 1-d uint16 or float32 tensor")
    cap_px = int(depth.shape[0])
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (cap_px,) or not mask.is_contiguous()):
        raise ValueError("mask must be a contiguous (%d,) uint8 tensor" % cap_px)
    B = int(geom.shape[0])
    if geom.dtype != torch.int32 or tuple(geom.shape) != (B, GEOM_WORDS) or cam.dtype != torch.float32 or tuple(cam.shape) != (B, CAM_WORDS) \
            or not (geom.is_contiguous() and cam.is_contiguous()):
        raise ValueError("geom must be (B, 5) int32 and cam (B, 7) float32, contiguous")
    if out is None:
        capacity = cap_px if capacity is None else int(capacity)
        out = (torch.zeros((capacity, 3), dtype=torch.float32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev),
               torch.zeros((B,), dtype=torch.int32, device=dev))
    rows, offsets, counts = out
    if scratch is None:
        scratch = torch.empty((max(1, B) * MAX_CHUNKS,), dtype=torch.int32, device=dev)
    _lib.call("ancsh_depth_unproject_stream", B, kinds[depth.dtype], _lib.ptr(depth), _lib.ptr(mask), cap_px, _lib.ptr(geom), _lib.ptr(cam),
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
    if not depth.is_cuda:
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    dev = depth.device
    kinds = {torch.float32: 1, torch.int16: 0}
    if hasattr(torch, "uint16"):
        kinds[torch.uint16] = 0
    if depth.dtype not in kinds or depth.dim() != 1 or not depth.is_contiguous():
        raise ValueError("depth must be a contiguous 1-d uint16 or float32 tensor")
    cap_px = int(depth.shape[0])
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (cap_px,) or not mask.is_contiguous()):
        raise ValueError("mask must be a contiguous (%d,) uint8 tensor" % cap_px)
    B = int(geom.shape[0])
    if geom.dtype != torch.int32 or tuple(geom.shape) != (B, GEOM_WORDS) or not geom.is_contiguous():
        raise ValueError("geom must be (B, 5) int32, contiguous")
    for name, t, n in (("dest", dest, B), ("offsets", offsets, B + 1)):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous (%d,) int32 tensor" % (name, n))
    cap = int(labels.shape[0]) if labels.dim() == 1 else -1
    if labels.dtype != torch.int32 or values.dtype != torch.float32 or cap < 0 or tuple(values.shape) != (cap, LABEL_VALUES) \
            or not (labels.is_contiguous() and values.is_contiguous()):
        raise ValueError("labels must be (capacity,) int32 and values (capacity, %d) float32, contiguous" % LABEL_VALUES)
    if scratch is None or scratch.dtype != torch.int32 or scratch.numel() < B * MAX_CHUNKS or not scratch.is_contiguous():
        raise ValueError("scratch must be the (>= %d,) int32 tensor depth_unproject() was given" % (B * MAX_CHUNKS))
    if out is None:
        out = (torch.full((cap_px,), -1, dtype=torch.int32, device=dev),
               torch.full((cap_px, LABEL_VALUES), float("nan"), dtype=torch.float32, device=dev))
    img_labels, img_values = out
    icap = int(img_labels.shape[0]) if img_labels.dim() == 1 else -1
    if img_labels.dtype != torch.int32 or img_values.dtype != torch.float32 or icap < 0 or tuple(img_values.shape) != (icap, LABEL_VALUES) \
            or not (img_labels.is_contiguous() and img_values.is_contiguous()):
        raise ValueError("out must be contiguous (img_labels (n,) int32, img_values (n, %d) float32)" % LABEL_VALUES)
    if any(not t.is_cuda for t in (geom, dest, offsets, labels, values, scratch, img_labels, img_values)) or (mask is not None and not mask.is_cuda):
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    _lib.call("ancsh_depth_label_images", B, kinds[depth.dtype], _lib.ptr(depth), _lib.ptr(mask), cap_px, _lib.ptr(geom), _lib.ptr(offsets),
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
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    depths, masks, origins, _, cam = check_depth_frames(frames, np.ones(len(frames)) if isinstance(frames, (list, tuple)) else None,
                                                        cameras, depth_scale, depth_dtype)
    name = check_depth_dtype(depth_dtype)
    total = sum(d.size for d in depths)
    pix, mask, geom = np.zeros(total, DEPTH_DTYPES[name][0]), np.zeros(total, np.uint8), np.zeros((len(depths), GEOM_WORDS), np.int32)
    pack_depth_frames(depths, masks, origins, pix, mask, geom)
    d_pix = torch.from_numpy(pix.view(np.int16) if name == "uint16" else pix).to(dev)
    rows, off, cnt = depth_unproject(d_pix, torch.from_numpy(mask).to(dev), torch.from_numpy(geom).to(dev), torch.from_numpy(cam).to(dev))
    rows, off, cnt = rows.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    return [rows[off[b]:off[b + 1]].copy() for b in range(len(depths))], cnt
