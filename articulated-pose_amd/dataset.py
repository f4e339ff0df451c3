"""The sampling step in front of the network, batched on the MI355X: counterpart of
lib/dataset.py::Dataset.create_unit_data_from_hdf5 (:262-432, the part after the .h5 frame has been parsed into
per-part arrays) and of the batch assembly in Dataset.__next__ (:119-155).

Reference: per cloud, on the host -- concatenate parts, tile small clouds, np.random.permutation, one fancy-index per
array, scale by norm_factor, build the masks; then np.stack over the batch.  Here the whole ragged batch is packed once
(one 18-channel row per raw point) and ONE kernel launch (ancsh_input_sample) gathers / scales / one-hots every cloud
straight into the (B, N, .) tensors the network and the test-time losses read.  The permutation is an explicit input
(replay numpy's stream for parity) or drawn on the device.
"""
import numpy as np
import torch

from . import _lib

# channel layout of a packed raw row
_COLS = (("parts_pts", 3), ("parts_cls", 1), ("nocs_p", 3), ("nocs_g", 3), ("offset_heatmap", 1), ("offset_unitvec", 3),
         ("joint_orient", 3), ("joint_cls", 1))
NCHAN = sum(c for _, c in _COLS)
_CLS_COL, _JCLS_COL = 3, NCHAN - 1
# (record key, first output channel, width) in the (B, N, NCHAN-3) gathered tensor
_OUT = (("cls_gt", 0, 1), ("nocs_gt", 1, 3), ("nocs_gt_g", 4, 3), ("heatmap_gt", 7, 1), ("unitvec_gt", 8, 3), ("orient_gt", 11, 3),
        ("joint_cls_gt", 14, 1))


def pack_cloud(parts):
    """parts: dict keyed like create_data_shape2motion's return lists (parts_pts, parts_cls, nocs_p, nocs_g, offset_heatmap,
    offset_unitvec, joint_orient, joint_cls), each a list of per-part arrays or one concatenated array -> (n_raw, 18) float32."""
    cols = []
    for key, width in _COLS:
        v = parts[key]
        v = np.concatenate(v, axis=0) if isinstance(v, (list, tuple)) else np.asarray(v)
        cols.append(np.asarray(v, np.float32).reshape(v.shape[0], width))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def tiled_size(n_raw, num_points):
    """Rows of the cloud after the reference's tiling rule (lib/dataset.py:290-293)."""
    return n_raw if n_raw >= num_points else (int(num_points / n_raw) + 1) * n_raw


def create_unit_data_batch(clouds, num_points, norm_factors, n_parts, perms=None, seed=None, device="cuda:0"):
    """clouds: list of `parts` dicts (see pack_cloud) or packed (n_raw, 18) arrays; norm_factors: one float per cloud
    (norm_factors[0] of the instance, lib/dataset.py:346); perms: optional list of int permutations of the TILED clouds
    (np.random.permutation(tiled_size)), else drawn on the device from `seed`.
    Returns the nocs_type 'A' record (:378-391) as (B, N, .) float32 device tensors:
    P, cls_gt, mask_array, nocs_gt, nocs_gt_g, heatmap_gt, unitvec_gt, orient_gt, joint_cls_gt, joint_cls_mask."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    packed = [c if isinstance(c, np.ndarray) else pack_cloud(c) for c in clouds]
    B = len(packed)
    if B == 0:
        raise ValueError("create_unit_data_batch: empty batch")
    if any(p.ndim != 2 or p.shape[1] != NCHAN or p.shape[0] == 0 for p in packed):
        raise ValueError("every cloud must pack to a non-empty (n_raw, %d) array" % NCHAN)
    sizes = np.asarray([p.shape[0] for p in packed], np.int64)
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum(sizes)
    rows = torch.from_numpy(np.concatenate(packed, axis=0)).to(dev)
    if perms is not None:
        if len(perms) != B or any(len(p) < num_points for p in perms):
            raise ValueError("perms: one permutation of the tiled cloud (>= num_points entries) per cloud")
        # numpy's fancy index (lib/dataset.py:298-300) takes an entry in [-size, -1] as size + entry and raises IndexError outside
        # [-size, size); the kernel reads row perm % n_raw of the raw cloud, so entries are normalised / refused here
        host = []
        for p, n in zip(perms, sizes):
            p = np.asarray(p[:num_points]).astype(np.int64)
            size = tiled_size(int(n), num_points)
            if p.size and (int(p.min()) < -size or int(p.max()) >= size):
                bad = int(p.min()) if int(p.min()) < -size else int(p.max())
                raise IndexError("perms: index %d is out of bounds for the tiled cloud of %d rows" % (bad, size))
            host.append(np.where(p < 0, p + size, p))
        perm = torch.from_numpy(np.stack([p.astype(np.int32) for p in host])).to(dev)
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(0 if seed is None else int(seed))
        perm = torch.stack([torch.randperm(tiled_size(int(n), num_points), generator=g, device=dev)[:num_points].to(torch.int32)
                            for n in sizes])
    nf = torch.tensor(np.asarray(norm_factors, np.float32).reshape(B), device=dev)
    f = dict(dtype=torch.float32, device=dev)
    P = torch.empty((B, num_points, 3), **f)
    chan = torch.empty((B, num_points, NCHAN - 3), **f)
    mask_array = torch.empty((B, num_points, n_parts), **f)
    joint_cls_mask = torch.empty((B, num_points), **f)
    off = torch.from_numpy(offsets).to(dev)
    _lib.call("ancsh_input_sample", B, int(num_points), NCHAN, _lib.ptr(rows), _lib.ptr(off), _lib.ptr(perm), _lib.ptr(nf),
              _CLS_COL, _JCLS_COL, int(n_parts), _lib.ptr(P), _lib.ptr(chan), _lib.ptr(mask_array), _lib.ptr(joint_cls_mask))
    out = {"P": P, "mask_array": mask_array, "joint_cls_mask": joint_cls_mask}
    for key, c0, w in _OUT:
        out[key] = chan[:, :, c0] if w == 1 else chan[:, :, c0:c0 + w]
    return out


# ---- raw clouds for the streaming pipeline ---------------------------------------------------------------------------------
RAW_NCHAN, RAW_JCLS_COL = 4, 3      # a raw cloud row: x y z joint_cls (a pack_cloud row sliced with [:, [0, 1, 2, 17]])


def check_raw_clouds(clouds, norm_factors, max_clouds=None, xyz_only=False):
    """Validate a batch of raw clouds before anything is enqueued: 1..max_clouds non-empty (n_raw, 4) arrays and one finite
    norm factor per cloud.  -> (list of contiguous float32 (n_raw, 4) arrays, float32 (B,) norm factors); ValueError otherwise.
    xyz_only=True (a stream whose joint association comes from the network): (n_raw, 3) xyz clouds or (n_raw, 4) ones, whose 4th
    column is dropped, so one frame source drives both modes -> contiguous float32 (n_raw, 3) arrays."""
    if not isinstance(clouds, (list, tuple)):
        raise ValueError("clouds must be a list of (n_raw, %s) arrays" % ("3 or 4" if xyz_only else RAW_NCHAN))
    if not 1 <= len(clouds) <= (max_clouds or 65535):
        raise ValueError("a batch holds 1..%d clouds, got %d" % (max_clouds or 65535, len(clouds)))
    out = []
    for i, c in enumerate(clouds):
        c = np.asarray(c.cpu().numpy() if torch.is_tensor(c) else c)
        if xyz_only:
            if c.ndim != 2 or c.shape[1] not in (3, RAW_NCHAN) or c.shape[0] == 0:
                raise ValueError("cloud %d: expected a non-empty (n_raw, 3) array [x y z] (or (n_raw, 4), 4th column ignored), got shape %s"
                                 % (i, c.shape))
            out.append(np.ascontiguousarray(c[:, :3], np.float32))
            continue
        c = np.ascontiguousarray(c, np.float32)
        if c.ndim != 2 or c.shape[1] != RAW_NCHAN or c.shape[0] == 0:
            raise ValueError("cloud %d: expected a non-empty (n_raw, %d) array [x y z joint_cls], got shape %s" % (i, RAW_NCHAN, c.shape))
        out.append(c)
    nf = np.asarray(norm_factors, np.float32).reshape(-1)
    if nf.size != len(out) or not np.isfinite(nf).all():
        raise ValueError("norm_factors: one finite value per cloud (%d clouds, got %s)" % (len(out), nf.tolist()))
    return out, nf


def seed_bits(seed):
    """The uint64 generator key `seed` as the int64 with the same bits (how the device buffers hold it)."""
    return int(np.uint64(int(seed) % (1 << 64)).view(np.int64))


STREAM_KEY_PROBLEMS = 1 << 20       # (cloud_base + clouds) * K must stay below: the draw keys then keep clear of the sampler's tag bits


def check_stream_key(cloud_base, n_clouds, K):
    """Host-side bound of a key block (include/ancsh_hip.h, ancsh_stream_key): cloud_base >= 0 and (cloud_base + n_clouds) * K < 2^20,
    so no generator problem index of the launch reaches the sampler's tag bits.  -> int(cloud_base); ValueError otherwise."""
    cb = int(cloud_base)
    if cb < 0 or (cb + int(n_clouds)) * max(1, int(K)) >= STREAM_KEY_PROBLEMS:
        raise ValueError("cloud_base %d with %d clouds of %d parts: (cloud_base + clouds) * K must be in [0, 2^20)" % (cb, n_clouds, K))
    return cb


def stream_key_words(seed, cloud_base=0):
    """The 16-byte ancsh_stream_key {uint64 seed, int32 cloud_base, int32 reserved = 0} as four int32 words (how the device holds it)."""
    w = np.zeros(4, np.int32)
    w[:2].view(np.int64)[0] = seed_bits(seed)
    w[2] = int(cloud_base)
    return w


def sample_raw_batch(clouds, num_points, norm_factors, seed, device="cuda:0", return_perm=False, cloud_base=None, xyz_only=False):
    """Eager wrapper of the streaming sampler (ancsh_input_sample_stream, include/ancsh_hip.h): clouds = list of (n_raw, 4) float32
    arrays [x y z joint_cls]; cloud b's num_points rows are raw rows pi_b(i) % n_raw for the keyed bijection pi_b of the tiled cloud
    (the reference's tiling rule, tiled_size) drawn from `seed` (uint64).  cloud_base: None = the plain entry; an int = the key block
    (ancsh_input_sample_stream_keyed): cloud b is keyed as global cloud cloud_base + b.
    xyz_only=True: the xyz twins (ancsh_input_sample_stream_xyz / _xyz_keyed) on (n_raw, 3) clouds (a 4th column is dropped): the same
    P and perm, no joint_cls.
    -> dict(P (B,N,3) float32 = xyz * norm_factor, joint_cls (B,N) int32 [, perm (B,N) int32 = pi_b(i)]) on `device`."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")
    clouds, nf = check_raw_clouds(clouds, norm_factors, xyz_only=xyz_only)
    B = len(clouds)
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
    rows = torch.from_numpy(np.concatenate(clouds, axis=0)).to(dev)
    off = torch.from_numpy(offsets).to(dev)
    nf_d = torch.from_numpy(nf).to(dev)
    if cloud_base is None:
        entry, seed_d = "ancsh_input_sample_stream", torch.tensor([seed_bits(seed)], dtype=torch.int64, device=dev)
    else:
        entry = "ancsh_input_sample_stream_keyed"
        seed_d = torch.from_numpy(stream_key_words(seed, check_stream_key(cloud_base, B, 1))).to(dev)
    P = torch.empty((B, num_points, 3), dtype=torch.float32, device=dev)
    perm = torch.empty((B, num_points), dtype=torch.int32, device=dev) if return_perm else None
    if xyz_only:
        _lib.call(entry.replace("_stream", "_stream_xyz"), B, int(num_points), 3, _lib.ptr(rows), int(rows.shape[0]), _lib.ptr(off),
                  _lib.ptr(nf_d), _lib.ptr(seed_d), _lib.ptr(P), _lib.ptr(perm))
        return dict(P=P, perm=perm) if return_perm else dict(P=P)
    jcls = torch.empty((B, num_points), dtype=torch.int32, device=dev)
    _lib.call(entry, B, int(num_points), RAW_NCHAN, _lib.ptr(rows), int(rows.shape[0]), _lib.ptr(off),
              _lib.ptr(nf_d), RAW_JCLS_COL, _lib.ptr(seed_d), _lib.ptr(P), _lib.ptr(jcls), _lib.ptr(perm))
    out = dict(P=P, joint_cls=jcls)
    if return_perm:
        out["perm"] = perm
    return out


DENSE_VALUES = 7        # per raw row: [W_label | part NOCS (3) | NAOCS (3)] (include/ancsh_hip.h, ancsh_raw_point_labels)


def raw_point_labels(raw_rows, offsets, norm_factors, P, npcs_pred, ancsh_pred, out=None):
    """Part label and head values of every RAW row of a streamed batch (ancsh_raw_point_labels, one launch): the FP module's 3-NN
    inverse-distance upsampling (pointnet_util.py:219-229) from each cloud's sampled points P to its raw rows.
    raw_rows (capacity, >= 3) float32 [x y z ...], offsets (B+1,) int32 (cloud b owns rows [offsets[b], offsets[b+1])), norm_factors (B,)
    float32, P (B, N, 3) the sampled points (raw xyz * norm factor), npcs_pred / ancsh_pred the two networks' output dicts (the NPCS W and
    nocs_per_point heads, the ANCSH gocs_per_point head).  -> (labels (capacity,) int32, values (capacity, 7) float32) device tensors:
    labels = the first argmax of the interpolated W (-1 for a non-finite point or W), values = [W_label | nocs of the label's part | gocs of
    the label's part (or the 3-channel gocs)], NaN with label -1.  Rows beyond offsets[B] are left as `out` holds them (freshly allocated:
    -1 / NaN).  out = (labels, values): preallocated outputs (the captured streaming step passes slot-owned buffers); no host sync."""
    dev = P.device if torch.is_tensor(P) else torch.device("cuda:0")
    if dev.type != "cuda":
        raise RuntimeError("articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)")

    def f32(a):
        return torch.as_tensor(a).to(dev, torch.float32).contiguous()
    rows, P = f32(raw_rows), f32(P)
    off = torch.as_tensor(offsets).to(dev, torch.int32).contiguous()
    nf = f32(norm_factors).reshape(-1)
    if "gocs_per_point" not in ancsh_pred:
        raise ValueError("raw_point_labels reads the ANCSH network's gocs_per_point head (mixed_pred weights)")
    W, nocs, gocs = f32(npcs_pred["W"]), f32(npcs_pred["nocs_per_point"]), f32(ancsh_pred["gocs_per_point"])
    if P.dim() != 3 or P.shape[2] != 3 or rows.dim() != 2:
        raise ValueError("P must be (B, N, 3) and raw_rows (capacity, channels)")
    B, N = P.shape[:2]
    K = W.shape[2] if W.dim() == 3 else 0
    if tuple(W.shape) != (B, N, K) or tuple(nocs.shape) != (B, N, 3 * K) or gocs.dim() != 3 or tuple(gocs.shape[:2]) != (B, N):
        raise ValueError("heads must be W (B, N, K), nocs_per_point (B, N, 3K) and gocs_per_point (B, N, 3 or 3K) for P (B, N, 3)")
    if tuple(off.shape) != (B + 1,) or tuple(nf.shape) != (B,):
        raise ValueError("offsets must be (B+1,) and norm_factors (B,) for %d clouds" % B)
    cap = rows.shape[0]
    if out is None:
        labels = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        values = torch.full((cap, DENSE_VALUES), float("nan"), dtype=torch.float32, device=dev)
    else:
        labels, values = out
        if labels.dtype != torch.int32 or values.dtype != torch.float32 or tuple(labels.shape) != (cap,) or \
                tuple(values.shape) != (cap, DENSE_VALUES) or not (labels.is_contiguous() and values.is_contiguous()):
            raise ValueError("out must be contiguous (labels (%d,) int32, values (%d, %d) float32)" % (cap, cap, DENSE_VALUES))
    _lib.call("ancsh_raw_point_labels", B, N, K, int(gocs.shape[2]), int(rows.shape[1]), _lib.ptr(rows), cap, _lib.ptr(off),
              _lib.ptr(nf), _lib.ptr(P), _lib.ptr(W), _lib.ptr(nocs), _lib.ptr(gocs), _lib.ptr(labels), _lib.ptr(values))
    return labels, values
