"""The sampling step in front of the network, batched on the MI355X: counterpart of
lib/dataset.py::Dataset.create_unit_data_from_hdf5 (:262-432, the part after the .h5 frame has been parsed into
per-part arrays) and of the batch assembly in Dataset.__next__ (:119-155).

Reference: per cloud, on the host -- concatenate parts, tile small clouds, np.random.permutation, one fancy-index per
array, scale by norm_factor, build the masks; then np.stack over the batch.  Here the whole ragged batch is packed once
(one 18-channel row per raw point) and ONE kernel launch (ancsh_input_sample) gathers / scales / one-hots every cloud
straight into the (B, N, .) tensors the network and the test-time losses read.  The permutation is an explicit input
(replay numpy's stream for parity) or drawn on the device.

The per-part arrays themselves -- create_data_shape2motion / create_data_mobility (:434-700) behind their two h5py lookups -- are built on
the GPU too: pack_annotated_cloud / pack_joint_rig / build_point_gt_rows below (ancsh_point_gt_build).
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
    dev = _lib.cuda_device(device)
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
    dev = _lib.cuda_device(device)
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
    dev = _lib.cuda_device(P.device if torch.is_tensor(P) else "cuda:0")

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


# ---- the per-point ground truth from annotated clouds (ancsh_point_gt_build) ------------------------------------------------------------
ANNOTATED_NCHAN = 7                 # an annotated row: x y z | c (3) | part
ANNOTATED_COLUMNS = "x y z | cx cy cz | part"
MAX_RIG_PARTS = 8
# the rig's layout (include/ancsh_hip.h, ancsh_point_gt_build)
_RIG_ROT, _RIG_GMAP, _RIG_HEAD, _RIG_ENTRY = 4, 13, 22, 9
RIG_DATASETS = ("shape2motion", "sapien")


def _rig_part(K):
    return 15 + _RIG_ENTRY * K


def RIG_WIDTH(K):
    """float64 values of one cloud's rig for K parts (ANCSH_RIG_WIDTH); ValueError for K outside 1..8."""
    K = int(K)
    if not 1 <= K <= MAX_RIG_PARTS:
        raise ValueError("a rig holds 1..%d parts, got K=%d" % (MAX_RIG_PARTS, K))
    return _RIG_HEAD + K * _rig_part(K)


def _groups(v, parts_map, what):
    """The per-link arrays of `what` (a dict keyed like the .h5 groups, str or int, or a sequence indexed by link) concatenated per group
    of parts_map (lib/dataset.py:475-485) -> one (n_j, 3) array per part, dtype kept."""
    def link(i):
        if isinstance(v, dict):
            a = v[str(i)] if str(i) in v else v[i]
        else:
            a = v[i]
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("%s[%s] must be an (n, >= 3) array, got shape %s" % (what, i, a.shape))
        return a[:, :3]
    return [np.concatenate([link(i) for i in group], axis=0) for group in parts_map]


def pack_annotated_cloud(gt_points, gt_coords, parts_map):
    """One frame's annotated rows: gt_points / gt_coords = the frame's per-link camera points and canonical coordinates (the .h5 groups
    f['gt_points'], f['gt_coords'] as dicts keyed '0', '1', ... or sequences indexed by link); the links of each group of parts_map are
    concatenated in order (lib/dataset.py:475-485) and a row is [x y z | cx cy cz | part], part = the group's index in parts_map.
    -> (n_raw, 7) float32, the rows build_point_gt_rows and a build_point_gt pipeline take."""
    pts, crd = _groups(gt_points, parts_map, "gt_points"), _groups(gt_coords, parts_map, "gt_coords")
    out = []
    for j, (p, c) in enumerate(zip(pts, crd)):
        if p.shape[0] != c.shape[0]:
            raise ValueError("part %d: %d points but %d coordinates" % (j, p.shape[0], c.shape[0]))
        out.append(np.concatenate([np.asarray(p, np.float32), np.asarray(c, np.float32), np.full((p.shape[0], 1), j, np.float32)], axis=1))
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def identity_rig(K):
    """A rig without joints whose maps are the identity: g0 = p0 = c, cls = part, heatmap = 0, joint_cls = 0 (what a build_point_gt
    pipeline's slots hold until the first submit)."""
    rig = np.zeros(RIG_WIDTH(K))
    rig[0] = 0.2
    rig[_RIG_ROT:_RIG_ROT + 9] = np.eye(3).reshape(9)
    rig[_RIG_GMAP + 3:_RIG_GMAP + 6] = 1.0
    rig[_RIG_GMAP + 6:_RIG_GMAP + 9] = 0.5
    for j in range(K):
        pt = rig[_RIG_HEAD + j * _rig_part(K):]
        pt[6:9], pt[9:12], pt[12], pt[13] = 1.0, 0.5, j, -1.0
    return rig


def _line_offset(P0, l, point):
    """lib/d3_utils.py:192-203 (point_3d_offset_joint), the same numpy statements."""
    l = np.asarray(l, np.float64).reshape(1, 3)
    d = np.asarray(point, np.float64) - P0
    return np.dot(d, l.T) * l / np.linalg.norm(l) ** 2 - d


def pack_joint_rig(norm_corners, norm_factors, joints, parts_map, dataset="shape2motion", target_order=None, thres_r=0.2):
    """The list logic of lib/dataset.py:466-528 (shape2motion) / :590-658 (sapien), once per frame on the host: which joints a part's points
    are measured against, in which order, and every constant of the arithmetic, as one table for ancsh_point_gt_build.
    norm_corners[0] / norm_factors[0]: the instance's global normalisation box (two corners) and factor (a scalar or one per axis),
    [j + 1]: part j's; joints: the URDF dict (joints['link']['xyz'], joints['joint']['axis' | 'parent' | 'type' | 'rpy']); parts_map: the
    link groups; dataset="sapien" needs target_order = ctgy_spec.spec_map[instance] (part target_order[j] is relabelled j, :697-699, and
    the rig rotates by the base joint's rpy, joints['joint']['rpy'][target_order[0]], :371-379).
    Per part: the parent joint of group[0] (shape2motion: when it is not 0, with axis[j] as the reference pairs them, :508-515), then the
    child joints whose parent is group[-1] (sapien: parent - 1, and link['xyz'][1:]); sapien's 'fixed' joints are dropped (:680-681), its
    'prismatic' ones become constant entries and its
    revolute ones origin entries (the reference measures the NAOCS origin there, :638, and marks the part's first point only); P0 is mapped into the unrotated NAOCS frame.
    -> (rig (RIG_WIDTH(K),) float64, joint_params (K, 7) float64 = the reference's joint_params_gt of line_space='orth' (:500-506, :642-645)).
    ValueError for K outside 1..8, a part with more than K entries, ragged corners or factors, a sapien call without target_order."""
    if dataset not in RIG_DATASETS:
        raise ValueError("dataset must be one of %s, got %r" % (RIG_DATASETS, dataset))
    K = len(parts_map)
    width = RIG_WIDTH(K)
    sapien = dataset == "sapien"
    if sapien and target_order is None:
        raise ValueError("dataset='sapien' relabels the parts and rotates by the base joint: pack_joint_rig needs target_order")
    order = [int(i) for i in target_order] if sapien else []
    if any(not 0 <= i < K for i in order) or (sapien and not order):
        raise ValueError("target_order %s must name parts in [0, %d)" % (order, K))
    thres_r = float(thres_r)
    if len(norm_corners) < K + 1 or len(norm_factors) < K + 1:
        raise ValueError("norm_corners and norm_factors need %d entries (the instance's and one per part), got %d and %d"
                         % (K + 1, len(norm_corners), len(norm_factors)))
    maps = []
    for i in range(K + 1):
        try:
            c = np.asarray(norm_corners[i], np.float64).reshape(2, 3)
            nf = np.broadcast_to(np.asarray(norm_factors[i], np.float64).reshape(-1), (3,))
        except (ValueError, TypeError):
            raise ValueError("norm_corners[%d] must be two corners of 3 values and norm_factors[%d] a scalar or 3 values" % (i, i))
        maps.append((c[0], nf, 0.5 * (c[1] - c[0]) * nf))
    lo0, nf0, tail0 = maps[0]
    to_g = lambda xyz: (-np.asarray(xyz, np.float64).reshape(3) - lo0) * nf0 + 0.5 - tail0
    kind_of = lambda t: (t.decode() if isinstance(t, bytes) else str(t))
    axis, parent = joints["joint"]["axis"], joints["joint"]["parent"]
    link_xyz = joints["link"]["xyz"][1:] if sapien else joints["link"]["xyz"]
    position = (lambda m: link_xyz[m][0]) if sapien else (lambda m: link_xyz[m])
    jtype = (lambda m: kind_of(joints["joint"]["type"][m])) if sapien else (lambda m: "revolute")
    rig = np.zeros(width)
    rig[0], rig[1], rig[2], rig[3] = thres_r, (K if sapien else 0), (1 if sapien else 0), (1 if sapien else 0)
    R = np.eye(3)
    if sapien:
        from .pose.evaluation import euler_matrix_sxyz
        R = euler_matrix_sxyz(*[float(a) for a in joints["joint"]["rpy"][order[0]]])
    rig[_RIG_ROT:_RIG_ROT + 9] = R.reshape(9)
    rig[_RIG_GMAP:_RIG_GMAP + 9] = np.concatenate([lo0, nf0, tail0])
    joint_params = np.zeros((K, 7))
    origin = np.zeros((1, 3))
    for j, group in enumerate(parts_map):
        pt = rig[_RIG_HEAD + j * _rig_part(K):_RIG_HEAD + (j + 1) * _rig_part(K)]
        if sapien:
            pt[0:3] = np.asarray(link_xyz[j][0], np.float64)
        pt[3:12] = np.concatenate(maps[j + 1])
        pt[12], pt[13] = j, -1.0
        if sapien:
            children = [m for m, x in enumerate(parent) if x - 1 == group[-1]]
            members = [(group[0], group[0])] + [(m, m) for m in children]             # (the joint read, the label)
        else:
            children = [m for m, x in enumerate(parent) if x == group[-1]]
            # the parent entry pairs joint_xyz[group[0]] with the axis of joint j (:509-511)
            members = ([(group[0], j)] if group[0] != 0 else []) + [(m, m) for m in children]
        entries = []
        for m, a in members:
            t = jtype(m)
            if t == "fixed":
                continue
            l = np.asarray(axis[a], np.float64).reshape(3)
            # sapien measures a revolute joint from the NAOCS origin (:638), one offset that np.where (:683) can hand to the part's first
            # point only: an "origin" entry
            kind = (1.0 if t == "prismatic" else 2.0) if sapien else 0.0
            entries.append(np.concatenate([to_g(position(m)), l, [m, kind, np.linalg.norm(l) ** 2]]))
        if len(entries) > K:
            raise ValueError("part %d is measured against %d joints; a rig of %d parts holds %d per part" % (j, len(entries), K, K))
        pt[14] = len(entries)
        for k, e in enumerate(entries):
            pt[15 + _RIG_ENTRY * k:15 + _RIG_ENTRY * (k + 1)] = e
        # joint_params_gt
        if sapien:
            t = jtype(j)
            l = np.array([0.0, 0.0, 1.0]) if t == "fixed" else np.asarray(axis[j], np.float64).reshape(3)
            orth = np.ones((1, 3)) * 0.5 * thres_r if t in ("fixed", "prismatic") else _line_offset(to_g(position(j)).reshape(1, 3), l, origin)
        elif j > 0:
            l = np.asarray(axis[j], np.float64).reshape(3)
            orth = _line_offset(to_g(position(j)).reshape(1, 3), l, origin)
        else:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            joint_params[j, 0:3] = l
            joint_params[j, 6] = np.linalg.norm(orth)
            joint_params[j, 3:6] = orth / joint_params[j, 6]
    if sapien:
        for j, idx in enumerate(order):
            pt = rig[_RIG_HEAD + idx * _rig_part(K):]
            pt[12] = pt[13] = j
    return rig, joint_params


def check_rigs(rigs, n, K):
    """-> rigs as a C-contiguous (n, RIG_WIDTH(K)) float64 numpy array; ValueError (before anything touches a device) otherwise."""
    try:
        a = np.ascontiguousarray(rigs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("rig must be an (n, %d) array of real numbers (dataset.pack_joint_rig's tables)" % RIG_WIDTH(K))
    if a.shape != (n, RIG_WIDTH(K)):
        raise ValueError("rig must be (%d, %d) -- one dataset.pack_joint_rig table of %d parts per cloud --, got %s" % (n, RIG_WIDTH(K), K, a.shape))
    return a


def check_annotated_clouds(clouds, norm_factors, K, max_clouds=None):
    """check_raw_clouds for annotated clouds: 1..max_clouds non-empty (n_raw, 7) arrays [x y z | cx cy cz | part] whose part column holds
    integers in [0, K), and (norm_factors not None) one finite norm factor per cloud.  -> (list of contiguous float32 arrays, float32
    norm factors or None); ValueError, before anything touches a device, otherwise."""
    if not isinstance(clouds, (list, tuple)):
        raise ValueError("clouds must be a list of (n_raw, %d) arrays [%s]" % (ANNOTATED_NCHAN, ANNOTATED_COLUMNS))
    if not 1 <= len(clouds) <= (max_clouds or 65535):
        raise ValueError("a batch holds 1..%d clouds, got %d" % (max_clouds or 65535, len(clouds)))
    out = []
    for i, c in enumerate(clouds):
        c = np.asarray(c.cpu().numpy() if torch.is_tensor(c) else c)
        if c.ndim != 2 or c.shape[1] != ANNOTATED_NCHAN or c.shape[0] == 0:
            raise ValueError("cloud %d: expected a non-empty (n_raw, %d) array [%s] (dataset.pack_annotated_cloud), got shape %s"
                             % (i, ANNOTATED_NCHAN, ANNOTATED_COLUMNS, c.shape))
        c = np.ascontiguousarray(c, np.float32)
        part = c[:, 6]
        if not ((part >= 0) & (part < K) & (part == np.floor(part))).all():
            raise ValueError("cloud %d: the part column must hold integers in [0, %d)" % (i, K))
        out.append(c)
    if norm_factors is None:
        return out, None
    nf = np.asarray(norm_factors, np.float32).reshape(-1)
    if nf.size != len(out) or not np.isfinite(nf).all():
        raise ValueError("norm_factors: one finite value per cloud (%d clouds, got %s)" % (len(out), nf.tolist()))
    return out, nf


def point_gt_build(src, offsets, rig, K, out):
    """ancsh_point_gt_build on device tensors, one launch, no host sync and no allocation (the captured streaming step calls it): src
    (capacity, 7) float32, offsets (B+1,) int32, rig (B, RIG_WIDTH(K)) float64 -> out (capacity, 18) float32, which it returns."""
    _lib.require_cuda(src, offsets, rig, out)
    cap, B = int(src.shape[0]), int(rig.shape[0])
    if src.dtype != torch.float32 or src.dim() != 2 or src.shape[1] != ANNOTATED_NCHAN or not src.is_contiguous():
        raise ValueError("src must be a contiguous (capacity, %d) float32 tensor [%s]" % (ANNOTATED_NCHAN, ANNOTATED_COLUMNS))
    if out.dtype != torch.float32 or tuple(out.shape) != (cap, NCHAN) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (%d, %d) float32 tensor" % (cap, NCHAN))
    if rig.dtype != torch.float64 or rig.dim() != 2 or not rig.is_contiguous():
        raise ValueError("rig must be a contiguous (B, RIG_WIDTH) float64 tensor")
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (B + 1,) or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous (B+1,) int32 tensor")
    _lib.call("ancsh_point_gt_build", B, int(K), _lib.ptr(src), cap, _lib.ptr(offsets), _lib.ptr(rig), int(rig.shape[1]), _lib.ptr(out))
    return out


def build_point_gt_rows(clouds7, rigs, device="cuda:0", K=None, capacity=None):
    """Eager wrapper of ancsh_point_gt_build: clouds7 = list of (n_raw, 7) float32 arrays (pack_annotated_cloud), rigs = one
    pack_joint_rig table per cloud (all of the same K; K is read from their width unless given) -> (rows (n_total, 18) float32 device
    tensor in dataset.pack_cloud's layout, offsets (B+1,) int32 device tensor).  capacity: rows of the buffers (>= n_total); rows beyond
    n_total are left as allocated.  The host refuses a non-integer or out-of-range part column before anything touches the device."""
    dev = _lib.cuda_device(device)
    rigs = np.asarray(rigs, np.float64)
    if K is None:
        K = next((k for k in range(1, MAX_RIG_PARTS + 1) if rigs.ndim == 2 and RIG_WIDTH(k) == rigs.shape[1]), None)
        if K is None:
            raise ValueError("rigs must be (B, RIG_WIDTH(K)) for a K in 1..%d, got shape %s" % (MAX_RIG_PARTS, rigs.shape))
    clouds7, _ = check_annotated_clouds(clouds7, None, K)
    rigs = check_rigs(rigs, len(clouds7), K)
    B = len(clouds7)
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum([c.shape[0] for c in clouds7])
    n_total = int(offsets[-1])
    cap = n_total if capacity is None else int(capacity)
    if cap < n_total:
        raise ValueError("capacity %d is below the batch's %d rows" % (cap, n_total))
    src = torch.empty((cap, ANNOTATED_NCHAN), dtype=torch.float32, device=dev)
    src[:n_total].copy_(torch.from_numpy(np.concatenate(clouds7, axis=0)))
    rows = torch.empty((cap, NCHAN), dtype=torch.float32, device=dev)
    off = torch.from_numpy(offsets).to(dev)
    point_gt_build(src, off, torch.from_numpy(rigs).to(dev), K, rows)
    return rows, off
