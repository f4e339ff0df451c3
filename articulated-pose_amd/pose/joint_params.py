"""Joint parameters from the networks' per-point heads, batched on the GPU: the per-sample body of
evaluation/eval_joint_params.py (:143-256) -- similarity global NOCS -> part NOCS per part, offset voting
`nocs_g + unitvec * (1 - heatmap) * 0.2` with per-joint medians, transformation into camera space by part 0's fitted pose,
and the two joint errors -- for a whole batch in one kernel launch (ancsh_joint_params, csrc/metrics.hip) plus a handful of
(B, K-1, 3) float64 tensor operations.  The metric functions are pose/metrics.py's (lib/d3_utils.py:137-142,165-174)."""
import torch

from .. import _lib
from .metrics import axis_diff_degree_batch, dist_between_3d_lines_batch


def _f32(t, dev):
    return torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous() if not torch.is_tensor(t) else t.to(dev, torch.float32).contiguous()


def _launch(gocs, nocs, mask, heatmap, unitvec, axis, joint_cls, K, axis_mean):
    dev = gocs.device
    _lib.require_cuda(gocs)
    B, N, G = gocs.shape
    st = torch.empty((B, K, 4), dtype=torch.float64, device=dev) if nocs is not None else None
    joint = torch.empty((B, max(K - 1, 0), 6), dtype=torch.float64, device=dev)
    if K > 1 or nocs is not None:
        _lib.call("ancsh_joint_params", B, N, K, G, 1 if axis_mean else 0, _lib.ptr(gocs), _lib.ptr(nocs), _lib.ptr(mask), _lib.ptr(heatmap),
                  _lib.ptr(unitvec), _lib.ptr(axis), _lib.ptr(joint_cls), _lib.ptr(st), _lib.ptr(joint))
    return st, joint


def joint_params_batch(pred, num_parts, pose_scale, pose_rotation, pose_translation, device="cuda:0"):
    """pred: the record's prediction arrays (B, N, .) -- gocs_per_point (3K or 3 channels), nocs_per_point (3K),
    instance_per_point (K), heatmap_per_point (1 or none), unitvec_per_point (3), joint_axis_per_point (3), index_per_point (K);
    pose_*: part 0's fitted pose per cloud (the 'nonlinear' entries of the pose pickle, :201-203): scale (B,), rotation (B,3,3),
    translation (B,3).  Returns float64 device tensors:
      scale (B,K), translation (B,K,3)            st_dict of :160-171
      joint_pt, joint_axis (B,K-1,3)              joints['pred'] in global-NOCS space (:176-187)
      joint_pt_cam, joint_axis_cam (B,K-1,3)      t_joints['pred'] in camera space (:214-222)"""
    dev = torch.device(device)
    K = num_parts
    g = _f32(pred["gocs_per_point"], dev)
    B, N = g.shape[:2]
    jc = torch.argmax(_f32(pred["index_per_point"], dev), dim=2).to(torch.int32).contiguous()       # np.argmax(index_per_point, 1) (:134)
    st, joint = _launch(g, _f32(pred["nocs_per_point"], dev), _f32(pred["instance_per_point"], dev),
                        _f32(pred["heatmap_per_point"], dev).reshape(B, N), _f32(pred["unitvec_per_point"], dev),
                        _f32(pred["joint_axis_per_point"], dev), jc, K, False)
    out = {"scale": st[..., 0], "translation": st[..., 1:], "joint_pt": joint[..., :3], "joint_axis": joint[..., 3:]}
    s2, t2 = st[:, 0, 0], st[:, 0, 1:]                                           # part 0 is the platform (:215-217)
    R = torch.as_tensor(pose_rotation, dtype=torch.float64, device=dev).reshape(B, 3, 3)
    s = torch.as_tensor(pose_scale, dtype=torch.float64, device=dev).reshape(B, 1, 1)
    t = torch.as_tensor(pose_translation, dtype=torch.float64, device=dev).reshape(B, 1, 3)
    p_part = out["joint_pt"] * s2[:, None, None] + t2[:, None, :]
    out["joint_pt_cam"] = (s * p_part) @ R.transpose(1, 2) + t                   # np.dot(s[0] * p, r[0].T) + t[0]
    out["joint_axis_cam"] = out["joint_axis"] @ R.transpose(1, 2)
    return out


def joint_params_gt_batch(gt, num_parts, gt_scale, gt_rt, device="cuda:0"):
    """gt: nocs_gt_g (B,N,3), heatmap_gt (B,N), unitvec_gt, joint_axis_gt (B,N,3), joint_cls_gt (B,N); gt_scale (B,), gt_rt (B,4,4):
    part 0's ground-truth global-NOCS pose (:205-206).  -> joint_pt / joint_axis (global NOCS; the axis is the MEAN, :195) and
    their camera-space images (:224-231)."""
    dev = torch.device(device)
    g = _f32(gt["nocs_gt_g"], dev)
    B, N = g.shape[:2]
    jc = torch.as_tensor(gt["joint_cls_gt"], device=dev).to(torch.int32).reshape(B, N).contiguous()
    _st, joint = _launch(g, None, None, _f32(gt["heatmap_gt"], dev).reshape(B, N), _f32(gt["unitvec_gt"], dev),
                         _f32(gt["joint_axis_gt"], dev), jc, num_parts, True)
    rt = torch.as_tensor(gt_rt, dtype=torch.float64, device=dev).reshape(B, 4, 4)
    s = torch.as_tensor(gt_scale, dtype=torch.float64, device=dev).reshape(B, 1, 1)
    R = rt[:, :3, :3]
    return {"joint_pt": joint[..., :3], "joint_axis": joint[..., 3:],
            "joint_pt_cam": (s * joint[..., :3]) @ R.transpose(1, 2) + rt[:, None, :3, 3],
            "joint_axis_cam": joint[..., 3:] @ R.transpose(1, 2)}


def joint_errors(pred, gt):
    """(angle_err, dist_err), each (B, K-1): axis_diff_degree and dist_between_3d_lines of the camera-space joints (:244-256)."""
    return (axis_diff_degree_batch(gt["joint_axis_cam"], pred["joint_axis_cam"]),
            dist_between_3d_lines_batch(gt["joint_pt_cam"], gt["joint_axis_cam"], pred["joint_pt_cam"], pred["joint_axis_cam"]))


ARTICULATION_MAX_N = 4096       # include/ancsh_hip.h, ANCSH_ARTICULATION_MAX_N: the medians' six LDS columns of the next power of two of N


def articulation_batch(ancsh_pred, npcs_pred, record, debug=False):
    """The articulation block of a batch in ONE launch (ancsh_articulation_rec, csrc/metrics.hip): ancsh_pred / npcs_pred = the two
    networks' output dicts (device tensors, (B, N, .) float32: the ANCSH gocs / nocs / W / heatmap / unitvec / joint_axis / index heads and
    the NPCS nocs / W), record = the (B, K, 26) float64 pose record (the nonlinear R | s | t in columns 13..25).  Returns art (B, K, 12)
    float64 on the device, row j = [box size (3) | box centre (3) | joint j pivot (3) | joint j axis (3)] in camera space (row 0: NaN
    joint columns; a poisoned record: an all-NaN block; include/ancsh_hip.h).  debug=True: (art, dict(joint_nocs (B, K-1, 6), st0 (B, 4),
    extent (B, K, 3) float32)) -- bit-equal to ancsh_joint_params' joint / st row 0 and ancsh_part_extents' scale_pred.
    No host synchronisation and no allocation beyond the outputs: the captured streaming step calls it."""
    dev = record.device
    _lib.require_cuda(record)
    g = _f32(ancsh_pred["gocs_per_point"], dev)
    B, N, G = g.shape
    K = record.shape[1]
    idx = _f32(ancsh_pred["index_per_point"], dev)
    if record.dtype != torch.float64 or tuple(record.shape) != (B, K, 26) or not record.is_contiguous():
        raise ValueError("record must be a contiguous (B, K, 26) float64 tensor")
    art = torch.empty((B, K, 12), dtype=torch.float64, device=dev)
    dbg = dict(joint_nocs=torch.empty((B, max(K - 1, 0), 6), dtype=torch.float64, device=dev),
               st0=torch.empty((B, 4), dtype=torch.float64, device=dev),
               extent=torch.empty((B, K, 3), dtype=torch.float32, device=dev)) if debug else {}
    _lib.call("ancsh_articulation_rec", B, N, K, G, idx.shape[2], _lib.ptr(g), _lib.ptr(_f32(ancsh_pred["nocs_per_point"], dev)),
              _lib.ptr(_f32(ancsh_pred["W"], dev)), _lib.ptr(_f32(ancsh_pred["heatmap_per_point"], dev)),
              _lib.ptr(_f32(ancsh_pred["unitvec_per_point"], dev)), _lib.ptr(_f32(ancsh_pred["joint_axis_per_point"], dev)), _lib.ptr(idx),
              _lib.ptr(_f32(npcs_pred["nocs_per_point"], dev)), _lib.ptr(_f32(npcs_pred["W"], dev)), _lib.ptr(record), _lib.ptr(art),
              _lib.ptr(dbg.get("joint_nocs") if K > 1 else None), _lib.ptr(dbg.get("st0")), _lib.ptr(dbg.get("extent")))
    return (art, dbg) if debug else art


JOINT_STATE_WIDTH = 20          # include/ancsh_hip.h, ancsh_joint_state_rec: the articulation block's 12 columns + 8 of joint state


def check_joint_states(joint_states, articulation):
    """-> bool(joint_states); ValueError (before anything touches the GPU) when it is asked for without the articulation block, whose joint
    axes it reads and whose columns it carries."""
    if joint_states and not articulation:
        raise ValueError("joint_states=True rides inside the articulation block and reads its joint axes: it needs articulation=True")
    return bool(joint_states)


def joint_state_batch(P, npcs_pred, record, art):
    """The joint states of a batch in ONE launch (ancsh_joint_state_rec, csrc/joint_state.hip), behind articulation_batch: P (B, N, C >= 3)
    float32 sampled points, npcs_pred = the NPCS network's output dict (nocs_per_point (B, N, 3K), W (B, N, K)), record (B, K, 26) float64,
    art = articulation_batch's (B, K, 12) block.  Returns the (B, K, 20) float64 block on the device, row j = [art row j (12, bit for bit) |
    angle of R_0^T R_j, degrees | the same, signed about the joint axis | t_j - t_0 (3) | its slide along the axis | boundary slide
    dynam_j - canon_j | points of part j] (row 0: NaN in 12..17; include/ancsh_hip.h has the NaN rules).  No host synchronisation and no
    allocation beyond the output: the captured streaming step calls it."""
    dev = record.device
    _lib.require_cuda(record, art, P)
    B, K = record.shape[:2]
    if record.dtype != torch.float64 or tuple(record.shape) != (B, K, 26) or not record.is_contiguous():
        raise ValueError("record must be a contiguous (B, K, 26) float64 tensor")
    if art.dtype != torch.float64 or tuple(art.shape) != (B, K, 12) or not art.is_contiguous():
        raise ValueError("art must be a contiguous (B, K, 12) float64 tensor (articulation_batch's block)")
    P = _f32(P, dev)
    nocs, mask = _f32(npcs_pred["nocs_per_point"], dev), _f32(npcs_pred["W"], dev)
    N = P.shape[1] if P.dim() == 3 else -1
    if P.dim() != 3 or P.shape[0] != B or P.shape[2] < 3 or tuple(nocs.shape) != (B, N, 3 * K) or tuple(mask.shape) != (B, N, K):
        raise ValueError("P (B, N, >= 3), nocs_per_point (B, N, 3K) and W (B, N, K) must agree with the record's B = %d, K = %d" % (B, K))
    wide = torch.empty((B, K, JOINT_STATE_WIDTH), dtype=torch.float64, device=dev)
    _lib.call("ancsh_joint_state_rec", B, N, K, _lib.ptr(P), P.shape[2], _lib.ptr(nocs), _lib.ptr(mask), _lib.ptr(record), _lib.ptr(art),
              _lib.ptr(wide))
    return wide
