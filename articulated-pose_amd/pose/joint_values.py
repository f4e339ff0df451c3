"""The joint values q of a posed frame read off its part poses (ancsh_joint_values_rec, csrc/joint_values.hip): ancsh_pose_scene_build's forward
kinematics inverted on the predicted link maps.  Row j of a frame reports part j's bridging joint -- the lowest revolute or prismatic link of
part j whose parent link belongs to another part -- under four pose groups (the record's baseline and nonlinear poses, the refinement's two kept
poses): the joint value in the kinematic table's own parametrisation, its error against the value the posed stream submitted, the angle and
the gap by which the two sides of the joint miss one axis, and the ratio of the two sides' scales.  The 24 columns ride behind the
articulation block, as the joint states do; include/ancsh_hip.h states every formula."""
import numpy as np
import torch

from .. import _lib

JOINT_VALUES_WIDTH = 24         # include/ancsh_hip.h, ANCSH_JOINT_VALUES_WIDTH: the columns behind the carried articulation row
GROUPS = ("baseline", "nonlinear", "refined_baseline", "refined_nonlinear")
GROUP_COLUMNS = ("q", "q_err", "off_axis", "gap", "scale_ratio")
COLUMN_NAMES = ("link", "kind", "parent_part", "q_true") + tuple("%s_%s" % (g, c) for g in GROUPS for c in GROUP_COLUMNS)
assert len(COLUMN_NAMES) == JOINT_VALUES_WIDTH
BUILT_WITH = "kinematics=<depth.pack_kinematics(...)>, articulation=True"


def check_joint_values(joint_values, posed, articulation):
    """-> bool(joint_values); ValueError (before anything touches the GPU) naming what is missing when it is asked for without the kinematic
    table whose joints it reports or without the articulation block whose columns it rides behind."""
    if joint_values and not (posed and articulation):
        raise ValueError("joint_values=True inverts the kinematic table's forward kinematics on the part poses and rides behind the articulation "
                         "block: it needs " + ", ".join(["kinematics=<depth.pack_kinematics(...)>"] * (not posed) +
                                                        ["articulation=True"] * (not articulation)))
    return bool(joint_values)


def named_columns(art):
    """The trailing JOINT_VALUES_WIDTH columns of a block (..., >= 24) -> {name: (...) array}, by COLUMN_NAMES."""
    if art.shape[-1] < JOINT_VALUES_WIDTH:
        raise ValueError("expected at least %d trailing columns, got %d" % (JOINT_VALUES_WIDTH, art.shape[-1]))
    tail = art[..., art.shape[-1] - JOINT_VALUES_WIDTH:]
    return {name: tail[..., k] for k, name in enumerate(COLUMN_NAMES)}


def joint_values_batch(kin, render, scene, rig, norm_factor, record, art, pose=None, refined=None, out=None):
    """ancsh_joint_values_rec on device tensors (no host sync, no allocation beyond the output): kin = the object's kinematic table (672,) or
    a library's (ninst, 672); the frames' render (B, 208), scene (B, 240) and rig (B, RIG_WIDTH(K)) tables, norm factors (B,) float32, the
    record (B, K, >= 26) and the articulation block art (B, K, 12 or 20), float64; pose (B, 32) = the submitted poses (depth.pack_pose) or
    None: q_true and every q_err are NaN; refined (B, K, 2, 18) = the refinement's kept poses (refine_buffers' best) or None: the refined
    groups are NaN.  -> (B, K, art's width + 24) float64: art's row bit for bit and COLUMN_NAMES behind it."""
    from ..depth import KIN_WIDTH, POSE_WIDTH
    from .reprojection import _tables
    _lib.require_device(record)
    B, K = (int(v) for v in record.shape[:2]) if record.dim() == 3 else (0, 0)
    if not 1 <= K <= 8:
        raise ValueError("record must be a contiguous (B, K, >= 26) float64 tensor with K in [1, 8]")
    _tables(render, scene, rig, norm_factor, record, None, K, B=B)
    if kin.dtype != torch.float64 or kin.dim() not in (1, 2) or kin.shape[-1] != KIN_WIDTH or kin.shape[0] < 1 or not kin.is_contiguous():
        raise ValueError("kin must be a contiguous (%d,) or (ninst, %d) float64 tensor (depth.pack_kinematics)" % (KIN_WIDTH, KIN_WIDTH))
    ninst = int(kin.shape[0]) if kin.dim() == 2 else 1
    if art.dtype != torch.float64 or art.dim() != 3 or tuple(art.shape[:2]) != (B, K) or art.shape[2] not in (12, 20) or not art.is_contiguous():
        raise ValueError("art must be a contiguous (%d, %d, 12 or 20) float64 tensor (articulation_batch's or joint_state_batch's block)" % (B, K))
    ld = int(art.shape[2])
    for name, t, shape in (("pose", pose, (B, POSE_WIDTH)), ("refined", refined, (B, K, 2, 18))):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s float64 tensor" % (name, shape))
    if out is None:
        out = torch.empty((B, K, ld + JOINT_VALUES_WIDTH), dtype=torch.float64, device=record.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (B, K, ld + JOINT_VALUES_WIDTH) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (%d, %d, %d) float64 tensor" % (B, K, ld + JOINT_VALUES_WIDTH))
    _lib.require_cuda(kin, render, scene, rig, norm_factor, art, pose, refined, out)
    _lib.call("ancsh_joint_values_rec", B, K, _lib.ptr(kin), ninst, _lib.ptr(pose), _lib.ptr(render), _lib.ptr(scene), _lib.ptr(rig),
              int(rig.shape[1]), _lib.ptr(norm_factor), _lib.ptr(record), int(record.shape[2]), _lib.ptr(refined), _lib.ptr(art), ld,
              _lib.ptr(out))
    return out


def joint_value_table(art, K):
    """A summary of streamed blocks as text lines: art (n, K, >= 24) (a list of retired blocks is concatenated) -> per part row the frames
    that report a joint and the mean and median |q_err| of each of the four groups, a revolute joint's in degrees, a prismatic one's in
    length units; NaNs are left out ('-' where nothing is left)."""
    if isinstance(art, (list, tuple)):
        art = np.concatenate([np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in art], 0)
    art = np.asarray(art.cpu() if torch.is_tensor(art) else art, np.float64)
    if art.ndim != 3 or art.shape[1] != K:
        raise ValueError("expected (n, %d, >= %d) blocks, got shape %s" % (K, JOINT_VALUES_WIDTH, art.shape))
    cols = named_columns(art)
    lines = ["part  link  kind       frames  " + "  ".join("%-27s" % (g + " |q_err| mean / median") for g in GROUPS)]
    for j in range(K):
        kind = cols["kind"][:, j]
        has = np.isfinite(kind)
        if not has.any():
            lines.append("%4d     -  -               0" % j)
            continue
        k = int(kind[has][0])
        unit = np.degrees if k == 1 else (lambda x: x)
        cells = []
        for g in GROUPS:
            e = np.abs(cols[g + "_q_err"][:, j])
            e = unit(e[np.isfinite(e)])
            cells.append("%-27s" % ("%.6g / %.6g %s" % (e.mean(), np.median(e), "deg" if k == 1 else "len") if e.size else "-"))
        lines.append("%4d  %4d  %-9s  %6d  %s" % (j, int(cols["link"][:, j][has][0]), "revolute" if k == 1 else "prismatic", int(has.sum()),
                                                 "  ".join(cells)))
    return lines
