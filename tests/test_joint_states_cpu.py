"""CPU (no GPU): the joint-state entry (ancsh_joint_state_rec) is exported without a new ABI number and checks its arguments before any
launch; joint_states=True without the articulation block is refused before anything touches a device; and the numpy mirror the GPU tests
compare against (tests/joint_state_mirror.py) reproduces the pred-side expressions of pose/evaluation.relative_errors."""
import ctypes

import numpy as np
import pytest
import torch

from joint_state_mirror import joint_state_reference, relative_pose, rotation_angle


def _rotation(rs, angle=None):
    """A random rotation (Rodrigues); angle in radians, or uniform in (-pi, pi]."""
    a = rs.normal(size=3)
    a /= np.linalg.norm(a)
    th = rs.uniform(-np.pi, np.pi) if angle is None else angle
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * (A @ A)


def test_entry_is_exported_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "ancsh_joint_state_rec") and "ancsh_joint_state_rec" in _lib.SIGNATURES
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    p8 = ctypes.c_void_p(8)
    call = lambda b, n, K, ldp, wide=p8: L.ancsh_joint_state_rec(b, n, K, p8, ldp, p8, p8, p8, p8, wide, None)
    assert call(1, 16, 9, 3) == -1 and b"K=9" in L.ancsh_last_error()
    assert call(1, 0, 3, 3) == -1 and b"n=0" in L.ancsh_last_error()
    assert call(1, 16, 3, 2) == -1 and b"ldp=2" in L.ancsh_last_error()
    assert call(1, 16, 3, 3, None) == -1 and b"null pointer" in L.ancsh_last_error()
    assert L.ancsh_joint_state_rec(0, 16, 3, None, 3, None, None, None, None, None, None) == 0


def test_joint_states_need_the_articulation_block():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.joint_params import check_joint_states
    with pytest.raises(ValueError, match="needs articulation=True"):
        check_joint_states(True, False)
    assert check_joint_states(True, True) is True and check_joint_states(False, False) is False and check_joint_states(0, True) is False
    # the constructors call it before they build a network or touch a device
    with pytest.raises(ValueError, match="joint_states=True .* needs articulation=True"):
        AncshPipeline(3, {}, {}, 2, 64, "cuda:0", articulation=False, joint_states=True)
    with pytest.raises(ValueError, match="joint_states=True .* needs articulation=True"):
        ShardedPipeline(3, {}, {}, 2, 64, "cuda:0", raw_capacity=1024, joint_states=True)


def test_mirror_reproduces_relative_errors_pred_side():
    """pose/evaluation.relative_errors: r_diff_pred = r[:, :1].transpose(-1, -2) @ r[:, 1:] and (NAOCS) t_diff_pred = t[:, 1:] - t[:, :1],
    float64 -- the mirror's Rrel and t_j - t_0, exactly, on 50 random poses."""
    rs = np.random.RandomState(0)
    K = 4
    for _ in range(50):
        R = np.stack([_rotation(rs) for _ in range(K)])
        t = rs.normal(size=(K, 3))
        r, tt = torch.as_tensor(R)[None], torch.as_tensor(t)[None]
        r_diff_pred = (r[:, :1].transpose(-1, -2) @ r[:, 1:])[0].numpy()
        t_diff_pred = (tt[:, 1:] - tt[:, :1])[0].numpy()
        Rrel, dt = relative_pose(R, t)
        np.testing.assert_array_equal(Rrel, r_diff_pred)
        np.testing.assert_array_equal(dt, t_diff_pred)


def test_mirror_angle_is_rot_diff_degree():
    """Column 12 = rot_diff_degree(I, Rrel) for angles in [5, 175] degrees.  1e-9 degrees: the cosine (tr - 1) / 2 carries about 4 ulp
    (~1e-15) and d acos / dc = 1 / sin <= 1 / sin 5 deg < 12, so the two disagree by ~1e-14 rad ~ 1e-12 degrees; 1e-9 leaves a factor of
    1000."""
    from articulated_pose_amd.pose.d3_utils import rot_diff_degree
    rs = np.random.RandomState(1)
    worst = 0.0
    for _ in range(200):
        deg = rs.uniform(5.0, 175.0)
        R0 = _rotation(rs)
        Rj = R0 @ _rotation(rs, np.radians(deg))
        Rrel, _ = relative_pose(np.stack([R0, Rj]), np.zeros((2, 3)))
        _, _, angle = rotation_angle(Rrel[0])
        want = rot_diff_degree(np.eye(3), Rrel[0])
        worst = max(worst, abs(angle - want))
        assert abs(angle - deg) <= 1e-9
    assert worst <= 1e-9, worst


def test_mirror_rows_and_nan_rules():
    """The mirror on a hand-made cloud: the layout, identical rotations -> angle exactly 0, a pure slide along a known axis, the NaN rules."""
    rs = np.random.RandomState(2)
    B, N, K = 3, 40, 3
    P = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    nocs = rs.uniform(0, 1, (B, N, 3 * K)).astype(np.float32)
    mask = rs.uniform(0, 1, (B, N, K)).astype(np.float32)
    mask[0, :, 2] = -1.0                                                # cloud 0: part 2 has no point
    rec = rs.normal(size=(B, K, 26))
    for b in range(B):
        R0 = _rotation(rs)
        rec[b, :, 13:22] = np.stack([R0, R0, R0 @ _rotation(rs, np.radians(30.0))]).reshape(K, 9)
    rec[2, 1, 24] = np.nan                                              # cloud 2: part 1's pose is poisoned
    art = rs.normal(size=(B, K, 12))
    art[:, 0, 6:] = np.nan
    art[1, 2, 9:12] = np.nan                                            # cloud 1: joint 2 has no axis
    w = joint_state_reference(P, nocs, mask, rec, art)
    assert w.shape == (B, K, 20) and np.array_equal(w[:, :, :12].view(np.int64), art.view(np.int64))
    assert np.isnan(w[:, 0, 12:18]).all() and np.isfinite(w[0, 0, 18]) and np.isfinite(w[1, :, 18]).all()
    assert (w[0, :, 12][1] == 0.0) and abs(w[0, 2, 12] - 30.0) < 1e-9 and abs(abs(w[0, 2, 13]) - abs(w[0, 2, 12])) > 1e-3
    assert w[0, 2, 19] == 0 and np.isnan(w[0, 2, 18]) and w[0, :, 19].sum() == N
    assert np.isnan(w[1, 2, [13, 17]]).all() and np.isfinite(w[1, 2, [12, 14, 15, 16, 18]]).all()
    assert np.isnan(w[2, 1, 12:19]).all() and np.isfinite(w[2, 2, 12:19]).all() and np.isfinite(w[2, 0, 18])
    u = art[0, 1, 9:12] / np.linalg.norm(art[0, 1, 9:12])
    np.testing.assert_array_equal(w[0, 1, 14:17], rec[0, 1, 23:26] - rec[0, 0, 23:26])
    assert abs(w[0, 1, 17] - (rec[0, 1, 23:26] - rec[0, 0, 23:26]) @ u) < 1e-15
    rec[1, 0, 13] = np.nan                                              # part 0 poisoned: the whole cloud's state
    w = joint_state_reference(P, nocs, mask, rec, art)
    assert np.isnan(w[1, :, 12:19]).all() and (w[1, :, 19].sum() == N)
