"""CPU tests of the posed-object front end (no GPU): the numpy mirror of ancsh_pose_scene_build and ancsh_render_centre_crops
(tests/pose_scene_mirror.py) against depth.pack_render_scene / depth.pack_frame_scene fed depth.forward_kinematics' link poses, analytic
forward kinematics, hand-computed crop origins, the host helpers' refusals, the entries' argument checks before any launch, and the
pipeline's option rules."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pose_scene_mirror as PM
from test_depth_annotate_cpu import random_rotation, random_scene
from test_render_cpu import box_mesh, pinhole_table

P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first


# ---- trees, tables and poses the GPU tests share ---------------------------------------------------------------------------------------------
def tree(rs, L, shape="chain", kinds=None):
    """A random kinematic tree of L links: shape "chain" (depth L - 1) or "star" (link 0 with L - 1 children); the joint kinds cycle through
    revolute, prismatic, fixed unless given.  -> dict(parents, kinds, joint_xyz, joint_rpy, joint_axis)."""
    parents = [-1] + [(l - 1 if shape == "chain" else 0) for l in range(1, L)]
    kinds = list(kinds) if kinds is not None else ["fixed"] + [("revolute", "prismatic", "fixed")[(l - 1) % 3] for l in range(1, L)]
    return dict(parents=parents, kinds=kinds, joint_xyz=rs.uniform(-0.3, 0.3, (L, 3)), joint_rpy=rs.uniform(-3, 3, (L, 3)),
                joint_axis=rs.normal(size=(L, 3)) * rs.uniform(0.5, 2.0, (L, 1)))


def kin_table(S, Tr, parts_map, depth_scale=1.0, z_min=1e-6, min_link_pixels=10, base=None):
    """depth.pack_kinematics for the camera and URDF frames of a scene dictionary S (random_scene / object_scene) and a tree Tr."""
    from articulated_pose_amd.depth import pack_kinematics
    return pack_kinematics(S["projMat"], S["H"], S["W"], Tr["parents"], Tr["kinds"], Tr["joint_xyz"], Tr["joint_rpy"], Tr["joint_axis"],
                           S["link_xyz"], S["link_rpy"], S["joint_xyz"], parts_map, depth_scale=depth_scale, z_min=z_min,
                           min_link_pixels=min_link_pixels, base=base)


def quaternion_xyzw(R):
    """A rotation matrix -> its unit quaternion [x y z w] (the largest component first, for accuracy)."""
    t = np.trace(R)
    cand = [1.0 + t, 1.0 + 2 * R[0, 0] - t, 1.0 + 2 * R[1, 1] - t, 1.0 + 2 * R[2, 2] - t]          # 4 w^2, 4 x^2, 4 y^2, 4 z^2
    k = int(np.argmax(cand))
    r = np.sqrt(cand[k]) * 2.0                                          # 4 |component k|
    if k == 0:
        w, x, y, z = r / 4, (R[2, 1] - R[1, 2]) / r, (R[0, 2] - R[2, 0]) / r, (R[1, 0] - R[0, 1]) / r
    elif k == 1:
        w, x, y, z = (R[2, 1] - R[1, 2]) / r, r / 4, (R[0, 1] + R[1, 0]) / r, (R[0, 2] + R[2, 0]) / r
    elif k == 2:
        w, x, y, z = (R[0, 2] - R[2, 0]) / r, (R[0, 1] + R[1, 0]) / r, r / 4, (R[1, 2] + R[2, 1]) / r
    else:
        w, x, y, z = (R[1, 0] - R[0, 1]) / r, (R[0, 2] + R[2, 0]) / r, (R[1, 2] + R[2, 1]) / r, r / 4
    return np.array([x, y, z, w])


def random_view(rs):
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = random_rotation(rs)[0], rs.uniform(-1, 1, 3)
    return V


# ---- the mirror against the host packers ---------------------------------------------------------------------------------------------------------
CASES = [(1, "chain", [[0]]), (2, "chain", [[0], [1]]), (3, "star", [[0], [2, 1]]), (16, "chain", [[k] for k in range(15, -1, -1)])]


@pytest.mark.parametrize("L,shape,parts_map", CASES, ids=["L1", "L2-offset-rule", "L3-two-children", "L16-depth-15"])
def test_mirror_equals_the_host_packers(L, shape, parts_map):
    """Random trees (revolute, prismatic and fixed joints), joint values and rigid views: depth.forward_kinematics' link poses, as [x y z w]
    quaternions, through pack_render_scene / pack_frame_scene equal the mirror's tables to 1e-10 per entry; the heads are bit-equal."""
    from articulated_pose_amd.depth import forward_kinematics, pack_frame_scene, pack_pose, pack_render_scene
    rs = np.random.RandomState(40 + L)
    worst = 0.0
    for trial in range(4):
        S = random_scene(rs, L, H=480 if trial % 2 else 512, W=640 if trial % 2 else 512)
        Tr = tree(rs, L, shape)
        kin = kin_table(S, Tr, parts_map, depth_scale=0.5, z_min=1e-3, min_link_pixels=7)
        q, V = rs.uniform(-2, 2, L), random_view(rs)
        q[rs.randint(0, L)] = 0.0
        W = forward_kinematics(kin, q)
        assert W.shape == (L, 4, 4) and W.dtype == np.float64 and all(np.array_equal(w[3], [0, 0, 0, 1]) for w in W)
        for l in range(L):                                              # the helper is the contract's own order: bit-equal to the mirror
            assert np.array_equal(W[l, :3], PM.world_pose(kin, np.concatenate([q, np.zeros(32 - L)]), l))
        pos, orn = W[:, :3, 3], np.stack([quaternion_xyzw(w[:3, :3]) for w in W])
        rt = pack_render_scene(V, S["projMat"], pos, orn, S["H"], S["W"], depth_scale=0.5, z_min=1e-3)
        sc = pack_frame_scene(V, S["projMat"], pos, orn, S["link_xyz"], S["link_rpy"], S["joint_xyz"], parts_map, S["H"], S["W"],
                              depth_scale=0.5, min_link_pixels=7)
        render, scene = PM.build_tables(kin, pack_pose(q, V))
        assert render.shape == (1, 208) and scene.shape == (1, 240)
        assert np.array_equal(render[0, :16].view(np.uint64), rt[:16].view(np.uint64)) and np.array_equal(scene[0, :16].view(np.uint64), sc[:16].view(np.uint64))
        worst = max(worst, np.abs(render[0] - rt).max(), np.abs(scene[0] - sc).max())
        assert np.abs(render[0] - rt).max() <= 1e-10 and np.abs(scene[0] - sc).max() <= 1e-10, (L, trial, worst)
        assert (render[0, 16 + 12 * L:] == 0).all() and (scene[0, 16 + 14 * L:] == 0).all()
    print("L = %d: worst |mirror - host packers| = %.3g" % (L, worst))


def test_analytic_forward_kinematics():
    """q = 0: W_l is the product of the joint origins.  A revolute joint about z at pi / 2 and a prismatic slide, by hand."""
    from articulated_pose_amd.depth import _rotation_from_rpy, forward_kinematics
    rs = np.random.RandomState(5)
    S = random_scene(rs, 4)
    Tr = tree(rs, 4, "chain", ["fixed", "revolute", "prismatic", "revolute"])
    base = np.eye(4)
    base[:3, :3], base[:3, 3] = random_rotation(rs)[0], (0.1, -0.2, 0.3)
    kin = kin_table(S, Tr, [[0], [1], [2, 3]], base=base)
    want, W = base.copy(), forward_kinematics(kin, np.zeros(4))
    assert np.abs(W[0] - base).max() <= 1e-15
    for l in range(1, 4):
        T = _rotation_from_rpy(*Tr["joint_rpy"][l])
        T[:3, 3] = Tr["joint_xyz"][l]
        want = want @ T
        assert np.abs(W[l] - want).max() <= 1e-14, l
    zero = np.zeros((3, 3))
    Tr = dict(parents=[-1, 0, 1], kinds=["fixed", "revolute", "fixed"], joint_xyz=[(0, 0, 0), (1, 0, 0), (0, 0, 2)], joint_rpy=zero,
              joint_axis=[(0, 0, 0), (0, 0, 3.0), (0, 0, 0)])
    S3 = random_scene(rs, 3)
    W = forward_kinematics(kin_table(S3, Tr, [[0], [1], [2]]), [9.0, np.pi / 2, 9.0])     # link 0's value and a fixed joint's are not read
    assert np.array_equal(W[0], np.eye(4))
    assert np.abs(W[1] - np.array([[0, -1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])).max() <= 1e-16
    assert np.abs(W[1] @ [1, 0, 0, 1] - [1, 1, 0, 1]).max() <= 1e-16 and np.abs(W[2][:3, 3] - [1, 0, 2]).max() <= 1e-16
    Tr["kinds"], Tr["joint_axis"] = ["fixed", "prismatic", "fixed"], [(0, 0, 0), (0, 2.0, 0), (0, 0, 0)]
    W = forward_kinematics(kin_table(S3, Tr, [[0], [1], [2]]), [0.0, 0.25, 0.0])
    assert np.array_equal(W[1][:3, :3], np.eye(3)) and np.array_equal(W[1][:3, 3], [1, 0.25, 0]) and np.array_equal(W[2][:3, 3], [1, 0.25, 2])


# ---- the host helpers' refusals ----------------------------------------------------------------------------------------------------------------
def test_pack_kinematics_and_poses_refuse_what_they_must():
    from articulated_pose_amd import depth as D
    rs = np.random.RandomState(6)
    S, Tr = random_scene(rs, 3), tree(rs, 3, "star")
    kin = kin_table(S, Tr, [[0], [1], [2]])
    assert kin.shape == (672,) and kin.dtype == np.float64 and D.check_kinematics(kin, 3).flags.c_contiguous
    L = kin[32:32 + 40 * 3].reshape(3, 40)
    assert L[:, 2].tolist() == [-1, 0, 0] and L[:, 3].tolist() == [0, 1, 2] and np.allclose(np.linalg.norm(L[1:, 16:19], axis=1), 1.0, atol=1e-15)
    assert (kin[23:32] == 0).all() and (L[:, 31:] == 0).all() and (kin[32 + 120:] == 0).all() and kin[14] == 3
    for change in (dict(joint_axis=np.where(np.arange(3)[:, None] == 1, 0.0, Tr["joint_axis"])),        # a zero axis on a moving joint
                   dict(parents=[-1, 2, 0]), dict(parents=[-1, 1, 0]), dict(parents=[0, 0, 0]),          # a parent that is not < l; no root
                   dict(joint_xyz=np.where(np.arange(3)[:, None] == 2, np.nan, Tr["joint_xyz"])),        # a non-finite value
                   dict(joint_rpy=np.where(np.arange(3)[:, None] == 1, np.inf, Tr["joint_rpy"])), dict(kinds=["fixed", "hinge", "fixed"])):
        with pytest.raises(ValueError):
            kin_table(S, dict(Tr, **change), [[0], [1], [2]])
    with pytest.raises(ValueError, match="1..16 links"):
        kin_table(random_scene(rs, 17), tree(rs, 17), [[0]])
    for kw in (dict(z_min=0.0), dict(depth_scale=np.nan), dict(base=np.ones((4, 4)))):
        with pytest.raises(ValueError):
            kin_table(S, Tr, [[0], [1], [2]], **kw)
    # a zero axis on a FIXED joint is fine
    assert kin_table(S, dict(Tr, kinds=["fixed"] * 3, joint_axis=np.zeros((3, 3))), [[0], [1], [2]])[14] == 3
    for at, bad in ((14, 0), (14, 17), (14, 2.5), (22, 0.0), (6, -1.0), (25, 1.0), (32 + 40 + 2, 1.0), (32 + 80 + 2, 0.5), (32 + 40 + 3, 3.0),
                    (32 + 40 + 16, 0.5), (32 + 4, 2.0), (32 + 19, 2.0), (32 + 35, 1.0), (32 + 120, 1.0), (40, np.nan)):
        k = kin.copy()
        k[at] = bad
        with pytest.raises(ValueError):
            D.check_kinematics(k, 3)
    with pytest.raises(ValueError):
        D.check_kinematics(kin, 2)                                      # a part outside [0, K)
    with pytest.raises(ValueError):
        D.check_kinematics(kin[:600])
    V = random_view(rs)
    pose = D.pack_pose([0.1, 0.2, 0.3], V)
    assert pose.shape == (32,) and pose[:3].tolist() == [0.1, 0.2, 0.3] and (pose[3:16] == 0).all() and (pose[28:] == 0).all()
    assert np.array_equal(pose[16:28].reshape(3, 4), V[:3]) and D.check_poses(pose, 3).shape == (3, 32)
    skew = V.copy()
    skew[0, 0] += 1e-6
    mirror = V.copy()
    mirror[:3, :3] = -mirror[:3, :3]
    for q, view in (([0.0], skew), ([0.0], mirror), ([np.nan], V), ([0.0] * 17, V), ([0.0], V[:3]), ([0.0], np.where(np.eye(4) == 1, V, V + np.eye(4)[::-1]))):
        with pytest.raises(ValueError):
            D.pack_pose(q, view)
    for at, bad in ((0, np.inf), (16, 2.0), (30, 1.0)):
        p = pose.copy()
        p[at] = bad
        with pytest.raises(ValueError):
            D.check_poses(p, 1)
    for bad in (pose[:31], np.stack([pose, pose]), None):
        with pytest.raises(ValueError):
            D.check_poses(bad, 3)
    shapes, origins = D.check_posed_crops([(3, 4, None), (5, 6, (7, -8))], 2)
    assert shapes == [(3, 4), (5, 6)] and origins.tolist() == [[D.CROP_CENTRE] * 2, [7, -8]] and origins.dtype == np.int32
    for bad in ([(0, 4, None)], [(3, 4, None)] * 3, [(3, 4)], None):
        with pytest.raises(ValueError):
            D.check_posed_crops(bad, 2)


# ---- the pipeline's rules ------------------------------------------------------------------------------------------------------------------------
def test_options_and_submit_refusals_before_gpu_work():
    from articulated_pose_amd import stream
    from articulated_pose_amd.dataset import identity_rig
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    rs = np.random.RandomState(7)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin = kin_table(random_scene(rs, 1, 64, 64), tree(rs, 1), [[0]])
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    for kw in (annotated, dict(raw_capacity=1000), dict()):
        with pytest.raises(ValueError, match="kinematics .* render_mesh"):
            check_options(kinematics=kin, **kw)
        with pytest.raises(ValueError, match="kinematics"):
            AncshPipeline(3, None, None, 2, 64, "cpu", kinematics=kin, **kw)
    off, on = check_options(render_mesh=mesh, **annotated), check_options(render_mesh=mesh, kinematics=kin, **annotated)
    assert on.posed and on.render and not off.posed
    assert [i.name for i in off.inputs] == ["render", "scene", "frame", "rig"] and [i.name for i in on.inputs] == ["pose", "frame", "rig"]
    assert on._replace(posed=False, inputs=()) == off._replace(inputs=())
    for extra in (dict(ground_truth=True, build_gt_pose=True), dict(fit_quality=True, joint_states=True, keyed=True, range_guard=True)):
        assert check_options(render_mesh=mesh, kinematics=kin, **dict(annotated, **extra)).posed
    # the pinned tuples are what they were; the pose is a constant of its own beside them
    assert [i.name for i in stream.SIDE_INPUTS] == ["scene", "gt", "frame", "rig"] and stream.ALL_INPUTS == (stream.RENDER_INPUT,) + stream.SIDE_INPUTS
    p = stream.POSE_INPUT
    assert p not in stream.ALL_INPUTS and stream.SIDE["pose"] is p and (str(p.dtype), p.shape(3), p.pad) == ("torch.float64", (32,), "first") and p.missing
    from articulated_pose_amd.depth import check_poses
    assert check_poses(stream.unit_pose(3, None), 1).shape == (1, 32)     # the slot's default pose is a valid one
    # each submit method refuses the wrong pipeline, naming the right method
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.B, pipe.K = on, 2, 3
    frame = [(np.ones((3, 4), np.uint16), np.zeros((3, 4), int), (0, 0))]
    with pytest.raises(RuntimeError, match="submit_posed"):
        pipe.submit_depth(frame, [1.0], scene=np.zeros(240), rig=np.zeros((1, 10)))
    with pytest.raises(RuntimeError, match="submit_posed"):
        pipe.submit_render([(3, 4, (0, 0))], [1.0], np.zeros(208), np.zeros(240), np.zeros((1, 10)))
    for opts, right in ((off, "submit_render"), (check_options(**annotated), "submit_depth"),
                        (check_options(depth_capacity=4096, joint_source="predicted"), "submit_depth"), (check_options(raw_capacity=1000), r"submit\(\)")):
        pipe.opts = opts
        with pytest.raises(RuntimeError, match="kinematics=.*" + right):
            pipe.submit_posed([(3, 4, None)], [1.0], np.zeros(32), np.zeros((1, 10)))
    # the front end's own checks come before anything is enqueued (no device is touched: the options alone decide)
    pipe.opts = on
    pipe._inflight, pipe.slots = [], []
    good = dict(crops=[(3, 4, None)], norm_factors=[1.0], pose=stream.unit_pose(3, None), rig=identity_rig(3)[None])
    bad_pose = good["pose"].copy()
    bad_pose[17] = 0.5
    for kw in (dict(pose=None), dict(rig=None), dict(crops=[(0, 4, None)]), dict(crops=[(3, 4, None)] * 3), dict(norm_factors=[np.nan]), dict(pose=bad_pose),
               dict(pose=good["pose"][:30]), dict(crops=[(64, 65, (0, 0))]), dict(frame=np.zeros((2, 13))), dict(gt=np.zeros((1, 3, 19)))):
        with pytest.raises(ValueError):
            pipe.submit_posed(**dict(good, **kw))
    assert not pipe._inflight


# ---- the symbols and their argument checks ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd import depth as D
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name, nargs in (("ancsh_pose_scene_build", 6), ("ancsh_render_centre_crops", 10)):
        assert name in declared_symbols() and name in exported and len(_lib.SIGNATURES[name]) == nargs
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ancsh_hip.h")).read()
    for name, value in (("ANCSH_KIN_WIDTH", D.KIN_WIDTH), ("ANCSH_KIN_HEAD", D.KIN_HEAD), ("ANCSH_KIN_LINK", D.KIN_LINK), ("ANCSH_POSE_WIDTH", D.POSE_WIDTH)):
        assert "#define %s %d\n" % (name, value) in header
    assert "#define ANCSH_CROP_CENTRE (-2147483647 - 1)\n" in header and D.CROP_CENTRE == -2147483648 == PM.CROP_CENTRE
    assert D.KIN_WIDTH == 672 == D.KIN_HEAD + D.SCENE_MAX_LINKS * D.KIN_LINK
    assert (PM.KIN_WIDTH, PM.KIN_HEAD, PM.KIN_LINK, PM.POSE_WIDTH) == (D.KIN_WIDTH, D.KIN_HEAD, D.KIN_LINK, D.POSE_WIDTH)


def test_entries_reject_bad_arguments_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def build(nframes=2, kin=P16, pose=P16, render=P16, scene=P16):
        return L.ancsh_pose_scene_build(nframes, kin, pose, render, scene, None)

    def centre(nframes=2, verts=P16, tris=P16, tri_link=P16, V=8, T=12, render=P16, geom=P16, bounds=P16):
        return L.ancsh_render_centre_crops(nframes, verts, tris, tri_link, V, T, render, geom, bounds, None)
    for call, cases, names in ((build, ((dict(nframes=-1), b"bad shape"), (dict(nframes=65536), b"65535"), (dict(kin=ctypes.c_void_p(4)), b"8-byte aligned"),
                                        (dict(pose=ctypes.c_void_p(12)), b"8-byte aligned"), (dict(render=ctypes.c_void_p(20)), b"8-byte aligned"),
                                        (dict(scene=ctypes.c_void_p(4)), b"8-byte aligned")), ("kin", "pose", "render", "scene")),
                               (centre, ((dict(nframes=-1), b"bad shape"), (dict(nframes=65536), b"65535"), (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T=16777216"),
                                         (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V=16777216"), (dict(render=ctypes.c_void_p(4)), b"8-byte aligned"),
                                         (dict(geom=ctypes.c_void_p(2)), b"4-byte aligned"), (dict(bounds=ctypes.c_void_p(18)), b"4-byte aligned")),
                                ("verts", "tris", "tri_link", "render", "geom", "bounds"))):
        for kw, msg in cases:
            assert call(**kw) == -1, kw
            assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
        for k in names:
            assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
            assert call(nframes=0, **{k: None}) == -1         # nulls are refused even for an empty batch
        assert call(nframes=0) == 0                           # no frame: nothing launched, no device touched
    assert centre(nframes=0, T=0, V=0) == 0


# ---- the centring mirror, by hand ------------------------------------------------------------------------------------------------------------------
def hand_mesh():
    """Two triangles at unit depth whose x spans [-0.5, 0.26] and y spans [-0.25, 0.5], and one with a vertex behind the camera far to the
    right (that vertex does not count; its two others lie inside the span and do)."""
    v = np.array([(-0.5, -0.25, 1), (0.26, 0.1, 1), (0.0, 0.5, 1), (-0.1, 0.0, 1), (0.1, 0.2, 1), (30.0, 30.0, -1)], np.float32)
    return v, np.array([(0, 1, 2), (2, 1, 0), (3, 4, 5)], np.int32), np.zeros(3, np.int32)


def test_centring_mirror_on_hand_made_vertices():
    """col = 32 x + cx, row = 32 y + 32 in 1/256 pixel.  cx = 32: X in [4096, 10322], sum 14418 >> 9 = 28.  cx = -50: X in [-16896, -10670],
    sum -27566 = -53.84 * 512: floor gives -54 (truncation would give -53).  Y in [6144, 12288], sum 18432 >> 9 = 36.  Even and odd h, w."""
    C = PM.CROP_CENTRE
    v, tris, link = hand_mesh()
    I = np.eye(4)[:3]
    right, left = pinhole_table(32.0, 32.0, 32.0, 32.0, [I]), pinhole_table(32.0, 32.0, -50.0, 32.0, [I])
    geom = np.array([(0, 10, 10, C, C), (100, 11, 11, C, C), (300, 10, 11, C, C), (500, 9, 7, 5, -6), (600, 4, 4, C, 3), (700, 4, 4, 3, C)], np.int32)
    out = PM.centre_origins(v, tris, link, 6, geom, np.stack([right, right, left, left, right, right]))
    assert out[:, :3].tolist() == geom[:, :3].tolist()                  # start, h, w are untouched
    assert out[0, 3:].tolist() == [36 - 5, 28 - 5] and out[1, 3:].tolist() == [36 - 5, 28 - 5]
    assert out[2, 3:].tolist() == [36 - 5, -54 - 5]                     # the negative centre: floor, not truncation
    assert out[3:].tolist() == geom[3:].tolist()                        # real origins, and a sentinel in one place only: left alone
    assert PM.centre_origins(v, tris, link, 6, out, np.stack([left] * 6)).tolist() == out.tolist()      # a second call is a no-op
    # the vertex behind z_min does not count: with it, Xmax would be far to the right -- and alone, it leaves nothing to count
    only = np.array([(5, 5, 5)], np.int32)
    assert PM.centre_origins(v, only, link[:1], 6, geom[:1], right[None])[0, 3:].tolist() == [0, 0]
    # no counted vertex: T == 0, every link beyond nlinks, an index outside [0, V), a table that is none
    none = right.copy()
    none[8] = 0
    for args in ((v, np.zeros((0, 3), np.int32), np.zeros(0, np.int32), 6, right), (v, tris, link + 1, 6, right), (v, tris, link, 0, right), (v, tris, link, 6, none)):
        assert PM.centre_origins(args[0], args[1], args[2], args[3], geom[:1], args[4][None])[0, 3:].tolist() == [0, 0]
    # vertices count one by one: an index outside [0, V) drops that vertex alone (V = 2 keeps vertices 0 and 1: Y in [6144, 8960])
    assert PM.centre_origins(v, tris, link, 2, geom[:1], right[None])[0, 3:].tolist() == [((6144 + 8960) >> 9) - 5, 28 - 5]
