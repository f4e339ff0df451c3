"""CPU tests of the annotated depth frames (no GPU): the numpy float64 restatement of tools/preprocess_data.py:259-320 and
lib/dataset.py:475-485 that every comparison of ancsh_depth_annotate_stream uses (written here, shared with the GPU tests), the host
helpers against it (depth.pack_frame_scene, depth.coord_unprojection_from_projmat), the symbol / ABI, the entry's argument checks before
any launch, and the host-side validation of frames, scenes and pipeline arguments."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "ancsh_depth_annotate_stream"
P16 = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails its checks first


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def axis_rotation(axis, angle):
    """(4, 4): the rotation by `angle` about a coordinate axis, from Rodrigues' formula."""
    k = np.zeros(3)
    k[axis] = 1.0
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)
    return T


def euler_sxyz(ai, aj, ak):
    """(4, 4): static-axes x, then y, then z rotations -- what the reference's euler_matrix(ai, aj, ak) with its default axes returns."""
    return axis_rotation(2, ak) @ axis_rotation(1, aj) @ axis_rotation(0, ai)


def quaternion_wxyz(q):
    """(4, 4): the rotation of the quaternion [w x y z], column a = q e_a q* (what the reference's quaternion_matrix returns)."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    w, v = q[0], q[1:]
    T = np.eye(4)
    for a in range(3):
        e = np.eye(3)[a]
        T[:3, a] = e + 2.0 * w * np.cross(v, e) + 2.0 * np.cross(v, np.cross(v, e))
    return T


def link_matrices(S):
    """:231-256 and :312-318: parts_model2world[k] and my_canon2urdf_mat[k] of a synthetic scene S (random_scene)."""
    L = len(S["world_pos"])
    model2world, canon2urdf = [], []
    for k in range(L):
        o = S["world_orn"][k]
        m = quaternion_wxyz([o[3], o[0], o[1], o[2]])
        m[:3, 3] = S["world_pos"][k]
        model2world.append(m)
        pos = S["joint_xyz"][k - 1] if (k == 1 and L == 2) else -S["link_xyz"][k]
        c = euler_sxyz(*S["link_rpy"][k])
        c[:3, 3] = pos
        canon2urdf.append(c)
    return model2world, canon2urdf


def chain(S, link, cloud_cam):
    """:298-320 for the (n, 3) camera points cloud_cam of one link -> parts_cloud_urdf[link][:, :3], in the reference's own products."""
    model2world, canon2urdf = link_matrices(S)
    full = np.concatenate((cloud_cam, np.ones((cloud_cam.shape[0], 1))), axis=1)
    camera_pose_mat = np.linalg.pinv(S["viewMat"].T)
    camera_pose_mat[:3, :] = -camera_pose_mat[:3, :]
    cloud_world = np.dot(full, camera_pose_mat)
    cloud_canon = np.dot(cloud_world, np.linalg.pinv(model2world[link].T))
    space = np.concatenate((cloud_canon[:, :3], np.ones((cloud_canon.shape[0], 1))), axis=1)
    return np.dot(space, canon2urdf[link].T)[:, :3]


def valid_depth(depth):
    return depth != 0 if depth.dtype == np.uint16 else (depth > 0) & np.isfinite(depth)


def restate_frame(S, depth, label, origin, depth_scale=1.0):
    """One frame by the reference's statements, on a crop whose pixel (0, 0) is pixel `origin` of the H x W image: per link s, the pixels
    with label == s in np.where order (:262-263) -- of those whose depth the front end accepts; the reference keeps every labelled pixel --,
    cloud_cam_real (:293-296) and parts_cloud_urdf (:288-291, 298-320).  -> {link: (gt_points (n, 3), gt_coords (n, 3))} float64."""
    H, W, P = S["H"], S["W"], S["projMat"]
    d = depth.astype(np.float64) * depth_scale
    xmap, ymap = np.indices(depth.shape)
    xmap, ymap = xmap + origin[0], ymap + origin[1]
    u_map, v_map, v1_map = ymap * 2 / W - 1, (H - xmap) * 2 / H - 1, xmap * 2 / H - 1
    w_channel = -d
    with np.errstate(invalid="ignore"):                                  # holes of a float32 frame may be NaN or Inf: never selected below
        projected_map = np.stack([u_map * w_channel, v_map * w_channel, d, w_channel]).transpose([1, 2, 0])
        projected_map1 = np.stack([u_map * w_channel, v1_map * w_channel, d, w_channel]).transpose([1, 2, 0])
    out = {}
    for s in range(len(S["world_pos"])):
        x_set, y_set = np.where((label == s) & valid_depth(depth))
        pp, pp1 = projected_map[x_set, y_set, :].reshape(-1, 4), projected_map1[x_set, y_set, :].reshape(-1, 4)
        depth_channel = -pp[:, 3:4]
        Minv = np.linalg.pinv(P[:2, :2].T)
        cloud_cam = np.dot(pp[:, 0:2] - np.dot(depth_channel, P[0:2, 2:3].T), Minv)
        cloud_cam_real = np.dot(pp1[:, 0:2] - np.dot(depth_channel, P[0:2, 2:3].T), Minv)
        cloud_cam_real = np.concatenate((cloud_cam_real, depth_channel), axis=1)
        cloud_cam = np.concatenate((cloud_cam, depth_channel), axis=1)
        out[s] = (cloud_cam_real, chain(S, s, cloud_cam))
    return out


def restate_cloud(S, depth, label, origin, parts_map, depth_scale=1.0, min_link_pixels=10):
    """lib/dataset.py:475-485 over restate_frame: the links group by group of parts_map -> (rows (n, 7) float64 [gt_points | gt_coords |
    part], per-link counts {link: n}, the pixel (crop row, crop column) of every row); None for the rows of a frame the reference skips
    (:279-281: a link of the map with fewer than min_link_pixels pixels)."""
    per = restate_frame(S, depth, label, origin, depth_scale)
    counts = {s: len(per[s][0]) for s in per}
    used = [s for group in parts_map for s in group]
    if any(counts[s] < min_link_pixels for s in used) or not used:
        return None, counts, None
    rows, pix = [], []
    for idx, group in enumerate(parts_map):
        for s in group:
            rows.append(np.concatenate([per[s][0], per[s][1], np.full((counts[s], 1), float(idx))], axis=1))
            pix.append(np.stack(np.where((label == s) & valid_depth(depth)), axis=1))
    return np.concatenate(rows), counts, np.concatenate(pix)


def random_rotation(rs):
    q = rs.normal(size=4)
    return quaternion_wxyz(q)[:3, :3], q / np.linalg.norm(q)


def random_scene(rs, L, H=512, W=512):
    """A synthetic scene of L links: a projMat of the reference's form (PyBullet's computeProjectionMatrixFOV, `.reshape(4, 4).T`), a
    rigid viewMat and random rigid link poses and URDF frames; link 0 sits at the world's origin as the reference sets it."""
    t, near, far = np.tan(np.radians(rs.uniform(15, 25))), 0.1, 100.0
    P = np.array([[1.0 / (t * W / H), 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1.0, 0]])
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = random_rotation(rs)[0], rs.uniform(-1, 1, 3)
    orn = np.stack([np.roll(random_rotation(rs)[1], -1) for _ in range(L)])      # [w x y z] -> [x y z w]
    pos = rs.uniform(-1, 1, (L, 3))
    pos[0], orn[0] = 0.0, (0, 0, 0, 1)
    return dict(H=H, W=W, projMat=P, viewMat=V, world_pos=pos, world_orn=orn, link_xyz=rs.uniform(-0.5, 0.5, (L, 3)),
                link_rpy=rs.uniform(-3, 3, (L, 3)), joint_xyz=rs.uniform(-0.5, 0.5, (max(L - 1, 1), 3)))


def scene_table(S, parts_map, depth_scale=1.0, min_link_pixels=10):
    from articulated_pose_amd.depth import pack_frame_scene
    return pack_frame_scene(S["viewMat"], S["projMat"], S["world_pos"], S["world_orn"], S["link_xyz"], S["link_rpy"], S["joint_xyz"],
                            parts_map, S["H"], S["W"], depth_scale=depth_scale, min_link_pixels=min_link_pixels)


# ---- the host helpers against it ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,parts_map", [(1, [[0]]), (2, [[0], [1]]), (3, [[0], [2, 1]]), (4, [[3], [0, 1]]), (16, [[k] for k in range(15, -1, -1)])],
                         ids=["L1", "L2-joint-rule", "L3", "L4-unused-link", "L16"])
def test_scene_maps_equal_the_restated_chain(L, parts_map):
    """M_s . (x', y', z, 1) against the chain of :298-320 evaluated product by product, at coordinates of magnitude <= 10: 1e-12 absolute."""
    from articulated_pose_amd.depth import SCENE_HEAD, SCENE_LINK, SCENE_WIDTH
    rs = np.random.RandomState(L)
    for trial in range(5):
        S = random_scene(rs, L)
        sc = scene_table(S, parts_map, depth_scale=0.25, min_link_pixels=7)
        assert sc.shape == (SCENE_WIDTH,) and sc.dtype == np.float64 and sc[6] == 0.25 and sc[13] == 7 and sc[14] == L and sc[15] == 0
        flat = [s for g in parts_map for s in g]
        pts = rs.uniform(-10, 10, (200, 3))
        for s in range(L):
            e = sc[SCENE_HEAD + SCENE_LINK * s:SCENE_HEAD + SCENE_LINK * (s + 1)]
            if s in flat:
                assert e[0] == flat.index(s) and e[1] == [j for j, g in enumerate(parts_map) if s in g][0]
            else:
                assert e[0] == -1
            got = np.concatenate([pts, np.ones((200, 1))], 1) @ e[2:].reshape(3, 4).T
            want = chain(S, s, pts)
            assert np.abs(want).max() < 40 and np.abs(got - want).max() <= 1e-12, (L, trial, s, np.abs(got - want).max())
    assert (sc[SCENE_HEAD + SCENE_LINK * L:] == 0).all()


def test_coefficients_equal_the_reference_statements():
    """Both sets of six coefficients against :271-296 on random pixels: x = d (A00 col + A01 row + A02) is the reference's cloud_cam_real /
    cloud_cam column to a few float64 roundings."""
    from articulated_pose_amd.depth import coord_unprojection_from_projmat, unprojection_from_projmat
    rs = np.random.RandomState(3)
    S = random_scene(rs, 1, H=480, W=640)
    S["projMat"][0, 1], S["projMat"][1, 0], S["projMat"][0, 2], S["projMat"][1, 2] = 0.01, -0.02, 0.03, -0.04      # a general matrix
    depth = rs.uniform(0.5, 3.0, (40, 50))
    label = np.zeros((40, 50), int)
    origin = (211, 97)
    pts = restate_frame(S, depth, label, origin)[0][0]
    A, C = unprojection_from_projmat(S["projMat"], 480, 640), coord_unprojection_from_projmat(S["projMat"], 480, 640)
    assert C.dtype == np.float64 and C.shape == (6,)
    row, col = (v.reshape(-1).astype(np.float64) for v in np.indices(depth.shape))
    row, col, d = row + origin[0], col + origin[1], depth.reshape(-1)
    real = np.stack([d * (A[0] * col + A[1] * row + A[2]), d * (A[3] * col + A[4] * row + A[5]), d], 1)
    assert np.abs(real - pts).max() <= 1e-13
    # cloud_cam itself: the chain with identity matrices returns it
    I = dict(S, viewMat=np.eye(4), world_pos=np.zeros((1, 3)), world_orn=np.array([[0, 0, 0, 1.0]]), link_xyz=np.zeros((1, 3)), link_rpy=np.zeros((1, 3)))
    cam = -restate_frame(I, depth, label, origin)[0][1]                  # minus: camera_pose_mat negates the three coordinates
    coord = np.stack([d * (C[0] * col + C[1] * row + C[2]), d * (C[3] * col + C[4] * row + C[5]), d], 1)
    assert np.abs(coord - cam).max() <= 1e-13
    assert not np.allclose(coord[:, 1], real[:, 1])                      # the flipped row matters
    with pytest.raises(ValueError):
        coord_unprojection_from_projmat(np.eye(3), 480, 640)


def test_pack_frame_scene_refusals():
    rs = np.random.RandomState(0)
    S = random_scene(rs, 3)
    for kw in (dict(viewMat=np.eye(3)), dict(projMat=np.eye(3)), dict(world_pos=np.zeros((3, 2))), dict(world_orn=np.zeros((2, 4))),
               dict(link_xyz=np.zeros((2, 3))), dict(link_rpy=np.zeros((3, 4))), dict(world_pos=np.zeros((17, 3)), world_orn=np.zeros((17, 4)))):
        with pytest.raises(ValueError):
            scene_table(dict(S, **kw), [[0], [1, 2]])
    for parts_map in ([[0], [0, 1]], [[0], [3]], [[-1]]):
        with pytest.raises(ValueError, match="parts_map"):
            scene_table(S, parts_map)


# ---- the symbol and its argument checks ---------------------------------------------------------------------------------------------------------
def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_14():
    from articulated_pose_amd import _lib
    from articulated_pose_amd import depth as D
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in declared_symbols() and NAME in exported and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME]) == 14
    assert _L().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    for name, value in (("ANCSH_SCENE_WIDTH", D.SCENE_WIDTH), ("ANCSH_SCENE_MAX_LINKS", D.SCENE_MAX_LINKS), ("ANCSH_SCENE_HEAD", D.SCENE_HEAD),
                        ("ANCSH_SCENE_LINK", D.SCENE_LINK)):
        assert "#define %s %d\n" % (name, value) in header
    assert D.SCENE_WIDTH == 240 == D.SCENE_HEAD + D.SCENE_MAX_LINKS * D.SCENE_LINK


def test_entry_rejects_bad_arguments_before_launch():
    L = _L()

    def call(nclouds=2, kind=0, depth=P16, labels=P16, px=100, geom=P16, scene=P16, rows=P16, cap=100, off=P16, cnt=P16, lc=P16, scratch=P16):
        return L.ancsh_depth_annotate_stream(nclouds, kind, depth, labels, px, geom, scene, rows, cap, off, cnt, lc, scratch, None)
    for kw, msg in ((dict(nclouds=-1), b"bad shape"), (dict(nclouds=65536), b"65535"), (dict(kind=2), b"depth_type=2"),
                    (dict(kind=-1), b"depth_type=-1"), (dict(px=-1), b"pixel_capacity=-1"), (dict(px=1 << 30, cap=1 << 30), b"pixel_capacity"),
                    (dict(px=101), b"capacity=100 rows"), (dict(cap=1 << 30), b"capacity=1073741824"),
                    (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(labels=ctypes.c_void_p(4)), b"8-byte aligned"),
                    (dict(scene=ctypes.c_void_p(4)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for k in ("depth", "labels", "geom", "scene", "rows", "off", "cnt", "lc", "scratch"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nclouds=0, **{k: None}) == -1             # nulls are refused even for an empty batch
    for kind in (0, 1):
        assert call(nclouds=0, kind=kind) == 0                # both depth types; no cloud: nothing launched, no device touched


# ---- the host-side validation -------------------------------------------------------------------------------------------------------------------
def test_check_annotated_frames():
    from articulated_pose_amd.depth import NOT_OBJECT, SCENE_HEAD, SCENE_LINK, check_annotated_frames
    rs = np.random.RandomState(1)
    sc = scene_table(random_scene(rs, 3), [[0], [2, 1]])
    u = np.arange(1, 13, dtype=np.uint16).reshape(3, 4)
    lab = np.array([[0, 1, 2, 3], [-1, 255, 2, 1], [0, 0, 7, 2]], np.int64)
    d, ls, org, nf, scenes = check_annotated_frames([(u, lab, (5, 6)), (u[:, ::2], lab[:, ::2].astype(np.uint8), (0, 0))], [1.0, 2.0], sc, "uint16", 2, 4)
    assert [x.shape for x in d] == [(3, 4), (3, 2)] and d[1].flags.c_contiguous and all(l.dtype == np.uint8 and l.flags.c_contiguous for l in ls)
    assert ls[0].tolist() == [[0, 1, 2, NOT_OBJECT], [NOT_OBJECT, NOT_OBJECT, 2, 1], [0, 0, NOT_OBJECT, 2]] and NOT_OBJECT == 255
    assert ls[1].tolist() == [[0, 2], [NOT_OBJECT, 2], [0, NOT_OBJECT]]
    assert org.tolist() == [[5, 6], [0, 0]] and nf.dtype == np.float32 and scenes.shape == (2, 240) and scenes.dtype == np.float64
    assert np.array_equal(scenes[0], sc) and np.array_equal(scenes[1], sc) and scenes.flags.c_contiguous
    two = check_annotated_frames([(u, lab, (0, 0))] * 2, [1, 1], np.stack([sc, sc]), np.uint16, 2)[4]
    assert two.shape == (2, 240)

    def scene(**kw):
        s = sc.copy()
        for k, v in kw.items():
            s[int(k[1:])] = v
        return s
    r0, r1, r2 = SCENE_HEAD, SCENE_HEAD + SCENE_LINK, SCENE_HEAD + 2 * SCENE_LINK
    bad = [dict(frames=[(u, lab.astype(np.float32), (0, 0))]), dict(frames=[(u, lab != 0, (0, 0))]), dict(frames=[(u, None, (0, 0))]),
           dict(frames=[(u, lab[:2], (0, 0))]), dict(frames=[(u.astype(np.float32), lab, (0, 0))]), dict(frames=[(u[:0], lab[:0], (0, 0))]),
           dict(frames=[(u, lab, (0.5, 0))]), dict(frames=[(u, lab)]), dict(frames=[]), dict(frames=u),
           dict(frames=[(u, lab, (0, 0))] * 5),                                      # more than max_clouds
           dict(norm_factors=[np.nan]), dict(norm_factors=[1.0, 1.0]), dict(depth_dtype="float64"),
           dict(scenes=sc[:239]), dict(scenes=np.stack([sc, sc])), dict(scenes=None), dict(scenes=scene(i3=np.nan)), dict(scenes=scene(i40=np.inf)),
           dict(scenes=scene(i14=0)), dict(scenes=scene(i14=17)), dict(scenes=scene(i14=2.5)), dict(scenes=scene(i13=-1)), dict(scenes=scene(i15=1)),
           dict(scenes=scene(**{"i%d" % r1: 1})),                                   # rank 1 twice
           dict(scenes=scene(**{"i%d" % r0: 3})),                                   # ranks 3 2 1: no permutation of 0..2
           dict(scenes=scene(**{"i%d" % r2: 0.5})), dict(scenes=scene(**{"i%d" % (r2 + 1): 2})),      # a fractional rank; a part beyond K
           dict(scenes=scene(**{"i%d" % (r0 + 1): -1})), dict(scenes=scene(**{"i%d" % (r0 + 1): 0.5}))]
    for kw in bad:
        args = dict(dict(frames=[(u, lab, (0, 0))], norm_factors=[1.0], scenes=sc, depth_dtype="uint16", K=2, max_clouds=4), **kw)
        with pytest.raises(ValueError):
            check_annotated_frames(**args)
    # a link that is not used: rank -1, whatever its part; the others still rank 0 .. used - 1
    ok = scene(**{"i%d" % r1: -1, "i%d" % (r1 + 1): 99, "i%d" % r2: 1})
    assert check_annotated_frames([(u, lab, (0, 0))], [1.0], ok, "uint16", 2)[4][0, r1] == -1


def test_pipelines_refuse_unsupported_combinations_before_gpu_work():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_sharded_stream_cpu import _FakeStreamPipeline
    base = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    for kw, msg in ((dict(build_point_gt=False), "point_ground_truth=True .* depth.*build_point_gt=True"), (dict(label_images=True), "label_images"),
                    (dict(point_ground_truth=False), "build_point_gt=True .* point_ground_truth=True"), (dict(articulation=False), "articulation=True"),
                    (dict(joint_source="gt"), "predicted"), (dict(dense=True), "dense"), (dict(raw_capacity=100), "raw_capacity")):
        with pytest.raises(ValueError, match=msg):
            AncshPipeline(3, None, None, 2, 64, "cpu", **dict(base, **kw))
    with pytest.raises(ValueError, match="depth"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", pipeline_factory=_FakeStreamPipeline, **base)
    # a pipeline of plain depth frames refuses the annotated frames' arguments, one of annotated frames a call without them
    from articulated_pose_amd.stream import check_options
    pipe = AncshPipeline.__new__(AncshPipeline)
    depth = dict(depth_capacity=4096, joint_source="predicted")
    pipe.opts, pipe.B, pipe.K = check_options(**depth), 2, 3
    u = np.ones((3, 4), np.uint16)
    with pytest.raises(ValueError, match="scene needs AncshPipeline"):
        pipe.submit_depth([(u, None, (0, 0))], [1.0], [1, 0, 0, 0, 1, 0], scene=np.zeros(240))
    with pytest.raises(RuntimeError, match="link_counts=True"):
        pipe.retire(link_counts=True)
    pipe.opts = check_options(articulation=True, point_ground_truth=True, build_point_gt=True, **depth)
    for kw in (dict(), dict(scene=np.zeros(240)), dict(rig=np.zeros((1, 10))), dict(scene=np.zeros(240), rig=np.zeros((1, 10)), cameras=[1, 0, 0, 0, 1, 0])):
        with pytest.raises(ValueError, match="annotated frames"):
            pipe.submit_depth([(u, np.zeros((3, 4), int), (0, 0))], [1.0], **kw)
