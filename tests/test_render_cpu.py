"""CPU tests of the renderer (no GPU): the numpy mirror of ancsh_render_depth_labels (tests/render_mirror.py) against analytic ray-box
distances -- the mirror is validated independently of the code under test --, the symbol / ABI, the entry's argument checks before any
launch, depth.pack_mesh's refusals, depth.pack_render_scene against depth.pack_frame_scene, and the pipeline's option rules."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import render_mirror as RM
from test_depth_annotate_cpu import link_matrices, random_scene, scene_table

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "ancsh_render_depth_labels"
P16 = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails its checks first


# ---- meshes and tables the GPU tests share -------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """(vertices (8, 3), faces (12, 3)) of the axis-aligned box [lo, hi]: vertex k has hi's coordinate a where bit a of k is set."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[hi[a] if (k >> a) & 1 else lo[a] for a in range(3)] for k in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)
    return v, f


def pinhole_table(fx, fy, cx, cy, maps, depth_scale=1.0, z_min=1e-6):
    """A render table written directly: col = fx s + cx, row = fy t + cy, and one (3, 4) model -> camera map per link."""
    t = np.zeros(RM.RENDER_WIDTH)
    t[0:6] = fx, 0.0, cx, 0.0, fy, cy
    t[6], t[7], t[8] = depth_scale, z_min, len(maps)
    for l, R in enumerate(maps):
        t[RM.RENDER_HEAD + RM.RENDER_LINK * l:RM.RENDER_HEAD + RM.RENDER_LINK * (l + 1)] = np.asarray(R, np.float64).reshape(12)
    return t


def ray_box(origin, direction, lo, hi):
    """Slab test for rays origin + u direction ((n, 3) directions, one origin): (hit, u of the entry point)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - origin) / direction, (hi - origin) / direction
    near, far = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
    return (near <= far) & (far > 0), near


# ---- the mirror, on its own ---------------------------------------------------------------------------------------------------------------
def test_mirror_equals_analytic_ray_box_distances():
    """An axis-aligned box off the optical axis, three faces in view, in front of a pinhole camera whose principal point is off the pixel
    grid; every vertex projects onto the 1/256-pixel grid exactly, so the fixed point moves nothing and the mirror's perspective-correct
    depth is the ray's.  Depth: 1e-9 relative at every compared pixel.  Coverage: equal to "the ray hits the box", but for the pixels whose
    ray passes within 1e-9 of the silhouette (it hits the box grown by 1e-9 and misses the box shrunk by 1e-9), which neither side
    compares; at most 1 % of the covered pixels are left out."""
    H = W = 128
    fx = fy = 128.0
    cx, cy = 64.0 + 37.0 / 256.0, 64.0 - 91.0 / 256.0
    lo, hi = np.array([0.25, 0.125, 2.0]), np.array([0.75, 0.75, 4.0])
    shift = np.array([0.125, -0.25, 1.0])                                # the link's pose: model = camera - shift
    v, f = box_mesh(lo - shift, hi - shift)
    R = np.concatenate([np.eye(3), shift[:, None]], 1)
    rt = pinhole_table(fx, fy, cx, cy, [R])
    cols = (fx * (v + shift)[:, 0] / (v + shift)[:, 2] + cx) * 256.0
    assert np.abs(cols - np.rint(cols)).max() < 1e-9                      # on the fixed-point grid by construction
    d64 = np.full((H, W), np.nan)
    keys = RM.raster_keys(v.astype(np.float32), f, np.zeros(len(f), int), H, W, 0, 0, rt, depth64=d64)
    covered = keys != RM.EMPTY
    row, col = np.indices((H, W))
    rays = np.stack([(col - cx) / fx, (row - cy) / fy, np.ones((H, W))], -1).reshape(-1, 3)
    eps = 1e-9
    hit, near = ray_box(np.zeros(3), rays, lo, hi)
    grown, shrunk = ray_box(np.zeros(3), rays, lo - eps, hi + eps)[0], ray_box(np.zeros(3), rays, lo + eps, hi - eps)[0]
    compare = ~(grown & ~shrunk).reshape(H, W)
    hit, near = hit.reshape(H, W), near.reshape(H, W)
    left_out = (covered & ~compare).sum()
    print("covered %d pixels, %d on the silhouette left out" % (covered.sum(), left_out))
    assert covered.sum() > 1000 and left_out <= 0.01 * covered.sum()
    assert np.array_equal(covered[compare], hit[compare])
    both = covered & compare
    rel = np.abs(d64[both] - near[both]) / near[both]
    print("worst relative depth error %.3g" % rel.max())
    assert rel.max() <= 1e-9
    assert len(np.unique(keys[covered] & np.uint64(0xFFFFFFFF))) == 6     # three faces in view, two triangles each
    # the resolve: float32 depths are the winners' bits; uint16 at 1 mm keeps every pixel and rounds to nearest
    d32, lab, _ = RM.render_crop(v.astype(np.float32), f, np.zeros(len(f), int), H, W, 0, 0, rt, np.float32)
    assert np.array_equal(d32[covered], d64[covered].astype(np.float32)) and (d32[~covered] == 0).all()
    assert (lab[covered] == 0).all() and (lab[~covered] == RM.NOT_OBJECT).all()
    rt[6] = 1e-3
    d16, lab16, _ = RM.render_crop(v.astype(np.float32), f, np.zeros(len(f), int), H, W, 0, 0, rt, np.uint16)
    assert d16.dtype == np.uint16 and np.array_equal(lab16, lab) and np.abs(d16[covered] * 1e-3 - d64[covered]).max() <= 0.5e-3 + 1e-6


def test_mirror_rules():
    """The drop rules, the tie rule and the edge rule on hand-made triangles at unit depth (col = 8 x + 8, row = 8 y + 8 on a 16 x 16 image)."""
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    rt = pinhole_table(8.0, 8.0, 8.0, 8.0, [I, I])
    tri = lambda *p: np.array(p, np.float32)
    # a right triangle whose hypotenuse passes exactly through sample points: pixels (row 8 + k, col 12 - k) lie on the edge, and are covered
    v = tri((0, 0, 1), (0.5, 0, 1), (0, 0.5, 1))
    keys = RM.raster_keys(v, [[0, 1, 2]], [0], 16, 16, 0, 0, rt)
    cov = keys != RM.EMPTY
    assert cov.sum() == 15 and all(cov[8 + k, 12 - k] for k in range(5)) and not cov[9, 12] and cov[8, 8] and not cov[7, 8]
    assert np.array_equal(RM.raster_keys(v, [[0, 2, 1]], [0], 16, 16, 0, 0, rt) != RM.EMPTY, cov)      # either orientation
    # dropped whole: a vertex behind z_min, a non-finite vertex, a link beyond nlinks, a zero area, an index outside the mesh
    for verts, tris, link in ((tri((0, 0, 1), (0.5, 0, 1), (0, 0.5, -1)), [[0, 1, 2]], [0]), (tri((0, 0, 1), (0.5, 0, np.nan), (0, 0.5, 1)), [[0, 1, 2]], [0]),
                              (v, [[0, 1, 2]], [2]), (tri((0, 0, 1), (0.25, 0.25, 1), (0.5, 0.5, 1)), [[0, 1, 2]], [0]), (v, [[0, 1, 3]], [0]),
                              (tri((0, 0, 1), (0.5, 0, 1), (0, 2.0 ** 22, 1)), [[0, 1, 2]], [0])):
        assert (RM.raster_keys(verts, tris, link, 16, 16, 0, 0, rt) == RM.EMPTY).all()
    # coplanar triangles of two links: the lower index wins wherever both cover
    v2 = np.concatenate([v, v])
    d, lab, keys = RM.render_crop(v2, [[3, 4, 5], [0, 1, 2]], [1, 0], 16, 16, 0, 0, rt, np.float32)
    assert (lab[cov] == 1).all() and ((keys[cov] & np.uint64(0xFFFFFFFF)) == 0).all() and (d[cov] == 1).all()
    # a table that is none: background
    for k, bad in ((8, 0), (8, 17), (8, np.nan), (7, 0.0), (7, np.nan)):
        t = rt.copy()
        t[k] = bad
        assert (RM.raster_keys(v, [[0, 1, 2]], [0], 16, 16, 0, 0, t) == RM.EMPTY).all()
    # crops: the sample point of crop pixel (i, j) is (row0 + i, col0 + j)
    assert np.array_equal(RM.raster_keys(v, [[0, 1, 2]], [0], 5, 7, 6, 7, rt), keys_crop(v, rt, 6, 7, 5, 7))


def keys_crop(v, rt, row0, col0, h, w):
    return RM.raster_keys(v, [[0, 1, 2]], [0], 16, 16, 0, 0, rt)[row0:row0 + h, col0:col0 + w]


# ---- the symbol and its argument checks ----------------------------------------------------------------------------------------------------
def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound():
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
    for name, value in (("ANCSH_RENDER_WIDTH", D.RENDER_WIDTH), ("ANCSH_RENDER_HEAD", D.RENDER_HEAD), ("ANCSH_RENDER_LINK", D.RENDER_LINK)):
        assert "#define %s %d\n" % (name, value) in header
    assert D.RENDER_WIDTH == 208 == D.RENDER_HEAD + D.SCENE_MAX_LINKS * D.RENDER_LINK
    assert (RM.RENDER_WIDTH, RM.RENDER_HEAD, RM.RENDER_LINK, RM.NOT_OBJECT) == (D.RENDER_WIDTH, D.RENDER_HEAD, D.RENDER_LINK, D.NOT_OBJECT)


def test_entry_rejects_bad_arguments_before_launch():
    L = _L()

    def call(nframes=2, kind=0, verts=P16, tris=P16, tri_link=P16, V=8, T=12, geom=P16, render=P16, depth=P16, labels=P16, zbuf=P16, px=100):
        return L.ancsh_render_depth_labels(nframes, kind, verts, tris, tri_link, V, T, geom, render, depth, labels, zbuf, px, None)
    for kw, msg in ((dict(nframes=-1), b"bad shape"), (dict(nframes=65536), b"65535"), (dict(kind=2), b"depth_type=2"), (dict(kind=-1), b"depth_type=-1"),
                    (dict(px=-1), b"pixel_capacity=-1"), (dict(px=1 << 30), b"pixel_capacity"), (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T=16777216"),
                    (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V=16777216"), (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"),
                    (dict(labels=ctypes.c_void_p(4)), b"8-byte aligned"), (dict(render=ctypes.c_void_p(4)), b"8-byte aligned"),
                    (dict(zbuf=ctypes.c_void_p(4)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for k in ("verts", "tris", "tri_link", "geom", "render", "depth", "labels", "zbuf"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nframes=0, **{k: None}) == -1             # nulls are refused even for an empty batch
    for kind in (0, 1):
        assert call(nframes=0, kind=kind) == 0                # both depth types; no frame: nothing launched, no device touched
        assert call(nframes=0, kind=kind, T=0, V=0) == 0


# ---- the host helpers -----------------------------------------------------------------------------------------------------------------------
def test_pack_mesh():
    from articulated_pose_amd.depth import pack_mesh
    v, f = box_mesh([0, 0, 0], [1, 2, 3])
    verts, tris, tri_link = pack_mesh([(v, f), None, (v + 5, f[:4])])
    assert verts.shape == (16, 3) and verts.dtype == np.float32 and tris.shape == (16, 3) and tris.dtype == np.int32 and tri_link.dtype == np.int32
    assert all(a.flags.c_contiguous for a in (verts, tris, tri_link)) and tri_link.tolist() == [0] * 12 + [2] * 4
    assert np.array_equal(tris[:12], f) and np.array_equal(tris[12:], f[:4] + 8) and np.array_equal(verts[8:], (v + 5).astype(np.float32))
    empty = pack_mesh([None, None])
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0,)]
    bad_v = v.copy()
    bad_v[3, 1] = np.inf
    for links in ([(bad_v, f)], [(v * 1e39, f)], [(v, f + 1)], [(v, -f)], [(v, f.astype(np.float64))], [(v[:, :2], f)], [(v, f[:, :2])], [(v, f)] * 17, [v], (v, f)):
        with pytest.raises(ValueError):
            pack_mesh(links)


@pytest.mark.parametrize("L,parts_map", [(1, [[0]]), (2, [[0], [1]]), (3, [[0], [2, 1]])], ids=["L1", "L2-joint-rule", "L3"])
def test_render_scene_inverts_the_frame_scene(L, parts_map):
    """Random views and model points: M_l of the frame's scene applied to R_l v is canon2urdf_l v, and coordinate-unprojecting the pixel
    the render table projects v to, at depth z, returns R_l v -- both to 1e-10."""
    from articulated_pose_amd.depth import RENDER_HEAD, RENDER_LINK, SCENE_HEAD, SCENE_LINK, pack_render_scene
    rs = np.random.RandomState(10 + L)
    for trial in range(6):
        S = random_scene(rs, L, H=480 if trial % 2 else 512, W=640 if trial % 2 else 512)
        sc = scene_table(S, parts_map, depth_scale=0.5)
        rt = pack_render_scene(S["viewMat"], S["projMat"], S["world_pos"], S["world_orn"], S["H"], S["W"], depth_scale=0.5, z_min=1e-3)
        assert rt.shape == (208,) and rt.dtype == np.float64 and rt[6] == 0.5 and rt[7] == 1e-3 and rt[8] == L and (rt[9:16] == 0).all()
        assert (rt[RENDER_HEAD + RENDER_LINK * L:] == 0).all()
        _, canon2urdf = link_matrices(S)
        v = rs.uniform(-1, 1, (200, 3))
        v1 = np.concatenate([v, np.ones((200, 1))], 1)
        for l in range(L):
            R = rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)].reshape(3, 4)
            M = sc[SCENE_HEAD + SCENE_LINK * l + 2:SCENE_HEAD + SCENE_LINK * (l + 1)].reshape(3, 4)
            q = v1 @ R.T                                                 # the camera point (x', y', z)
            got = np.concatenate([q, np.ones((200, 1))], 1) @ M.T
            want = (v1 @ canon2urdf[l].T)[:, :3]
            assert np.abs(got - want).max() <= 1e-10, (L, trial, l, np.abs(got - want).max())
            keep = np.abs(q[:, 2]) > 0.05                                 # away from the camera's plane, where s and t are unbounded
            q = q[keep]
            assert keep.sum() > 150
            s, t, z = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], q[:, 2]
            col, row = (rt[0] * s + rt[1] * t) + rt[2], (rt[3] * s + rt[4] * t) + rt[5]
            back = np.stack([z * ((sc[7] * col + sc[8] * row) + sc[9]), z * ((sc[10] * col + sc[11] * row) + sc[12]), z], 1)
            assert np.abs(back - q).max() <= 1e-10, (L, trial, l, np.abs(back - q).max())
    S = random_scene(rs, 2)
    for kw in (dict(viewMat=np.eye(3)), dict(projMat=np.eye(3)), dict(world_pos=np.zeros((2, 2))), dict(world_orn=np.zeros((3, 4))),
               dict(world_pos=np.zeros((17, 3)), world_orn=np.zeros((17, 4))), dict(depth_scale=0.0), dict(z_min=0.0), dict(z_min=np.nan)):
        a = dict(dict(viewMat=S["viewMat"], projMat=S["projMat"], world_pos=S["world_pos"], world_orn=S["world_orn"], depth_scale=1.0, z_min=1e-6), **kw)
        with pytest.raises(ValueError):
            pack_render_scene(a["viewMat"], a["projMat"], a["world_pos"], a["world_orn"], 512, 512, a["depth_scale"], a["z_min"])


def test_render_tables_and_crops_are_checked():
    from articulated_pose_amd.depth import check_crops, check_render_tables
    rt = pinhole_table(64, 64, 32, 32, [np.eye(4)[:3]] * 2)
    assert check_render_tables(rt, 3).shape == (3, 208) and check_render_tables(np.stack([rt, rt]), 2).flags.c_contiguous
    for k, bad in ((6, 0.0), (7, -1.0), (8, 0), (8, 17), (8, 1.5), (9, 1.0), (40, np.nan)):
        t = rt.copy()
        t[k] = bad
        with pytest.raises(ValueError):
            check_render_tables(t, 1)
    for bad in (rt[:207], np.stack([rt, rt]), None):
        with pytest.raises(ValueError):
            check_render_tables(bad, 3)
    shapes, origins = check_crops([(3, 4, (5, 6)), (1, 1, (-2, 0))], 2)
    assert shapes == [(3, 4), (1, 1)] and origins.tolist() == [[5, 6], [-2, 0]] and origins.dtype == np.int32
    for bad in ([], [(3, 4, (5, 6))] * 3, [(0, 4, (0, 0))], [(3, 4)], [(3.5, 4, (0, 0))], [(3, 4, (1 << 24, 0))], (3, 4, (0, 0)), [(40000, 40000, (0, 0))]):
        with pytest.raises(ValueError):
            check_crops(bad, 2)


# ---- the pipeline's rules -------------------------------------------------------------------------------------------------------------------
def test_options_and_submit_refusals_before_gpu_work():
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import ALL_INPUTS, SIDE, SIDE_INPUTS, check_options
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    for kw in (dict(raw_capacity=1000), dict(depth_capacity=4096, joint_source="predicted"), dict(),
               dict(raw_capacity=1000, articulation=True, point_ground_truth=True, build_point_gt=True)):
        with pytest.raises(ValueError, match="render_mesh .* depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True"):
            check_options(render_mesh=mesh, **kw)
        with pytest.raises(ValueError, match="render_mesh"):
            AncshPipeline(3, None, None, 2, 64, "cpu", render_mesh=mesh, **kw)
    off, on = check_options(**annotated), check_options(render_mesh=mesh, **annotated)
    assert on.render and not off.render and [i.name for i in on.inputs] == ["render"] + [i.name for i in off.inputs]
    assert on._replace(render=False, inputs=()) == off._replace(inputs=())
    for extra in (dict(ground_truth=True, build_gt_pose=True), dict(fit_quality=True, joint_states=True, keyed=True, range_guard=True)):
        assert check_options(render_mesh=mesh, **dict(annotated, **extra)).render
    r = SIDE["render"]
    assert ALL_INPUTS == (r,) + SIDE_INPUTS and (str(r.dtype), r.shape(3), r.pad) == ("torch.float64", (208,), "first") and r.missing
    # each submit refuses the other's pipeline
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.B, pipe.K = on, 2, 3
    with pytest.raises(RuntimeError, match="submit_render"):
        pipe.submit_depth([(np.ones((3, 4), np.uint16), np.zeros((3, 4), int), (0, 0))], [1.0], scene=np.zeros(240), rig=np.zeros((1, 10)))
    for opts in (off, check_options(depth_capacity=4096, joint_source="predicted"), check_options(raw_capacity=1000)):
        pipe.opts = opts
        with pytest.raises(RuntimeError, match="render_mesh=.*submit_depth"):
            pipe.submit_render([(3, 4, (0, 0))], [1.0], np.zeros(208), np.zeros(240), np.zeros((1, 10)))
    # the front end's own checks come before anything is enqueued (no device is touched: the options alone decide)
    pipe.opts = on
    pipe._inflight, pipe.slots = [], []
    rt = pinhole_table(64, 64, 32, 32, [np.eye(4)[:3]])
    from articulated_pose_amd.stream import unit_scene
    from articulated_pose_amd.dataset import identity_rig
    good = dict(crops=[(3, 4, (0, 0))], norm_factors=[1.0], render=rt, scene=unit_scene(3, (1, 0, 0, 0, 1, 0, 1)), rig=identity_rig(3)[None])
    for kw in (dict(render=None), dict(scene=None), dict(rig=None), dict(crops=[(0, 4, (0, 0))]), dict(crops=[(3, 4, (0, 0))] * 3), dict(norm_factors=[np.nan]),
               dict(render=rt[:100]), dict(render=np.where(np.arange(208) == 8, 0, rt)), dict(crops=[(64, 65, (0, 0))]), dict(frame=np.zeros((2, 13)))):
        with pytest.raises(ValueError):
            pipe.submit_render(**dict(good, **kw))


# ---- an articulated object in front of a camera of the reference's conventions (shared with the GPU tests) ---------------------------------------
BOX_LO, BOX_HI = np.array([-0.16, -0.11, -0.06]), np.array([0.16, 0.11, 0.06])


def object_mesh(L):
    """L equal boxes, one per link, each in its link's model frame -> depth.pack_mesh's arrays."""
    from articulated_pose_amd.depth import pack_mesh
    return pack_mesh([box_mesh(BOX_LO, BOX_HI)] * L)


def object_scene(rs, L, H=64, W=64, opening=0.6):
    """random_scene's dictionary for an object of L <= 3 links the camera looks at from about 1.5 units: link 0 at the world's origin as the
    reference sets it, link 1 beside it and opened by `opening` radians about its hinge, link 2 on the other side; a slightly random view."""
    from test_depth_annotate_cpu import axis_rotation, euler_sxyz, random_rotation
    t, near, far = np.tan(np.radians(20.0)), 0.1, 100.0
    P = np.array([[1.0 / (t * W / H), 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1.0, 0]])
    V = np.eye(4)
    V[:3, :3] = euler_sxyz(*rs.uniform(-0.5, 0.5, 3))[:3, :3]
    V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
    pos = np.array([[0.0, 0.0, 0.0], [0.3, 0.02, 0.12], [-0.34, -0.03, 0.02]])[:L]
    orn = np.array([[0, 0, 0, 1.0], [0, np.sin(opening / 2), 0, np.cos(opening / 2)], [0, 0, np.sin(0.2), np.cos(0.2)]])[:L]      # [x y z w]
    return dict(H=H, W=W, projMat=P, viewMat=V, world_pos=pos, world_orn=orn, link_xyz=rs.uniform(-0.1, 0.1, (L, 3)),
                link_rpy=rs.uniform(-0.5, 0.5, (L, 3)), joint_xyz=rs.uniform(-0.1, 0.1, (max(L - 1, 1), 3)))


def render_table(S, depth_scale=1.0, z_min=1e-6):
    from articulated_pose_amd.depth import pack_render_scene
    return pack_render_scene(S["viewMat"], S["projMat"], S["world_pos"], S["world_orn"], S["H"], S["W"], depth_scale=depth_scale, z_min=z_min)


def test_object_scenes_show_every_link():
    """The shared scenes are fit for their tests: every link of the two- and three-link objects shows some hundred pixels of a 64 x 64 image."""
    rs = np.random.RandomState(0)
    for L in (2, 3):
        verts, tris, tri_link = object_mesh(L)
        for _ in range(3):
            S = object_scene(rs, L)
            _, lab, _ = RM.render_crop(verts, tris, tri_link, 64, 64, 0, 0, render_table(S, 1e-3), np.uint16)
            hist = np.bincount(lab.reshape(-1), minlength=256)
            print(L, hist[:L], hist[255])
            assert (hist[:L] > 100).all() and hist[255] > 1000 and hist[L:255].sum() == 0
