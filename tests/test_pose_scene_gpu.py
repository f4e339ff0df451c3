"""GPU: ancsh_pose_scene_build and ancsh_render_centre_crops against their numpy mirror (tests/pose_scene_mirror.py, validated on its own in
tests/test_pose_scene_cpu.py) inside red zones; the round trip tables -> renderer -> annotation back onto the boxes' surfaces; and
AncshPipeline(render_mesh=..., kinematics=...) against the rendering pipeline fed the eager operators' tables and origins."""
import numpy as np
import pytest
import torch

import pose_scene_mirror as PM
from redzone import Arena
from test_depth_annotate_cpu import random_scene
from test_pose_scene_cpu import hand_mesh, kin_table, random_view, tree
from test_render_cpu import BOX_HI, BOX_LO, object_mesh, object_scene, pinhole_table
from test_render_gpu import B_, CAP_, DTYPES, K_, LINKS_, MAP_, N_, SCALE, _bytes, _surface_distance, _weights

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
C = PM.CROP_CENTRE


# ---- the table builder ------------------------------------------------------------------------------------------------------------------------
def _build(dev, kin, poses):
    """One call of the entry on redzone-guarded outputs prefilled with a sentinel -> (render (n, 208), scene (n, 240)) as numpy arrays."""
    from articulated_pose_amd import _lib
    n = poses.shape[0]
    arena = Arena()
    d_kin, d_pose = arena.empty((PM.KIN_WIDTH,), dtype=torch.float64, device=dev), arena.empty((n, PM.POSE_WIDTH), dtype=torch.float64, device=dev)
    render, scene = arena.empty((n, PM.RENDER_WIDTH), dtype=torch.float64, device=dev), arena.empty((n, PM.SCENE_WIDTH), dtype=torch.float64, device=dev)
    d_kin.copy_(torch.from_numpy(kin))
    d_pose.copy_(torch.from_numpy(poses))
    render.fill_(SENTINEL)
    scene.fill_(SENTINEL)
    _lib.call("ancsh_pose_scene_build", n, _lib.ptr(d_kin), _lib.ptr(d_pose), _lib.ptr(render), _lib.ptr(scene))
    torch.cuda.synchronize()
    out = render.cpu().numpy(), scene.cpu().numpy()
    arena.check()
    return out


def _object(rs, L):
    """(kin, parts_map) of an L-link object: L = 3 has one revolute and one prismatic joint, L = 16 is a chain of depth 15 that mixes all
    three kinds."""
    parts_map = [[k] for k in range(L - 1, -1, -1)]
    Tr = tree(rs, L, "chain") if L != 3 else tree(rs, 3, "star", ["fixed", "revolute", "prismatic"])
    return kin_table(random_scene(rs, L), Tr, parts_map, depth_scale=0.5, z_min=1e-3, min_link_pixels=7)


@pytest.mark.parametrize("L", [1, 3, 16])
def test_table_builder_equals_the_mirror(dev, L):
    """nframes = 1, 3 and 65 (65 x 16 threads cross a block boundary), random joint values and rigid views, every third frame at q = 0.  The
    heads and every link whose chain passes no revolute joint at q != 0 are bit-equal (the device's sincos(0) is (0, 1) exactly, so frames
    with all q = 0 are bit-equal whole); every other entry differs by sincos' last bits alone, through at most 15 joints: within 1e-12 (1 +
    max |translation entry|) of the mirror.  Links >= nlinks and reserved fields read 0; a second call gives the same bytes."""
    from articulated_pose_amd.depth import pack_pose
    rs = np.random.RandomState(60 + L)
    kin = _object(rs, L)
    for n in (1, 3, 65):
        poses = np.stack([pack_pose(np.zeros(L) if f % 3 == 2 else rs.uniform(-2, 2, L), random_view(rs)) for f in range(n)])
        want_r, want_s = PM.build_tables(kin, poses)
        got_r, got_s = _build(dev, kin, poses)
        free = PM.sincos_free(kin, poses)
        assert _bytes(got_r[:, :16], want_r[:, :16]) and _bytes(got_s[:, :16], want_s[:, :16]), (L, n)
        assert (got_r[:, 9:16] == 0).all() and (got_r[:, 16 + 12 * L:] == 0).all() and (got_s[:, 16 + 14 * L:] == 0).all()
        links_r, links_s = (lambda a: a[:, 16:].reshape(n, 16, 12)), (lambda a: a[:, 16:].reshape(n, 16, 14))
        assert free[:, 0].all() and free[2::3].all()
        assert _bytes(links_r(got_r)[free], links_r(want_r)[free]) and _bytes(links_s(got_s)[free], links_s(want_s)[free]), (L, n)
        trans = max(np.abs(links_r(want_r)[:, :, 3::4]).max(), np.abs(links_s(want_s)[:, :, 5::4]).max())
        tol = 1e-12 * (1.0 + trans)
        worst = max(np.abs(got_r - want_r).max(), np.abs(got_s - want_s).max())
        print("L = %d, %d frames: worst |device - mirror| = %.3g (bound %.3g, %d of %d links pass a sincos)" % (L, n, worst, tol, (~free[:, :L]).sum(), n * L))
        assert worst <= tol, (L, n, worst, tol)
        if L > 1 and n > 1:
            assert (~free[:, :L]).any()
        again_r, again_s = _build(dev, kin, poses)
        assert _bytes(again_r, got_r) and _bytes(again_s, got_s), (L, n)


# ---- the crop centring -------------------------------------------------------------------------------------------------------------------------
def _centre(dev, mesh, geom, tables, nframes=None):
    """Two calls of the entry on redzone-guarded geom / bounds -> (geom after the first call, geom after the second)."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import mesh_to_device
    verts, tris, tri_link, V, T = mesh_to_device(mesh, dev)
    geom, tables = np.ascontiguousarray(geom, np.int32).reshape(-1, 5), np.ascontiguousarray(tables, np.float64).reshape(-1, PM.RENDER_WIDTH)
    n = geom.shape[0]
    arena = Arena()
    d_geom, bounds = arena.empty((n, 5), dtype=torch.int32, device=dev), arena.empty((n, 4), dtype=torch.int32, device=dev)
    d_tables = arena.empty((n, PM.RENDER_WIDTH), dtype=torch.float64, device=dev)
    d_geom.copy_(torch.from_numpy(geom))
    d_tables.copy_(torch.from_numpy(tables))
    out = []
    for _ in range(2):
        _lib.call("ancsh_render_centre_crops", n if nframes is None else nframes, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), V, T,
                  _lib.ptr(d_tables), _lib.ptr(d_geom), _lib.ptr(bounds))
        torch.cuda.synchronize()
        out.append(d_geom.cpu().numpy())
    arena.check()
    return out


def _posed_object(rs, dtype="uint16", far=False):
    """The three-link object of the rendering tests as a kinematic tree in front of object_scene's camera: link 1 hinged about y beside link 0,
    link 2 sliding along its x on the other side.  -> (kin, the scene dictionary; its view is one valid view).  far: the camera stands 2.6
    units off and to the side, so the whole object shows off the image's centre."""
    S = object_scene(rs, LINKS_)
    if far:
        S["viewMat"][:3, 3] = (0.3, -0.2, -2.6)
    Tr = dict(parents=[-1, 0, 0], kinds=["fixed", "revolute", "prismatic"], joint_xyz=[(0, 0, 0), (0.3, 0.02, 0.12), (-0.34, -0.03, 0.02)],
              joint_rpy=[(0, 0, 0), (0, 0, 0), (0, 0, 0.4)], joint_axis=[(0, 0, 0), (0, 1, 0), (1, 0, 0)])
    return kin_table(S, Tr, MAP_, depth_scale=SCALE[dtype]), S


def _poses(rs, S, n, far=False):
    from articulated_pose_amd.depth import pack_pose
    out = []
    for _ in range(n):
        V = object_scene(rs, LINKS_)["viewMat"]
        if far:
            V[:3, 3] = S["viewMat"][:3, 3]
        out.append(pack_pose([0.0, rs.uniform(0.2, 1.1), rs.uniform(-0.03, 0.03)], V))
    return np.stack(out)


def test_centring_equals_the_mirror(dev):
    """One frame and three frames of the posed object (the mirror is fed the device-built render tables), centred and fixed crops mixed --
    the fixed ones are left alone --, T == 0, a vertex behind z_min, nframes == 0: origins byte for byte, a second call is a no-op, and the
    guards around geom and bounds stay intact."""
    from articulated_pose_amd.depth import pose_scene_tables
    rs = np.random.RandomState(21)
    kin, S = _posed_object(rs)
    mesh = object_mesh(LINKS_)
    tables, _ = pose_scene_tables(kin, _poses(rs, S, 3), dev)
    cases = [("one frame", mesh, [(0, 64, 64, C, C)], tables[:1]),
             ("three frames, mixed", mesh, [(0, 40, 33, C, C), (1320, 64, 64, 3, -2), (5416, 17, 64, C, C)], tables),
             ("a sentinel in one place only", mesh, [(0, 8, 8, C, 0), (64, 8, 8, 0, C), (128, 9, 8, C, C)], tables),
             ("T == 0", (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0,), np.int32)), [(0, 64, 64, C, C)], tables[:1])]
    I = np.eye(4)[:3]
    hand = hand_mesh()
    cases.append(("a vertex behind z_min", hand, [(0, 10, 11, C, C), (110, 11, 10, C, C)],
                  np.stack([pinhole_table(32.0, 32.0, 32.0, 32.0, [I]), pinhole_table(32.0, 32.0, -50.0, 32.0, [I])])))
    for what, m, geom, rt in cases:
        geom = np.asarray(geom, np.int32)
        want = PM.centre_origins(m[0], m[1], m[2], m[0].shape[0], geom, rt)
        first, second = _centre(dev, m, geom, rt)
        assert _bytes(first, want), (what, first.tolist(), want.tolist())
        assert _bytes(second, first), what
        assert np.array_equal(first[:, :3], geom[:, :3]), what
    assert want[:, 3:].tolist() == [[36 - 5, 28 - 5], [36 - 5, -54 - 5]]      # the hand-computed origins of the CPU test, floor included
    untouched = np.asarray([(0, 64, 64, C, C)], np.int32)
    first, second = _centre(dev, mesh, untouched, tables[:1], nframes=0)
    assert _bytes(first, untouched) and _bytes(second, untouched)          # nframes == 0 launches nothing
    # the eager wrapper returns the same origins
    from articulated_pose_amd.depth import centre_crops
    got = centre_crops(mesh, tables, [(40, 33), (64, 64), (17, 64)], dev)
    want = PM.centre_origins(mesh[0], mesh[1], mesh[2], mesh[0].shape[0], [(0, 40, 33, C, C), (0, 64, 64, C, C), (0, 17, 64, C, C)], tables)
    assert got.dtype == np.int32 and got.tolist() == want[:, 3:].tolist()


# ---- the round trip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_round_trip_lands_on_the_boxes_and_centred_crops_hold_the_object(dev, dtype):
    """Tables from the entry -> ancsh_render_depth_labels -> ancsh_depth_annotate_stream: every row's canonical coordinates, taken back into
    its link's model frame with the table's own Rc_l and offset_l, lie on the link's box within the bound the rendering tests use
    ((depth_scale / 2) max |(s, t, 1)| over the image corners plus 4 * 2^-24 max |c|): the forward kinematics are tied to the geometry, not
    only to the mirror.  And a centred 64 x 64 crop of an object that stands off the image's centre holds every object pixel of the
    full-image render of the same frame, with the same bytes."""
    from articulated_pose_amd.depth import annotate_depth_batch, centre_crops, pose_scene_tables, render_depth_frames
    rs = np.random.RandomState(33)
    scale, mesh = SCALE[dtype], object_mesh(LINKS_)
    kin, S = _posed_object(rs, dtype)
    tables, scenes = pose_scene_tables(kin, _poses(rs, S, 3), dev)
    crops = [(64, 64, (0, 0)), (40, 64, (12, 0)), (64, 64, (0, 0))]
    frames = render_depth_frames(mesh, tables, crops, dtype, dev)
    rows, off, cnt, lc = annotate_depth_batch(frames, scenes, dtype, K_)
    links = kin[PM.KIN_HEAD:PM.KIN_HEAD + PM.KIN_LINK * LINKS_].reshape(LINKS_, PM.KIN_LINK)
    lo, hi = BOX_LO.astype(np.float32).astype(np.float64), BOX_HI.astype(np.float32).astype(np.float64)
    for b in range(3):
        hist = np.bincount(frames[b][1].reshape(-1), minlength=256)
        assert lc[b].tolist() == hist[:LINKS_].tolist() + [0] * 13 and cnt[b] == hist[:LINKS_].sum() and (hist[:LINKS_] > 60).all(), (b, lc[b])
        got = rows[off[b]:off[b] + cnt[b]].astype(np.float64)
        sc = scenes[b]
        corners = np.array([[(sc[7] * c + sc[8] * r) + sc[9], (sc[10] * c + sc[11] * r) + sc[12], 1.0] for r in (0, 63) for c in (0, 63)])
        bound = scale / 2 * np.linalg.norm(corners, axis=1).max() + 4 * 2.0 ** -24 * np.abs(got[:, 3:6]).max()
        for l in range(LINKS_):
            part = MAP_.index([l])
            c = got[got[:, 6] == part, 3:6]
            Rc, offset = links[l, 19:28].reshape(3, 3), links[l, 28:31]
            dist = _surface_distance((c - offset) @ Rc, lo, hi)          # Rc is a rotation: its inverse keeps distances
            print("%s frame %d link %d: %d rows, worst distance / bound = %.3f (bound %.3g)" % (dtype, b, l, len(c), dist.max() / bound, bound))
            assert len(c) == hist[l] and dist.max() <= bound, (dtype, b, l, dist.max(), bound)
    # the centred crop
    kin, S = _posed_object(rs, dtype, far=True)
    tables, _ = pose_scene_tables(kin, _poses(rs, S, 2, far=True), dev)
    origins = centre_crops(mesh, tables, [(64, 64)] * 2, dev)
    full = render_depth_frames(mesh, tables, [(64, 64, (0, 0))] * 2, dtype, dev)
    centred = render_depth_frames(mesh, tables, [(64, 64, (int(r), int(c))) for r, c in origins], dtype, dev)
    for f in range(2):
        r0, c0 = (int(v) for v in origins[f])
        i, j = np.nonzero(full[f][1] != 255)
        print("frame %d: origin (%d, %d), %d object pixels in the full image, %d in the centred crop" % (f, r0, c0, len(i), (centred[f][1] != 255).sum()))
        assert len(i) > 100 and max(abs(r0), abs(c0)) >= 4                # the object stands off the image's centre
        assert (i - r0 >= 0).all() and (i - r0 < 64).all() and (j - c0 >= 0).all() and (j - c0 < 64).all(), (f, r0, c0)
        assert np.array_equal(centred[f][1][i - r0, j - c0], full[f][1][i, j]) and _bytes(centred[f][0][i - r0, j - c0], full[f][0][i, j])
        assert (centred[f][1] != 255).sum() >= len(i)


# ---- the stream ------------------------------------------------------------------------------------------------------------------------------------
def _pipes(pb, dtype, mesh, kin, **kw):
    """(the posed pipeline, the rendering pipeline) with the same arguments otherwise."""
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=4, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype, render_mesh=mesh), **kw)
    mk = lambda **more: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **more))
    return mk(kinematics=kin), mk()


@pytest.mark.parametrize("dtype,slots,options", [("uint16", 1, {}), ("float32", 4, {}), ("uint16", 4, dict(ground_truth=True, build_gt_pose=True)),
                                                 ("uint16", 2, dict(range_guard=True, arithmetic="f16x2", joint_states=True,
                                                                    joint_types=["revolute", "prismatic"]))],
                         ids=["u16-1slot", "f32-4slots", "gt-pose", "guard-states-prismatic"])
def test_posed_stream_equals_the_rendered_stream(dev, dtype, slots, options):
    """Six batches, one of them short, half of the crops centred and half at fixed origins: records, articulation blocks, counts and link
    counts of stream_posed_batches equal, byte for byte, those of stream_render_batches on a render_mesh= pipeline fed pose_scene_tables'
    tables and centre_crops' origins for the same poses.  One graph per slot serves every batch; the refusals leave nothing in flight."""
    from articulated_pose_amd.depth import centre_crops, pose_scene_tables
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    pb, mesh = _weights(), object_mesh(LINKS_)
    rs = np.random.RandomState(13)
    kin, S = _posed_object(rs, dtype)
    Pp, R = _pipes(pb, dtype, mesh, kin, slots=slots, **options)
    Pp.prepare()
    sl = Pp.slots[0]
    assert sl.pose.shape == (B_, 32) and sl.render.shape == (B_, 208) and sl.scene.shape == (B_, 240) and sl.bounds.shape == (B_, 4)
    assert not hasattr(sl, "h_render") and not hasattr(sl, "h_scene") and sl.h_pose.is_pinned() and Pp.kin.shape == (672,) and R.kin is None
    graphs = [s.graph for s in Pp.slots]
    feed_p, feed_r = [], []
    for k in range(6):
        n = 1 if k == 2 else 2
        poses = _poses(rs, S, n)
        sizes = [(int(rs.randint(56, 65)), int(rs.randint(56, 65))) for _ in range(n)]
        fixed = [(int(rs.randint(0, 3)), int(rs.randint(0, 3))) for _ in range(n)]
        centred = [(f + k) % 2 == 0 for f in range(n)]
        nf = rs.uniform(0.9, 1.1, n).astype(np.float32)
        side = dict(rig=np.tile(stream_rig(), (n, 1)))
        if options.get("build_gt_pose"):
            side["gt"] = pack_box_extents([np.tile(BOX_HI - BOX_LO, (K_, 1))] * n)
        else:
            side["frame"] = random_frames(rs, n)
        rt, sc = pose_scene_tables(kin, poses, dev)
        org = centre_crops(mesh, rt, sizes, dev)
        feed_p.append(([(h, w, None if c else o) for (h, w), c, o in zip(sizes, centred, fixed)], nf, dict(side, pose=poses), "t%d" % k))
        feed_r.append(([(h, w, (int(g[0]), int(g[1])) if c else o) for (h, w), c, o, g in zip(sizes, centred, fixed, org)], nf,
                       dict(side, render=rt, scene=sc), "t%d" % k))
    got = list(Pp.stream_posed_batches(feed_p, articulation=True, link_counts=True))
    want = list(R.stream_render_batches(feed_r, articulation=True, link_counts=True))
    assert all(g is not None and g is s.graph for g, s in zip(graphs, Pp.slots))       # one graph per slot served every batch
    assert len(got) == len(want) == 6 and [g[0] for g in got] == ["t%d" % k for k in range(6)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 6 and g[:2] == w[:2], k
        for a, b in zip(g[2:], w[2:]):                                   # record, articulation block, counts, link counts
            assert _bytes(a, b), k
    assert got[2][2].shape[0] == 1 and got[0][2].shape == (2, K_, got[0][2].shape[2]) and np.isfinite(got[0][2][:, :, :26]).any()
    assert all((g[4] > 300).all() for g in got)
    # bad input: ValueError before anything is enqueued; the wrong method: RuntimeError that names the right one; the pipeline stays usable
    crops, nf, side, _ = feed_p[0]
    good = dict(side, crops=crops, norm_factors=nf)
    skew = side["pose"].copy()
    skew[0, 16] += 1e-3
    for kw in (dict(pose=None), dict(rig=None), dict(pose=skew), dict(pose=side["pose"][:, :30]), dict(crops=[(64, 64, None)] * 3),
               dict(crops=[(100, 90, None)] * 2), dict(crops=[(64, 0, None)] * 2), dict(norm_factors=[1.0])):
        with pytest.raises(ValueError):
            Pp.submit_posed(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="submit_posed"):
        Pp.submit_render(**dict(feed_r[0][2], crops=feed_r[0][0], norm_factors=nf))
    with pytest.raises(RuntimeError, match="submit_posed"):
        Pp.submit_depth([(np.ones((4, 4), DTYPES[dtype]), np.zeros((4, 4), int), (0, 0))], [1.0], rig=side["rig"][:1])
    with pytest.raises(RuntimeError, match="submit_render"):
        R.submit_posed(**good)
    assert not Pp._inflight and not R._inflight
    Pp.submit_posed(seed=got[0][1], **good)
    again = Pp.retire(articulation=True, link_counts=True)
    assert all(_bytes(a, b) for a, b in zip(again[2:], got[0][2:]))


def test_launch_budget(dev):
    """The posed step is the rendering step behind TWO more ABI calls, in front of ancsh_render_depth_labels; a pipeline without
    kinematics= issues neither."""
    from test_fit_quality_gpu import _launch_names
    kin, _ = _posed_object(np.random.RandomState(2))
    Pp, R = _pipes(_weights(), "uint16", object_mesh(LINKS_), kin, slots=1)
    on, off = _launch_names(Pp.prepare()), _launch_names(R.prepare())
    assert on[:3] == ["ancsh_pose_scene_build", "ancsh_render_centre_crops", "ancsh_render_depth_labels"] and on[2:] == off
    assert "ancsh_pose_scene_build" not in off and "ancsh_render_centre_crops" not in off
