"""GPU: the three *_lib entries against the single-object entries on each instance's own mesh or table, byte for byte and inside red zones
at a misalignment (the mirror of a library frame is the existing mirror called on that instance's own mesh: tests/render_mirror.py,
tests/pose_scene_mirror.py); frames whose instance value names none; and AncshPipeline(render_mesh=<library>, kinematics=<stack>) against the
annotated depth pipeline fed frames rendered eagerly instance by instance."""
import numpy as np
import pytest
import torch

import pose_scene_mirror as PM
import render_mirror as RM
from redzone import Arena
from test_mesh_library_cpu import fan_mesh
from test_render_cpu import BOX_HI, BOX_LO, box_mesh, object_mesh, object_scene, pinhole_table, render_table

pytestmark = pytest.mark.gpu
DTYPES = {"uint16": np.uint16, "float32": np.float32}
FILL = {"uint16": 0x5A5A, "float32": -7.0}
SCALE = {"uint16": 1e-3, "float32": 1.0}
LABEL_FILL, SENTINEL = 77, -7.0
C = PM.CROP_CENTRE
BAD = (-1.0, None, 0.5, np.nan)          # instance values that name no instance; None stands for ninst itself


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the library of the renderer's tests ----------------------------------------------------------------------------------------------------------
def _instances():
    """Four instances, in the issue's order: 0: one box, 12 triangles of link 0; 1: a fan of 70 triangles over 3 links (no multiple of the 4
    waves of a block, 18 blocks), a disc of radius 0.6 through the box's centre, so it covers the box's pixels under the box's own maps; 2: no
    triangle; 3: two coincident triangles, the lower index on link 1, the higher on link 0."""
    from articulated_pose_amd.depth import pack_mesh
    tie = (np.array([(0, 0, 1), (0.5, 0, 1), (0, 0.5, 1)], np.float32), np.array([(0, 1, 2), (2, 1, 0)], np.int32), np.array([1, 0], np.int32))
    return [object_mesh(1), pack_mesh(fan_mesh(70, 3, radius=0.6)), pack_mesh([]), tie]


FRAMES = [3, 0, 1, 0, 2, 1]
CROPS = [(24, 32, (28, 24)), (17, 9, (24, 27)), (33, 40, (14, 10)), (1, 1, (32, 32)), (17, 9, (20, 30)), (24, 32, (20, 16))]


def _frame_tables(rs, dtype, frames=FRAMES):
    """One render table per frame, its instance in value 9: a general three-link view, but for the frames of the coincident triangles, which
    stand at unit depth under col = 32 x + 32, row = 32 y + 32 with the identity map on every link."""
    I = np.eye(4)[:3]
    out = []
    for i in frames:
        t = pinhole_table(32.0, 32.0, 32.0, 32.0, [I, I, I], SCALE[dtype]) if i == 3 else render_table(object_scene(rs, 3), SCALE[dtype])
        t[9] = i
        out.append(t)
    return np.stack(out)


def _geom(crops, first=3, gap=5):
    geom, a = [], first
    for h, w, origin in crops:
        geom.append((a, h, w) + ((C, C) if origin is None else tuple(origin)))
        a += h * w + gap
    return np.asarray(geom, np.int32), a + 7


class _Device(object):
    """A library (or one mesh) and per-call buffers carved out of red zones: the 4-byte arrays 4 bytes off their natural alignment, the 8- and
    16-byte ones 16 bytes off a 512-byte boundary."""

    def __init__(self, dev, mesh):
        self.dev, self.small, self.wide = dev, Arena(misalign=4), Arena(misalign=16)
        verts, tris, tri_link = (np.ascontiguousarray(a) for a in mesh[:3])
        self.V, self.T = verts.shape[0], tris.shape[0]
        self.verts, self.tris, self.tri_link = (self.put(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype), self.small) for a in (verts, tris, tri_link))
        self.tri_off = self.ninst = None
        if len(mesh) == 4:
            self.tri_off, self.ninst, self.Tmax = self.put(mesh[3], self.small), len(mesh[3]) - 1, int(np.diff(mesh[3]).max())

    def put(self, a, arena):
        a = np.ascontiguousarray(a)
        t = arena.empty(tuple(a.shape), dtype=torch.from_numpy(a).dtype, device=self.dev)
        t.copy_(torch.from_numpy(a))
        return t

    def render(self, geom, tables, cap, dtype):
        """ancsh_render_depth_labels(_lib) on sentinel-filled outputs -> (depth (cap,), labels (cap,)) as numpy arrays."""
        from articulated_pose_amd import _lib
        depth = self.put(np.full(cap, FILL[dtype], DTYPES[dtype]).view(np.int16 if dtype == "uint16" else np.float32), self.wide)
        labels, zbuf = self.put(np.full(cap, LABEL_FILL, np.uint8), self.wide), self.wide.empty((cap,), dtype=torch.int64, device=self.dev)
        d_geom, d_tables = self.put(np.asarray(geom, np.int32).reshape(-1, 5), self.small), self.put(np.asarray(tables, np.float64).reshape(-1, 208), self.wide)
        assert depth.data_ptr() % 512 == 16 and d_geom.data_ptr() % 8 == 4
        head = (d_geom.shape[0], 0 if dtype == "uint16" else 1, _lib.ptr(self.verts), _lib.ptr(self.tris), _lib.ptr(self.tri_link), self.V, self.T)
        tail = (_lib.ptr(d_geom), _lib.ptr(d_tables), _lib.ptr(depth), _lib.ptr(labels), _lib.ptr(zbuf), cap)
        if self.tri_off is None:
            _lib.call("ancsh_render_depth_labels", *(head + tail))
        else:
            _lib.call("ancsh_render_depth_labels_lib", *(head + (_lib.ptr(self.tri_off), self.ninst, self.Tmax) + tail))
        torch.cuda.synchronize()
        return depth.cpu().numpy().view(DTYPES[dtype]), labels.cpu().numpy()

    def centre(self, geom, tables):
        """Two calls of ancsh_render_centre_crops(_lib) -> (geom after the first, geom after the second)."""
        from articulated_pose_amd import _lib
        d_geom, d_tables = self.put(np.asarray(geom, np.int32).reshape(-1, 5), self.small), self.put(np.asarray(tables, np.float64).reshape(-1, 208), self.wide)
        bounds = self.small.empty((d_geom.shape[0], 4), dtype=torch.int32, device=self.dev)
        head = (d_geom.shape[0], _lib.ptr(self.verts), _lib.ptr(self.tris), _lib.ptr(self.tri_link), self.V, self.T)
        out = []
        for _ in range(2):
            if self.tri_off is None:
                _lib.call("ancsh_render_centre_crops", *(head + (_lib.ptr(d_tables), _lib.ptr(d_geom), _lib.ptr(bounds))))
            else:
                _lib.call("ancsh_render_centre_crops_lib", *(head + (_lib.ptr(self.tri_off), self.ninst, _lib.ptr(d_tables), _lib.ptr(d_geom), _lib.ptr(bounds))))
            torch.cuda.synchronize()
            out.append(d_geom.cpu().numpy())
        return out

    def check(self):
        self.small.check()
        self.wide.check()


def _pixels(g):
    return slice(int(g[0]), int(g[0]) + int(g[1]) * int(g[2]))


@pytest.fixture(scope="module")
def library():
    from articulated_pose_amd.depth import pack_mesh_library
    inst = _instances()
    lib = pack_mesh_library(inst)
    assert lib[3].tolist() == [0, 12, 82, 82, 84]
    return inst, lib


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_library_frames_equal_each_instance_rendered_alone(dev, library, dtype):
    """Frames [3, 0, 1, 0, 2, 1] on ragged crops: the library entry's buffers equal, byte for byte, the mirror's and the single-object entry's
    on each frame's own instance, twice; the tie of instance 3 goes to the lower index, instance 2 is background, nothing outside the crops
    is written and the red zones stay intact.  The box's frames would differ if a wave ran on into the fan's triangles."""
    inst, lib = library
    rs = np.random.RandomState(7)
    tables = _frame_tables(rs, dtype)
    geom, cap = _geom(CROPS)
    want_d, want_l = np.full(cap, FILL[dtype], DTYPES[dtype]), np.full(cap, LABEL_FILL, np.uint8)
    for f, i in enumerate(FRAMES):                                      # the mirror, frame by frame on the instance's own mesh
        d, l = RM.render_flat(inst[i][0], inst[i][1], inst[i][2], geom[f:f + 1], tables[f:f + 1], cap, DTYPES[dtype], FILL[dtype], LABEL_FILL)
        want_d[_pixels(geom[f])], want_l[_pixels(geom[f])] = d[_pixels(geom[f])], l[_pixels(geom[f])]
    D = _Device(dev, lib)
    got_d, got_l = D.render(geom, tables, cap, dtype)
    assert _bytes(got_d, want_d) and _bytes(got_l, want_l), (int((got_d != want_d).sum()), int((got_l != want_l).sum()), np.flatnonzero(got_l != want_l)[:8])
    again = D.render(geom, tables, cap, dtype)
    assert _bytes(again[0], got_d) and _bytes(again[1], got_l)
    D.check()
    for i in range(4):                                                  # the single-object entry, instance by instance on its frames
        fs = [f for f, k in enumerate(FRAMES) if k == i]
        S = _Device(dev, inst[i])
        one_d, one_l = S.render(geom[fs], tables[fs], cap, dtype)
        S.check()
        for f in fs:
            assert _bytes(one_d[_pixels(geom[f])], got_d[_pixels(geom[f])]) and _bytes(one_l[_pixels(geom[f])], got_l[_pixels(geom[f])]), (i, f)
    # what the frames show
    tie = got_l[_pixels(geom[0])].reshape(24, 32)
    assert set(np.unique(tie)) == {1, 255} and (tie == 1).sum() > 100 and tie[40 - 28, 36 - 24] == 1       # the lower index carries link 1
    assert (got_l[_pixels(geom[4])] == 255).all() and (got_d[_pixels(geom[4])] == 0).all()                 # the empty instance
    assert all(set(np.unique(got_l[_pixels(geom[f])])) >= {0, 1, 2} for f in (2, 5))                     # the fan shows all of its links
    for f in (1, 3):                                                    # the fan under the box's own maps covers the box's pixels, nearer
        both = [np.concatenate(p) for p in zip((inst[0][0], inst[0][1], inst[0][2]), (inst[1][0], inst[1][1] + 8, inst[1][2]))]
        d, l = RM.render_flat(both[0], both[1], both[2], geom[f:f + 1], tables[f:f + 1], cap, DTYPES[dtype], FILL[dtype], LABEL_FILL)
        assert not _bytes(d[_pixels(geom[f])], got_d[_pixels(geom[f])]), f
    inside = np.zeros(cap, bool)
    for g in geom:
        inside[_pixels(g)] = True
    assert (got_l[~inside] == LABEL_FILL).all() and (got_l[inside] != LABEL_FILL).all()


def _bad_frames(ninst):
    return [ninst if v is None else v for v in BAD]


def test_a_frame_without_an_instance_is_background_and_centres_to_zero(dev, library):
    """render[9] = -1, ninst, 0.5 and NaN written straight into device tables, past the host checks, between good frames of the fan and the
    box: those crops are all background, their centred origins (0, 0), and the frames beside them what they are without them."""
    inst, lib = library
    rs = np.random.RandomState(8)
    values = [1.0, -1.0, 0.0, 4.0, 1.0, 0.5, 0.0, np.nan, 1.0]
    tables = _frame_tables(rs, "uint16", [1] * len(values))
    tables[:, 9] = values
    good = [f for f, v in enumerate(values) if v in (0.0, 1.0)]
    crops = [(17, 9, (24, 27)) if f % 2 else (24, 32, (20, 16)) for f in range(len(values))]
    geom, cap = _geom(crops)
    D = _Device(dev, lib)
    got_d, got_l = D.render(geom, tables, cap, "uint16")
    for f, v in enumerate(values):
        if f in good:
            m = inst[int(v)]
            d, l = RM.render_flat(m[0], m[1], m[2], geom[f:f + 1], tables[f:f + 1], cap, np.uint16, FILL["uint16"], LABEL_FILL)
            assert _bytes(got_d[_pixels(geom[f])], d[_pixels(geom[f])]) and _bytes(got_l[_pixels(geom[f])], l[_pixels(geom[f])]), f
            assert (got_l[_pixels(geom[f])] != 255).any(), f
        else:
            assert (got_l[_pixels(geom[f])] == 255).all() and (got_d[_pixels(geom[f])] == 0).all(), (f, v)
    centred, _ = _geom([(h, w, None) for h, w, _ in crops])
    first, second = D.centre(centred, tables)
    D.check()
    assert _bytes(first, second) and np.array_equal(first[:, :3], centred[:, :3])
    for f, v in enumerate(values):
        if f in good:
            m = inst[int(v)]
            want = PM.centre_origins(m[0], m[1], m[2], m[0].shape[0], centred[f:f + 1], tables[f:f + 1])
            assert first[f].tolist() == want[0].tolist() and first[f, 3:].tolist() != [0, 0], f
        else:
            assert first[f, 3:].tolist() == [0, 0], (f, v)


def test_library_centring_equals_each_instance_centred_alone(dev, library):
    """The frames of the renderer's test, half of them centred: origins byte for byte those of the single-object entry on the frame's own
    instance, and of the mirror; frames with a real origin are untouched; a second call is a no-op."""
    inst, lib = library
    rs = np.random.RandomState(7)
    tables = _frame_tables(rs, "uint16")
    crops = [(h, w, None if f != 3 else o) for f, (h, w, o) in enumerate(CROPS)]      # frame 3 keeps its real origin
    geom, _ = _geom(crops)
    D = _Device(dev, lib)
    first, second = D.centre(geom, tables)
    D.check()
    assert _bytes(first, second) and np.array_equal(first[:, :3], geom[:, :3]) and first[3].tolist() == geom[3].tolist()
    for i in range(4):
        fs = [f for f, k in enumerate(FRAMES) if k == i]
        S = _Device(dev, inst[i])
        one, _ = S.centre(geom[fs], tables[fs])
        S.check()
        want = PM.centre_origins(inst[i][0], inst[i][1], inst[i][2], inst[i][0].shape[0], geom[fs], tables[fs])
        assert _bytes(one, first[fs]) and _bytes(want, first[fs]), (i, one.tolist(), first[fs].tolist(), want.tolist())
    assert first[4, 3:].tolist() == [0, 0]                              # the empty instance counts no vertex
    assert all(first[f, 3:].tolist() != [0, 0] for f in (0, 1, 2, 5))
    assert first[1, 3:].tolist() != first[2, 3:].tolist()               # the box and the fan centre differently


# ---- the table builder ------------------------------------------------------------------------------------------------------------------------
def test_library_tables_equal_each_instance_built_alone(dev):
    """Kinematic tables of 1, 3 and 16 links in one stack, 13 frames in mixed order: both tables equal, byte for byte (sincos included: one
    device function), those of ancsh_pose_scene_build on the frame's own table, but for render[9], which reads the instance; a pose[28] that
    names no instance gives all-zero tables; the red zones stay intact."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import pack_pose
    from test_pose_scene_cpu import random_view
    from test_pose_scene_gpu import _build, _object
    rs = np.random.RandomState(17)
    kins = np.stack([_object(rs, L) for L in (1, 3, 16)])
    order = [2, 0, 1, 1, 2, 0, 2, 1, 0, 0, 1, 2, 2]
    poses = np.stack([pack_pose(rs.uniform(-2, 2, 16), random_view(rs), instance=i) for i in order])
    bad = np.stack([pack_pose(rs.uniform(-2, 2, 16), random_view(rs)) for _ in BAD])
    bad[:, 28] = _bad_frames(3)
    every = np.concatenate([poses[:5], bad[:2], poses[5:], bad[2:]])    # 17 frames: 17 x 16 threads cross a block boundary
    where = np.array([True] * 5 + [False] * 2 + [True] * 8 + [False] * 2)
    n = every.shape[0]
    arena = Arena(misalign=8)
    d_kin, d_pose = arena.empty((3, 672), dtype=torch.float64, device=dev), arena.empty((n, 32), dtype=torch.float64, device=dev)
    render, scene = arena.empty((n, 208), dtype=torch.float64, device=dev), arena.empty((n, 240), dtype=torch.float64, device=dev)
    d_kin.copy_(torch.from_numpy(kins))
    d_pose.copy_(torch.from_numpy(every))
    render.fill_(SENTINEL)
    scene.fill_(SENTINEL)
    _lib.call("ancsh_pose_scene_build_lib", n, _lib.ptr(d_kin), 3, _lib.ptr(d_pose), _lib.ptr(render), _lib.ptr(scene))
    torch.cuda.synchronize()
    got_r, got_s = render.cpu().numpy(), scene.cpu().numpy()
    arena.check()
    assert not got_r[~where].view(np.uint64).any() and not got_s[~where].view(np.uint64).any()       # +0.0 everywhere
    got_r, got_s = got_r[where], got_s[where]
    assert got_r[:, 9].tolist() == [float(i) for i in order]
    single = poses.copy()
    single[:, 28] = 0
    for i in range(3):
        fs = [f for f, k in enumerate(order) if k == i]
        want_r, want_s = _build(dev, kins[i], single[fs])
        assert (want_r[:, 9] == 0).all()
        want_r[:, 9] = i
        assert _bytes(got_r[fs], want_r) and _bytes(got_s[fs], want_s), i
        assert (got_r[fs, 8] == (1, 3, 16)[i]).all()
    # the eager wrapper takes the stack and the instances from the poses
    from articulated_pose_amd.depth import pose_scene_tables
    eager_r, eager_s = pose_scene_tables(kins, poses, dev)
    assert _bytes(eager_r, got_r) and _bytes(eager_s, got_s)
    with pytest.raises(ValueError, match=r"pose 1: .*\[0, 3\)"):
        pose_scene_tables(kins, np.stack([poses[0], bad[1]]), dev)


# ---- the stream ------------------------------------------------------------------------------------------------------------------------------------
def _stream_library(rs, dtype):
    """Three three-link instances of unequal triangle counts (36, 48, 36) and different sizes, each with a kinematic table of its own."""
    from articulated_pose_amd.depth import pack_mesh
    from test_pose_scene_gpu import _posed_object
    small = box_mesh(0.5 * BOX_LO, 0.5 * BOX_HI)
    meshes = [object_mesh(3),
              pack_mesh([(np.concatenate([box_mesh(0.9 * BOX_LO, 0.9 * BOX_HI)[0], small[0] + (0, 0, 0.1)]), np.concatenate([small[1], small[1] + 8])),
                         box_mesh(0.9 * BOX_LO, 0.9 * BOX_HI), box_mesh(BOX_LO, BOX_HI)]),
              pack_mesh([box_mesh(1.1 * BOX_LO, 1.1 * BOX_HI), box_mesh(BOX_LO, BOX_HI), box_mesh(0.8 * BOX_LO, 0.8 * BOX_HI)])]
    objects = [_posed_object(rs, dtype) for _ in range(3)]
    return meshes, np.stack([kin for kin, _ in objects]), [S for _, S in objects]


@pytest.mark.parametrize("slots,options", [(1, {}), (4, dict(ground_truth=True, build_gt_pose=True))], ids=["1slot", "4slots-gt-pose"])
def test_posed_library_stream_equals_the_annotated_depth_stream(dev, slots, options):
    """Six batches that mix three instances, one of them short, half of the crops centred: records, articulation blocks, counts and link
    counts of stream_posed_batches on the library pipeline equal, byte for byte, those of stream_depth_batches on an annotated-depth pipeline
    fed the same batches as frames rendered eagerly instance by instance (render_depth_frames, scenes from pose_scene_tables, origins from
    centre_crops).  Batch composition is the same, so the RANSAC keys are.  One graph per slot serves every batch."""
    from articulated_pose_amd.depth import centre_crops, pack_mesh_library, pack_pose, pose_scene_tables, render_depth_frames
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    from test_render_gpu import B_, CAP_, K_, LINKS_, N_, _weights
    dtype = "uint16"
    rs = np.random.RandomState(29)
    meshes, kins, scenes = _stream_library(rs, dtype)
    lib = pack_mesh_library(meshes)
    assert np.diff(lib[3]).tolist() == [36, 48, 36]
    pb = _weights()
    kw = dict(dict(couple=True, slots=slots, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype), **options)
    mk = lambda **more: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **more))
    Pl, A = mk(render_mesh=lib, kinematics=kins), mk()
    Pl.prepare()
    assert Pl.ninst == 3 and Pl.kin.shape == (3, 672) and Pl.mesh.Tmax == 48 and Pl.mesh.host_tri_off.tolist() == [0, 36, 84, 120] and A.ninst is None
    graphs = [s.graph for s in Pl.slots]
    feed_p, feed_a = [], []
    for k in range(6):
        n = 1 if k == 2 else 2
        which = [(k + f) % 3 for f in range(n)] if k != 4 else [1, 1]     # every batch but one mixes two instances
        poses, frames, scs = [], [], []
        sizes = [(int(rs.randint(56, 65)), int(rs.randint(56, 65))) for _ in range(n)]
        fixed = [(int(rs.randint(0, 3)), int(rs.randint(0, 3))) for _ in range(n)]
        centred = [(f + k) % 2 == 0 for f in range(n)]
        for f, i in enumerate(which):
            V = object_scene(rs, LINKS_)["viewMat"]
            q = [0.0, rs.uniform(0.2, 1.1), rs.uniform(-0.03, 0.03)]
            poses.append(pack_pose(q, V, instance=i))
            rt, sc = pose_scene_tables(kins[i], np.stack([pack_pose(q, V)]), dev)
            origin = tuple(int(v) for v in centre_crops(meshes[i], rt, [sizes[f]], dev)[0]) if centred[f] else fixed[f]
            frames += render_depth_frames(meshes[i], rt, [sizes[f] + (origin,)], dtype, dev)
            scs.append(sc[0])
        nf = rs.uniform(0.9, 1.1, n).astype(np.float32)
        side = dict(rig=np.tile(stream_rig(), (n, 1)))
        if options.get("build_gt_pose"):
            side["gt"] = pack_box_extents([np.tile(BOX_HI - BOX_LO, (K_, 1))] * n)
        else:
            side["frame"] = random_frames(rs, n)
        feed_p.append(([(h, w, None if c else o) for (h, w), c, o in zip(sizes, centred, fixed)], nf, dict(side, pose=np.stack(poses)), "t%d" % k))
        feed_a.append((frames, nf, "t%d" % k, dict(side, scene=np.stack(scs))))
    got = list(Pl.stream_posed_batches(feed_p, articulation=True, link_counts=True))
    want = list(A.stream_depth_batches(feed_a, articulation=True, link_counts=True))
    assert all(g is not None and g is s.graph for g, s in zip(graphs, Pl.slots))        # one graph per slot served every batch
    assert len(got) == len(want) == 6 and [g[0] for g in got] == ["t%d" % k for k in range(6)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 6 and g[:2] == w[:2], k
        for a, b in zip(g[2:], w[2:]):                                   # record, articulation block, counts, link counts
            assert _bytes(a, b), k
    assert got[2][2].shape[0] == 1 and got[0][2].shape == (2, K_, got[0][2].shape[2]) and np.isfinite(got[0][2][:, :, :26]).any()
    assert all((g[4] > 300).all() for g in got)
    # an instance the library does not hold: ValueError before anything is enqueued, and the pipeline stays usable
    crops, nf, side, _ = feed_p[0]
    good = dict(side, crops=crops, norm_factors=nf)
    for value in (3.0, -1.0, 0.5, np.nan):
        bad = side["pose"].copy()
        bad[1, 28] = value
        with pytest.raises(ValueError, match=r"pose 1: .*\[0, 3\)"):
            Pl.submit_posed(**dict(good, pose=bad))
    assert not Pl._inflight
    Pl.submit_posed(seed=got[0][1], **good)
    again = Pl.retire(articulation=True, link_counts=True)
    assert all(_bytes(a, b) for a, b in zip(again[2:], got[0][2:]))


def test_launch_budget(dev):
    """The library step issues the single-object posed step's ABI calls, one for one: the three *_lib entries in the places of theirs."""
    from articulated_pose_amd.depth import pack_mesh_library
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_fit_quality_gpu import _launch_names
    from test_render_gpu import B_, CAP_, K_, N_, _weights
    meshes, kins, _ = _stream_library(np.random.RandomState(2), "uint16")
    pb = _weights()
    kw = dict(couple=True, slots=1, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
              point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype="uint16")
    mk = lambda **more: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **more))
    lib_names = _launch_names(mk(render_mesh=pack_mesh_library(meshes), kinematics=kins).prepare())
    one_names = _launch_names(mk(render_mesh=meshes[0], kinematics=kins[0]).prepare())
    assert lib_names[:3] == ["ancsh_pose_scene_build_lib", "ancsh_render_centre_crops_lib", "ancsh_render_depth_labels_lib"]
    assert len(lib_names) == len(one_names) and [n[:-4] if n.endswith("_lib") else n for n in lib_names] == one_names
