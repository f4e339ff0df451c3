"""CPU tests of the instance library (no GPU): depth.pack_mesh_library's layout and refusals, the instance argument of depth.pack_pose and
depth.pack_render_scene and the checkers' rules with and without a library, stream.check_options' rule between the two counts, and the three
*_lib symbols with their argument checks before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_pose_scene_cpu import kin_table, random_view, tree
from test_render_cpu import box_mesh, object_scene, pinhole_table

P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the library the GPU tests share ------------------------------------------------------------------------------------------------------------
def fan_mesh(n, links, radius=1.0, z=0.0):
    """n triangles of a fan about the z axis in the plane z = `z`, reaching out to `radius`: triangle k belongs to link k % links -> one
    (vertices, faces) pair per link, as depth.pack_mesh takes them."""
    a = 2 * np.pi * np.arange(n + 1) / n
    rim = np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n + 1, z)], 1)
    out = []
    for l in range(links):
        ks = np.arange(l, n, links)
        v = np.concatenate([[(0.0, 0.0, z)], rim[ks], rim[ks + 1]])
        out.append((v, np.stack([np.zeros(len(ks), np.int64), 1 + np.arange(len(ks)), 1 + len(ks) + np.arange(len(ks))], 1)))
    return out


# ---- pack_mesh_library -----------------------------------------------------------------------------------------------------------------------
def test_pack_mesh_library_offsets_and_bases():
    """Instances of 12, 0 and 70 triangles: tri_off, the vertex base added to every face, and each instance's slice equal to its own
    pack_mesh shifted; link lists and packed meshes mix."""
    from articulated_pose_amd.depth import mesh_to_device, pack_mesh, pack_mesh_library
    box = pack_mesh([box_mesh([0, 0, 0], [1, 2, 3])])
    empty = pack_mesh([])
    fan = pack_mesh(fan_mesh(70, 3))
    assert [m[1].shape[0] for m in (box, empty, fan)] == [12, 0, 70]
    verts, tris, tri_link, tri_off = pack_mesh_library([box, [], fan_mesh(70, 3)])
    assert tri_off.dtype == np.int32 and tri_off.tolist() == [0, 12, 12, 82]
    assert verts.dtype == np.float32 and tris.dtype == np.int32 and tri_link.dtype == np.int32
    assert verts.shape == (8 + fan[0].shape[0], 3) and tris.shape == (82, 3) and tri_link.shape == (82,)
    assert all(a.flags.c_contiguous for a in (verts, tris, tri_link, tri_off))
    assert np.array_equal(tris[:12], box[1]) and np.array_equal(tris[12:], fan[1] + 8) and np.array_equal(verts[8:], fan[0])
    assert np.array_equal(tri_link[:12], box[2]) and np.array_equal(tri_link[12:], fan[2]) and set(fan[2].tolist()) == {0, 1, 2}
    assert tris[:12].max() < 8 <= tris[12:].min()                       # the indices are global and stay inside their own instance
    one = pack_mesh_library([box])
    assert one[3].tolist() == [0, 12] and all(np.array_equal(a, b) for a, b in zip(one[:3], box))
    import torch
    dm = mesh_to_device((verts, tris, tri_link, tri_off), torch.device("cpu"))     # the upload keeps Tmax and a host copy of tri_off
    assert len(dm) == 5 and dm[3:] == (verts.shape[0], 82) and (dm.ninst, dm.Tmax) == (3, 70) and dm.host_tri_off.tolist() == [0, 12, 12, 82]
    assert dm.tri_off.dtype == torch.int32 and dm.tri_off.tolist() == [0, 12, 12, 82]
    single = mesh_to_device(box, torch.device("cpu"))
    assert len(single) == 5 and single.tri_off is None and single.ninst is None


def test_pack_mesh_library_refusals():
    from articulated_pose_amd.depth import mesh_to_device, pack_mesh, pack_mesh_library
    box = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    reach = (box[0], box[1].copy(), box[2])
    reach[1][3, 1] = 8                                                  # vertex 8 is the neighbour instance's first: in range globally, not locally
    with pytest.raises(ValueError, match="instance 0.*outside its own instance"):
        pack_mesh_library([reach, box])
    back = (box[0], box[1].copy(), box[2])
    back[1][0, 0] = -1
    with pytest.raises(ValueError, match="instance 1"):
        pack_mesh_library([box, back])
    with pytest.raises(ValueError, match="instance 0"):                 # a single pack_mesh result is no list of them
        pack_mesh_library(box)
    for bad in ([], None, [box] * 4097):
        with pytest.raises(ValueError, match="1..4096 instances"):
            pack_mesh_library(bad)
    assert pack_mesh_library([pack_mesh([])] * 4096)[3].shape == (4097,)
    # 2^24 triangles in all, from the shapes alone: the arrays are zero-stride views of one row, nothing of that size is ever allocated
    half = 1 << 23
    big = (box[0], np.broadcast_to(np.zeros((1, 3), np.int32), (half, 3)), np.broadcast_to(np.zeros(1, np.int32), (half,)))
    with pytest.raises(ValueError, match="fewer than 2\\^24"):
        pack_mesh_library([big, big])
    many = (np.broadcast_to(np.zeros((1, 3), np.float32), (half, 3)), box[1], box[2])
    with pytest.raises(ValueError, match="fewer than 2\\^24"):
        pack_mesh_library([many, many])
    # mesh_to_device refuses offsets that are no partition of the triangles, on the host
    import torch
    for off in ([0, 5, 3, 12], [1, 12], [0, 11], [0], np.zeros(4098, np.int32), [0.0, 12.0]):
        with pytest.raises(ValueError, match="tri_off"):
            mesh_to_device(box + (np.asarray(off),), torch.device("cpu"))


# ---- the instance in the per-frame tables -----------------------------------------------------------------------------------------------------
def _render_args(rs):
    S = object_scene(rs, 2)
    return S["viewMat"], S["projMat"], S["world_pos"], S["world_orn"], S["H"], S["W"]


def test_instance_round_trip_and_checker_refusals():
    """The instance rides in pose[28] / render[9] and nowhere else; the single-object checkers still refuse a non-zero reserved value; the
    library checkers refuse -1, ninst, 1.5 and NaN, naming the frame and the value."""
    from articulated_pose_amd.depth import check_poses, check_render_tables, pack_pose, pack_render_scene
    rs = np.random.RandomState(1)
    V, args = random_view(rs), _render_args(rs)
    p0, p7 = pack_pose([0.1, 0.2], V), pack_pose([0.1, 0.2], V, instance=7)
    assert p0[28] == 0 and p7[28] == 7.0 and np.array_equal(np.delete(p0, 28), np.delete(p7, 28)) and (p7[29:] == 0).all()
    r0, r7 = pack_render_scene(*args), pack_render_scene(*args, instance=7)
    assert r0[9] == 0 and r7[9] == 7.0 and np.array_equal(np.delete(r0, 9), np.delete(r7, 9)) and (r7[10:16] == 0).all()
    assert np.array_equal(pack_pose([0.1, 0.2], V, instance=0), p0) and np.array_equal(pack_render_scene(*args, instance=np.int64(0)), r0)
    for bad in (-1, 4096, 1.5, np.nan, "a", None):
        with pytest.raises(ValueError, match="instance"):
            pack_pose([0.1], V, instance=bad)
        with pytest.raises(ValueError, match="instance"):
            pack_render_scene(*args, instance=bad)
    # single-object use: a non-zero reserved value is refused as before
    assert check_poses(p0, 2).shape == (2, 32) and check_render_tables(r0, 2).shape == (2, 208)
    with pytest.raises(ValueError, match="pose 0.*reserved"):
        check_poses(p7, 1)
    with pytest.raises(ValueError, match="render table 1.*reserved"):
        check_render_tables(np.stack([r0, r7]), 2)
    # with a library
    assert check_poses(np.stack([p0, p7]), 2, 8)[:, 28].tolist() == [0.0, 7.0] and check_poses(p7, 3, 8).shape == (3, 32)
    assert check_render_tables(np.stack([r7, r0]), 2, 8)[:, 9].tolist() == [7.0, 0.0]
    for value, shown in ((-1.0, "-1.0"), (8.0, "8.0"), (1.5, "1.5"), (np.nan, "nan")):
        p, r = p0.copy(), r0.copy()
        p[28], r[9] = value, value
        with pytest.raises(ValueError, match=r"pose 2: .*\[0, 8\).*got " + shown):
            check_poses(np.stack([p0, p7, p]), 3, 8)
        with pytest.raises(ValueError, match=r"render table 1: .*\[0, 8\).*got " + shown):
            check_render_tables(np.stack([r0, r]), 2, 8)
    for row, bad in ((p7, 29), (p7, 31)):                               # the other reserved values stay reserved
        p = row.copy()
        p[bad] = 1.0
        with pytest.raises(ValueError, match="reserved"):
            check_poses(p, 1, 8)
    r = r7.copy()
    r[10] = 1.0
    with pytest.raises(ValueError, match="reserved"):
        check_render_tables(r, 1, 8)
    for ninst in (0, 4097, 1.5):
        with pytest.raises(ValueError, match="ninst"):
            check_poses(p0, 1, ninst)


def _kin(rs, L):
    from test_depth_annotate_cpu import random_scene
    return kin_table(random_scene(rs, L), tree(rs, L, "chain"), [[l] for l in range(L)][:3] if L <= 3 else [[0], [1], list(range(2, L))])


def test_kinematics_library_is_checked_row_by_row():
    from articulated_pose_amd.depth import check_kinematics, check_kinematics_library
    rs = np.random.RandomState(2)
    stack = np.stack([_kin(rs, 1), _kin(rs, 3), _kin(rs, 16)])          # link counts may differ
    got = check_kinematics_library(stack)
    assert got.shape == (3, 672) and got.flags.c_contiguous and np.array_equal(got, stack)
    bad = stack.copy()
    bad[1, 14] = 2.5
    with pytest.raises(ValueError, match="instance 1: kinematics: nlinks"):
        check_kinematics_library(bad)
    with pytest.raises(ValueError, match="instance 0"):                 # all instances share K parts: part 2 of a K = 2 object is refused
        check_kinematics_library(np.stack([_kin(rs, 3)]), K=2)
    for shape in ((672,), (0, 672), (2, 671), (4097, 672)):
        with pytest.raises(ValueError, match="ninst"):
            check_kinematics_library(np.zeros(shape))
    with pytest.raises(ValueError):                                     # the single-table checker keeps refusing a stack
        check_kinematics(stack)


def test_options_pair_the_two_counts():
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    rs = np.random.RandomState(3)
    box = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    lib3, lib2 = pack_mesh_library([box] * 3), pack_mesh_library([box] * 2)
    kin = _kin(rs, 1)
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    on = check_options(render_mesh=lib3, kinematics=np.stack([kin] * 3), **annotated)
    assert on.posed and on.render and on == check_options(render_mesh=box, kinematics=kin, **annotated)
    assert check_options(render_mesh=lib3, **annotated).render          # a library without kinematics: submit_render carries the instance
    assert check_options(render_mesh=pack_mesh_library([box]), kinematics=kin[None], **annotated).posed     # ninst = 1 is a library too
    for mesh, k, text in ((lib2, np.stack([kin] * 3), "a stack of 3 tables.*a mesh library of 2 instances"),
                          (box, np.stack([kin] * 3), "a stack of 3 tables.*a single mesh"),
                          (box, kin[None], "a stack of 1 tables.*a single mesh"),
                          (lib3, kin, "a single table.*a mesh library of 3 instances")):
        with pytest.raises(ValueError, match="kinematics is " + text):
            check_options(render_mesh=mesh, kinematics=k, **annotated)
        with pytest.raises(ValueError, match="kinematics is " + text):
            AncshPipeline(3, None, None, 2, 64, "cpu", render_mesh=mesh, kinematics=k, **annotated)
    # the library's poses are checked against its size before anything is enqueued (no device is touched: the options alone decide)
    from articulated_pose_amd import stream
    from articulated_pose_amd.dataset import identity_rig
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.B, pipe.K, pipe.ninst, pipe._inflight, pipe.slots = on, 2, 3, 3, [], []
    pose = stream.unit_pose(3, None)
    for value in (3.0, -1.0, 0.5, np.nan):
        bad = pose.copy()
        bad[28] = value
        with pytest.raises(ValueError, match=r"pose 1: .*\[0, 3\)"):
            pipe.submit_posed([(3, 4, None)] * 2, [1.0, 1.0], np.stack([pose, bad]), np.tile(identity_rig(3), (2, 1)))
    pipe.ninst = None                                                   # a single-object pipeline keeps refusing the reserved value
    two = pose.copy()
    two[28] = 2.0
    with pytest.raises(ValueError, match="reserved"):
        pipe.submit_posed([(3, 4, None)], [1.0], two, identity_rig(3)[None])
    assert not pipe._inflight


# ---- the symbols and their argument checks ----------------------------------------------------------------------------------------------------------
NAMES = (("ancsh_render_depth_labels_lib", 17), ("ancsh_render_centre_crops_lib", 12), ("ancsh_pose_scene_build_lib", 7))


def test_symbols_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd import depth as D
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name, nargs in NAMES:
        assert name in declared_symbols() and name in exported and len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_LIBRARY_MAX_INSTANCES %d\n" % D.LIBRARY_MAX_INSTANCES in header and D.LIBRARY_MAX_INSTANCES == 4096


def test_entries_reject_bad_arguments_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def render(nframes=2, kind=0, verts=P16, tris=P16, tri_link=P16, V=8, T=12, tri_off=P16, ninst=2, Tmax=7, geom=P16, render=P16, depth=P16,
               labels=P16, zbuf=P16, px=100):
        return L.ancsh_render_depth_labels_lib(nframes, kind, verts, tris, tri_link, V, T, tri_off, ninst, Tmax, geom, render, depth, labels, zbuf, px,
                                               None)

    def centre(nframes=2, verts=P16, tris=P16, tri_link=P16, V=8, T=12, tri_off=P16, ninst=2, render=P16, geom=P16, bounds=P16):
        return L.ancsh_render_centre_crops_lib(nframes, verts, tris, tri_link, V, T, tri_off, ninst, render, geom, bounds, None)

    def build(nframes=2, kin=P16, ninst=2, pose=P16, render=P16, scene=P16):
        return L.ancsh_pose_scene_build_lib(nframes, kin, ninst, pose, render, scene, None)
    library = ((dict(ninst=0), b"ninst=0"), (dict(ninst=4097), b"ninst=4097"), (dict(ninst=-3), b"ninst=-3"))
    offsets = ((dict(tri_off=None), b"tri_off"), (dict(tri_off=ctypes.c_void_p(18)), b"tri_off"))
    for call, cases, names in (
            (render, library + offsets + ((dict(Tmax=-1), b"Tmax=-1"), (dict(Tmax=13), b"Tmax=13"), (dict(nframes=-1), b"bad shape"), (dict(nframes=65536), b"65535"),
                                          (dict(kind=2), b"depth_type=2"), (dict(px=1 << 30), b"pixel_capacity"), (dict(T=1 << 24), b"T=16777216"),
                                          (dict(V=-1), b"V=-1"), (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(zbuf=ctypes.c_void_p(4)), b"8-byte aligned")),
             ("verts", "tris", "tri_link", "geom", "render", "depth", "labels", "zbuf")),
            (centre, library + offsets + ((dict(nframes=-1), b"bad shape"), (dict(T=-1), b"T=-1"), (dict(V=1 << 24), b"V=16777216"),
                                          (dict(geom=ctypes.c_void_p(2)), b"4-byte aligned")), ("verts", "tris", "tri_link", "render", "geom", "bounds")),
            (build, library + ((dict(nframes=-1), b"bad shape"), (dict(nframes=65536), b"65535"), (dict(kin=ctypes.c_void_p(4)), b"8-byte aligned"),
                               (dict(pose=ctypes.c_void_p(12)), b"8-byte aligned")), ("kin", "pose", "render", "scene"))):
        for kw, msg in cases:
            assert call(**kw) == -1, kw
            assert msg in L.ancsh_last_error() and b"_lib" in L.ancsh_last_error(), (kw, L.ancsh_last_error())
            assert "nframes" in kw or call(nframes=0, **kw) == -1     # refused even for an empty batch
        for k in names:
            assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nframes=0) == 0                                     # no frame: nothing launched, no device touched
    assert render(nframes=0, T=0, V=0, Tmax=0) == 0 and render(nframes=0, Tmax=12) == 0 and centre(nframes=0, T=0, V=0) == 0
    # the single-object entries keep their names in their messages
    assert L.ancsh_pose_scene_build(-1, P16, P16, P16, P16, None) == -1 and L.ancsh_last_error().startswith(b"pose_scene_build: bad shape")
