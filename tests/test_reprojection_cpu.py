"""CPU (no GPU): render-and-compare's place in the ABI and in check_options, the entries' argument checks before any launch, and the numpy
mirror (tests/reprojection_mirror.py) validated on its own: against the closed-form record that undoes a frame's own maps -- the mirror's
predicted render table must then be the frame's own to float64 rounding --, and on rendered frames, where that record must reproduce the
observed silhouette and depth.  The object, views and crops here are the GPU tests' too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pose_scene_mirror as PM
import render_mirror as RM
import reprojection_mirror as RP
from test_pose_scene_cpu import kin_table
from test_render_cpu import box_mesh, object_scene

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = (("ancsh_reproject_scene_build", 14), ("ancsh_reproject_compare_rec", 14))
P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first or has no frame
DTYPES = {"uint16": np.uint16, "float32": np.float32}
SCALE = {"uint16": 1e-3, "float32": 1.0}


# ---- the object, its views and crops (shared with the GPU tests) ---------------------------------------------------------------------------
LINKS = 4
MAPS = {3: [[0], [2], [1]], 2: [[0], [1, 2]]}                          # link 3 is in no group: its pixels belong to no part
SIZES = [(24, 40), (17, 33), (24, 40)]                                 # crops of the 64 x 64 image: non-square, one with odd sizes


def wedge_mesh(lo, hi):
    """A triangular prism along y: the box's bottom face and its edge (x = lo, z = hi); 6 vertices, 8 triangles."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x0, y0, z1], [x0, y1, z0], [x1, y1, z0], [x0, y1, z1]], np.float64)
    f = np.array([[0, 1, 2], [3, 5, 4], [0, 3, 4], [0, 4, 1], [0, 2, 5], [0, 5, 3], [1, 4, 5], [1, 5, 2]])
    return v, f


def object_links():
    """Link 0 a box, link 1 a wedge, link 2 a small box in front of link 1 (in link 1's frame: the two are one rigid body), link 3 a bar
    that stands clear of the others on the left, so that it hides no pixel of a part."""
    return [box_mesh([-0.16, -0.11, -0.06], [0.16, 0.11, 0.06]), wedge_mesh([-0.16, -0.11, -0.06], [0.16, 0.11, 0.06]),
            box_mesh([-0.15, -0.06, 0.06], [-0.03, 0.06, 0.13]), box_mesh([-0.04, -0.09, -0.03], [0.04, 0.09, 0.03])]


def object_mesh4():
    from articulated_pose_amd.depth import pack_mesh
    return pack_mesh(object_links())


TREE = dict(parents=[-1, 0, 1, 0], kinds=["fixed", "revolute", "fixed", "prismatic"],
            joint_xyz=[(0, 0, 0), (0.3, 0.02, 0.12), (0, 0, 0), (-0.27, -0.03, 0.02)], joint_rpy=[(0, 0, 0)] * 4,
            joint_axis=[(0, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, 0)])


def posed_object(rs, K, dtype):
    """-> (kin, view): the four-link object's kinematic table for K parts (MAPS) behind object_scene's camera.  Links 1 and 2 share one URDF
    frame and a fixed identity joint, so one pose serves both when they are one part (K = 2)."""
    S = object_scene(rs, 3)
    xyz, rpy = rs.uniform(-0.1, 0.1, (LINKS, 3)), rs.uniform(-0.5, 0.5, (LINKS, 3))
    xyz[2], rpy[2] = xyz[1], rpy[1]
    S = dict(S, link_xyz=xyz, link_rpy=rpy, joint_xyz=rs.uniform(-0.1, 0.1, (LINKS - 1, 3)))
    return kin_table(S, TREE, MAPS[K], depth_scale=SCALE[dtype]), S["viewMat"]


def poses(rs, n):
    from articulated_pose_amd.depth import pack_pose
    from test_depth_annotate_cpu import euler_sxyz
    out = []
    for _ in range(n):
        V = euler_sxyz(*rs.uniform(-0.25, 0.25, 3))
        V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
        out.append(pack_pose([0.0, rs.uniform(0.2, 0.8), 0.0, rs.uniform(-0.02, 0.02)], V))
    return np.stack(out)


def crop_origins(mesh, render):
    """The crops' origins: SIZES centred on the parts' pixels in the full image; the last crop starts two columns left of the unused link."""
    out = []
    for k, ((h, w), rt) in enumerate(zip(SIZES, render)):
        _, lab, _ = RM.render_crop(mesh[0], mesh[1], mesh[2], 64, 64, 0, 0, rt, np.uint16)
        ii, jj = np.nonzero(lab < 3)
        r0, c0 = (int(ii.min()) + int(ii.max())) // 2 - h // 2, (int(jj.min()) + int(jj.max())) // 2 - w // 2
        if k == len(SIZES) - 1:
            c0 = int(np.nonzero(lab == 3)[1].min()) - 2
        out.append((r0, c0))
    return out


def random_rigs(rs, n, K, sapien):
    from test_point_gt_build_gpu import random_rig
    return np.stack([random_rig(rs, K, sapien) for _ in range(n)])


def frames_problem(K, dtype, seed=5, sapien=False):
    """Three frames of the object: (mesh, kin, render (3, 208), scene (3, 240), rigs, norm factors -- no powers of two --, geom (3, 5),
    capacity, observed frames [(depth, labels, origin)] from the render mirror)."""
    rs = np.random.RandomState(seed + 10 * K)
    kin, _ = posed_object(rs, K, dtype)
    render, scene = PM.build_tables(kin, poses(rs, 3))
    rigs, nf = random_rigs(rs, 3, K, sapien), rs.uniform(0.7, 1.3, 3).astype(np.float32)
    mesh = object_mesh4()
    geom, a = [], 3
    for (h, w), (r0, c0) in zip(SIZES, crop_origins(mesh, render)):
        geom.append((a, h, w, r0, c0))
        a += h * w + 5
    frames = []
    for g, rt in zip(geom, render):
        d, l, _ = RM.render_crop(mesh[0], mesh[1], mesh[2], g[1], g[2], g[3], g[4], rt, DTYPES[dtype])
        frames.append((d, l, (g[3], g[4])))
    return mesh, kin, render, scene, rigs, nf, np.asarray(geom, np.int32), a + 2, frames


def predicted_frames(mesh, tables, geom, dtype):
    """The render mirror on the mirror's tables -> per frame ((depth, labels) baseline, (depth, labels) nonlinear)."""
    n = len(geom)
    out = []
    for f, g in enumerate(geom):
        out.append(tuple(RM.render_crop(mesh[0], mesh[1], mesh[2], int(g[1]), int(g[2]), int(g[3]), int(g[4]), tables[v * n + f], DTYPES[dtype])[:2]
                         for v in (0, 1)))
    return out


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose import reprojection as R
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name, nargs in NAMES:
        assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_REPROJECTION_WIDTH %d\n" % R.REPROJECTION_WIDTH in header
    assert R.REPROJECTION_WIDTH == RP.WIDTH == 15 == len(R.COLUMN_NAMES) and R.COLUMN_NAMES[R.COL_OBSERVED] == "n_obs"
    assert R.COLUMN_NAMES[R.COL_BASELINE] == "baseline_n_pred" and R.COLUMN_NAMES[R.COL_NONLINEAR] == "nonlinear_n_pred"
    assert R.COLUMN_NAMES[R.COL_NONLINEAR + 2] == "nonlinear_iou"
    named = R.named_columns(np.arange(2 * 3 * 41.0).reshape(2, 3, 41))
    assert named["n_obs"][1, 2] == 41 * 5 + 26 and named["nonlinear_mean_signed"][0, 0] == 40
    with pytest.raises(ValueError, match="15"):
        R.named_columns(np.zeros((2, 14)))
    src = open(os.path.join(os.path.dirname(HERE), "articulated-pose_amd", "csrc", "Makefile")).read()
    assert "reprojection.hip" in src


def test_entries_refuse_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device (no pointer is read on the host); an accepted call here has nframes == 0, which launches
    nothing -- after all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    rig3 = 22 + 3 * (15 + 27)
    good = dict(n=0, K=3, render=P16, scene=P16, rig=P16, rig_ld=rig3, nf=P16, record=P16, ld=26, geom=P16, cap=4096, render_out=P16, geom_out=P16)
    order = ("n", "K", "render", "scene", "rig", "rig_ld", "nf", "record", "ld", "geom", "cap", "render_out", "geom_out")
    build = lambda **over: L.ancsh_reproject_scene_build(*[dict(good, **over)[k] for k in order], None)
    assert build() == 0 and build(K=8, rig_ld=22 + 8 * (15 + 72), ld=81) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"65535"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(rig_ld=rig3 + 1), b"rig_ld"),
                       (dict(ld=25), b"ld=25"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"),
                       (dict(render=ctypes.c_void_p(4)), b"aligned"), (dict(scene=ctypes.c_void_p(12)), b"aligned"), (dict(rig=ctypes.c_void_p(4)), b"aligned"),
                       (dict(record=ctypes.c_void_p(4)), b"aligned"), (dict(render_out=ctypes.c_void_p(4)), b"aligned"),
                       (dict(nf=ctypes.c_void_p(2)), b"aligned"), (dict(geom=ctypes.c_void_p(2)), b"aligned"), (dict(geom_out=ctypes.c_void_p(6)), b"aligned")):
        assert build(**over) == -1 and what in L.ancsh_last_error() and b"reproject_scene_build" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ("render", "scene", "rig", "nf", "record", "geom", "render_out", "geom_out"):
        assert build(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    good = dict(n=0, K=3, kind=0, od=P16, ol=P16, cap=4096, pd=ctypes.c_void_p(32), pl=P16, geom=P16, scene=P16, carried=P16, ld=26,
                wide=ctypes.c_void_p(64))
    order = ("n", "K", "kind", "od", "ol", "cap", "pd", "pl", "geom", "scene", "carried", "ld", "wide")
    comp = lambda **over: L.ancsh_reproject_compare_rec(*[dict(good, **over)[k] for k in order], None)
    assert comp() == 0 and comp(kind=1) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(kind=-1), b"depth_type=-1"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"), (dict(ld=25), b"ld=25"),
                       (dict(od=ctypes.c_void_p(17)), b"aligned"), (dict(kind=1, pd=ctypes.c_void_p(18)), b"aligned"), (dict(geom=ctypes.c_void_p(2)), b"aligned"),
                       (dict(scene=ctypes.c_void_p(4)), b"aligned"), (dict(carried=ctypes.c_void_p(4)), b"aligned"), (dict(wide=ctypes.c_void_p(4)), b"aligned"),
                       (dict(wide=P16), b"overlap")):
        assert comp(**over) == -1 and what in L.ancsh_last_error() and b"reproject_compare_rec" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ("od", "ol", "pd", "pl", "geom", "scene", "carried", "wide"):
        assert comp(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k


# ---- the option -------------------------------------------------------------------------------------------------------------------------------
def test_the_option_is_one_rule_of_check_options():
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, pack_sensor
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import OPTION_FLAGS, RESULT_NAMES, check_options
    assert "reprojection" in OPTION_FLAGS and "record_reproj" not in RESULT_NAMES and "reprojection" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    # valid on every pipeline that holds a mesh: rendered, posed, a library, with a sensor, the images, keyed, guarded -- and nothing else moves
    for extra in (dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(render_mesh=pack_mesh_library([mesh, mesh])),
                  dict(render_mesh=mesh, sensor=pack_sensor(p_hole=0.1), annotated_images=True, keyed=True),
                  dict(render_mesh=mesh, ground_truth=True, build_gt_pose=True, range_guard=True, fit_quality=True, joint_states=True)):
        off, on = check_options(batch_size=2, **dict(annotated, **extra)), check_options(batch_size=2, reprojection=True, **dict(annotated, **extra))
        assert on.reprojection and not off.reprojection and on.record_key == "record_reproj" and on.record_width == off.record_width + 15
        assert on._replace(reprojection=False, record_key=off.record_key, record_width=off.record_width) == off
    # the record's width and the name the step leaves it under, for every combination of fit_quality / ground_truth
    for fq in (False, True):
        for gt in (False, True):
            o = check_options(batch_size=2, render_mesh=mesh, reprojection=True, fit_quality=fq, ground_truth=gt, **annotated)
            assert o.record_width == (39 if fq else 26) + (12 if gt else 0) + 21 + 15 and o.record_key == "record_reproj", (fq, gt)
    # anywhere else: ValueError that names what is missing
    for kw in (dict(), dict(raw_capacity=1000), dict(depth_capacity=4096, joint_source="predicted"), annotated,
               dict(annotated, sensor=pack_sensor(p_hole=0.1)), dict(raw_capacity=1000, articulation=True, point_ground_truth=True, build_point_gt=True)):
        with pytest.raises(ValueError, match="reprojection=True .* render_mesh"):
            check_options(reprojection=True, **kw)
        with pytest.raises(ValueError, match="render_mesh"):
            AncshPipeline(3, None, None, 2, 64, "cpu", reprojection=True, **kw)
    with pytest.raises(ValueError, match="ShardedPipeline .* reprojection=True .* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, reprojection=True)
    with pytest.raises(ValueError, match="ShardedPipeline .* reprojection=True .* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", reprojection=True)


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------------
# The closed form's bound.  With the exact record, a link's predicted map is  D (1 / nf) P Q (M_l o R_l)  with  P = nf D R_l N^-1 Q^-1 , which is
# R_l itself in exact arithmetic.  Every factor is a 4 x 4 product whose entry is a sum of at most 4 terms, so a product costs at most 4 roundings
# relative to the sum of its terms' magnitudes; counted along the chain:
#   the mirror: M o R 4, Q's offset and entries 5, Q o N 4, s R 1, P o T1 4, the division by nf 1                                          = 19
#   the record: Q^-1 (Rr^T 0.5, the subtraction, two divisions) 4, N^-1 (-Rc^T offset) 3, four 4 x 4 products 16, nf 1, s and / s 2         = 26
#   the rotations are orthonormal only to rounding: Rc and Rr are products of three axis rotations (2 products x 3 + 2 trig roundings = 8
#   each), Ra = -R_l's rotation is V o X_0 o X_1 o X_2 with X = T o J (up to 6 products x 3 = 18, J's entries 6, T's 8 as Rc)               = 48
# 93 roundings, each relative to at most G = the product of the infinity norms of the six factors R_l, N^-1, Q^-1, Q, M_l, R_l.  The stated
# multiple is the next power of two, 128; it is derived, not tuned.
ROUNDINGS = 128


def _norm(A):
    return np.abs(np.vstack([np.asarray(A).reshape(3, 4), [0, 0, 0, 1.0]])).sum(1).max()


@pytest.mark.parametrize("K,sapien", [(2, False), (3, False), (3, True)], ids=["K2", "K3", "K3-sapien-rotation"])
def test_exact_record_gives_back_the_frames_own_render_table(K, sapien):
    mesh, kin, render, scene, rigs, nf, geom, cap, _ = frames_problem(K, "uint16", sapien=sapien)
    assert (rigs[:, 3] != 0).all() == sapien and not any(float(v) in (0.5, 1.0, 2.0) for v in nf)
    rec = RP.exact_record(render, scene, rigs, nf, kin, K)
    assert np.isfinite(rec).all()
    tables, gout = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    assert tables.shape == (6, 208) and gout.shape == (6, 5)
    worst = 0.0
    for v in range(2):
        for f in range(3):
            row = tables[v * 3 + f]
            assert row[:16].tobytes() == render[f, :16].tobytes()
            assert gout[v * 3 + f].tolist() == [geom[f, 0] + v * cap] + geom[f, 1:].tolist()
            parts, nl = RP.link_parts(scene[f], K)
            assert nl == LINKS and parts[3] == -1 and (parts[:3] >= 0).all()
            assert np.isnan(row[16 + 12 * 3:16 + 12 * 4]).all() and (row[16 + 12 * 4:] == 0).all()       # the unused link; links the object lacks
            for l in range(3):
                j = parts[l]
                own, got = render[f, 16 + 12 * l:28 + 12 * l], row[16 + 12 * l:28 + 12 * l]
                k = kin[PM.KIN_HEAD + PM.KIN_LINK * l:PM.KIN_HEAD + PM.KIN_LINK * (l + 1)]
                _, factors = RP.exact_pose(render[f], rigs[f], np.float64(nf[f]), (k[19:28].reshape(3, 3), k[28:31]), l, j, K)
                G = _norm(own) ** 2 * _norm(scene[f, 16 + 14 * l + 2:16 + 14 * (l + 1)]) * _norm(RP.nocs_map(rigs[f], j, K))
                G *= np.abs(factors[1]).sum(1).max() * np.abs(factors[2] @ factors[3]).sum(1).max()
                err = np.abs(got - own).max()
                worst = max(worst, err / (2.0 ** -52 * G))
                assert err <= ROUNDINGS * 2.0 ** -52 * G, (K, v, f, l, err, G)
    print("worst error / (2^-52 G): %.3g of %d allowed" % (worst, ROUNDINGS))


def test_scene_mirror_nan_rules_and_geometry():
    """A part with a NaN pose, a norm factor of 0 and of inf, a link outside parts_map, a start that does not fit: NaN maps, not garbage."""
    K = 3
    mesh, kin, render, scene, rigs, nf, geom, cap, _ = frames_problem(K, "uint16")
    rec = RP.exact_record(render, scene, rigs, nf, kin, K)
    rec[0, 1, 13 + 9] = np.nan                                           # frame 0, part 1 (link 2), the nonlinear pose's scale
    rec[1, 0, 3] = np.inf                                                # frame 1, part 0 (link 0), the baseline pose
    nf2 = nf.copy()
    nf2[2] = 0.0
    g2 = geom.copy()
    g2[1, 0] = -4
    tables, gout = RP.scene_tables(render, scene, rigs, nf2, rec, g2, cap)
    link = lambda row, l: tables[row, 16 + 12 * l:28 + 12 * l]
    assert np.isnan(link(3 + 0, 2)).all() and np.isfinite(link(0, 2)).all() and np.isfinite(link(3 + 0, 0)).all()
    assert np.isnan(link(1, 0)).all() and np.isfinite(link(3 + 1, 0)).all()
    assert all(np.isnan(link(r, l)).all() for r in (2, 5) for l in range(4))
    assert gout[1, 0] == -4 and gout[4, 0] == -4 and gout[3, 0] == geom[0, 0] + cap
    nf2[2] = np.inf
    assert np.isnan(RP.scene_tables(render, scene, rigs, nf2, rec, g2, cap)[0][2, 16:16 + 48]).all()


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_exact_poses_reproduce_the_frame_and_a_shifted_pose_does_not(K, dtype):
    """The two bars the GPU test holds the kernels to, met by the mirror alone: with the exact record every part's IoU is >= 0.99 and, for
    uint16, max |d| <= one depth quantum.  A pose translated by a tenth of the part's extent has a strictly lower IoU and a strictly larger
    mean |d|.  Every used link shows at least the scene's minimum of pixels in every crop, and the unused link shows in one."""
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = frames_problem(K, dtype)
    hist = np.array([np.bincount(l.reshape(-1), minlength=256) for _, l, _ in frames])
    print(hist[:, :4], hist[:, 255])
    assert (hist[:, :3] >= scene[:, 13:14]).all() and hist[:, 3].max() > 0 and hist[:, 4:255].sum() == 0
    rec = RP.exact_record(render, scene, rigs, nf, kin, K)
    shifted = rec.copy()
    shifted[:, :, 13 + 10] += 0.1 * 0.32 * nf[:, None]                   # the nonlinear pose only: a tenth of the box's 0.32 along camera x
    cols = []
    for r in (rec, shifted):
        tables, _ = RP.scene_tables(render, scene, rigs, nf, r, geom, cap)
        pred = predicted_frames(mesh, tables, geom, dtype)
        cols.append(RP.compare([(d, l) for d, l, _ in frames], pred, scene, r)[:, :, 26:])
    exact, moved = cols
    print(exact[:, :, [0, 8, 9, 10, 11, 13]], moved[:, :, [10, 11]])
    assert np.isfinite(exact).all() and (exact[:, :, 0] > 0).all()
    assert (exact[:, :, 3] >= 0.99).all() and (exact[:, :, 10] >= 0.99).all()
    if dtype == "uint16":
        assert (exact[:, :, 6] <= SCALE[dtype] * (1 + 1e-12)).all() and (exact[:, :, 13] <= SCALE[dtype] * (1 + 1e-12)).all()
    assert moved[:, :, 1:8].tobytes() == exact[:, :, 1:8].tobytes()      # the baseline pose did not move
    assert (moved[:, :, 10] < exact[:, :, 10]).all() and (moved[:, :, 11] > exact[:, :, 11]).all()


def test_compare_mirror_on_hand_made_crops():
    """Empty intersection, empty union, one pixel, a part only the prediction has, holes on either side (depth 0 / label 255), a link of no
    part: counts, IoU and the NaN rules by hand."""
    K = 3
    sc = np.zeros(240)
    sc[6], sc[14] = 0.5, 4
    for l, (rank, part) in enumerate(((0, 0), (1, 1), (2, 2), (-1, 0))):
        sc[16 + 14 * l], sc[16 + 14 * l + 1] = rank, part
    lab_o = np.array([[0, 0, 1, 255, 3, 0]], np.uint8)
    dep_o = np.array([[10, 0, 20, 30, 40, 12]], np.uint16)               # pixel 1: a hole in the observation
    lab_p = np.array([[0, 0, 2, 2, 0, 255]], np.uint8)
    dep_p = np.array([[14, 11, 21, 31, 41, 13]], np.uint16)
    carried = np.arange(3 * 26.0).reshape(1, 3, 26)
    carried[0, 2, 13:] = np.nan                                          # part 2: no nonlinear pose
    wide = RP.compare([(dep_o, lab_o)], [((dep_p, lab_p), (dep_p, lab_p))], sc[None], carried)
    assert wide.shape == (1, 3, 41) and wide[:, :, :26].tobytes() == carried.tobytes()
    c = wide[0, :, 26:]
    # part 0: observed pixels 0 and 5 (pixel 1 is a hole, pixel 4 is the unused link), predicted 0, 1, 4; both: pixel 0, dq = 4
    assert c[0, :8].tolist() == [2, 3, 1, 1 / 4, 2.0, 2.0, 2.0, 2.0] and c[0, 8:].tolist() == c[0, 1:8].tolist()
    # part 1: observed pixel 2 only, never predicted: empty intersection, IoU 0, the depth columns NaN
    assert c[1, :4].tolist() == [1, 0, 0, 0.0] and np.isnan(c[1, 4:8]).all()
    # part 2: only the prediction has it; its nonlinear pose is not finite
    assert c[2, :4].tolist() == [0, 2, 0, 0.0] and np.isnan(c[2, 4:]).all()
    # an empty union, and a poisoned row
    blank = (np.zeros((1, 6), np.uint16), np.full((1, 6), 255, np.uint8))
    c = RP.compare([blank], [(blank, blank)], sc[None], carried)[0, :, 26:]
    assert c[0, :3].tolist() == [0, 0, 0] and np.isnan(c[0, 3:8]).all()
    c = RP.compare([(dep_o, lab_o)], [((dep_p, lab_p), (dep_p, lab_p))], sc[None], np.full((1, 3, 26), np.nan))[0, :, 26:]
    assert np.isnan(c).all()
    # float32: the same pixels, depths in metres; +inf and NaN are holes
    wide = RP.compare([(np.array([[1.0, np.nan, 2.0, 3.0, 4.0, np.inf]], np.float32), lab_o)],
                      [((dep_p.astype(np.float32), lab_p), (dep_p.astype(np.float32), lab_p))], sc[None], carried)
    assert wide[0, 0, 26:30].tolist() == [1, 3, 1, 1 / 3] and wide[0, 0, 30] == 6.5
