"""CPU (no GPU): the joint step of render-and-compare ICP.  pack_refine(joints=)'s table and check_refine_table's refusals in their order, the
rule in check_options, the entry's place in the ABI and its argument checks before any launch, and the mirror (tests/joint_step_mirror.py)
validated on its own: the residual rows of an exact posed record vanish to rounding whatever the tree, a step of zero and today's cost there,
and the rows' Jacobians against central differences of the mirror's own residuals through ancsh_reproject_scene_build's mirror.  The inputs of
the GPU tests' two behavioural bars are derived here, as test_refinement_cpu derives its perturbation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import joint_step_mirror as JS
import pose_scene_mirror as PM
import refinement_mirror as RF
import reprojection_mirror as RP
from test_pose_scene_cpu import kin_table
from test_refinement_cpu import MAX_DIST, SHIFT, TILT_DEG, centroids, perturbed_record, refine_problem
from test_render_cpu import box_mesh, object_scene
from test_reprojection_cpu import LINKS, MAPS, SCALE, TREE, poses, posed_object, random_rigs

HERE = os.path.dirname(os.path.abspath(__file__))
P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first or has no frame
EPS = 2.0 ** -52
# the trees of the mirror's own tests: test_reprojection_cpu's four links (1 revolute on 0, 2 fixed on 1, 3 prismatic on 0) grouped so that
# the revolute joint, the prismatic joint, both, and a part of two links (1 and 2) are all met, at K = 2 and 3
TREES = {"K2-revolute-two-link-part": (2, MAPS[2]), "K3-revolute": (3, MAPS[3]), "K2-prismatic": (2, [[0, 1, 2], [3]]),
         "K3-both-two-link-part": (3, [[0], [1, 2], [3]])}
ACTIVE = {"K2-revolute-two-link-part": {1: 1}, "K3-revolute": {1: 1}, "K2-prismatic": {3: 2}, "K3-both-two-link-part": {1: 1, 3: 2}}


def joints_table(**over):
    from articulated_pose_amd.pose.refinement import pack_refine
    return pack_refine(**dict(dict(iters=3, max_dist=MAX_DIST, joints=dict(weight=1.0, axis_length=0.5)), **over))


def tree_problem(K, maps, seed=5):
    """Three posed frames of the four-link object grouped by `maps`, without pixels: (kin, render (3, 208), scene (3, 240), rigs, nf, geom,
    cap, the exact record (3, K, 26))."""
    rs = np.random.RandomState(seed + 10 * K)
    S = object_scene(rs, 3)
    xyz, rpy = rs.uniform(-0.1, 0.1, (LINKS, 3)), rs.uniform(-0.5, 0.5, (LINKS, 3))
    xyz[2], rpy[2] = xyz[1], rpy[1]
    S = dict(S, link_xyz=xyz, link_rpy=rpy, joint_xyz=rs.uniform(-0.1, 0.1, (LINKS - 1, 3)))
    kin = kin_table(S, TREE, maps, depth_scale=1e-3)
    render, scene = PM.build_tables(kin, poses(rs, 3))
    rigs, nf = random_rigs(rs, 3, K, False), rs.uniform(0.7, 1.3, 3).astype(np.float32)
    geom = np.array([(3 + 1000 * f, 24, 40, 10, 12) for f in range(3)], np.int32)
    return kin, render, scene, rigs, nf, geom, 4000, RP.exact_record(render, scene, rigs, nf, kin, K)


def chain_problem(nlinks=8, n=2, seed=9):
    """A chain of `nlinks` links, each a part of its own, joints alternately revolute and prismatic with random origins, rotations and axes:
    the 6 * nlinks solve without a pixel.  -> tree_problem's tuple for n frames."""
    from articulated_pose_amd.depth import pack_pose
    from test_depth_annotate_cpu import euler_sxyz
    rs = np.random.RandomState(seed)
    S = object_scene(rs, 3)
    S = dict(S, link_xyz=rs.uniform(-0.1, 0.1, (nlinks, 3)), link_rpy=rs.uniform(-0.5, 0.5, (nlinks, 3)), joint_xyz=rs.uniform(-0.1, 0.1, (nlinks - 1, 3)))
    axes = rs.normal(size=(nlinks, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    tree = dict(parents=[-1] + list(range(nlinks - 1)), kinds=["fixed"] + [("revolute", "prismatic")[l % 2] for l in range(nlinks - 1)],
                joint_xyz=[(0, 0, 0)] + [tuple(v) for v in rs.uniform(-0.15, 0.15, (nlinks - 1, 3))],
                joint_rpy=[(0, 0, 0)] + [tuple(v) for v in rs.uniform(-0.6, 0.6, (nlinks - 1, 3))],
                joint_axis=[(0, 0, 0)] + [tuple(v) for v in axes[1:]])
    kin = kin_table(S, tree, [[l] for l in range(nlinks)], depth_scale=1e-3)
    ps = []
    for _ in range(n):
        V = euler_sxyz(*rs.uniform(-0.25, 0.25, 3))
        V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
        ps.append(pack_pose([0.0] + [rs.uniform(0.2, 0.8) if l % 2 == 0 else rs.uniform(-0.05, 0.05) for l in range(nlinks - 1)], V))
    render, scene = PM.build_tables(kin, np.stack(ps))
    rigs, nf = random_rigs(rs, n, nlinks, False), rs.uniform(0.7, 1.3, n).astype(np.float32)
    geom = np.array([(3 + 1000 * f, 24, 40, 10, 12) for f in range(n)], np.int32)
    return kin, render, scene, rigs, nf, geom, 1000 * n + 1000, RP.exact_record(render, scene, rigs, nf, kin, nlinks)


def moved_record(rs, rec, scale):
    """Every pose of a record moved by a random step of size `scale` with the pass's own update."""
    out = rec.copy()
    for f, j, v in np.ndindex(rec.shape[0], rec.shape[1], 2):
        p = list(rec[f, j, 13 * v:13 * v + 13])
        out[f, j, 13 * v:13 * v + 13] = JS.pose_step(list(rs.normal(scale=scale, size=6)), p, RF.centre(p))
    return out


def frame_joints(kin, scene, tables, nf, rec, K, f, v, axis_len=0.5, frozen=None):
    p = [[float(x) for x in rec[f, j, 13 * v:13 * v + 13]] for j in range(K)]
    nfv = float(np.float32(nf[f]))
    live = [RF.pose_ok(q, nfv) for q in p]
    return JS.joints(kin, scene[f], tables[v * len(rec) + f], nfv, live, [RF.centre(q) if ok else None for q, ok in zip(p, live)], K, axis_len, frozen)


# ---- the behavioural bars' inputs (shared with the GPU tests) ------------------------------------------------------------------------------
# (a) every part of the exact record is perturbed DIFFERENTLY: test_refinement_cpu's perturbation (a tilt about an axis through the part's
# observed centroid and a shift along its ray; the axis already differs per frame, part and pose) with another angle and another shift per
# part, so the two sides of the hinge come apart.  Nothing here is tuned against the joint step: the sizes are test_refinement_cpu's SHIFT and
# TILT_DEG scaled by simple factors.
# (b) the part that is too small to be refined on its own is the wedge's (link 1, the revolute joint's child): min_pixels is one above the
# pixels it shows in any frame.  Its record is the exact one with THAT part alone perturbed as in (a): the base must use more pixels than the
# wedge's part shows, which a perturbed base does not (it uses fewer pixels than it shows), and a base that slides along its one flat face
# drags the part it is hinged to along -- a weakness of the base's own rows, not what this bar is about.
PART_SHIFT, PART_TILT = (1.0, -0.5, 0.75), (1.0, 1.5, 0.5)


def split_record(rec, cen):
    out = rec.copy()
    for j in range(rec.shape[1]):
        out[:, j] = perturbed_record(rec, cen, shift=SHIFT * PART_SHIFT[j], deg=TILT_DEG * PART_TILT[j])[:, j]
    return out


def joint_problem(K, dtype):
    """refine_problem and the record whose parts are perturbed differently: (problem tuple, exact, split)."""
    prob, rec, _ = refine_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    return prob, rec, split_record(rec, centroids(scene, nf, frames, K))


def small_part_problem(prob, rec, split, K):
    """Bar (b)'s inputs: (the wedge's part j, min_pixels, the exact record with part j alone perturbed)."""
    j, min_pixels = small_part(prob, K)
    one = rec.copy()
    one[:, j] = split[:, j]
    return j, min_pixels, one


def kept_gaps(prob, columns, K):
    """The hinge gap |x_c - x_p| of the kept poses (the 36 columns' two refined poses): (3 frames, 2 poses) of the revolute joint, link 1."""
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    b = columns.reshape(3, K, 2, 18)
    rec = np.concatenate([b[:, :, 0, :13], b[:, :, 1, :13]], 2)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    gaps = JS.hinge_gaps(kin, scene, tables, nf, rec, K)
    return np.array([[g[v][1] for v in range(2)] for g in gaps])


def as_columns(rec):
    """A (3, K, 26) record as the 36 columns kept_gaps reads (the costs left 0)."""
    z = np.zeros(rec.shape[:2] + (5,))
    return np.concatenate([rec[:, :, :13], z, rec[:, :, 13:26], z], 2)


def small_part(prob, K):
    """The part of link 1 (the wedge) and a min_pixels one above its largest observed pixel count over the frames: the plain loop never moves it."""
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    j = int(RP.link_parts(scene[0], K)[0][1])
    counts = [int((RP.part_image(d, l, RP.link_parts(scene[f], K)[0]) == j).sum()) for f, (d, l, _) in enumerate(frames)]
    return j, max(counts) + 1


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def test_pack_refine_joints_layout_and_refusals_in_order():
    from articulated_pose_amd.pose import refinement as R
    t = R.pack_refine(joints=dict(weight=2.0, axis_length=0.25))
    assert t.shape == (24,) and t.dtype == np.float64 and t[:8].tobytes() == R.pack_refine().tobytes() and (t[8:16] == 0).all()
    assert t[16:].tolist() == [2.0, 0.25, 0, 0, 0, 0, 0, 0] and R.has_joints(t) and not R.has_silhouette(t)
    assert R.pack_refine(joints={})[16:18].tolist() == [1.0, 0.5] and R.pack_refine(joints=(3.0, 0.0))[16:18].tolist() == [3.0, 0.0]
    both = R.pack_refine(iters=2, silhouette=(1.5, 0.1), joints=(1.0, 0.5))
    assert both.shape == (24,) and both[:16].tobytes() == R.pack_refine(iters=2, silhouette=(1.5, 0.1)).tobytes() and R.has_silhouette(both)
    assert not R.has_joints(R.pack_refine()) and not R.has_joints(R.pack_refine(silhouette=(1.0, 0.1))) and R.has_silhouette(R.pack_refine(silhouette=(1.0, 0.1)))
    assert R.REFINE_JOINT_PARAMS == JS.PARAMS == 24 and R.REFINE_OBJ == JS.OBJ == len(R.OBJ_COLUMNS) == 8 and R.JOINT_XI == JS.XI == 48
    for kw, what in ((dict(joints=dict(weight=0.0)), "joints weight"), (dict(joints=dict(weight=float("nan"))), "joints weight"),
                     (dict(joints=(1.0, -0.1)), "joints axis_length"), (dict(joints=(1.0, float("inf"))), "joints axis_length"),
                     (dict(joints=dict(length=1.0)), "joints takes"), (dict(joints=("a", 1.0)), "joints is"), (dict(joints=1.0), "joints is"),
                     (dict(iters=0, joints=(0.0, 0.5)), "iters"), (dict(silhouette=(0.0, 0.1), joints=(0.0, 0.5)), "silhouette weight")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            R.pack_refine(**kw)
    # check_refine_table's order: the head, the reserved values 6..7, the silhouette values, the joints' values, the reserved values 18..23
    bad = t.copy()
    bad[[0, 7, 9, 16, 23]] = [0.0, 1.0, 1.0, -1.0, 1.0]
    for fix, what in ((0, "iters"), (7, "reserved values 6..7"), (9, "silhouette weight"), (16, "joints weight"), (23, r"reserved values 18\.\.23")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            R.check_refine_table(bad)
        bad[fix] = t[fix]
    assert R.check_refine_table(bad).tobytes() == t.tobytes()
    sil = both.copy()
    sil[12] = 1.0
    with pytest.raises(ValueError, match=r"refine: the reserved values 11\.\.15 must be 0"):
        R.check_refine_table(sil)
    for shape in ((7,), (17,), (23,), (25,), (2, 24)):
        with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table \(pose.refinement.pack_refine\), or \(16,\) with silhouette=, got shape"):
            R.check_refine_table(np.zeros(shape))
    assert "nobody has tuned" in R.pack_refine.__doc__.split("joints =")[1]


def test_the_option_needs_kinematics_and_options_keeps_its_tail():
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.refinement import pack_refine
    from articulated_pose_amd.stream import RESULT_NAMES, Options, check_options
    assert Options._fields[-3:] == ("refine_joints", "silhouette", "refine") and "refine_object" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    plain, sil = pack_refine(), pack_refine(silhouette=(1.0, 0.1))
    for table, silhouette in ((pack_refine(joints=(1.0, 0.5)), False), (pack_refine(silhouette=(1.0, 0.1), joints=(1.0, 0.5)), True)):
        on = check_options(batch_size=2, render_mesh=mesh, kinematics=kin, refine=table, **annotated)
        off = check_options(batch_size=2, render_mesh=mesh, kinematics=kin, refine=sil if silhouette else plain, **annotated)
        assert on.refine_joints is True and off.refine_joints is False and on.silhouette is silhouette and on._replace(refine_joints=False) == off
        with pytest.raises(ValueError, match=r"refine=.*joints=.*kinematics=<depth.pack_kinematics\(\.\.\.\)>"):
            check_options(batch_size=2, render_mesh=mesh, refine=table, **annotated)
        with pytest.raises(ValueError, match="kinematics=<depth.pack_kinematics"):
            AncshPipeline(3, None, None, 2, 64, "cpu", render_mesh=mesh, refine=table, **annotated)
        with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
            ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, refine=table)
    assert check_options(batch_size=2, render_mesh=mesh, kinematics=kin, refine=plain, **annotated).refine_joints is False
    assert check_options(batch_size=2, render_mesh=mesh, kinematics=kin, **annotated).refine_joints is False


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    name = "ancsh_refine_joint_step"
    assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 20
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_REFINE_JOINT_PARAMS 24\n" in header and "#define ANCSH_REFINE_OBJ 8\n" in header


def test_entry_refuses_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device; an accepted call here has nframes == 0, which launches nothing -- after all the checks."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    ptrs = ("kin", "scene", "rt", "nf", "params", "pin", "sums", "pout", "best", "state", "obj", "xi")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, ninst=1, p=0, last=0, ld=26, sld=32, pout=ctypes.c_void_p(32), state=ctypes.c_void_p(64))
    order = ("n", "K", "kin", "ninst", "scene", "rt", "nf", "params", "p", "last", "pin", "ld", "sums", "sld", "pout", "best", "state", "obj", "xi")
    run = lambda **over: L.ancsh_refine_joint_step(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(K=8, ninst=65535, p=8, last=1, ld=77, sld=36, xi=None) == 0 and run(K=1) == 0
    odd = lambda a: ctypes.c_void_p(a)
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(ninst=0), b"ninst=0"),
                       (dict(ninst=65536), b"ninst=65536"), (dict(p=-1), b"pass=-1"), (dict(p=9), b"pass=9"), (dict(last=2), b"is_last=2"),
                       (dict(ld=25), b"ld_in=25"), (dict(sld=30), b"sums_ld=30"), (dict(sld=33), b"sums_ld=33"), (dict(nf=odd(18)), b"aligned"),
                       (dict(pout=P16), b"overlap"), (dict(state=P16), b"overlap")) + \
            tuple((dict({k: odd(20)}), b"aligned") for k in ptrs if k != "nf"):
        assert run(**over) == -1 and what in L.ancsh_last_error() and b"refine_joint_step" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs[:-1]:
        assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TREES))
def test_exact_records_have_no_residual_whatever_the_tree(name):
    """At a record that reproduces the frame's own tables the two sides of every joint agree: W_l = W_p o T_l o J_l(q), so x_c = x_p for a
    revolute joint, x_c - x_p lies along the axis for a prismatic one (the projection removes it), and the directions agree.  Every residual
    row is within 64 eps of its operands' magnitude: the larger |coordinate| of the two points (times |P| <= 1), axis_length for a direction."""
    K, maps = TREES[name]
    kin, render, scene, rigs, nf, geom, cap, rec = tree_problem(K, maps)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    worst = 0.0
    for f in range(3):
        for v in range(2):
            J = frame_joints(kin, scene, tables, nf, rec, K, f, v)
            assert {jt["l"]: jt["kind"] for jt in J} == ACTIVE[name], (name, f, v, [(jt["l"], jt["kind"]) for jt in J])
            for jt in J:
                assert len(jt["r0"]) == (6 if jt["kind"] == 1 else 9) and jt["a"] != jt["b"]
                mag = max(max(abs(x) for x in jt["xc"]), max(abs(x) for x in jt["xp"]))
                pos, dirs = np.abs(jt["r0"][:3]).max(), np.abs(jt["r0"][3:]).max()
                worst = max(worst, pos / (EPS * mag), dirs / (EPS * 0.5))
                assert pos <= 64 * EPS * mag and dirs <= 64 * EPS * 0.5, (name, f, v, jt["l"], pos / (EPS * mag), dirs / (EPS * 0.5))
                if jt["kind"] == 2:                                      # the slide itself is not a residual: the raw gap is the joint value
                    raw = np.subtract(jt["xc"], jt["xp"])
                    assert np.linalg.norm(raw) > 1e-4 and abs(abs(np.dot(raw, jt["up"])) - np.linalg.norm(raw)) <= 64 * EPS * mag
    print(name, "worst residual / (eps * magnitude): %.3g" % worst)


def test_a_chain_of_eight_parts_has_seven_joints_and_no_residual():
    K = 8
    kin, render, scene, rigs, nf, geom, cap, rec = chain_problem()
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    for f, v in np.ndindex(2, 2):
        J = frame_joints(kin, scene, tables, nf, rec, K, f, v)
        assert [(jt["l"], jt["kind"], jt["a"], jt["b"]) for jt in J] == [(l, 1 if l % 2 else 2, l, l - 1) for l in range(1, 8)]
        for jt in J:
            mag = max(max(abs(x) for x in jt["xc"]), max(abs(x) for x in jt["xp"]))
            assert np.abs(jt["r0"][:3]).max() <= 64 * EPS * mag and np.abs(jt["r0"][3:]).max() <= 64 * EPS * 0.5, (f, v, jt["l"], jt["r0"])
    table = joints_table(max_angle_deg=90.0, max_dist=10.0)
    rs = np.random.RandomState(2)
    moved = moved_record(rs, rec, 0.01)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, moved, geom, cap)
    S = hand_sums(rs, K, b_scale=1e-3)
    ob = np.zeros(8)
    xi, out, best, J = JS.joint_step(kin, scene[0], tables[0], float(nf[0]), table, 0, False, moved[0, :, :13], S, moved[0, :, :13], np.full((K, 18), np.nan), ob)
    H, g = JS.system(J, S, [True] * K, list(S[:, 28]), K, table, table[16] ** 2 * S[:, 28].mean())
    want = np.linalg.solve(np.array(H), -np.array(g))
    assert ob[5] == 7 and ob[6] == 1 and np.abs(xi - want).max() <= 1e-10 * np.abs(want).max()


def hand_sums(rs, K, b_scale=0.0, n=(400.0, 90.0, 250.0, 70.0, 333.0, 150.0, 200.0, 100.0), width=32):
    """One pose's sums rows (K, width): A = n_j times a random SPD 6 x 6, b = b_scale * n_j * noise, a cost and counts."""
    S = np.zeros((K, width))
    for j in range(K):
        M = rs.normal(size=(6, 6))
        A = n[j] * (M @ M.T / 6 + 0.1 * np.eye(6))
        S[j, :21], S[j, 21:27] = A[np.triu_indices(6)], b_scale * n[j] * rs.normal(size=6)
        S[j, 27], S[j, 28], S[j, 29], S[j, 31] = 1e-6 * n[j], n[j], n[j] + 10 * j, 1.0
        S[j, 30] = RF.cost(S[j], [0, MAX_DIST])
    return S


@pytest.mark.parametrize("name", list(TREES))
def test_exact_records_take_no_step_and_cost_what_they_cost_today(name):
    """With b_j = 0 the only right-hand side is G^T r0 of rounding size: |xi| <= |g| / lambda_min(H); and Cobj is the parts' costs weighted by
    their observed pixels -- today's cost of the object -- to the rounding of the sums and the residuals' 64 eps squared."""
    K, maps = TREES[name]
    kin, render, scene, rigs, nf, geom, cap, rec = tree_problem(K, maps)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    table = joints_table()
    rs = np.random.RandomState(3)
    for f in range(3):
        S = hand_sums(rs, K)
        poses_f = rec[f, :, :13]
        state, obj = np.full((K, 18), np.nan), np.zeros(8)
        xi, out, best, J = JS.joint_step(kin, scene[f], tables[f], float(nf[f]), table, 0, False, poses_f, S, poses_f, state, obj)
        live = [True] * K
        nbar = S[:, 28].mean()
        H, g = JS.system(J, S, live, list(S[:, 28]), K, table, table[16] ** 2 * nbar)
        bound = np.linalg.norm(g) / np.linalg.eigvalsh(np.array(H)).min()
        assert obj[5] == len(ACTIVE[name]) and obj[6] == 1 and np.abs(xi).max() <= 2 * bound + 1e-300 and bound < 1e-12, (name, f, bound)
        today = (S[:, 30] * S[:, 29]).sum() / S[:, 29].sum()
        assert abs(obj[4] - today) <= 8 * EPS * today + table[16] ** 2 * nbar * 9 * len(J) * (64 * EPS * 2) ** 2 and obj[0] == obj[1] == obj[4]
        assert np.abs(out - poses_f).max() <= 4 * bound + 8 * EPS * np.abs(poses_f).max()
        assert best[:, :13].tobytes() == poses_f.tobytes() and (best[:, 16] == 0).all() and (best[:, 17] == 1).all()
        assert (best[:, 13] == S[:, 30]).all() and (best[:, 14] == S[:, 30]).all() and (best[:, 15] == S[:, 28]).all()


@pytest.mark.parametrize("name", list(TREES))
def test_jacobians_equal_central_differences_of_the_residuals(name):
    """Every part's pose is stepped by +-h along each of its six directions with the pass's own update, the predicted tables are rebuilt by
    ancsh_reproject_scene_build's mirror, and the residual rows recomputed (a prismatic joint's projection held at the unperturbed u_p, as
    the rows are linearised).  Central differences have a truncation error of h^2 / 6 times the third derivative: a point at distance rho
    from the centre turning through the quaternion of (1, w / 2) has one of at most rho (1 + 1 / 4), rho <= 2 in the cloud's unit; the
    rounding of the residuals (64 eps) is divided by 2 h.  h = 1e-4: the bound is 2 h^2 + 64 eps / h."""
    K, maps = TREES[name]
    kin, render, scene, rigs, nf, geom, cap, rec0 = tree_problem(K, maps)
    rs = np.random.RandomState(11)
    rec = rec0.copy()
    for j in range(K):                                                   # away from the exact record: the rows are general, not only at zero residual
        for v in range(2):
            for f in range(3):
                p = rec0[f, j, 13 * v:13 * v + 13]
                rec[f, j, 13 * v:13 * v + 13] = JS.pose_step(list(rs.normal(scale=0.02, size=6)), list(p), RF.centre(list(p)))
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    h, f, v = 1e-4, 1, 0
    J0 = frame_joints(kin, scene, tables, nf, rec, K, f, v)
    frozen = {jt["l"]: jt["up"] for jt in J0}
    r0, G = JS.stacked(J0, K)
    assert len(J0) == len(ACTIVE[name]) and np.abs(r0).max() > 1e-4
    worst = 0.0
    for j in range(K):
        p = list(rec[f, j, :13])
        c = RF.centre(p)
        for k in range(6):
            side = []
            for sgn in (1.0, -1.0):
                xi = [0.0] * 6
                xi[k] = sgn * h
                moved = rec.copy()
                moved[f, j, :13] = JS.pose_step(xi, p, c)
                t2, _ = RP.scene_tables(render, scene, rigs, nf, moved, geom, cap)
                J = frame_joints(kin, scene, t2, nf, moved, K, f, v, frozen=frozen)
                side.append(JS.stacked(J, K)[0])
            fd = (side[0] - side[1]) / (2 * h)
            err = np.abs(fd - G[:, 6 * j + k]).max()
            worst = max(worst, err)
            assert err <= 2 * h * h + 64 * EPS / h, (name, j, k, err, fd, G[:, 6 * j + k])
    print(name, "worst |central difference - G|: %.3g (bound %.3g)" % (worst, 2 * h * h + 64 * EPS / h))


def test_solve_matches_numpy_and_the_special_cases_follow_the_header():
    """The 6 K Cholesky against numpy's solver; the object's clamp; nothing to solve (no active joint at K = 1 and under another tree, is_last,
    all-zero sums of one part: a failed Cholesky needs a pivot <= 0, which the damping's 1e-12 prevents unless a value is not finite); NaN
    poses, a zero norm factor, an instance or a parent out of range."""
    name = "K3-both-two-link-part"
    K, maps = TREES[name]
    kin, render, scene, rigs, nf, geom, cap, rec0 = tree_problem(K, maps)
    rs = np.random.RandomState(5)
    rec = rec0.copy()
    for j in range(K):
        p = rec0[0, j, :13]
        rec[0, j, :13] = JS.pose_step(list(rs.normal(scale=0.01, size=6)), list(p), RF.centre(list(p)))
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    table = joints_table(max_angle_deg=90.0, max_dist=10.0)
    S = hand_sums(rs, K, b_scale=1e-3)
    run = lambda tab=table, sums=S, kin_=kin, rt=tables[0], nfv=float(nf[0]), poses_=rec[0, :, :13], p=0, last=False, st=None, ob=None: \
        JS.joint_step(kin_, scene[0], rt, nfv, tab, p, last, poses_, sums, poses_, np.full((K, 18), np.nan) if st is None else st,
                      np.zeros(8) if ob is None else ob)
    ob = np.zeros(8)
    xi, out, best, J = run(ob=ob)
    H, g = JS.system(J, S, [True] * K, list(S[:, 28]), K, table, table[16] ** 2 * S[:, 28].mean())
    want = np.linalg.solve(np.array(H), -np.array(g))
    assert ob[6] == 1 and ob[5] == 2 and np.abs(xi[:6 * K] - want).max() <= 1e-10 * np.abs(want).max() and (xi[6 * K:] == 0).all()
    assert np.array(H).tobytes() == np.array(H).T.tobytes()
    for j in range(K):                                                   # the update is the pass's, part by part
        assert out[j].tobytes() == np.array(JS.pose_step(list(xi[6 * j:6 * j + 6]), list(rec[0, j, :13]), RF.centre(list(rec[0, j, :13])))).tobytes()
    # the clamp: one factor for the object, from the part whose step is largest against its limit
    tight = joints_table(max_angle_deg=np.degrees(np.linalg.norm(xi[6:9])) / 2, max_dist=10.0)
    x2 = run(tab=tight)[0]
    ratios = [np.linalg.norm(x2[6 * j:6 * j + 3]) / tight[4] for j in range(K)]
    assert max(ratios) <= 1 + 4 * EPS and abs(max(ratios) - 1) <= 4 * EPS or max(ratios) < 1
    assert np.abs(x2[:6 * K] / xi[:6 * K] - (x2[0] / xi[0])).max() <= 1e-12 and x2[0] / xi[0] < 1
    # is_last: nothing is solved, the object is still scored
    ob2 = ob.copy()
    x3, out3, _, _ = run(p=1, last=True, ob=ob2, st=np.zeros((K, 18)))
    assert (x3 == 0).all() and out3.tobytes() == rec[0, :, :13].tobytes() and ob2[6] == 0 and ob2[4] == ob[4] and ob2[3] == ob[3] + 1      # (sums[31] = 1)
    # all-zero sums: H = 1e-12 I + the joints' rows is still positive definite -- the solve runs; a non-finite sum fails it
    Z = np.zeros_like(S)
    Z[:, 28:30] = S[:, 28:30]
    obz = np.zeros(8)
    assert run(sums=Z, ob=obz) and obz[6] == 1
    N = S.copy()
    N[1, 3] = np.inf
    obn = np.zeros(8)
    xn, outn, _, _ = run(sums=N, ob=obn)
    assert obn[6] == 0 and (xn == 0).all() and outn.tobytes() == rec[0, :, :13].tobytes() and obn[3] == 1
    # a part below min_pixels: its block counts as 0, and it still moves with its joint
    few = S.copy()
    few[1, 28] = 5.0
    obf = np.zeros(8)
    xf = run(sums=few, ob=obf)[0]
    assert obf[6] == 1 and np.abs(xf[6:12]).max() > 0
    assert run(sums=np.where(np.arange(32) == 28, 5.0, S))[0].tolist() == [0.0] * 48                      # no part solves on its own: no nbar
    # a NaN pose: its joints are not active, the part reads NaN; a zero norm factor: nothing is live
    bad = rec[0, :, :13].copy()
    bad[2, 4] = np.nan
    obb = np.zeros(8)
    xb, outb, bestb, Jb = run(poses_=bad, ob=obb)
    assert [jt["l"] for jt in Jb] == [1] and obb[5] == 1 and np.isnan(bestb[2]).all() and np.isfinite(bestb[:2]).all() and (xb[12:18] == 0).all()
    assert np.array_equal(outb[2], bad[2], equal_nan=True)
    obz = np.zeros(8)
    xz, outz, bestz, Jz = run(nfv=0.0, ob=obz)
    assert Jz == [] and np.isnan(bestz).all() and np.isnan(obz[[0, 1, 4, 7]]).all() and obz[5] == 0 and (xz == 0).all()
    # an instance or a parent outside its range makes no joint (depth.check_kinematics refuses such a table on the host)
    rt = tables[0].copy()
    rt[9] = 1.0
    assert run(rt=rt)[3] == [] and len(run(rt=rt, kin_=np.stack([kin, kin]))[3]) == 2
    for value in (3.0, 5.0, -1.0, 0.5, np.nan):
        k2 = kin.copy()
        k2[32 + 40 * 3 + 2] = value
        assert [jt["l"] for jt in run(kin_=k2)[3]] == [1], value
    from articulated_pose_amd.depth import check_kinematics
    k2 = kin.copy()
    k2[32 + 40 * 3 + 2] = 3.0
    with pytest.raises(ValueError, match="kinematics"):
        check_kinematics(k2, K)
    # K = 1: no joint, no solve, the best-of still runs
    one = run(poses_=rec[0, :1, :13], sums=S[:1], st=np.full((1, 18), np.nan))
    assert one[3] == [] and (one[0] == 0).all() and one[2][0, :13].tobytes() == rec[0, 0, :13].tobytes()


# ---- the behavioural bars, by the mirror alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
def test_behavioural_bars_inputs(K):
    """The GPU tests' two bars met by the mirrors alone (the plain loop: refinement_mirror; with joints: joint_step_mirror), uint16 frames.
    (a) with every part perturbed differently the kept poses' hinge gap is lower with joints= than without, on every frame and pose;
    (b) with min_pixels above the wedge part's pixel count the plain loop keeps its pose, the joint step moves it and closes the gap."""
    dtype = "uint16"
    prob, rec, split = joint_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = joints_table()
    plain = RF.refine(mesh, render, scene, rigs, nf, split, geom, frames, dtype, table[:8])[0]
    cols, obj, poses_, sums = JS.refine(mesh, kin, render, scene, rigs, nf, split, geom, frames, table)
    g_plain, g_joint = kept_gaps(prob, plain, K), kept_gaps(prob, cols, K)
    start = kept_gaps(prob, as_columns(split), K)
    print("hinge gap at the start", start.ravel(), "\nplain loop", g_plain.ravel(), "\nwith joints", g_joint.ravel())
    assert (start > 1e-3).all() and (obj[:, :, :, 5] == 1).all() and (obj[:3, :, :, 6] == 1).all() and (obj[-1, :, :, 1] <= obj[-1, :, :, 0]).all()
    assert (g_joint < g_plain).all(), (g_joint, g_plain)
    # (b)
    j, min_pixels, split = small_part_problem(prob, rec, split, K)
    start = kept_gaps(prob, as_columns(split), K)
    t2 = joints_table(min_pixels=min_pixels)
    plain2 = RF.refine(mesh, render, scene, rigs, nf, split, geom, frames, dtype, t2[:8])[0].reshape(3, K, 2, 18)
    assert (plain2[:, j, :, 16] == 0).all() and plain2[:, j, :, :13].tobytes() == split[:, j].reshape(3, 2, 13).tobytes()
    assert (plain2[:, 0, :, 17] >= 1).all()                             # the base still solves on its own: there is an nbar
    cols2, obj2, _, _ = JS.refine(mesh, kin, render, scene, rigs, nf, split, geom, frames, t2)
    b2 = cols2.reshape(3, K, 2, 18)
    g2 = kept_gaps(prob, cols2, K)
    print("min_pixels", min_pixels, "gap at the start", start.ravel(), "with joints", g2.ravel())
    assert (start > 1e-3).all() and (b2[:, j, :, :13] != split[:, j].reshape(3, 2, 13)).any(axis=2).all() and (g2 < start).all(), (g2, start)
