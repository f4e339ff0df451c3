"""CPU (no GPU): the streamed joint values.  The mirror (tests/joint_values_mirror.py) validated on its own -- on exact posed records the
closed form returns the submitted q whatever the tree, a record posed at q + delta reads delta, a scaled part reads its scale, the wrap, the
row choice and the NaN rules --, the entry's place in the ABI and its refusals before any launch, the option's rule in check_options and the
column names.  The problems here are shared with the GPU tests."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import joint_values_mirror as JV
import pose_scene_mirror as PM
import reprojection_mirror as RP
from test_pose_scene_cpu import kin_table
from test_refine_joints_cpu import P16, TREES, chain_problem
from test_render_cpu import box_mesh, object_scene
from test_reprojection_cpu import LINKS, TREE, poses, posed_object, random_rigs

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12            # the issue's bar on exact records: the prototype measured at most 5e-16; room for another order of operations
BRIDGES = {"K2-revolute-two-link-part": {1: (1, 1.0, 0)}, "K3-revolute": {2: (1, 1.0, 0)}, "K2-prismatic": {1: (3, 2.0, 0)},
           "K3-both-two-link-part": {1: (1, 1.0, 0), 2: (3, 2.0, 0)}}      # part -> (link, kind, parent's part)


def tree_poses(K, maps, seed=5, change=None):
    """tree_problem's three frames with their pose table: the same draws in the same order.  change(pose table) edits the joint values before
    the tables are built.  -> (kin, pose (3, 32), render, scene, rigs, nf, the exact record)."""
    rs = np.random.RandomState(seed + 10 * K)
    S = object_scene(rs, 3)
    xyz, rpy = rs.uniform(-0.1, 0.1, (LINKS, 3)), rs.uniform(-0.5, 0.5, (LINKS, 3))
    xyz[2], rpy[2] = xyz[1], rpy[1]
    S = dict(S, link_xyz=xyz, link_rpy=rpy, joint_xyz=rs.uniform(-0.1, 0.1, (LINKS - 1, 3)))
    kin = kin_table(S, TREE, maps, depth_scale=1e-3)
    ps = poses(rs, 3)
    if change is not None:
        change(ps)
    render, scene = PM.build_tables(kin, ps)
    rigs, nf = random_rigs(rs, 3, K, False), rs.uniform(0.7, 1.3, 3).astype(np.float32)
    return kin, ps, render, scene, rigs, nf, RP.exact_record(render, scene, rigs, nf, kin, K)


def chain_poses(nlinks=8, n=2, seed=9):
    """chain_problem's pose table, rebuilt the way chain_problem builds it (the same draws in the same order).  -> (n, 32)."""
    from articulated_pose_amd.depth import pack_pose
    from test_depth_annotate_cpu import euler_sxyz
    rs = np.random.RandomState(seed)
    object_scene(rs, 3)
    for shape in ((nlinks, 3), (nlinks, 3), (nlinks - 1, 3)):
        rs.uniform(-0.1, 0.1, shape)
    rs.normal(size=(nlinks, 3))
    rs.uniform(-0.15, 0.15, (nlinks - 1, 3))
    rs.uniform(-0.6, 0.6, (nlinks - 1, 3))
    ps = []
    for _ in range(n):
        V = euler_sxyz(*rs.uniform(-0.25, 0.25, 3))
        V[:3, 3] = (rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), -rs.uniform(1.45, 1.6))
        ps.append(pack_pose([0.0] + [rs.uniform(0.2, 0.8) if l % 2 == 0 else rs.uniform(-0.05, 0.05) for l in range(nlinks - 1)], V))
    return np.stack(ps)


def problems():
    """name -> (K, kin, pose, render, scene, rigs, nf, exact record): the four trees (3 frames), the chain (2 frames x 8 parts) and a
    two-instance library mixing two trees of K = 3 (frame 1 is instance 1's)."""
    out = {}
    for name, (K, maps) in TREES.items():
        out[name] = (K,) + tree_poses(K, maps)
    kin, render, scene, rigs, nf, _, _, rec = chain_problem()
    ps = chain_poses()
    r2, s2 = PM.build_tables(kin, ps)
    assert r2.tobytes() == render.tobytes() and s2.tobytes() == scene.tobytes()      # the pose table IS chain_problem's
    out["chain"] = (8, kin, ps, render, scene, rigs, nf, rec)
    a, b = out["K3-revolute"], out["K3-both-two-link-part"]
    pick = lambda k: np.stack([a[k][0], b[k][1], a[k][2]])
    ps, render = pick(2).copy(), pick(3).copy()
    ps[1, 28] = render[1, 9] = 1.0
    out["library"] = (3, np.stack([a[1], b[1]]), ps, render, pick(4), pick(5), pick(6), pick(7))
    return out


def art_block(rs, n, K, ld):
    """An articulation block of arbitrary numbers with NaNs of two payloads in it."""
    art = rs.normal(size=(n, K, ld))
    art[0, 0, 6:12] = np.nan
    art.view(np.uint64)[-1, -1, 3] = 0x7ff8000000abcdef
    return art


def tail(wide):
    return wide[:, :, wide.shape[2] - 24:]


def group(wide, g):
    return tail(wide)[:, :, 4 + 5 * g:9 + 5 * g]


# ---- the mirror on its own ---------------------------------------------------------------------------------------------------------------------
PROBLEMS = {}


def problem(name):
    if not PROBLEMS:
        PROBLEMS.update(problems())
    return PROBLEMS[name]


@pytest.mark.parametrize("name", list(TREES) + ["chain", "library"])
def test_exact_records_return_the_submitted_joint_values(name):
    K, kin, ps, render, scene, rigs, nf, rec = problem(name)
    n = len(rec)
    art = art_block(np.random.RandomState(0), n, K, 12)
    refined = np.concatenate([rec.reshape(n, K, 2, 13), np.zeros((n, K, 2, 5))], 3)
    wide = JV.joint_values(kin, render, scene, rigs, nf, rec, art, pose=ps, refined=refined)
    assert wide.shape == (n, K, 36) and wide[:, :, :12].tobytes() == art.tobytes()
    t = tail(wide)
    reported = np.isfinite(t[:, :, 0])
    worst = np.zeros(4)
    for f, j in np.ndindex(n, K):
        want = None
        if name == "chain":
            want = (j, 1.0 if j % 2 else 2.0, j - 1) if j else None
        elif name == "library":
            want = BRIDGES["K3-both-two-link-part" if f == 1 else "K3-revolute"].get(j)
        else:
            want = BRIDGES[name].get(j)
        if want is None:
            assert np.isnan(t[f, j]).all(), (name, f, j, t[f, j])
            continue
        l, kind, b = want
        assert t[f, j, :4].tolist() == [l, kind, b, ps[f, l]], (name, f, j, t[f, j, :4])
        for g in range(4):
            q, err, off, gap, ratio = group(wide, g)[f, j]
            worst = np.maximum(worst, [abs(q - ps[f, l]), off, gap, abs(ratio - 1.0)])
            assert abs(q - ps[f, l]) <= TOL and abs(err) <= TOL and 0.0 <= off <= TOL and 0.0 <= gap <= TOL and abs(ratio - 1.0) <= TOL, (name, f, j, g)
    assert reported.any()
    print(name, "worst |q - q_true|, off_axis, gap, |scale_ratio - 1|:", worst)


@pytest.mark.parametrize("name,link,delta", [("K3-revolute", 1, 0.1), ("K3-both-two-link-part", 1, 0.1), ("K2-prismatic", 3, 0.02),
                                             ("K3-both-two-link-part", 3, 0.02)])
def test_a_record_posed_at_q_plus_delta_reads_delta(name, link, delta):
    K, maps = TREES[name]
    kin, ps, render, scene, rigs, nf, rec = tree_poses(K, maps)

    def change(p):
        p[:, link] += delta
    moved = tree_poses(K, maps, change=change)
    assert moved[0].tobytes() == kin.tobytes() and moved[4].tobytes() == rigs.tobytes() and moved[5].tobytes() == nf.tobytes()
    wide = JV.joint_values(kin, render, scene, rigs, nf, moved[6], np.zeros((3, K, 12)), pose=ps)
    j = [j for j, (l, _, _) in BRIDGES[name].items() if l == link][0]
    for g in range(2):
        q, err, off, gap, ratio = group(wide, g)[:, j].T
        assert (np.abs(err - delta) <= TOL).all() and (np.abs(q - (ps[:, link] + delta)) <= TOL).all() and (off <= TOL).all() and (gap <= TOL).all()
        assert (np.abs(ratio - 1.0) <= TOL).all()
    assert np.isnan(group(wide, 2)).all() and np.isnan(group(wide, 3)).all()


@pytest.mark.parametrize("name", ["K3-revolute", "K2-prismatic"])
def test_a_scaled_child_part_reads_its_scale(name):
    K, kin, ps, render, scene, rigs, nf, rec = problem(name)
    (j, (l, kind, b)), = BRIDGES[name].items()
    scaled = rec.copy()
    scaled[:, j, [9, 22]] *= 1.1
    wide = JV.joint_values(kin, render, scene, rigs, nf, scaled, np.zeros((3, K, 12)), pose=ps)
    for g in range(2):
        assert (np.abs(group(wide, g)[:, j, 4] - 1.1) <= TOL).all(), group(wide, g)[:, j, 4]
        if kind == 1.0:                                                  # the rotation does not see the scale
            assert (np.abs(group(wide, g)[:, j, 1]) <= TOL).all() and (group(wide, g)[:, j, 2] <= TOL).all()


def test_a_revolute_error_wraps_once():
    K, maps = TREES["K3-revolute"]

    def change(p):
        p[:, 1] = -3.1
    kin, ps, render, scene, rigs, nf, rec = tree_poses(K, maps, change=change)
    said = ps.copy()
    said[:, 1] = 3.1
    wide = JV.joint_values(kin, render, scene, rigs, nf, rec, np.zeros((3, K, 12)), pose=said)
    for g in range(2):
        q, err = group(wide, g)[:, 2, 0], group(wide, g)[:, 2, 1]
        assert (np.abs(q + 3.1) <= TOL).all() and (np.abs(err - (2 * math.pi - 6.2)) <= TOL).all(), (q, err)
    assert (tail(wide)[:, 2, 3] == 3.1).all()


def test_a_part_of_two_bridging_links_reports_the_lower_one():
    maps = [[0], [1, 3]]                                                 # part 1 owns the revolute link 1 and the prismatic link 3, both on link 0
    kin, ps, render, scene, rigs, nf, rec = tree_poses(2, maps)
    wide = JV.joint_values(kin, render, scene, rigs, nf, rec, np.zeros((3, 2, 12)), pose=ps)
    assert (tail(wide)[:, 1, :3] == [1.0, 1.0, 0.0]).all() and np.isnan(tail(wide)[:, 0]).all()
    assert (np.abs(group(wide, 0)[:, 1, 1]) <= TOL).all()               # the record follows the part's link of lowest rank: link 1
    maps = [[0, 1], [2, 3]]                                              # part 1's lower link 2 is fixed: the row reports link 3
    kin, ps, render, scene, rigs, nf, rec = tree_poses(2, maps)
    wide = JV.joint_values(kin, render, scene, rigs, nf, rec, np.zeros((3, 2, 12)), pose=ps)
    assert (tail(wide)[:, 1, :3] == [3.0, 2.0, 0.0]).all() and np.isnan(tail(wide)[:, 0]).all()


def special_cases():
    """name -> (arguments of the entry as a dict, a check of the mirror's result): the NaN rules, each on a problem of its own."""
    K, kin, ps, render, scene, rigs, nf, rec = problem("K3-both-two-link-part")
    n = 3
    refined = np.concatenate([rec.reshape(n, K, 2, 13), np.ones((n, K, 2, 5))], 3)
    base = dict(kin=kin, render=render, scene=scene, rig=rigs, norm_factor=nf, record=rec, art=np.zeros((n, K, 12)), pose=ps, refined=refined)
    nanrows = lambda w, f, rows: np.isnan(tail(w)[f, rows]).all()
    cases = {}
    cases["base-row"] = (base, lambda w: nanrows(w, slice(None), 0) and np.isfinite(tail(w)[:, 1:]).all())
    cK, ckin, cps, crender, cscene, crigs, cnf, crec = problem("chain")
    gone = cscene.copy()
    gone[:, RP.SCENE_HEAD + RP.SCENE_LINK * 3 + 1] = -1.0                # link 3 belongs to no part: rows 3 (no link) and 4 (its parent has no part)
    chain = dict(kin=ckin, render=crender, scene=gone, rig=crigs, norm_factor=cnf, record=crec, art=np.zeros((2, 8, 20)), pose=cps, refined=None)
    cases["link-of-no-part"] = (chain, lambda w: all(nanrows(w, slice(None), r) for r in (0, 3, 4)) and np.isfinite(tail(w)[:, [1, 2, 5, 6, 7], :14]).all())
    child = rec.copy()
    child[0, 1, 4] = np.nan                                              # frame 0: part 1's baseline pose; frame 1: its nonlinear scale is infinite
    child[1, 1, 13 + 9] = np.inf
    cases["nan-child-pose"] = (dict(base, record=child), lambda w: np.isnan(group(w, 0)[0, 1]).all() and np.isfinite(group(w, 1)[0, 1]).all()
                               and np.isnan(group(w, 1)[1, 1]).all() and np.isfinite(group(w, 0)[1, 1]).all() and np.isfinite(tail(w)[:, 1:, :4]).all()
                               and np.isfinite(group(w, 0)[0, 2]).all() and np.isfinite(group(w, 2)[:, 1:]).all())
    parent = rec.copy()
    parent[2, 0, 13:26] = np.nan                                         # frame 2: the base's nonlinear pose: both children lose that group
    ref2 = refined.copy()
    ref2[1, 0, 0, 3] = np.nan                                            # frame 1: the base's kept baseline pose
    cases["nan-parent-pose"] = (dict(base, record=parent, refined=ref2),
                                lambda w: np.isnan(group(w, 1)[2, 1:]).all() and np.isfinite(group(w, 0)[2, 1:]).all() and np.isnan(group(w, 2)[1, 1:]).all()
                                and np.isfinite(group(w, 3)[1, 1:]).all() and np.isfinite(tail(w)[:, 1:, :4]).all())
    nf0 = nf.copy()
    nf0[0], nf0[2] = 0.0, np.inf
    cases["nf-zero"] = (dict(base, norm_factor=nf0), lambda w: np.isnan(tail(w)[[0, 2]]).all() and np.isfinite(tail(w)[1, 1:]).all())
    r9 = render.copy()
    r9[0, 9], r9[1, 9] = 2.0, 0.5
    cases["instance-out-of-range"] = (dict(base, render=r9), lambda w: np.isnan(tail(w)[:2]).all() and np.isfinite(tail(w)[2, 1:]).all())
    cases["refined-none"] = (dict(base, refined=None), lambda w: np.isnan(tail(w)[:, :, 14:]).all() and np.isfinite(tail(w)[:, 1:, :14]).all())
    cases["pose-none"] = (dict(base, pose=None), lambda w: np.isnan(tail(w)[:, :, 3]).all() and np.isnan(tail(w)[:, :, 5::5]).all()
                          and np.isfinite(tail(w)[:, 1:, [0, 1, 2, 4, 6, 7, 8]]).all())
    for value in (3.0, -1.0, 0.5, np.nan, 1e300):                        # a parent out of range (depth.check_kinematics refuses such a table on the host)
        k2 = kin.copy()
        k2[32 + 40 * 3 + 2] = value
        cases["parent=%r" % value] = (dict(base, kin=k2), lambda w: nanrows(w, slice(None), 2) and np.isfinite(tail(w)[:, 1]).all())
    k2 = kin.copy()
    k2[32 + 40 * 1 + 3] = 0.0                                            # part 1's links are both fixed now
    cases["all-joints-fixed"] = (dict(base, kin=k2), lambda w: nanrows(w, slice(None), 1) and np.isfinite(tail(w)[:, 2]).all())
    flat = rec.copy()
    flat[0, 1, 9] = 0.0                                                  # a zero scale: sigma_l = 0
    cases["zero-scale"] = (dict(base, record=flat), lambda w: np.isnan(group(w, 0)[0, 1]).all() and np.isfinite(group(w, 1)[0, 1]).all()
                           and np.isfinite(tail(w)[0, 1, :4]).all())
    return cases


@pytest.mark.parametrize("case", ["base-row", "link-of-no-part", "nan-child-pose", "nan-parent-pose", "nf-zero", "instance-out-of-range", "refined-none",
                                  "pose-none", "parent=3.0", "parent=-1.0", "parent=0.5", "parent=nan", "parent=1e+300", "all-joints-fixed",
                                  "zero-scale"])
def test_nan_pattern_follows_the_rules(case):
    args, check = special_cases()[case]
    wide = JV.joint_values(**args)
    assert check(wide), (case, tail(wide))
    ld = args["art"].shape[2]
    assert wide.shape[2] == ld + 24 and wide[:, :, :ld].tobytes() == args["art"].tobytes()


# ---- the entry, before any launch ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    name = "ancsh_joint_values_rec"
    assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 17
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_JOINT_VALUES_WIDTH 24\n" in header


def test_entry_refuses_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device; an accepted call here has nframes == 0, which launches nothing -- after all the checks."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    ptrs = ("kin", "pose", "render", "scene", "rig", "nf", "record", "refined", "art", "wide")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, ninst=1, rig_ld=22 + 3 * 42, ld=26, art_ld=12, wide=ctypes.c_void_p(32))
    order = ("n", "K", "kin", "ninst", "pose", "render", "scene", "rig", "rig_ld", "nf", "record", "ld", "refined", "art", "art_ld", "wide")
    run = lambda **over: L.ancsh_joint_values_rec(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(K=8, rig_ld=22 + 8 * 87, ninst=4096, ld=77, art_ld=20, pose=None, refined=None) == 0 and run(K=1, rig_ld=22 + 24) == 0
    odd = lambda a: ctypes.c_void_p(a)
    # every refusal in its order: each call is wrong in everything behind the argument it names, too
    wrong = dict(n=-1, K=0, ninst=0, rig_ld=1, ld=25, art_ld=13, kin=None, nf=odd(18), wide=P16)
    steps = ((dict(n=-1), b"nframes=-1"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(ninst=0), b"ninst=0"),
             (dict(ninst=-3), b"ninst=-3"), (dict(rig_ld=147), b"rig_ld=147"), (dict(ld=25), b"ld=25"), (dict(art_ld=13), b"art_ld=13"),
             (dict(art_ld=0), b"art_ld=0"), (dict(art_ld=44), b"art_ld=44"), (dict(kin=None), b"null pointer"), (dict(nf=odd(18)), b"aligned"),
             (dict(wide=P16), b"overlap"))
    names = list(wrong)
    for over, what in steps:
        first = names.index(list(over)[0])
        later = {k: wrong[k] for k in names[first + 1:]}
        if "K" in later:
            later.pop("K")                                               # n and K share one check
        assert run(**dict(later, **over)) == -1 and what in L.ancsh_last_error() and b"joint_values_rec" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs:
        if k != "nf":
            assert run(**{k: odd(20)}) == -1 and b"aligned" in L.ancsh_last_error(), k
        if k not in ("pose", "refined"):
            assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k


# ---- the option ------------------------------------------------------------------------------------------------------------------------------
def test_the_option_needs_kinematics_and_articulation_and_widens_the_block():
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.record import BLOCKS
    from articulated_pose_amd.stream import OPTION_FLAGS, RESULT_NAMES, RESULT_ORDER, Options, check_options
    assert Options._fields[-4:] == ("refine_coverage", "refine_joints", "silhouette", "refine")
    assert Options._fields[Options._fields.index("art_width") - 1] == "joint_values" and "joint_values" not in OPTION_FLAGS
    assert not any("joint_value" in n for n in RESULT_NAMES + tuple(RESULT_ORDER)) and not any("joint_value" in str(b) for b in BLOCKS)
    annotated = dict(depth_capacity=4096, joint_source="predicted", point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    for states, widths in ((False, (12, 36)), (True, (20, 44))):
        off = check_options(batch_size=2, render_mesh=mesh, kinematics=kin, articulation=True, joint_states=states, **annotated)
        on = check_options(batch_size=2, render_mesh=mesh, kinematics=kin, articulation=True, joint_states=states, joint_values=True, **annotated)
        assert (off.art_width, on.art_width) == widths and off.joint_values is False and on.joint_values is True
        assert on._replace(joint_values=False, art_width=off.art_width) == off and on.record_width == off.record_width
    with pytest.raises(ValueError, match=r"joint_values=True .* needs kinematics=<depth.pack_kinematics\(\.\.\.\)>$"):
        check_options(batch_size=2, render_mesh=mesh, articulation=True, joint_values=True, **annotated)
    with pytest.raises(ValueError, match=r"joint_values=True .* needs articulation=True$"):
        check_options(batch_size=2, render_mesh=mesh, kinematics=kin, joint_values=True, **annotated)
    with pytest.raises(ValueError, match=r"joint_values=True .* needs kinematics=<depth.pack_kinematics\(\.\.\.\)>, articulation=True$"):
        check_options(batch_size=2, joint_values=True)
    from articulated_pose_amd.pose.joint_values import check_joint_values
    assert check_joint_values(False, False, False) is False and check_joint_values(1, True, True) is True
    with pytest.raises(ValueError, match="joint_values=True"):
        AncshPipeline(3, None, None, 2, 64, "cpu", render_mesh=mesh, articulation=True, joint_values=True, **annotated)
    with pytest.raises(ValueError, match="ShardedPipeline .* joint_values=True .* kinematics="):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, joint_values=True)


def test_column_names_and_the_summary():
    from articulated_pose_amd.pose import joint_values as M
    assert M.JOINT_VALUES_WIDTH == JV.WIDTH == 24 and len(M.COLUMN_NAMES) == 24 and len(set(M.COLUMN_NAMES)) == 24
    assert M.COLUMN_NAMES[:4] == ("link", "kind", "parent_part", "q_true") and M.COLUMN_NAMES[4:9] == ("baseline_q", "baseline_q_err", "baseline_off_axis",
                                                                                                       "baseline_gap", "baseline_scale_ratio")
    assert [n.rsplit("_q_err", 1)[0] for n in M.COLUMN_NAMES if n.endswith("_q_err")] == ["baseline", "nonlinear", "refined_baseline", "refined_nonlinear"]
    K, kin, ps, render, scene, rigs, nf, rec = problem("K3-both-two-link-part")
    said = ps.copy()
    said[:, 1] -= np.radians([1.0, 2.0, 6.0])                            # the record sits 1, 2 and 6 degrees behind ... and 0.01 .. 0.03 units along
    said[:, 3] -= [0.01, 0.02, 0.03]
    wide = JV.joint_values(kin, render, scene, rigs, nf, rec, np.zeros((3, K, 20)), pose=said)
    cols = M.named_columns(wide)
    assert set(cols) == set(M.COLUMN_NAMES) and cols["link"].shape == (3, K) and np.array_equal(cols["nonlinear_q"], wide[:, :, 20 + 9], equal_nan=True)
    with pytest.raises(ValueError, match="at least 24"):
        M.named_columns(wide[:, :, :23])
    lines = M.joint_value_table(wide, K)
    assert len(lines) == 1 + K and lines[1].split()[:3] == ["0", "-", "-"] and lines[1].split()[3] == "0"
    one, two = lines[2].split(), lines[3].split()
    assert one[:4] == ["1", "1", "revolute", "3"] and two[:4] == ["2", "3", "prismatic", "3"]
    assert abs(float(one[4]) - 3.0) < 1e-9 and abs(float(one[6]) - 2.0) < 1e-9 and one[7] == "deg" and "-" in one[8:]
    assert abs(float(two[4]) - 0.02) < 1e-9 and abs(float(two[6]) - 0.02) < 1e-9 and two[7] == "len"
    assert M.joint_value_table([wide[:1], wide[1:]], K) == lines
