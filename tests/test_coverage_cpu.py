"""CPU (no GPU): the coverage term of render-and-compare ICP.  Its two entries' place in the ABI and their argument checks before any launch,
the joint step's wider sums, pack_refine(coverage=...) and the option flag, and the mirror (tests/coverage_mirror.py) validated on its own:
the gap rows' rules on hand-made frames where every number can be said in advance, the sums against silhouette_mirror's where no gap pixel
exists, and the behavioural bars -- on test_silhouette_cpu's lateral-shift frames no triple ends further from the truth than it started, which
the silhouette term alone does not achieve, and test_refinement_cpu's perturbation still ends strictly lower for every part."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coverage_mirror as CM
import refinement_mirror as RF
import silhouette_mirror as SM
from test_refinement_cpu import MAX_DIST, behavioural_bars, mirror, refine_table
from test_reprojection_cpu import posed_object
from test_render_cpu import box_mesh
from test_silhouette_cpu import CASES, IDS, P16, lateral_bar, problem, refined, sil_mirror, silhouette_table

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = (("ancsh_coverage_field", 10), ("ancsh_refine_pass_cov", 29))
COVERAGE = dict(weight=1.0, dist=0.1, slack=0.0)                          # the issue's values: the silhouette term's own, for its other side
PERTURBED = [(2, "uint16", False), (2, "float32", False), (3, "uint16", False), (3, "float32", False), (3, "uint16", True)]
PERTURBED_IDS = ["K2-uint16", "K2-float32", "K3-uint16", "K3-float32", "K3-sapien-rotation"]


def coverage_table(**over):
    """test_silhouette_cpu's table with the coverage term (shared with the GPU tests)."""
    return silhouette_table(**dict(dict(coverage=COVERAGE), **over))


def cov_mirror(prob, rec, dtype, table):
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    return CM.refine(mesh, render, scene, rigs, nf, rec, geom, frames, dtype, table)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose import refinement as R
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name, nargs in NAMES:
        assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.lib().ancsh_abi_version() == 14 and len(_lib.SIGNATURES["ancsh_refine_pass_sil"]) == 28
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_REFINE_COV_SUMS 40\n" in header and "#define ANCSH_REFINE_COV_PARAMS 32\n" in header
    assert R.REFINE_COV_SUMS == CM.SUMS == 40 and R.REFINE_COV_PARAMS == CM.PARAMS == 32
    assert R.COV_SUMS_COLUMNS["mm_c"] == 36 and R.COV_SUMS_COLUMNS["n_cov"] == 37 and R.COV_SUMS_COLUMNS["n_cfar"] == 38
    assert R.PARAMS_LENGTHS["ancsh_refine_pass_cov"] == (32,) and 32 in R.PARAMS_LENGTHS["ancsh_refine_joint_step"]
    assert R.PARAMS_LENGTHS["ancsh_refine_pass"] == (8, 24) and R.PARAMS_LENGTHS["ancsh_refine_pass_sil"] == (16, 24)
    assert R.RefineBuffers._fields == ("work", "best", "sums", "field", "state", "obj", "xi", "cover")


def test_entries_refuse_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device (no pointer is read on the host); an accepted call here has nframes == 0, which launches
    nothing -- after all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    odd = lambda a: ctypes.c_void_p(a)
    ptrs = ("verts", "tris", "tri_link", "od", "ol", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params", "field", "cover", "pin", "pout", "best",
            "sums")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, kind=0, V=10, T=12, cap=4096, p=0, last=0, ld=26, pout=ctypes.c_void_p(32))
    order = ("n", "K", "kind", "verts", "tris", "tri_link", "V", "T", "od", "ol", "cap", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params",
             "field", "cover", "p", "last", "pin", "ld", "pout", "best", "sums")
    run = lambda **over: L.ancsh_refine_pass_cov(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(kind=1, p=8, last=1, ld=77, K=8, V=0, T=0) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(kind=-1), b"depth_type=-1"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"),
                       (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T="), (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V="), (dict(p=-1), b"pass=-1"),
                       (dict(p=9), b"pass=9"), (dict(last=2), b"is_last=2"), (dict(ld=25), b"ld_in=25"), (dict(od=odd(17)), b"aligned"),
                       (dict(kind=1, pd=odd(18)), b"aligned"), (dict(verts=odd(18)), b"aligned"), (dict(tris=odd(18)), b"aligned"),
                       (dict(tri_link=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(nf=odd(18)), b"aligned"),
                       (dict(field=odd(18)), b"aligned"), (dict(cover=odd(18)), b"aligned"), (dict(zb=odd(20)), b"aligned"),
                       (dict(scene=odd(20)), b"aligned"), (dict(rt=odd(20)), b"aligned"), (dict(params=odd(20)), b"aligned"),
                       (dict(pin=odd(20)), b"aligned"), (dict(pout=odd(20)), b"aligned"), (dict(best=odd(20)), b"aligned"),
                       (dict(sums=odd(20)), b"aligned"), (dict(pout=P16), b"overlap")):
        assert run(**over) == -1 and what in L.ancsh_last_error() and b"refine_pass_cov" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs:
        assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    good = dict(n=0, K=3, kind=0, pd=P16, pl=P16, cap=4096, geom=P16, scene=P16, cover=P16)
    order = ("n", "K", "kind", "pd", "pl", "cap", "geom", "scene", "cover")
    fld = lambda **over: L.ancsh_coverage_field(*[dict(good, **over)[k] for k in order], None)
    assert fld() == 0 and fld(K=8, kind=1, cap=0) == 0 and fld(K=1, pl=odd(17)) == 0 and fld(cap=(1 << 29) - 1) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"), (dict(pd=odd(17)), b"aligned"),
                       (dict(kind=1, pd=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(cover=odd(18)), b"aligned"),
                       (dict(scene=odd(20)), b"aligned")):
        assert fld(**over) == -1 and what in L.ancsh_last_error() and b"coverage_field" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ("pd", "pl", "geom", "scene", "cover"):
        assert fld(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    # the joint step: sums of 40 values are its third width; 33 is still none
    step = lambda sld: L.ancsh_refine_joint_step(0, 3, P16, 1, P16, P16, P16, P16, 0, 0, P16, 26, P16, sld, ctypes.c_void_p(32), P16,
                                                 ctypes.c_void_p(48), P16, None, None)
    assert step(32) == 0 and step(36) == 0 and step(40) == 0
    for sld in (33, 39, 41, 44):
        assert step(sld) == -1 and b"sums_ld=%d" % sld in L.ancsh_last_error() and b"ancsh_refine_pass_cov" in L.ancsh_last_error()


# ---- the table and the option ----------------------------------------------------------------------------------------------------------------
def test_pack_refine_lays_out_the_32_value_table_and_leaves_the_shorter_ones_alone():
    from articulated_pose_amd.pose import refinement as R
    head = dict(iters=5, max_dist=0.02)
    plain, sil = R.pack_refine(**head), R.pack_refine(silhouette=dict(weight=2.0, dist=0.05, slack=0.5), **head)
    jt, both = R.pack_refine(joints=(2.0, 0.25), **head), R.pack_refine(silhouette=(1.5, 0.1), joints=(2.0, 0.25), **head)
    # the shorter tables' bytes, written out: what they were before the term existed
    want_head = [5.0, 0.02, 0.1, 1e-3, float(np.radians(10.0)), 32.0, 0.0, 0.0]
    assert plain.tolist() == want_head and sil.tolist() == want_head + [2.0, 0.05, 0.5, 0, 0, 0, 0, 0]
    assert jt.tolist() == want_head + [0.0] * 8 + [2.0, 0.25, 0, 0, 0, 0, 0, 0] and both.tolist() == want_head + [1.5, 0.1, 1.0, 0, 0, 0, 0, 0] + jt.tolist()[16:]
    for t in (plain, sil, jt, both):
        assert R.pack_refine(coverage=None, **head).tobytes() == plain.tobytes() and not R.has_coverage(t) and R.check_refine_table(t).tobytes() == t.tobytes()
    t = R.pack_refine(silhouette=dict(weight=2.0, dist=0.05, slack=0.5), coverage=dict(weight=3.0, dist=0.07, slack=0.25), **head)
    assert t.shape == (32,) and t.dtype == np.float64 and t[:16].tobytes() == sil.tobytes() and (t[16:24] == 0).all()
    assert t[24:].tolist() == [3.0, 0.07, 0.25, 0, 0, 0, 0, 0] and R.has_coverage(t) and R.has_silhouette(t) and not R.has_joints(t)
    tj = R.pack_refine(silhouette=(1.5, 0.1), joints=(2.0, 0.25), coverage=(3.0, 0.07), **head)
    assert tj.shape == (32,) and tj[:24].tobytes() == both.tobytes() and tj[24:27].tolist() == [3.0, 0.07, 1.0] and (tj[27:] == 0).all()
    assert R.has_joints(tj) and R.has_coverage(tj) and R.has_silhouette(tj) and R.has_joints(jt) and not R.has_joints(sil)
    assert R.pack_refine(silhouette=(1.0, 0.1), coverage=dict(dist=0.2))[24:27].tolist() == [1.0, 0.2, 1.0]
    assert R.check_refine_table(t).tobytes() == t.tobytes() and R.check_refine_table(tj).tobytes() == tj.tobytes()
    with pytest.raises(ValueError, match="refine: coverage needs the silhouette term"):
        R.pack_refine(coverage=dict(dist=0.1))
    with pytest.raises(ValueError, match="refine: coverage needs the silhouette term"):
        R.pack_refine(joints=(1.0, 0.5), coverage=(1.0, 0.1))
    with pytest.raises(ValueError, match="refine: coverage needs the silhouette term"):
        R.check_refine_table(np.r_[plain, np.zeros(16), [1.0, 0.1, 0.0], np.zeros(5)])
    for cov, what in ((dict(weight=0.0, dist=0.1), "coverage weight"), (dict(weight=-1.0, dist=0.1), "coverage weight"),
                      (dict(weight=float("nan"), dist=0.1), "coverage weight"), (dict(dist=0.0), "coverage dist"), (dict(dist=-0.1), "coverage dist"),
                      (dict(dist=float("inf")), "coverage dist"), (dict(dist=0.1, slack=-0.5), "coverage slack"),
                      (dict(dist=0.1, slack=float("nan")), "coverage slack"), (dict(weight=1.0), "coverage takes"),
                      (dict(dist=0.1, reach=2), "coverage takes"), ((1.0, 0.0), "coverage dist"), ((0.0, 0.1), "coverage weight"),
                      (dict(dist="far"), "coverage is"), (5.0, "coverage is")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            R.pack_refine(silhouette=(1.0, 0.1), coverage=cov)
    for at in range(27, 32):
        bad = t.copy()
        bad[at] = 1.0
        with pytest.raises(ValueError, match=r"refine: the reserved values 27\.\.31 must be 0"):
            R.check_refine_table(bad)
    for at, what in ((12, r"11\.\.15"), (19, r"18\.\.23")):                # the shorter tables' reserved values stay refused inside the long one
        bad = tj.copy()
        bad[at] = 1.0
        with pytest.raises(ValueError, match="refine: the reserved values " + what):
            R.check_refine_table(bad)
    bad = t.copy()
    bad[17] = 0.5                                                        # a joint value without a weight
    with pytest.raises(ValueError, match="refine: joints weight"):
        R.check_refine_table(bad)
    for shape in ((31,), (33,), (40,), (2, 32)):
        with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table"):
            R.check_refine_table(np.zeros(shape))
    with pytest.raises(ValueError, match="coverage=True.*silhouette=True"):
        R.refine_buffers(2, 3, "cpu", coverage=True, pixel_capacity=64)
    bufs = R.refine_buffers(2, 3, "cpu", silhouette=True, coverage=True, pixel_capacity=64)
    assert bufs.cover.shape == (3, 128) and bufs.cover.dtype.is_floating_point is False and bufs.sums.shape == (1, 2, 3, 2, 40) and bufs.field.shape == (3, 64)
    assert R.refine_buffers(2, 3, "cpu", silhouette=True, pixel_capacity=64).cover is None and R.refine_buffers(2, 3, "cpu").cover is None
    assert "nobody has tuned" in R.pack_refine.__doc__.split("coverage =")[1].lower()


def test_the_term_is_one_more_flag_in_front_of_the_options_tail():
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.refinement import pack_refine
    from articulated_pose_amd.stream import OPTION_FLAGS, RESULT_NAMES, Options, check_options
    assert Options._fields[-3:] == ("refine_joints", "silhouette", "refine") and Options._fields[-4] == "refine_coverage"
    assert "refine_coverage" not in OPTION_FLAGS and "refine_coverage" not in RESULT_NAMES and "cover" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    sil, cov = silhouette_table(), coverage_table()
    for extra in (dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(render_mesh=mesh, reprojection=True)):
        off, on = check_options(batch_size=2, refine=sil, **dict(annotated, **extra)), check_options(batch_size=2, refine=cov, **dict(annotated, **extra))
        assert on.refine_coverage is True and off.refine_coverage is False and on.silhouette is True and on.refine_joints is False
        assert on._replace(refine_coverage=False) == off and on.layout == off.layout
        assert check_options(batch_size=2, **dict(annotated, **extra)).refine_coverage is False
    jt = coverage_table(joints=(1.0, 0.5))
    on = check_options(batch_size=2, render_mesh=mesh, kinematics=kin, refine=jt, **annotated)
    assert on.refine_coverage is True and on.refine_joints is True and on.silhouette is True
    with pytest.raises(ValueError, match=r"refine=.*joints=.*kinematics=<depth.pack_kinematics\(\.\.\.\)>"):
        check_options(batch_size=2, render_mesh=mesh, refine=jt, **annotated)
    with pytest.raises(ValueError, match="kinematics=<depth.pack_kinematics"):
        AncshPipeline(3, None, None, 2, 64, "cpu", render_mesh=mesh, refine=jt, **annotated)
    with pytest.raises(ValueError, match="refine=.* render_mesh"):
        check_options(refine=cov, **annotated)
    with pytest.raises(ValueError, match="refine: coverage weight"):
        check_options(batch_size=2, render_mesh=mesh, refine=np.r_[sil, np.zeros(16)], **annotated)
    with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, refine=cov)


# ---- the rules on hand-made frames -----------------------------------------------------------------------------------------------------------
H, W, PITCH, NF = 8, 8, 0.01, 1.0


def hand_scene(K=2, scale=1e-3):
    """Link l is part l; the ray of pixel (row, col) is (PITCH col - 0.04, PITCH row - 0.04): a pixel is PITCH z wide at depth z."""
    sc = np.zeros(240)
    sc[6], sc[14] = scale, K
    sc[7], sc[9], sc[11], sc[12] = PITCH, -0.04, PITCH, -0.04
    for l in range(K):
        sc[16 + 14 * l], sc[16 + 14 * l + 1] = l, l
    return sc


def key_of(z):
    return np.uint64(int(np.array([z], np.float32).view(np.uint32)[0]) << 32)


def hand_frames(pred_cols=(6, 7), z_pred=1.0, other=None):
    """Observed: part 0 in columns 0..3 at 1000 units = depth 1.0.  Predicted: part 0 in pred_cols at z_pred (none: the part draws no pixel);
    other = z: predicted part 1 over the observed columns at that depth."""
    od, ol = np.zeros((H, W), np.uint16), np.full((H, W), 255, np.uint8)
    od[:, :4], ol[:, :4] = 1000, 0
    pd, pl, pz = np.zeros((H, W), np.uint16), np.full((H, W), 255, np.uint8), np.full((H, W), np.uint64(0xffffffffffffffff))
    for c in pred_cols:
        pd[:, c], pl[:, c], pz[:, c] = int(round(z_pred * 1000)), 0, key_of(z_pred)
    if other is not None:
        pd[:, :4], pl[:, :4], pz[:, :4] = int(round(other * 1000)), 1, key_of(other)
    return (od, ol), (pd, pl, pz)


def hand_sums(table, **frames):
    obs, pred = hand_frames(**frames)
    sc = hand_scene()
    pose = np.r_[np.eye(3).ravel(), 1.0, 0.0, 0.0, 1.0]
    S, M = CM.cov_sums(obs, pred, CM.cover_of(pred, sc, 2)[0], (0, 0), sc, NF, pose, 0, 2, table)
    return S, M


def test_gap_rows_on_a_prediction_beside_its_observation():
    """Part 0 is observed in columns 0..3 and predicted in columns 6..7 at the same depth: all 32 observed pixels are gap pixels, the nearest
    predicted pixel is in the same row at column 6, so m = (6 - col) PITCH.  With dist_c below the smallest gap every pixel is far: no row,
    n_cfar = 32.  With dist_c above the largest all give rows, sum m_c^2 is what the geometry says, and b pulls the part towards the bare
    pixels: the step's translation along x is negative.  slack_c, the sentinel and another predicted part in front skip pixels."""
    near = coverage_table(coverage=dict(weight=1.0, dist=0.02, slack=0.0))
    S, M = hand_sums(near)
    assert S[34] == 0 and S[35] == 32 and (S[:34] == 0).all() and (M == 0).all()
    wide = coverage_table(coverage=dict(weight=2.0, dist=1.0, slack=0.0))
    S, M = hand_sums(wide)
    want = H * sum(((6 - c) * PITCH) ** 2 for c in range(4))
    assert S[34] == 32 and S[35] == 0 and abs(S[33] - want) <= 1e-15 and (S[27:33] == 0).all()
    assert abs(S[24] - 4.0 * H * sum((6 - c) * PITCH for c in range(4))) <= 1e-13 and abs(S[25]) <= 1e-15 and S[26] == 0      # b_t = weight^2 sum g m
    assert abs(S[15] - 4.0 * 32) <= 1e-12                                # A[3][3] = weight^2 per row: g = (1, 0, 0)
    ok, out = RF.solve_update(np.r_[S[:27], np.zeros(13)], np.r_[np.eye(3).ravel(), 1.0, 0.0, 0.0, 1.0], coverage_table(max_dist=1.0))
    x = np.array([0.02, 0.0, 1.0])                                       # a surface point in column 6; the start pose is the identity about (0, 0, 1)
    moved = out[9] * out[:9].reshape(3, 3) @ (x - [0.0, 0.0, 1.0]) + out[10:13]
    assert ok and moved[0] < x[0] - 0.02, (out, moved)                   # towards the bare columns, by about the mean gap of 0.045
    for slack, rows in ((2.9, 32), (3.0, 24), (4.5, 16), (6.0, 0)):      # column c is 6 - c pixels away: (6 - c)^2 <= slack^2 is skipped
        S, _ = hand_sums(coverage_table(coverage=dict(weight=1.0, dist=1.0, slack=slack)))
        assert S[34] == rows and S[35] == 0, (slack, S[34])
    S, M = hand_sums(wide, pred_cols=())                                 # the sentinel: the part drew no pixel
    assert (S == 0).all() and (M == 0).all()
    S, _ = hand_sums(wide, other=0.9)                                    # another part predicted in front of the observation: skipped
    assert (S == 0).all()
    S, _ = hand_sums(wide, other=1.0)                                    # ... or at it: !(z_q > z_o)
    assert (S == 0).all()
    S, _ = hand_sums(wide, other=1.1)                                    # behind it: the gap rows stand
    assert S[34] == 32 and abs(S[33] - want) <= 1e-15
    S, _ = hand_sums(wide, z_pred=2.0)                                   # z_2 is the PREDICTED pixel's depth: a pixel is twice as wide there
    assert S[34] == 32 and abs(S[33] - 4.0 * want) <= 1e-14


def test_far_pixels_the_sentinel_the_cost_and_triples_without_a_gap_pixel():
    """On the problem's frames.  A record moved sixty pixels aside: with dist_c below the gap every gap pixel is far, gives no row, and C is
    what the formula says; a part moved out of the crop draws no pixel, so its cover is the sentinel: no row, no charge beyond the missed
    pixels', and the solve threshold counts nothing.  C equals cost(row) everywhere, and a (frame, part, pose) without a gap pixel has
    silhouette_mirror's first 36 sums byte for byte."""
    K, dtype = 3, "uint16"
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    side = SM.lateral_record(rec, cen, 0.6)
    near = coverage_table(iters=1, silhouette=dict(weight=1.0, dist=0.05, slack=0.0), coverage=dict(weight=1.5, dist=0.05, slack=0.0))
    S, _ = CM.evaluate(mesh, render, scene, rigs, nf, side, geom, frames, near)
    S36, _ = SM.evaluate(mesh, render, scene, rigs, nf, side, geom, frames, near[:16])
    seen = S[..., 38] > 0
    assert seen.any() and (S[..., 37] == 0).all() and (S[..., 28][seen] == 0).all() and (S[..., :30].tobytes() == S36[..., :30].tobytes())
    want = (MAX_DIST ** 2 * S[..., 29] + 0.05 ** 2 * S[..., 34] + 1.5 ** 2 * 0.05 ** 2 * S[..., 38]) / S[..., 29]
    assert np.abs(S[..., 30] - want)[seen].max() <= 1e-15 and (S[..., 30][seen] > S36[..., 30][seen]).all()
    gone = rec.copy()
    gone[0, 1, 10:13] += [10.0, 0.0, 0.0]                                # pose 0 of part 1 in frame 0 leaves the crop
    table = coverage_table(iters=1)
    S, _ = CM.evaluate(mesh, render, scene, rigs, nf, gone, geom, frames, table)
    S36, _ = SM.evaluate(mesh, render, scene, rigs, nf, gone, geom, frames, table[:16])
    assert S[0, 1, 0, 29] > 0 and (S[0, 1, 0, 36:] == 0).all() and S[0, 1, 0, 28] == 0 and S[0, 1, 0, :36].tobytes() == S36[0, 1, 0].tobytes()
    assert abs(S[0, 1, 0, 30] - MAX_DIST ** 2) <= 1e-18
    best = np.full((3, K, 2, RF.BEST), np.nan)
    out = CM.step(S.copy(), gone, best, 0, False, table)
    assert out[0, 1, :13].tobytes() == gone[0, 1, :13].tobytes() and best[0, 1, 0, 17] == 0
    mixed = rec.copy()
    mixed[:, 0] = SM.lateral_record(rec, cen, 0.04)[:, 0]                # part 0 slides, the others stay
    S, _ = CM.evaluate(mesh, render, scene, rigs, nf, mixed, geom, frames, table)
    S36, _ = SM.evaluate(mesh, render, scene, rigs, nf, mixed, geom, frames, table[:16])
    bare = (S[..., 37] + S[..., 38]) == 0
    assert bare.any() and (~bare).any() and (S[:, 0, :, 37] > 0).all()
    assert S[bare][:, :36].tobytes() == S36[bare].tobytes() and (S[..., 39] == 0).all() and (S[..., 35] == 0).all()
    rows = ~bare & (S[..., 37] > 0)
    assert (S[rows][:, :27].tobytes() != S36[rows][:, :27].tobytes()) and S[rows][:, 27:30].tobytes() == S36[rows][:, 27:30].tobytes()
    assert S[rows][:, 32:36].tobytes() == S36[rows][:, 32:36].tobytes()
    for idx in np.ndindex(3, K, 2):
        c = CM.cost(S[idx], table)
        assert np.array([c]).tobytes() == S[idx][30:31].tobytes()
    assert np.isnan(CM.cost(np.zeros(40), table))


# ---- the behavioural bars ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype,shift", CASES, ids=IDS)
def test_no_triple_ends_further_from_the_truth_than_it_started(K, dtype, shift):
    """test_silhouette_cpu's lateral-shift frames with the coverage term on, measured against the silhouette term alone and the plain loop on
    the same records: the existing lateral bar holds against the plain loop, NO triple ends above 1.0 of the shift (the silhouette term alone
    leaves one or two: a pose that slid along a face, its overhang rows skipped as an occlusion), and at least as many end at or below 0.5."""
    prob, rec, per, cen = problem(K, dtype)
    lat = SM.lateral_record(rec, cen, shift)
    cols = cov_mirror(prob, lat, dtype, coverage_table())[0]
    s_cols = sil_mirror(prob, lat, dtype, silhouette_table())[0]
    p_cols = mirror(prob, lat, dtype, refine_table())[0]
    behavioural_bars(cols, strict=False)
    r_cov, r_sil, r_plain = (SM.lateral_errors(rec, refined(c), cen) / shift for c in (cols, s_cols, p_cols))
    lateral_bar(r_cov, r_plain)
    print("coverage: median %.3f worst %.3f;  silhouette alone: median %.3f worst %.3f, above 1.0: %d, at or below 0.5: %d of %d"
          % (np.median(r_cov), r_cov.max(), np.median(r_sil), r_sil.max(), (r_sil > 1.0).sum(), (r_sil <= 0.5).sum(), r_sil.size))
    assert (r_cov > 1.0).sum() == 0, np.sort(r_cov.ravel())
    assert (r_cov <= 0.5).sum() >= (r_sil <= 0.5).sum(), (np.sort(r_cov.ravel()), np.sort(r_sil.ravel()))


@pytest.mark.parametrize("K,dtype,sapien", PERTURBED, ids=PERTURBED_IDS)
def test_the_existing_perturbation_still_ends_strictly_lower(K, dtype, sapien):
    """test_refinement_cpu's perturbation (along the ray, tilted) with both terms on: cost_best < cost_start for every part and pose on the
    new measure; the best row is one of the evaluated poses and its cost that pass's, which is cost() of that pass's sums."""
    prob, rec, per, cen = problem(K, dtype, sapien)
    table = coverage_table()
    cols, sums, bounds, poses = cov_mirror(prob, per, dtype, table)
    behavioural_bars(cols, strict=True)
    assert sums.shape == (int(table[0]) + 1, 3, K, 2, 40) and (sums[..., 37] > 0).any() and (sums[..., 39] == 0).all()
    for f in range(3):
        for j in range(K):
            for v in range(2):
                b = cols[f, j, 18 * v:18 * v + 18]
                p = int(b[16])
                assert b[:13].tobytes() == poses[p, f, j, 13 * v:13 * v + 13].tobytes() and b[14] == sums[p, f, j, v, 30] and b[15] == sums[p, f, j, v, 28]
                assert b[13] == sums[0, f, j, v, 30] and b[14] == np.nanmin(sums[:, f, j, v, 30])
                assert sums[p, f, j, v, 30] == CM.cost(sums[p, f, j, v], table)
