"""CPU (no GPU): the scale unknown of render-and-compare ICP (pack_refine(..., scale=...), ancsh_refine_pass_scale).  The entry's place in the
ABI and its argument checks before any launch, the 48-value table and the option flag, and the mirror (tests/scale_mirror.py) validated on
its own: the three kinds of rows on hand-made frames where every new sum can be said in advance, the 7 x 7 solve against numpy, the update as
a similarity about the centre, both clamps, columns 0..39 and the sigma = 0 step against coverage_mirror byte for byte -- and the behaviour:
on test_silhouette_cpu's frames with every part scaled about its centre, the coverage-only loop carries s bit for bit (rho exactly 1) while
the loop with scale= brings it back (no triple above 1, the median below, the pinned bars of SCALE_BARS)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coverage_mirror as CM
import refinement_mirror as RF
import reprojection_mirror as RP
import scale_mirror as SC
import silhouette_mirror as SM
from test_coverage_cpu import H, NF, PERTURBED, PERTURBED_IDS, PITCH, W, cov_mirror, coverage_table, hand_scene, key_of
from test_refinement_cpu import behavioural_bars
from test_reprojection_cpu import posed_object
from test_render_cpu import box_mesh
from test_silhouette_cpu import P16, problem, refined, silhouette_table

HERE = os.path.dirname(os.path.abspath(__file__))
NAME, NARGS = "ancsh_refine_pass_scale", 31
SCALE = dict(max_step=0.05, max_total=0.25)                              # the issue's values
FACTOR = 1.06
SCALE_CASES = [(K, dtype) for K in (2, 3) for dtype in ("uint16", "float32")]
SCALE_IDS = ["K%d-%s" % c for c in SCALE_CASES]
# the mirror's worst rho per case (printed by the behaviour test, written into DESIGN.md 6b); the pinned bar is twice that, at most 1
MIRROR_WORST = {(2, "uint16"): 0.448, (2, "float32"): 0.438, (3, "uint16"): 0.568, (3, "float32"): 0.950}
SCALE_BARS = {case: min(1.0, 2.0 * worst) for case, worst in MIRROR_WORST.items()}


def scale_table(**over):
    """test_coverage_cpu's table with the scale unknown (shared with the GPU tests)."""
    return coverage_table(**dict(dict(scale=SCALE), **over))


def scale_mirror(prob, rec, dtype, table):
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    return SC.refine(mesh, render, scene, rigs, nf, rec, geom, frames, dtype, table)


def scale_bars(case, exact, start, cols):
    """The behaviour gates on a loop's 36 columns (shared with the GPU test) -> rho (n, K, 2)."""
    r = SC.rho(exact, start, refined(cols))
    b = cols.reshape(cols.shape[:2] + (2, 18))
    print("K%d-%s: rho median %.3f worst %.3f" % (case + (np.median(r), r.max())))
    assert (r > 1.0).sum() == 0 and np.median(r) < 1.0 and r.max() <= SCALE_BARS[case], np.sort(r.ravel())
    solved = b[..., 17] > 0
    assert solved.any() and (b[..., 14][solved] < b[..., 13][solved]).all()
    return r


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose import refinement as R
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in declared_symbols() and NAME in exported and NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == NARGS
    assert _lib.lib().ancsh_abi_version() == 14 and len(_lib.SIGNATURES["ancsh_refine_pass_cov"]) == 29
    cov, scl = _lib.SIGNATURES["ancsh_refine_pass_cov"], _lib.SIGNATURES[NAME]
    assert scl[:21] == cov[:21] and scl[21:23] == [ctypes.c_void_p, ctypes.c_int] and scl[23:] == cov[21:]      # fitted, ld_fitted behind cover
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_REFINE_SCALE_SUMS 48\n" in header and "#define ANCSH_REFINE_SCALE_PARAMS 48\n" in header
    assert R.REFINE_SCALE_SUMS == SC.SUMS == 48 and R.REFINE_SCALE_PARAMS == SC.PARAMS == 48
    assert R.SCALE_SUMS_COLUMNS == dict(R.COV_SUMS_COLUMNS, A_s=slice(40, 47), b_s=47)
    assert R.PARAMS_LENGTHS[NAME] == (48,) and set(R.PARAMS_LENGTHS) == {"ancsh_refine_pass", "ancsh_refine_pass_sil", "ancsh_refine_pass_cov",
                                                                          "ancsh_refine_joint_step", NAME}
    assert R.PARAMS_LENGTHS["ancsh_refine_pass_cov"] == (32,) and R.PARAMS_LENGTHS["ancsh_refine_joint_step"] == (24, 32)
    assert R.RefineBuffers._fields == ("work", "best", "sums", "field", "state", "obj", "xi", "cover")


def test_entry_refuses_bad_arguments_before_any_launch():
    """test_coverage_cpu's list under the new name, and fitted / ld_fitted: an accepted call has nframes == 0, which launches nothing -- after
    all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    odd = lambda a: ctypes.c_void_p(a)
    ptrs = ("verts", "tris", "tri_link", "od", "ol", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params", "field", "cover", "fitted", "pin",
            "pout", "best", "sums")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, kind=0, V=10, T=12, cap=4096, p=0, last=0, ld=26, ldf=26, pout=ctypes.c_void_p(32))
    order = ("n", "K", "kind", "verts", "tris", "tri_link", "V", "T", "od", "ol", "cap", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params",
             "field", "cover", "fitted", "ldf", "p", "last", "pin", "ld", "pout", "best", "sums")
    run = lambda **over: L.ancsh_refine_pass_scale(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(kind=1, p=8, last=1, ld=77, ldf=62, K=8, V=0, T=0) == 0 and run(fitted=good["pin"]) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(kind=-1), b"depth_type=-1"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"),
                       (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T="), (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V="), (dict(p=-1), b"pass=-1"),
                       (dict(p=9), b"pass=9"), (dict(last=2), b"is_last=2"), (dict(ld=25), b"ld_in=25"), (dict(ldf=25), b"ld_fitted=25"),
                       (dict(ldf=0), b"ld_fitted=0"), (dict(od=odd(17)), b"aligned"),
                       (dict(kind=1, pd=odd(18)), b"aligned"), (dict(verts=odd(18)), b"aligned"), (dict(tris=odd(18)), b"aligned"),
                       (dict(tri_link=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(nf=odd(18)), b"aligned"),
                       (dict(field=odd(18)), b"aligned"), (dict(cover=odd(18)), b"aligned"), (dict(zb=odd(20)), b"aligned"),
                       (dict(scene=odd(20)), b"aligned"), (dict(rt=odd(20)), b"aligned"), (dict(params=odd(20)), b"aligned"),
                       (dict(pin=odd(20)), b"aligned"), (dict(pout=odd(20)), b"aligned"), (dict(best=odd(20)), b"aligned"),
                       (dict(sums=odd(20)), b"aligned"), (dict(fitted=odd(20)), b"aligned"), (dict(pout=P16), b"overlap")):
        assert run(**over) == -1 and what in L.ancsh_last_error() and b"refine_pass_scale" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs:
        assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    assert run(ld=25, ldf=25) == -1 and b"ld_in=25" in L.ancsh_last_error()          # the same order: ld_in first


# ---- the table and the option ----------------------------------------------------------------------------------------------------------------
def test_pack_refine_lays_out_the_48_value_table_and_leaves_the_shorter_ones_alone():
    from articulated_pose_amd.pose import refinement as R
    head = dict(iters=5, max_dist=0.02)
    sil, cov = dict(weight=2.0, dist=0.05, slack=0.5), dict(weight=3.0, dist=0.07, slack=0.25)
    want_head = [5.0, 0.02, 0.1, 1e-3, float(np.radians(10.0)), 32.0, 0.0, 0.0]
    older = (R.pack_refine(**head), R.pack_refine(silhouette=sil, **head), R.pack_refine(joints=(2.0, 0.25), **head),
             R.pack_refine(silhouette=sil, coverage=cov, **head))
    assert older[0].tolist() == want_head and older[1].tolist() == want_head + [2.0, 0.05, 0.5, 0, 0, 0, 0, 0]
    assert older[2].tolist() == want_head + [0.0] * 8 + [2.0, 0.25, 0, 0, 0, 0, 0, 0]
    assert older[3].tolist() == older[1].tolist() + [0.0] * 8 + [3.0, 0.07, 0.25, 0, 0, 0, 0, 0]
    for t in older:
        assert not R.has_scale(t) and R.check_refine_table(t).tobytes() == t.tobytes()
        assert R.pack_refine(scale=None, **head).tobytes() == older[0].tobytes()
    assert R.has_coverage(older[3]) and not R.has_coverage(older[1]) and not R.has_coverage(older[2])
    t = R.pack_refine(silhouette=sil, coverage=cov, scale=dict(max_step=0.1, max_total=0.3), **head)
    assert t.shape == (48,) and t.dtype == np.float64 and t[:32].tobytes() == older[3].tobytes()
    assert t[32:].tolist() == [0.1, 0.3] + [0.0] * 14 and t.tobytes() == np.array(older[3].tolist() + [0.1, 0.3] + [0.0] * 14).tobytes()
    assert R.has_scale(t) and R.has_coverage(t) and R.has_silhouette(t) and not R.has_joints(t) and R.check_refine_table(t).tobytes() == t.tobytes()
    assert R.pack_refine(silhouette=sil, coverage=cov, scale={})[32:34].tolist() == [0.05, 0.25]
    assert R.pack_refine(silhouette=sil, coverage=cov, scale=(0.5, 1.0))[32:34].tolist() == [0.5, 1.0]
    assert R.pack_refine(silhouette=sil, coverage=cov, scale=(0.2, 0.2))[32:34].tolist() == [0.2, 0.2]
    needs = r"refine: scale needs the silhouette and coverage terms \(their rows are what observes size\)"
    for kw in (dict(), dict(silhouette=sil), dict(joints=(1.0, 0.5)), dict(silhouette=sil, joints=(1.0, 0.5))):
        with pytest.raises(ValueError, match=needs):
            R.pack_refine(scale=SCALE, **kw)
    for bad in (np.r_[older[0], np.zeros(24), [0.05, 0.25], np.zeros(14)], np.r_[older[1], np.zeros(16), [0.05, 0.25], np.zeros(14)],
                np.r_[older[0], np.zeros(16), older[3][24:], [0.05, 0.25], np.zeros(14)]):
        with pytest.raises(ValueError, match=needs):
            R.check_refine_table(bad)
    with pytest.raises(ValueError, match="refine: scale with joints .*opens its joints.*6 K system has no scale unknown yet"):
        R.pack_refine(silhouette=sil, coverage=cov, joints=(1.0, 0.5), scale=SCALE)
    for at in range(16, 24):
        bad = t.copy()
        bad[at] = 1.0
        with pytest.raises(ValueError, match="refine: scale with joints .*opens its joints.*6 K system has no scale unknown yet"):
            R.check_refine_table(bad)
    for scale, what in ((dict(max_step=0.0), "max_step"), (dict(max_step=-0.1), "max_step"), (dict(max_step=0.51, max_total=0.6), "max_step"),
                        (dict(max_step=float("nan")), "max_step"), (dict(max_step=float("inf")), "max_step"), (dict(max_total=0.04), "max_total"),
                        (dict(max_total=1.01), "max_total"), (dict(max_total=float("nan")), "max_total"), (dict(max_total=float("inf")), "max_total"),
                        ((0.2, 0.1), "max_total"), ((0.0, 0.1), "max_step"), (dict(reach=2), "scale takes"), (dict(max_step="big"), "scale is"),
                        (5.0, "scale is"), ((1, 2, 3), "scale is")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            R.pack_refine(silhouette=sil, coverage=cov, scale=scale)
    for at in range(34, 48):
        bad = t.copy()
        bad[at] = 1.0
        with pytest.raises(ValueError, match=r"refine: the reserved values 34\.\.47 must be 0"):
            R.check_refine_table(bad)
    for at, what in ((0, "iters"), (12, r"reserved values 11\.\.15"), (25, "coverage dist"), (29, r"reserved values 27\.\.31")):
        bad = t.copy()                                                   # the front is held to the coverage table's own rules and messages
        bad[at] = -1.0
        with pytest.raises(ValueError, match="refine: .*" + what):
            R.check_refine_table(bad)
    for shape in ((40,), (47,), (49,), (2, 48)):
        with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table \(pose.refinement.pack_refine\), or \(16,\) with silhouette=, got shape"):
            R.check_refine_table(np.zeros(shape))
    with pytest.raises(ValueError, match="scale=True.*coverage=True"):
        R.refine_buffers(2, 3, "cpu", silhouette=True, scale=True, pixel_capacity=64)
    bufs = R.refine_buffers(2, 3, "cpu", silhouette=True, coverage=True, scale=True, pixel_capacity=64)
    assert bufs.sums.shape == (1, 2, 3, 2, 48) and bufs.cover.shape == (3, 128) and bufs.state is None
    assert R.refine_buffers(2, 3, "cpu", silhouette=True, coverage=True, pixel_capacity=64).sums.shape == (1, 2, 3, 2, 40)
    assert "nobody has tuned" in R.pack_refine.__doc__.split("scale =")[1].lower()


def test_the_unknown_is_one_more_flag_in_front_of_refine_coverage():
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.stream import OPTION_FLAGS, RESULT_NAMES, Options, check_options
    at = Options._fields.index("refine_coverage")
    assert Options._fields[at - 1] == "refine_scale" and Options._fields[at - 2] == "inputs"
    assert Options._fields[-4:] == ("refine_coverage", "refine_joints", "silhouette", "refine")
    assert "refine_scale" not in OPTION_FLAGS and "refine_scale" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    cov, scl = coverage_table(), scale_table()
    for extra in (dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(render_mesh=mesh, reprojection=True),
                  dict(render_mesh=mesh, kinematics=kin, joint_values=True)):
        off, on = check_options(batch_size=2, refine=cov, **dict(annotated, **extra)), check_options(batch_size=2, refine=scl, **dict(annotated, **extra))
        assert on.refine_scale is True and off.refine_scale is False and on.refine_coverage is True and on.silhouette is True and on.refine_joints is False
        assert on._replace(refine_scale=False) == off and on.layout == off.layout and on.record_width == off.record_width and on.inputs == off.inputs
        assert check_options(batch_size=2, **dict(annotated, **extra)).refine_scale is False
    with pytest.raises(ValueError, match="refine=.* render_mesh"):
        check_options(refine=scl, **annotated)
    bad = scl.copy()
    bad[16:18] = 1.0, 0.5
    with pytest.raises(ValueError, match="refine: scale with joints"):
        check_options(batch_size=2, render_mesh=mesh, kinematics=kin, refine=bad, **annotated)
    with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, refine=scl)


# ---- the rows on hand-made frames ------------------------------------------------------------------------------------------------------------
Z_PRED = float(np.float32(1.002))


def three_kinds():
    """test_coverage_cpu's 8 x 8 frame with all three kinds in it: part 0 observed in columns 0..3 at depth 1, predicted in columns 2, 3, 6, 7
    at Z_PRED on triangle 0, which faces the camera: columns 2..3 are depth rows, 0..1 gap rows (the nearest predicted pixel: column 2), 6..7
    overhang rows (the nearest observed pixel: column 3).  The pose is the identity at (0, 0, 1): its centre is (0.5, 0.5, 1.5)."""
    od, ol = np.zeros((H, W), np.uint16), np.full((H, W), 255, np.uint8)
    od[:, :4], ol[:, :4] = 1000, 0
    pd, pl, pz = np.zeros((H, W), np.uint16), np.full((H, W), 255, np.uint8), np.full((H, W), np.uint64(0xffffffffffffffff))
    for c in (2, 3, 6, 7):
        pd[:, c], pl[:, c], pz[:, c] = 1002, 0, key_of(Z_PRED)
    mesh = (np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32), np.array([[0, 1, 2]], np.int32), np.array([0], np.int32))
    rt = np.zeros(208)
    rt[16:28] = np.eye(4)[:3].ravel()
    sc = hand_scene()
    pose = np.r_[np.eye(3).ravel(), 1.0, 0.0, 0.0, 1.0]
    obs, pred = (od, ol), (pd, pl, pz)
    fld = SM.field_of_mask(RP.part_image(od, ol, RP.link_parts(sc, 2)[0]) == 0)
    return mesh, obs, pred, fld, CM.cover_of(pred, sc, 2)[0], (0, 0), sc, rt, NF, pose, 0, 2


def test_every_kind_of_row_adds_the_scale_sums_said_in_advance():
    """x of column c is PITCH c - 0.04, y of row i is -(PITCH i - 0.04) (the cloud flips y); c = (0.5, 0.5, 1.5).
    depth: n = (0, 0, -1), pc_z = Z_PRED - 1.5, Js = 1.5 - Z_PRED, r = -(Z_PRED - 1): 16 rows.
    overhang: g = (1, 0, 0), m = (c - 3) PITCH Z_PRED, Js = weight (Z_PRED x_c - 0.5): 16 rows.
    gap: g = (1, 0, 0), the nearest predicted pixel is column 2: m = (2 - c) PITCH Z_PRED, Js = weight_c (Z_PRED x_2 - 0.5): 16 rows."""
    table = scale_table(max_dist=0.1, silhouette=dict(weight=2.0, dist=1.0, slack=0.0), coverage=dict(weight=3.0, dist=1.0, slack=0.0))
    args = three_kinds()
    x = lambda c: Z_PRED * (PITCH * c - 0.04)
    S, M = SC.row_sums(SC.rows("depth", *args, table))
    js, r = 1.5 - Z_PRED, -(Z_PRED - 1.0)
    assert abs(S[27 + 5] - 16 * -1.0 * js) <= 1e-13 and abs(S[27 + 6] - 16 * js * js) <= 1e-13 and abs(S[27 + 7] - 16 * js * r) <= 1e-15
    assert abs(S[27 + 3]) <= 1e-15 and abs(S[27 + 4]) <= 1e-15 and abs(S[20] - 16.0) <= 1e-13          # A_55 = n_z^2 per row
    pcx = [x(c) - 0.5 for c in (2, 3)]                                   # J_1 = pc_2 n_0 - pc_0 n_2 = pc_0: A_1s = sum pc_x Js
    assert abs(S[27 + 1] - H * sum(pcx) * js) <= 1e-13 and (M[27:] >= np.abs(S[27:])).all()
    S, _ = SC.row_sums(SC.rows("overhang", *args, table))
    js = [2.0 * (x(c) - 0.5) for c in (6, 7)]
    m = [(c - 3) * PITCH * Z_PRED for c in (6, 7)]
    assert abs(S[27 + 3] - H * 2.0 * sum(js)) <= 1e-13 and abs(S[27 + 6] - H * sum(v * v for v in js)) <= 1e-13
    assert abs(S[27 + 7] - H * sum(a * 2.0 * b for a, b in zip(js, m))) <= 1e-14 and abs(S[27 + 4]) <= 1e-15 and abs(S[27 + 5]) <= 1e-15
    S, _ = SC.row_sums(SC.rows("gap", *args, table))
    js = 3.0 * (x(2) - 0.5)
    m = [(2 - c) * PITCH * Z_PRED for c in (0, 1)]
    assert abs(S[27 + 3] - 16 * 3.0 * js) <= 1e-12 and abs(S[27 + 6] - 16 * js * js) <= 1e-12 and abs(S[27 + 7] - H * js * 3.0 * sum(m)) <= 1e-14
    assert abs(S[15] - 9.0 * 16) <= 1e-12                                # A_33 = weight_c^2 per row
    # growing the part about a centre that lies to the right of and behind all of it moves every drawn pixel left and nearer: the gap rows
    # (bare pixels on the left) ask for sigma > 0, the overhang rows (drawn where nothing was seen, on the right) as well
    for kind in ("gap", "overhang"):
        S, _ = SC.row_sums(SC.rows(kind, *args, table))
        assert -S[27 + 7] / S[27 + 6] > 0, kind


# ---- thread 0 ---------------------------------------------------------------------------------------------------------------------------------
def random_sums(rs, rows=40):
    """A 48-value sums row of `rows` random 7-column rows: positive definite."""
    J = rs.normal(size=(rows, 7)) * [1.0, 1.0, 1.0, 3.0, 3.0, 3.0, 2.0]
    r = rs.normal(size=rows) * 1e-3
    A, b = J.T @ J, J.T @ r
    S = np.zeros(48)
    S[:21], S[21:27] = A[:6, :6][np.triu_indices(6)], b[:6]
    S[40:46], S[46], S[47] = A[:6, 6], A[6, 6], b[6]
    S[28] = S[29] = rows
    return S, A, b


def test_solve_matches_a_float64_solver_and_the_update_is_a_similarity_about_the_centre():
    rs = np.random.RandomState(5)
    table = scale_table()
    for _ in range(20):
        S, A, b = random_sums(rs)
        ok, xi = SC.solve7(S, table)
        Ad = A + np.diag(table[3] * np.diag(A) + 1e-12)
        assert ok and np.abs(np.array(xi) - np.linalg.solve(Ad, -b)).max() <= 1e-12 * np.abs(xi).max()
    assert SC.solve7(np.zeros(48), table)[0] and SC.solve7(np.zeros(48), table)[1] == [0.0] * 7      # nothing seen: the damping's 1e-12 alone
    bad = S.copy()
    bad[46] = -1.0
    assert not SC.solve7(bad, table)[0] and not SC.solve7(np.r_[S[:47], np.nan], table)[0]
    for _ in range(20):
        q = rs.normal(size=4)
        q /= np.linalg.norm(q)
        R0 = np.array([[1 - 2 * (q[2] ** 2 + q[3] ** 2), 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[1] * q[3] + q[0] * q[2])],
                       [2 * (q[1] * q[2] + q[0] * q[3]), 1 - 2 * (q[1] ** 2 + q[3] ** 2), 2 * (q[2] * q[3] - q[0] * q[1])],
                       [2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[2] * q[3] + q[0] * q[1]), 1 - 2 * (q[1] ** 2 + q[2] ** 2)]])
        pose = np.r_[R0.ravel(), rs.uniform(0.5, 2.0), rs.normal(size=3)]
        xi = list(rs.normal(size=3) * 0.1) + list(rs.normal(size=3) * 0.05) + [rs.uniform(-0.05, 0.05)]
        out = SC.update(xi, pose)
        c = np.array(RF.centre(list(pose)))
        dR = out[:9].reshape(3, 3) @ R0.T
        assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-14 and abs(out[9] - pose[9] * (1 + xi[6])) <= 1e-15
        X = rs.normal(size=(50, 3))                                      # model points: x = s R X + t -> x' = c + (1 + sigma) dR (x - c) + d
        before, after = pose[9] * X @ R0.T + pose[10:13], out[9] * X @ out[:9].reshape(3, 3).T + out[10:13]
        want = c + (1 + xi[6]) * (before - c) @ dR.T + np.array(xi[3:6])
        assert np.abs(after - want).max() <= 1e-14
        assert np.abs(np.array(RF.centre(list(out))) - (c + np.array(xi[3:6]))).max() <= 1e-14        # the centre only translates


def test_both_clamps():
    table = scale_table(max_dist=0.1, max_angle_deg=10.0, scale=dict(max_step=0.05, max_total=0.08))
    small = [0.01, 0.0, 0.0, 0.0, 0.02, 0.0]
    out = SC.clamp(small + [0.2], 1.0, 1.0, table)                       # only sigma exceeds: all seven by 0.05 / 0.2
    assert np.allclose(out, [v * 0.25 for v in small] + [0.05], rtol=1e-15, atol=0) and out[6] == 0.2 * (0.05 / 0.2)
    out = SC.clamp(small + [-0.2], 1.0, 1.0, table)
    assert np.allclose(out, [v * 0.25 for v in small] + [-0.05], rtol=1e-15, atol=0)
    assert SC.clamp(small + [0.05], 1.0, 1.0, table) == small + [0.05]   # at the clamp: untouched
    out = SC.clamp([0.0, 0.0, 0.0, 0.4, 0.0, 0.0, 0.04], 1.0, 1.0, table)      # only the translation exceeds: sigma shrinks with it
    assert out[3] == 0.4 * (0.1 / 0.4) and out[6] == 0.04 * (0.1 / 0.4)
    out = SC.clamp([0.5, 0.0, 0.0, 0.4, 0.0, 0.0, 0.2], 1.0, 1.0, table)       # all three: the smallest ratio, sigma's
    assert out[6] == 0.2 * (0.05 / 0.2) and out[0] == 0.5 * (0.05 / 0.2)
    # the total bound, reached from either side: s_0 = 2, the band is [2 / 1.08, 2.16]
    out = SC.clamp(small + [0.04], 2.12, 2.0, table)
    assert out[:6] == small and out[6] == 2.0 * 1.08 / 2.12 - 1.0 and abs(2.12 * (1.0 + out[6]) - 2.16) <= 1e-15
    out = SC.clamp(small + [-0.04], 1.88, 2.0, table)
    assert out[:6] == small and out[6] == (2.0 / 1.08) / 1.88 - 1.0 and abs(1.88 * (1.0 + out[6]) - 2.0 / 1.08) <= 1e-15
    assert SC.clamp(small + [0.01], 2.12, 2.0, table)[6] == 0.01         # inside the band: untouched
    S, _, _ = random_sums(np.random.RandomState(6))
    pose = np.r_[np.eye(3).ravel(), 2.12, 0.0, 0.0, 1.0]
    ok, out = SC.solve_update(S, pose, 2.0, table)
    assert ok and 2.0 / 1.08 <= out[9] <= 2.16
    assert not SC.solve_update(S, np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.0, 1.0], 2.0, table)[0]      # a working s of 0 cannot be scaled back into the band


def test_columns_0_to_39_and_the_sigma_0_step_are_the_coverage_mirrors_bytes():
    K, dtype = 2, "uint16"
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = scale_table()
    lat = SM.lateral_record(rec, cen, 0.02)
    S48, B48 = SC.evaluate(mesh, render, scene, rigs, nf, lat, geom, frames, table, lat)
    S40, B40 = CM.evaluate(mesh, render, scene, rigs, nf, lat, geom, frames, table[:32].copy())
    assert S48[..., :40].tobytes() == S40.tobytes() and B48[..., :40].tobytes() == B40.tobytes()
    assert np.isfinite(S48[..., 40:]).all() and (S48[..., 46] > 0).all() and (B48[..., 40:] > 0).all() and (S48[..., 37] > 0).any()
    for idx in np.ndindex(3, K, 2):                                      # A is positive semi-definite with the column: A_ss A_kk >= A_ks^2
        S = S48[idx]
        diag = [0, 6, 11, 15, 18, 20]
        assert all(S[46] * S[diag[k]] >= S[40 + k] ** 2 * (1 - 1e-12) for k in range(6))
    flat = S48.copy()
    flat[..., 40:] = 0.0
    for idx in np.ndindex(3, K, 2):
        f, j, v = idx
        pose = lat[f, j, 13 * v:13 * v + 13]
        ok, out = SC.solve_update(flat[idx], pose, pose[9], table)
        ok_c, out_c = RF.solve_update(S40[idx], pose, table)
        assert ok and ok_c and out.tobytes() == out_c.tobytes(), idx
    bad = lat.copy()
    bad[0, 0, 9], bad[1, 1, 13 + 9], bad[2, 0, 9] = 0.0, -1.0, np.inf      # s_0 not > 0 or not finite: the NaN branch; the working pose is fine
    S, _ = SC.evaluate(mesh, render, scene, rigs, nf, lat, geom, frames, table, bad)
    gone = np.zeros((3, K, 2), bool)
    gone[0, 0, 0] = gone[1, 1, 1] = gone[2, 0, 0] = True
    assert np.isnan(S[gone][:, 40:]).all() and np.isnan(S[gone][:, :31]).all() and (S[gone][:, [31, 35, 39]] == 0).all()
    assert S[~gone].tobytes() == S48[~gone].tobytes()
    best = np.full((3, K, 2, RF.BEST), np.nan)
    out = SC.step(S, lat, best, bad, 0, False, table)
    assert np.isnan(best[gone]).all() and out[0, 0, :13].tobytes() == lat[0, 0, :13].tobytes() and np.isfinite(best[~gone]).all()


# ---- the behaviour ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", SCALE_CASES, ids=SCALE_IDS)
def test_parts_of_the_wrong_size_come_back_and_the_coverage_loop_carries_them(K, dtype):
    """Every part of the exact record scaled about its centre by 1.06 or 1 / 1.06 in turn, the centre kept.  The coverage-only loop keeps s
    bit for bit: rho is exactly 1 for every triple.  With scale=: no triple above 1, the median strictly below 1, the worst within
    SCALE_BARS (twice the mirror's worst, at most 1), cost_best < cost_start for every triple that solved.
    The mirror's figures (median / worst rho): K2-uint16 0.157 / 0.448, K2-float32 0.184 / 0.438, K3-uint16 0.120 / 0.568, K3-float32
    0.141 / 0.950.  No input was dropped."""
    prob, rec, per, cen = problem(K, dtype)
    scl, fs = SC.scaled_record(rec, FACTOR)
    assert set(np.round(fs.ravel(), 12)) == {round(FACTOR, 12), round(1 / FACTOR, 12)}
    for f, j, v in np.ndindex(3, K, 2):                                  # the centre is kept
        a, b = rec[f, j, 13 * v:13 * v + 13], scl[f, j, 13 * v:13 * v + 13]
        assert np.abs(np.array(RF.centre(list(a))) - np.array(RF.centre(list(b)))).max() <= 1e-15
    c_cols = cov_mirror(prob, scl, dtype, coverage_table())[0]
    r0 = SC.rho(rec, scl, refined(c_cols))
    assert (r0 == 1.0).all() and refined(c_cols)[..., [9, 22]].tobytes() == scl[..., [9, 22]].tobytes()
    cols = scale_mirror(prob, scl, dtype, scale_table())[0]
    r = scale_bars((K, dtype), rec, scl, cols)
    assert abs(r.max() - MIRROR_WORST[(K, dtype)]) <= 5e-4                 # the figure the bar was pinned from


@pytest.mark.parametrize("K,dtype,sapien", PERTURBED, ids=PERTURBED_IDS)
def test_the_existing_perturbation_still_ends_strictly_lower(K, dtype, sapien):
    """test_refinement_cpu's perturbation (along the ray, tilted) with the 48-value table: cost_best < cost_start for every part and pose; the
    best row is one of the evaluated poses and its cost that pass's; the kept s stays in the fitted s's band."""
    prob, rec, per, cen = problem(K, dtype, sapien)
    table = scale_table()
    cols, sums, bounds, poses = scale_mirror(prob, per, dtype, table)
    behavioural_bars(cols, strict=True)
    assert sums.shape == (int(table[0]) + 1, 3, K, 2, 48) and (sums[..., 46] > 0).all()
    s0, s = per[..., [9, 22]], poses[..., [9, 22]]
    assert (s <= s0 * 1.25 * (1 + 1e-15)).all() and (s >= s0 / 1.25 * (1 - 1e-15)).all() and (np.abs(s[1:] / s[:-1] - 1) <= 0.05 + 1e-15).all()
    for f in range(3):
        for j in range(K):
            for v in range(2):
                b = cols[f, j, 18 * v:18 * v + 18]
                p = int(b[16])
                assert b[:13].tobytes() == poses[p, f, j, 13 * v:13 * v + 13].tobytes() and b[14] == sums[p, f, j, v, 30] and b[15] == sums[p, f, j, v, 28]
                assert sums[p, f, j, v, 30] == CM.cost(sums[p, f, j, v], table)
