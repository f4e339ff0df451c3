"""CPU (no GPU): the ground-truth error entry (ancsh_gt_error_rec) is declared, exported and bound without a new ABI number and checks
its arguments before any launch; the host side refuses bad ground truth, and ground truth on a pipeline built without the option,
before anything touches a device; the numpy mirror the GPU tests compare against (tests/gt_errors_mirror.py) agrees with the reference
restated in oracle/eval_oracle.py and oracle/metrics_oracle.py; pose.evaluation.stream_tables prints the scripts' tables; and
ShardedPipeline hands every gloo rank its shard's rows of the ground truth and gathers the wider rows in global cloud order.

Mirror against oracle.  The oracle gets the ground truth in float64.  The reference stores its ground-truth pickles in float32, which
moves a relative rotation error by up to about 1e-3 degrees; that is the storage format of a file, not arithmetic of the evaluation,
and not the kernel's to imitate.  IoU: intersection and union counts must be EQUAL; the test first shows the demand is fair -- no grid
point of any pair lies within 1e-9 of a face of either of the ORACLE's boxes, so the oracle's own counts do not depend on how a
projection is rounded.  Float columns agree to 1e-9 absolute (float64: d(angle) = d(trace) / (2 sin(angle)), about 2e-10 degrees at
0.01 degrees for a trace good to 1e-15).  Measured here over all cases: the largest difference is 5.2e-11 (a rotation error; the test
prints it)."""
import collections
import ctypes
import datetime
import os
import pickle

import numpy as np
import pytest
import torch.distributed as dist

import gt_errors_mirror as GM
from joint_state_mirror import part_extents
from oracle import eval_oracle as EO
from oracle import metrics_oracle as MO
from test_dist_cpu import _run_ranks
from test_sharded_stream_cpu import CAP, _batches, _expected, _FakeStreamPipeline

HERE = os.path.dirname(os.path.abspath(__file__))
P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


# ---- declared, exported, bound; refusals ---------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    L = _lib.lib()
    assert "ancsh_gt_error_rec" in declared_symbols() and hasattr(L, "ancsh_gt_error_rec")
    assert len(_lib.SIGNATURES["ancsh_gt_error_rec"]) == 13
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def call(b=1, n=64, K=3, nres=50, ldp=3, ld=26, gt=P8, wide=P8):
        return L.ancsh_gt_error_rec(b, n, K, nres, P8, ldp, P8, P8, P8, ld, gt, wide, None)
    for kw, word in ((dict(b=-1), b"b=-1"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(n=0), b"n=0"), (dict(ldp=2), b"ldp=2"),
                     (dict(ld=27), b"ld=27"), (dict(ld=38), b"ld=38"), (dict(nres=1), b"nres=1"), (dict(nres=65), b"nres=65"),
                     (dict(gt=None), b"null pointer"), (dict(wide=None), b"null pointer")):
        assert call(**kw) == -1 and word in L.ancsh_last_error(), kw
    assert L.ancsh_gt_error_rec(0, 64, 3, 50, None, 3, None, None, None, 26, None, None, None) == 0      # nothing to do: nothing enqueued


def test_ground_truth_is_checked_on_the_host():
    from articulated_pose_amd.pose import gt_errors as GE
    assert GE.GT_WIDTH == GM.GT_WIDTH == 19 and GE.GT_ERROR_WIDTH == GM.WIDTH == 12
    assert [GE.ERR_RPY, GE.ERR_XYZ, GE.ERR_SCALE, GE.ERR_IOU, GE.ERR_REL_ROT, GE.ERR_NL_RPY, GE.ERR_NL_XYZ, GE.ERR_NL_SCALE, GE.ERR_NL_IOU,
            GE.ERR_NL_REL_ROT, GE.ERR_NL_REL_TRANS, GE.ERR_POINTS] == list(range(12))
    good = np.zeros((2, 3, 19))
    good[1] = np.nan                                                    # a frame without ground truth is fine
    out = GE.check_ground_truth(good, 2, 3)
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (2, 3, 19)
    for bad, word in ((np.zeros((2, 3, 18)), r"gt must be \(2, 3, 19\)"), (np.zeros((1, 3, 19)), r"gt must be \(2, 3, 19\)"),
                      ("nonsense", "gt must be"), (np.where(np.arange(19) == 4, np.inf, 0.0) * np.ones((2, 3, 1)), r"gt\[0\]\[0\]\[4\] is infinite")):
        with pytest.raises(ValueError, match=word):
            GE.check_ground_truth(bad, 2, 3)
    with pytest.raises(ValueError, match=r"truth\[1\]"):
        GE.check_ground_truth(np.where(np.arange(19) == 4, np.inf, 0.0) * np.ones((2, 3, 1)), 2, 3, name="truth[1]")


def test_pack_ground_truth_reads_the_pickle_shapes():
    from articulated_pose_amd.pose.gt_errors import pack_ground_truth
    rs = np.random.RandomState(0)
    K = 3
    rt = [[np.vstack([rs.normal(size=(3, 4)), [0, 0, 0, 1]]).astype(np.float32) for _ in range(K)] for _ in range(2)]
    rt_g = [[np.vstack([rs.normal(size=(3, 4)), [0, 0, 0, 1]]).astype(np.float32) for _ in range(K)] for _ in range(2)]
    scale = [[np.array([rs.uniform(0.5, 2)], np.float32) for _ in range(K)] for _ in range(2)]
    boxes = [[rs.uniform(0, 1, (2, 1, 3)) for _ in range(K)] for _ in range(2)]
    gt = pack_ground_truth(rt, scale, boxes, rt_g)
    assert gt.shape == (2, K, 19) and gt.dtype == np.float64
    for f in range(2):
        for j in range(K):
            assert np.array_equal(gt[f, j, :9].reshape(3, 3), rt[f][j][:3, :3]) and np.array_equal(gt[f, j, 10:13], rt[f][j][:3, 3])
            assert gt[f, j, 9] == scale[f][j][0] and np.array_equal(gt[f, j, 13:16], boxes[f][j][1][0] - boxes[f][j][0][0])
            assert np.array_equal(gt[f, j, 16:19], rt_g[f][j][:3, 3])
    gt = pack_ground_truth(rt, scale, [np.arange(3 * K, dtype=np.float64).reshape(K, 3), None])      # extents as an array; a frame without
    assert np.isnan(gt[:, :, 16:]).all() and np.isnan(gt[1]).all() and np.array_equal(gt[0, 1, 13:16], [3, 4, 5])
    with pytest.raises(ValueError, match="one entry per frame"):
        pack_ground_truth(rt, scale[:1], boxes)


def test_constructors_and_submit_refuse_before_a_device_is_touched():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    # the constructors check before they build a network or touch a device ("cpu" never reaches a kernel)
    with pytest.raises(ValueError, match="ground_truth=True .* raw_capacity or depth_capacity"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", ground_truth=True)
    with pytest.raises(ValueError, match="ground_truth=True .* raw_capacity"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", ground_truth=True)
    # gt on a pipeline built without the option: AncshPipeline's shared enqueue path refuses right after the front end's own checks
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.K, pipe.B = check_options(raw_capacity=CAP), 3, 2
    front = lambda: (1, np.ones(1, np.float32), None)
    with pytest.raises(ValueError, match="gt needs AncshPipeline"):
        pipe._enqueue(front, None, None, 0, gt=np.zeros((1, 3, 19)))
    pipe.opts = check_options(raw_capacity=CAP, ground_truth=True)
    with pytest.raises(ValueError, match=r"gt must be \(1, 3, 19\)"):
        pipe._enqueue(front, None, None, 0, gt=np.zeros((2, 3, 19)))
    sp = ShardedPipeline(3, None, None, 2, 8, "cpu", pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP)
    with pytest.raises(ValueError, match="gt needs ShardedPipeline"):
        sp.submit([np.ones((3, 4), np.float32)], [1.0], gt=np.zeros((1, 3, 19)))


# ---- the mirror against the oracle ---------------------------------------------------------------------------------------------------
def _rotation(rs, angle_deg=None):
    """A random rotation (angle_deg: about a random axis by that angle), float64."""
    axis = rs.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.radians(rs.uniform(0, 180) if angle_deg is None else angle_deg)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def make_case(seed, K, n, B=1, exact=None, empty=None, nan_pose=None, ld=26):
    """A batch of B random clouds with ground truth, and records 0.01 .. 30 degrees and up to 0.1 away from it.  exact = (c, j, q): pose q
    of that part IS the ground truth (whose R and t are float32 numbers there, so that the float32 rounding of the predicted pose
    changes nothing); empty = (c, j): nobody is predicted to belong to that part; nan_pose = (c, j, q, column): a NaN in that pose."""
    rs = np.random.RandomState(seed)
    P = rs.uniform(-1, 1, (B, n, 3)).astype(np.float32)
    nocs = rs.uniform(0.05, 0.95, (B, n, 3 * K)).astype(np.float32)
    mask = rs.uniform(0, 1, (B, n, K)).astype(np.float32)
    if empty is not None:
        mask[empty[0], :, empty[1]] = -1.0
    gt = np.zeros((B, K, 19))
    rec = rs.normal(size=(B, K, ld))
    for c in range(B):
        for j in range(K):
            R, t = _rotation(rs), rs.uniform(-0.5, 0.5, 3)
            if exact is not None and exact[:2] == (c, j):
                R, t = R.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
            lo = rs.uniform(0.05, 0.35, 3)
            box = np.array([[lo], [lo + rs.uniform(0.3, 0.6, 3)]])                  # a corner table: [[min corner], [max corner]]
            gt[c, j] = np.concatenate([R.reshape(9), [rs.uniform(0.5, 1.5)], t, box[1][0] - box[0][0], rs.uniform(-0.5, 0.5, 3)])
            for q in range(2):
                ang = 10.0 ** rs.uniform(-2, np.log10(30.0))
                d = rs.normal(size=3)
                d *= rs.uniform(0, 0.1) / np.linalg.norm(d)
                pose = np.concatenate([(_rotation(rs, ang) @ R).reshape(9), [gt[c, j, 9] + rs.uniform(-0.1, 0.1)], t + d])
                if exact == (c, j, q):
                    pose = gt[c, j, :13].copy()
                rec[c, j, 13 * q:13 * q + 13] = pose
    if nan_pose is not None:
        c, j, q, col = nan_pose
        rec[c, j, 13 * q + col] = np.nan
    return P, nocs, mask, rec, gt


def oracle_numbers(P, nocs, mask, rec, gt):
    """One cloud through the oracle -> ({(j, q): [rpy, xyz, scale, (I, U) | None, clearance]}, {q: rows of relative rotation errors},
    rows of the nonlinear relative translation error)."""
    K = rec.shape[0]
    rt_gt = [np.vstack([np.hstack([gt[j, :9].reshape(3, 3), gt[j, 10:13].reshape(3, 1)]), [0, 0, 0, 1]]) for j in range(K)]
    rt_gn = [np.vstack([np.hstack([np.eye(3), gt[j, 16:19].reshape(3, 1)]), [0, 0, 0, 1]]) for j in range(K)]
    s_gt = [np.array([gt[j, 9]]) for j in range(K)]
    bbox_gt = [np.array([[np.zeros(3)], [gt[j, 13:16]]]) for j in range(K)]      # only the corner difference is read: exactly the extent
    frame = dict(nocs=nocs, P=P, instance_per_point=mask)
    per, datas, boundary = {}, {"pn_gt": {"f": dict(rt={"gt": rt_gt}, scale={"gt": s_gt})}, "gn_gt": {"f": dict(rt={"gt": rt_gn})}}, {}
    for q, key in enumerate(EO.KEYS):
        r = [rec[j, 13 * q:13 * q + 9].reshape(3, 3) for j in range(K)]
        s = [rec[j, 13 * q + 9] for j in range(K)]
        t = [rec[j, 13 * q + 10:13 * q + 13] for j in range(K)]
        datas[key] = {"f": dict(scale={key: s}, rotation={key: r}, translation={key: t})}
        for j in range(K):
            per[(j, q)] = [MO.rot_diff_degree(r[j], rt_gt[j][:3, :3]), np.linalg.norm(t[j] - rt_gt[j][:3, 3]), abs(s[j] - s_gt[j][0]), None, np.inf]
        try:                                                              # the scripts' bare except: a part without points raises
            fp = EO.frame_parts(frame, r, t, s, s_gt, bbox_gt, K)
        except ValueError:
            fp = None
        if fp is not None:
            for j in range(K):
                rt2 = EO.compose_rt(r[j], t[j])
                b1 = np.dot(fp["box_gt"][j] * s_gt[j][0], rt_gt[j][:3, :3].T) + rt_gt[j][:3, 3]
                b2 = np.dot(fp["box_pred"][j] * s[j], rt2[:3, :3].T) + rt2[:3, 3]
                _, I, U = MO.iou_3d(b1, b2, return_counts=True)
                per[(j, q)][3:] = [(I, U), GM.iou_counts(b1, b2, 50, True)[2]]
        # the boundary is the part pass's (pinned against the oracle's float32 pinv to 1e-6 by the joint-state tests): relative_errors
        # combines it with the ground truth, and that combination is what is compared here
        sc, dy, cnt = part_extents(P, nocs, mask, rec[0, 13:22].reshape(3, 3), rec[0, 23:26])
        boundary[key] = {"f": dict(canon=list(-sc[:, 0] / np.float32(2) + np.float32(0.5)), dynam=list(dy))}
    r_out, t_out = EO.relative_errors(datas, boundary, K)
    return per, {q: r_out[key] for q, key in enumerate(EO.KEYS)}, t_out["nonlinear"]


CASES = [dict(seed=100 + 10 * K + i, K=K, n=n) for K in (1, 2, 3) for i, n in enumerate((1, 64, 257))]
CASES[4].update(exact=(0, 1, 1))            # K = 2, n = 64: the nonlinear pose of part 1 is the ground truth
CASES[7].update(empty=(0, 2))               # K = 3, n = 64: part 2 has no points
CASES[8].update(nan_pose=(0, 1, 0, 4))      # K = 3, n = 257: a NaN in the baseline pose of part 1


@pytest.fixture(scope="module")
def worst():
    w = dict(v=0.0)
    yield w
    print("gt errors: max |mirror - oracle| over the float columns = %.3g" % w["v"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "K%d-n%d" % (c["K"], c["n"]))
def test_mirror_against_the_oracle(case, worst):
    P, nocs, mask, rec, gt = make_case(**case)
    K = case["K"]
    wide, counts = GM.gt_error_reference(P, nocs, mask, rec, gt, 50, return_counts=True)
    assert wide.shape == (1, K, 38) and np.array_equal(wide[:, :, :26].view(np.int64), rec.view(np.int64))
    lab = np.argmax(mask[0], 1)
    assert np.array_equal(wide[0, :, 37], [np.sum(lab == j) for j in range(K)])
    if case.get("nan_pose"):
        # the reference never sees such a frame (its NaN test drops it): the NaN rules alone
        c, j, q, _ = case["nan_pose"]
        assert np.isnan(wide[c, j, 26 + 5 * q:31 + 5 * q]).all() and np.isfinite(wide[c, j, 31 - 5 * q:36 - 5 * q]).all()
        assert np.isfinite(wide[c, 0, 26:30]).all() and np.isfinite(wide[c, 2, 26:36]).all() and np.isfinite(wide[c, 1:, 36]).all()
        rec = rec.copy()
        rec[c, j, 13 * q + case["nan_pose"][3]] = 0.5                  # the other parts' numbers go through the oracle below
        keep = [(jj, qq) for jj in range(K) for qq in range(2) if (jj, qq) != (j, q)]
    else:
        keep = [(j, q) for j in range(K) for q in range(2)]
    per, r_rel, t_rel = oracle_numbers(P[0], nocs[0], mask[0], rec[0], gt[0])
    diff = lambda a, b: 0.0 if (np.isnan(a) and np.isnan(b)) else abs(a - b)
    for j, q in keep:
        rpy, xyz, sc, cnt, clear = per[(j, q)]
        e = wide[0, j, 26 + 5 * q:31 + 5 * q]
        for got, want in ((e[0], rpy), (e[1], xyz), (e[2], sc)):
            worst["v"] = max(worst["v"], diff(got, want))
            assert diff(got, want) <= 1e-9, (j, q, got, want)
        if cnt is None:                                                  # the oracle raised (the scripts drop the frame): some part has no points
            assert np.isnan(e[3]) == (wide[0, j, 37] == 0) and ((0, j, q) in counts) == (wide[0, j, 37] > 0)
            continue
        assert clear > 1e-9, (j, q, clear)                               # the oracle's own counts are implementation-independent here
        assert counts[(0, j, q)][:2] == cnt, (j, q, counts[(0, j, q)], cnt)
        assert e[3] == (1.0 if cnt[1] == 0 else cnt[0] / cnt[1])
    for q in range(2):
        if case.get("nan_pose") and case["nan_pose"][2] == q:
            continue
        for j in range(1, K):
            got, want = wide[0, j, 30 + 5 * q], r_rel[q][0][j - 1]
            worst["v"] = max(worst["v"], diff(got, want))
            assert diff(got, want) <= 1e-9, (j, q, got, want)
    assert np.isnan(wide[0, 0, [30, 35, 36]]).all()                      # row 0 has no joint
    for j in range(1, K):
        got, want = wide[0, j, 36], t_rel[0][j - 1]
        worst["v"] = max(worst["v"], diff(got, want))
        assert diff(got, want) <= 1e-9, (j, got, want)
        if case.get("empty") and case["empty"][1] == j:
            assert np.isnan(got) and np.isnan(wide[0, j, [29, 34]]).all()
    if case.get("exact"):
        _, j, q = case["exact"]
        assert wide[0, j, 27 + 5 * q] == 0.0 and wide[0, j, 28 + 5 * q] == 0.0      # xyz_err and scale_err of the exact pose


def test_mirror_nan_rules_and_the_wide_record():
    """Everything the header says about NaN, on the mirror: ground truth without NAOCS translations, a frame without ground truth, a NaN
    in part 0's pose, and the 39-column input row."""
    P, nocs, mask, rec, gt = make_case(7, 3, 40, B=2, ld=39)
    gt[0, :, 16:] = np.nan                                               # cloud 0: pack_ground_truth without rt_naocs
    gt[1, 2] = np.nan                                                    # cloud 1: part 2 has no ground truth
    rec[1, 0, 13 + 9] = np.nan                                           # cloud 1: a NaN in part 0's nonlinear pose
    rec[0, 1, 30] = np.float64(np.frombuffer(np.uint64(0x7ff8000000001234).tobytes(), np.float64)[0])      # a NaN payload in the carried row
    w = GM.gt_error_reference(P, nocs, mask, rec, gt, 7)
    assert w.shape == (2, 3, 51) and np.array_equal(w[:, :, :39].view(np.uint64), rec.view(np.uint64))
    assert np.isnan(w[0, :, 49]).all() and np.isfinite(w[0, :, 39:43]).all() and np.isfinite(w[0, 1:, [43, 48]]).all()
    assert np.isnan(w[1, 2, 39:50]).all() and w[1, 2, 50] > 0             # no ground truth: every error column, not the point count
    assert np.isnan(w[1, 0, 44:50]).all() and np.isfinite(w[1, 0, 39:43]).all()      # the poisoned pose's own columns
    assert np.isnan(w[1, 1, [48, 49]]).all() and np.isfinite(w[1, 1, 39:48]).all()     # part 0's NaN blanks the relative columns of every row
    w1 = GM.gt_error_reference(P[:, :, :], nocs[:, :, :3], mask[:, :, :1], rec[:, :1], gt[:, :1], 7)
    assert w1.shape == (2, 1, 51) and np.isnan(w1[:, 0, [43, 48, 49]]).all() and np.array_equal(w1[:, 0, 50], [40, 40])      # K = 1: row 0 only


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def scripts_rows(name):
    """The (F, K, 38) streamed rows of a fixture's records -- the poses of the pickles, the errors the scripts computed from them -- and what
    the tables are compared with: -> (G, K, rows, error_skip, (r_raw, t_raw, iou_rat, r_diff, t_diff))."""
    from test_eval_scripts_cpu import boxes_of, datas_of, loader_of
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        G = pickle.load(f)
    K, info, datas, load = G["info"]["num_parts"], G["info"], datas_of(G), loader_of(G)
    skip = ("45841",)
    r_raw, t_raw = EO.raw_errors(datas, skip_instances=skip)
    iou_rat, bnd = EO.miou(datas, load, info["baseline"], boxes_of(G), K)
    r_diff, t_diff = EO.relative_errors(datas, bnd, K)
    names = list(datas["nonlinear"])
    assert all(list(datas[k]) == names for k in EO.KEYS)                 # one row per frame serves both keys
    rows = np.full((len(names), K, 38), np.nan)
    rows[:, :, 37] = 1.0
    for q, key in enumerate(EO.KEYS):
        boxed = [b for b in names if b in bnd[key]]
        assert len(boxed) == len(iou_rat[key]) == len(r_diff[key])
        for f, b in enumerate(names):
            rec = datas[key][b]
            if rec["scale"] is None:                                     # a failed fit: the poisoned record
                continue
            for j in range(K):
                rows[f, j, 13 * q:13 * q + 9] = np.asarray(rec["rotation"][key][j]).reshape(9)
                rows[f, j, 13 * q + 9] = np.asarray(rec["scale"][key][j]).reshape(-1)[0]
                rows[f, j, 13 * q + 10:13 * q + 13] = np.asarray(rec["translation"][key][j]).reshape(3)
            rows[f, :, 26 + 5 * q] = rec["rpy_err"][key]
            rows[f, :, 27 + 5 * q] = rec["xyz_err"][key]
            if b in boxed:
                i = boxed.index(b)
                rows[f, :, 29 + 5 * q] = iou_rat[key][i]
                rows[f, 1:, 30 + 5 * q] = r_diff[key][i]
                if key == "nonlinear":
                    rows[f, 1:, 36] = t_diff[key][i]
    return G, K, rows, [b.split("_")[0] in skip for b in names], (r_raw, t_raw, iou_rat, r_diff, t_diff)


@pytest.mark.parametrize("name", ["eval_scripts.pkl", "eval_scripts_drawer.pkl"])
def test_stream_tables_print_the_scripts_tables(name):
    """Rows built from the fixture's records -- the poses of the pickles, the errors the scripts computed from them -- give the lines the
    product's error_report, miou_report and relative_report give on the same records (and those are pinned against the scripts' own
    output by tests/test_eval_scripts_cpu.py)."""
    from articulated_pose_amd.pose import evaluation as EV
    G, K, rows, error_skip, (r_raw, t_raw, iou_rat, r_diff, t_diff) = scripts_rows(name)
    lines = EV.stream_tables(rows, K, G["item"], G["domain"], "ANCSH", error_skip=error_skip)
    t_want = dict(t_diff, baseline=np.full((len(t_diff["baseline"]), K - 1), np.nan).tolist())      # not streamed for the baseline pose
    want = (EV.error_report(r_raw, t_raw, K, G["domain"], "ANCSH", device="cpu") + EV.miou_report(iou_rat, K, G["domain"], "ANCSH") +
            EV.relative_report(r_diff, t_want, K, G["item"], G["domain"], "ANCSH"))
    assert lines == want
    assert sum(l.startswith("For ") for l in lines) == 6 and len(lines) == 6 * 4
    with pytest.raises(ValueError, match="rows must be"):
        EV.stream_tables(rows[:, :, :37], K, G["item"], G["domain"])


# ---- ShardedPipeline, two gloo ranks, a stand-in per-rank pipeline ------------------------------------------------------------------------
class _FakeGtPipeline(_FakeStreamPipeline):
    """The stand-in stream with 38-wide records: _FakeStreamPipeline's 26 columns, then the first 12 numbers of the ground-truth row the
    rank was handed for that cloud and part (NaN without ground truth)."""

    def __init__(self, *a, ground_truth=False, **kw):
        assert ground_truth                                             # what ShardedPipeline(ground_truth=True) must pass
        super().__init__(*a, **kw)
        self._gts = collections.deque()

    def submit(self, clouds, norm_factors, seed=None, tag=None, cloud_base=0, gt=None):
        from articulated_pose_amd.pose.gt_errors import check_ground_truth
        gt = np.full((len(clouds), self.K, 19), np.nan) if gt is None else check_ground_truth(gt, len(clouds), self.K)
        super().submit(clouds, norm_factors, seed=seed, tag=tag, cloud_base=cloud_base)
        self._gts.append(gt)

    def retire(self, flags=False):
        out = super().retire(flags)
        return out[:2] + (np.concatenate([out[2], self._gts.popleft()[:, :, :12]], axis=2),) + out[3:]


def _gt_of(k, n, K):
    """The ground truth of global batch k: entry e of cloud c, part j = 1e4 k + 100 c + 10 j + e / 100."""
    return 1e4 * k + 100 * np.arange(n)[:, None, None] + 10 * np.arange(K)[None, :, None] + np.arange(19)[None, None, :] / 100.0


def _gt_batches(G, K):
    sizes = [G, G - 1, 1, G]
    return [(clouds, nf, None if k == 2 else _gt_of(k, len(clouds), K), tag) for k, (clouds, nf, tag) in enumerate(_batches(G, sizes))]


def _gt_worker(rank, world, port, G, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import articulated_pose_amd  # noqa: F401
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from articulated_pose_amd.dist import ShardedPipeline
    K = 3
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeGtPipeline, raw_capacity=CAP, seed=10, ground_truth=True)
    assert sp.record_width == 38
    calls = []
    real = dist.gather
    dist.gather = lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1]
    try:
        got = list(sp.stream_batches(_gt_batches(G, K)))
    finally:
        dist.gather = real
    assert calls == [(sp.n_max, K, 38)] * 4                            # still one gather a batch
    try:                                                               # a bad ground truth is refused on every rank, whoever's shard it hits
        sp.submit(*_batches(G, [G])[0][:2], gt=np.zeros((G - 1, K, 19)))
        raise AssertionError("not refused")
    except ValueError as e:
        assert "gt must be (%d, %d, 19)" % (G, K) in str(e)
    if rank == sp.dst:
        q.put(got)
    else:
        assert all(g[2] is None for g in got)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_stream_hands_out_ground_truth_rows_and_gathers_in_global_order():
    G, K = 5, 3
    got = _run_ranks(_gt_worker, (G,), world=2)
    batches = _gt_batches(G, K)
    assert len(got) == len(batches)
    for k, (item, (clouds, nf, gt, tag)) in enumerate(zip(got, batches)):
        assert item[0] == tag and item[1] == 10 + 2 * k and len(item) == 3
        assert item[2].shape == (len(clouds), K, 38) and item[2].flags.c_contiguous
        np.testing.assert_array_equal(item[2][:, :, :26], _expected(clouds, nf, 10 + 2 * k, K))
        if gt is None:
            assert np.isnan(item[2][:, :, 26:]).all()
        else:
            np.testing.assert_array_equal(item[2][:, :, 26:], gt[:, :, :12])      # cloud c's row came from cloud c's ground truth
