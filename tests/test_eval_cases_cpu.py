"""CPU: the evaluation kernels' case builder and float64 reference (tests/eval_cases.py) against the project's other two statements of the
same lines -- oracle/joint_params_oracle.py (numpy float32, the reference file's own order) and tests/golden/joint_params.npz (the
reference file's lines executed) -- and the builder's claims (vote counts, layouts, shape coverage) against what np.where finds."""
import warnings

import numpy as np
import pytest

import eval_cases as EC
from test_joint_params_cpu import G as GOLDEN, cases, load

SEEDS = range(40)


@pytest.fixture(scope="module")
def built():
    return {s: EC.make_case(s) for s in SEEDS}


def test_shapes_cover_their_lists(built):
    sh = [EC.shape_of(s) for s in SEEDS]
    assert {v["n"] for v in sh} == set(EC.N_LIST) and {v["K"] for v in sh} == set(EC.K_LIST) and {v["B"] for v in sh} == {1, 2, 3, 4, 5}
    assert {v["G"] == 3 for v in sh if v["K"] > 1} == {True, False}
    for pick in range(4):
        assert any((s // 2) % 4 == pick and sh[s]["K"] > 1 for s in SEEDS)
    assert any(v["n"] == 4096 and v["B"] == 5 for v in sh)                       # the largest case
    votes = [v for s in SEEDS for v in built[s]["votes"]]
    assert {v["layout"] for v in votes if v["count"]} == set(EC.LAYOUTS)
    counts = {v["count"] for v in votes}
    assert {0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513} <= counts
    assert any(v["count"] == built[s]["n"] >= 1000 for s in SEEDS for v in built[s]["votes"])     # a joint that holds a whole large cloud


@pytest.mark.parametrize("seed", SEEDS)
def test_builder_places_what_it_states(built, seed):
    c = built[seed]
    n, K, JC = c["n"], c["K"], c["JC"]
    jc = np.argmax(c["index"], axis=2)
    assert len(c["votes"]) == c["B"] * (K - 1)
    for v in c["votes"]:
        b, j, msg = v["cloud"], v["joint"], EC.describe(c, v["cloud"], v["joint"])
        idx = np.where(jc[b] == j)[0]
        assert len(idx) == v["count"] and np.array_equal(idx, v["idx"]), msg
        assert np.array_equal(np.where(c["joint_cls"][b] == j)[0], idx), msg
        if v["count"] == 0:
            continue
        assert j < JC, msg
        run = np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))
        if v["layout"] == "run64":
            assert run and idx[0] % 64 == 0, msg
        elif v["layout"] == "straddle256":
            assert run and idx[0] // 256 != idx[-1] // 256, msg
        elif v["layout"] == "tail":
            assert run and idx[-1] == n - 1, msg
    assert sum(v["count"] for v in c["votes"] if v["cloud"] == 0) <= n
    for b in range(1, c["B"], 2):                                                 # labels outside 1..K-1 exist in odd clouds (when points are left)
        spare = int(((jc[b] == 0)).sum())
        if spare >= 3:
            assert {-1, K} <= set(c["joint_cls"][b].tolist()), seed
    lab = EC.labels_of(c["mask"])
    if K > 1:
        assert (lab[0] != K - 1).all()                                            # cloud 0: the last part is empty
    if K >= 3 and n >= 3 + K - 2 and c["B"] > 1:
        assert (lab[1] == 1).sum() == 1 and (lab[1] == 2).sum() == 2
    ties = c["mask"][:, ::7]
    assert (ties.max(-1) == 0.5).all() and (K == 1 or n < 64 or ((ties == 0.5).sum(-1) == 2).any())      # every 7th row: a tie at the top
    assert not EC.badly_conditioned(c) and len(c["redrawn"]) <= max(1, c["B"] * K // 20)
    if c["quantised"] and K > 1:
        ref = EC.reference(c)
        for name in ("joint_pt", "joint_axis", "gt_joint_pt"):
            fin = ref[name][np.isfinite(ref[name])]
            assert (fin * 16 == np.round(fin * 16)).all(), seed                   # medians of multiples of 1/8


def _oracle(c, b):
    from oracle import joint_params_oracle as JO
    K = c["K"]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                                           # empty parts / joints: numpy warns and gives NaN
        st = JO.st_and_joints(c["gocs"][b], c["nocs"][b], c["mask"][b], c["heatmap"][b], c["unitvec"][b], c["joint_axis"][b],
                              np.argmax(c["index"][b], axis=1), K)
        gt = JO.gt_joints(c["gocs"][b, :, :3], c["heatmap"][b], c["unitvec"][b], c["joint_axis"][b], c["joint_cls"][b], K) if K > 1 else None
    return st, gt


def test_oracle_gives_the_reference_medians_exactly_and_its_scale_within_ulps(built, capsys):
    worst, exact, parts = 0, 0, 0
    for seed in SEEDS:
        c = built[seed]
        ref = EC.reference(c)
        for b in range(c["B"]):
            (sc, _tr, pts, axes), gt = _oracle(c, b)
            msg = EC.describe(c, b)
            if c["K"] > 1:
                np.testing.assert_array_equal(pts, ref["joint_pt"][b], err_msg=msg)
                np.testing.assert_array_equal(axes, ref["joint_axis"][b], err_msg=msg)
                np.testing.assert_array_equal(gt[0], ref["gt_joint_pt"][b], err_msg=msg)
                np.testing.assert_array_equal(gt[1], ref["gt_joint_axis"][b], err_msg=msg)
            want = ref["scale"][b]
            assert np.array_equal(np.isfinite(sc), np.isfinite(want)), msg
            fin = np.isfinite(want)
            d = EC.ulps(sc[fin], want[fin])
            parts += int(fin.sum())
            exact += int((d == 0).sum())
            worst = max(worst, int(d.max()) if d.size else 0)
    with capsys.disabled():
        print("\noracle (numpy float32) scale vs float64 reference over %d seeds: worst %d float32 ulp, %d of %d parts exact"
              % (len(SEEDS), worst, exact, parts))
    assert worst <= 8                                   # "a few ulps": information, the kernels' bar is in the GPU file


def golden_case(c, gt=False):
    """one golden sample as a batch of one in the builder's layout (the NPCS heads, the points and the record play no part here)"""
    n, K = c["mask_pred"].shape
    one = lambda a: np.ascontiguousarray(a, np.float32)[None]
    case = dict(seed=-1, n=n, K=K, B=1, JC=c["index_per_point"].shape[1], votes=[], mask=one(c["mask_pred"]), nocs=one(c["nocs"]),
                index=one(c["index_per_point"]), npcs_nocs=one(c["nocs"]), npcs_mask=one(c["mask_pred"]), P=np.zeros((1, n, 3), np.float32),
                record=np.tile(np.concatenate([np.eye(3).reshape(9), [1.0, 0, 0, 0]] * 2), (1, K, 1)))
    src = ("nocs_gt_g", "heatmap_gt", "unitvec_gt", "orient_gt") if gt else ("gocs", "heatmap_pred", "unitvec_pred", "orient_pred")
    case.update(gocs=one(c[src[0]]), heatmap=one(c[src[1]]).reshape(1, n), unitvec=one(c[src[2]]), joint_axis=one(c[src[3]]),
                joint_cls=np.asarray(c["joint_cls_gt"]).reshape(1, n).astype(np.int32))
    case["G"] = case["gocs"].shape[2]
    return case


@pytest.mark.parametrize("tag", cases())
def test_reference_gives_the_golden_values(tag):
    with np.load(GOLDEN) as z:
        c = load(z, tag)
    ref = EC.reference(golden_case(c))
    np.testing.assert_array_equal(ref["joint_pt"][0], c["joint_p_pred"])
    np.testing.assert_array_equal(ref["joint_axis"][0], c["joint_l_pred"])
    np.testing.assert_allclose(ref["scale"][0], c["st_scale"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(ref["translation"][0], c["st_translation"], rtol=0, atol=1e-6)
    gt = EC.reference(golden_case(c, gt=True))
    np.testing.assert_array_equal(gt["gt_joint_pt"][0], c["joint_p_gt"])
    np.testing.assert_array_equal(gt["gt_joint_axis"][0], c["joint_l_gt"])
