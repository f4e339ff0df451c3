"""The bounds of test_pose_degenerate_gpu.py, held to the reference arithmetic (oracle/pose_oracle.py: transform_pts with LAPACK's SVD,
the float32 verifier) on the very same inputs: what the kernels are asked for there is what the reference delivers here, so the bounds
are pinned by the reference and not by the kernels."""
import numpy as np
import pytest

import pose_degenerate_cases as C
from oracle import pose_oracle as PO


def ref_scores(p, draws):
    ds = dict(source=p["src"], target=p["tgt"], nsource=len(p["src"]))
    out = np.empty(len(draws), np.int64)
    for h, d in enumerate(draws):
        model = PO.single_transformation_estimator(ds, d)
        out[h] = np.count_nonzero(PO.single_transformation_verifier(ds, model, C.TH)[1])
    return out


def test_reference_scores_every_point_of_a_collinear_part():
    b = C.collinear_batch()
    assert b["draws"].shape == (16, 2048, 3)
    for k, p in enumerate(b["problems"]):
        assert np.diff(np.sort((p["src"].astype(np.float64) - p["src"][0]) @ p["u"])).min() >= 0.04 - 1e-6       # 0.05 k + U[0, 0.01)
        sc = ref_scores(p, p["draws"])
        assert (sc == C.N_SMALL).all(), (k, int(sc.min()), int((sc < C.N_SMALL).sum()))
        R, s, _ = PO.transform_pts(p["src"], p["tgt"])                    # the refit on the full consensus set
        assert np.abs(R @ p["u"] - p["R"] @ p["u"]).max() <= 1e-5 and abs(s - p["s"]) <= 1e-5 and abs(np.linalg.det(R) - 1) <= 1e-6, k


def test_reference_on_a_thrice_repeated_index():
    b = C.collinear_batch()
    for k, p in enumerate(b["problems"]):
        lo, hi = C.same_index_window(p["tgt"])
        sc = ref_scores(p, b["same"][k])
        assert (lo <= sc).all() and (sc <= hi).all(), k
        assert (lo >= 1).all() and (hi < C.N_SMALL).all()                 # the bound says something


def test_reference_keeps_the_sample_line_on_general_parts():
    b = C.general_batch()
    viol = tot = 0
    slack = []
    for k, p in enumerate(b["problems"]):
        sc = ref_scores(p, p["draws"])
        viol += int((sc < b["lower"][k]).sum())
        tot += len(sc)
        slack.append(sc - b["lower"][k])
    assert tot == 8 * 1656 and viol == 0, (viol, tot, float(np.mean(slack)))


def test_reference_inside_the_float64_window_on_well_conditioned_samples():
    b = C.noisy_batch()
    use = b["use"]
    skipped = 1.0 - use.mean()
    assert skipped <= 0.10, skipped                                      # repeated indices and sigma2/sigma1 < 0.05 together
    assert int((b["hi"] > b["lo"])[use].sum()) >= 10                     # hypotheses with a point inside the window exist
    for k, p in enumerate(b["problems"]):
        sc = ref_scores(p, p["draws"])
        ok = (b["lo"][k] <= sc) & (sc <= b["hi"][k])
        assert ok[use[k]].all(), (k, np.flatnonzero(~ok & use[k])[:5])
