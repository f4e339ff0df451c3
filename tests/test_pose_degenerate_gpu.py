"""Every stage-A hypothesis' score on rank-deficient 3-point samples, through the product entry (ransac_single_batch returns the
inlier count of each hypothesis): samples with a repeated index, samples on a line, and -- two-sided -- well-conditioned samples.
The goldens pin only the winner, which is refitted with the Jacobi Horn; the 3-point models come from horn_quat_fast, whose
rank-<=1 branch these inputs reach.  The bounds are geometry or a float64 SVD-Kabsch model (tests/pose_degenerate_cases.py), and
test_pose_degenerate_cpu.py shows that the reference arithmetic meets every one of them on the same inputs.

On the commit before the rank-1 sign was fixed (DESIGN.md "Rank-1 samples"), on the MI355X:
  collinear parts    566 of 32768 hypotheses scored below 24 (lowest 1), in 8 of the 16 problems
  general parts      151 of 13248 hypotheses scored below the lower bound, some in each of the 8 problems
  the other two tests passed (well-conditioned: 2815 hypotheses checked, 27 with a point inside the window)."""
import numpy as np
import pytest
import torch

import pose_degenerate_cases as C

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_both(dev, b, draws):
    """both scoring kernels; their score arrays must be equal bit for bit -> the scalar-points result"""
    from articulated_pose_amd.pose import ransac_single_batch
    n = int(np.diff(b["off"]).max())
    r = [ransac_single_batch(T(b["off"], dev), T(b["src"], dev), T(b["tgt"], dev), C.TH, draws.shape[1], draws, max_n=n, scalar_points=sp)
         for sp in (True, False)]
    assert torch.equal(r[0]["scores"], r[1]["scores"]) and torch.equal(r[0]["best"], r[1]["best"])
    assert torch.equal(r[0]["inliers"], r[1]["inliers"])
    return r[0]


def test_collinear_parts_every_hypothesis_scores_all_points(dev):
    """every optimal rotation of a sample on the line maps the whole line correctly: all 16 x 2048 scores are 24, the mask is all ones
    and the refit recovers the direction and the scale."""
    b = C.collinear_batch()
    r = run_both(dev, b, b["draws"])
    sc = r["scores"].cpu().numpy()
    print(f"collinear: {int((sc < C.N_SMALL).sum())} of {sc.size} hypotheses below {C.N_SMALL}, min {int(sc.min())}, "
          f"per problem {(sc < C.N_SMALL).sum(1).tolist()}")
    assert (sc == C.N_SMALL).all(), (int((sc < C.N_SMALL).sum()), int(sc.min()))
    assert (r["best"].cpu().numpy()[:, 1] == C.N_SMALL).all()
    assert bool(r["inliers"].cpu().numpy().all())
    m = r["model"].cpu().numpy()
    for k, p in enumerate(b["problems"]):
        R, s = m[k, :9].reshape(3, 3), m[k, 9]
        assert np.abs(R @ p["u"] - p["R"] @ p["u"]).max() <= 1e-5, k
        assert abs(s - p["s"]) <= 1e-5 and abs(np.linalg.det(R) - 1) <= 1e-6, k


def test_thrice_repeated_index_scores_the_neighbours_of_one_target(dev):
    """(i,i,i): R = I, scale 0, t = tgt_i in the reference, so the score counts the targets within th of tgt_i"""
    b = C.collinear_batch()
    sc = run_both(dev, b, b["same"])["scores"].cpu().numpy()
    for k, p in enumerate(b["problems"]):
        lo, hi = C.same_index_window(p["tgt"])
        assert (lo <= sc[k]).all() and (sc[k] <= hi).all(), (k, sc[k].tolist(), lo.tolist(), hi.tolist())


def test_general_parts_repeated_index_keeps_the_sample_line(dev):
    """a sample (i,i,j) fixes only the line through src_i and src_j; a member of the optimal family spins the rest about it by an unknown
    angle, which moves a point at distance d from the line by at most 2 s d.  So at least the points with 2 s d < th - 1e-3 are inliers
    (the two sample points among them).  The rotation that minimises tr(R^T M) instead mirrors the part about the sample's centroid."""
    b = C.general_batch()
    sc = run_both(dev, b, b["draws"])["scores"].cpu().numpy()
    short = sc < b["lower"]
    print(f"general: {int(short.sum())} of {sc.size} hypotheses below the lower bound, per problem {short.sum(1).tolist()}, "
          f"mean slack {float((sc - b['lower']).mean()):.2f}")
    assert not short.any(), (int(short.sum()), np.argwhere(short)[:5].tolist())


def test_well_conditioned_samples_score_inside_the_float64_window(dev):
    """three distinct points, sigma2/sigma1 >= 0.05 on both sides: the count of the float64 SVD-Kabsch model at th -+ 1e-4 brackets
    the kernel's score, for every such hypothesis (2815 of the 3000 drawn; the rest repeat an index or are nearly collinear)."""
    b = C.noisy_batch()
    sc = run_both(dev, b, b["draws"])["scores"].cpu().numpy()
    use = b["use"]
    assert 1.0 - use.mean() <= 0.10
    ok = (b["lo"] <= sc) & (sc <= b["hi"])
    print(f"well-conditioned: {int(use.sum())} hypotheses checked, {int((~ok & use).sum())} outside the window, "
          f"{int(((b['hi'] > b['lo']) & use).sum())} with a non-empty window")
    assert ok[use].all(), np.argwhere(~ok & use)[:5].tolist()
