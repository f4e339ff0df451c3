"""GPU: the pose fit on TINY parts (1..12 predicted points) at the reference's budgets (10000 hypotheses per part, 200 per joint),
where RANSAC is fragile: most 3-point draws of a 4-point part repeat an index, so hundreds of hypotheses are degenerate contenders.

  a. parity with the reference arithmetic (oracle/pose_oracle.py on replayed draws, bars of oracle/pose_compare.py, own-mask refit
     of every fit that ends on another consensus set); the record is [baseline | nonlinear]; an empty part gives NaN rows;
  b. stage A's tie[..., 1] against the host recount of its contenders (pose_compare.stage_a_contenders): the sign is exact, the
     magnitude within [wd + max(c - 16, 0), wd + c]; both scoring kernels and a repeated call give the same bytes;
  c. stage B's tie[..., 1] equals pose_compare.stage_b_contenders exactly;
  d. the device-drawn paths (seed_dev, and key_dev shards with cloud_base) give the same bytes whole, sharded and repeated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NA, NB = 10000, 200                 # the reference's budgets (evaluation/parallel_ancsh_pose.py:262,299)
SEED0 = 100

# (cloud id, N, K, joint type, {part: predicted points kept}, kind of the kept points: oracle/pose_compare.py::squeezed_problem)
SPECS = [
    (41, 512, 2, "revolute", {1: 4}, "plain"),
    (42, 512, 2, "prismatic", {1: 1}, "plain"),
    (43, 512, 3, "revolute", {1: 2, 2: 5}, "plain"),
    (44, 1024, 3, "revolute", {2: 7}, "coincident"),
    (45, 512, 4, "prismatic", {1: 3, 3: 12}, "plain"),
    (46, 1024, 4, "revolute", {2: 5}, "collinear"),
    (47, 512, 3, "revolute", {1: 4, 2: 12}, "unrelated"),
    (48, 512, 2, "revolute", {1: 7}, "unrelated"),
    (49, 512, 4, "revolute", {1: 12, 3: 4}, "coincident"),
    (50, 1024, 2, "prismatic", {1: 4}, "collinear"),
    (51, 512, 3, "prismatic", {1: 5, 2: 3}, "unrelated"),
]


def _spec_kw(spec):
    return dict(joint_type=spec[3], keep=spec[4], kind=spec[5])


def _inputs(spec):
    from oracle import pose_compare as PC
    cid, N, K = spec[:3]
    c, p = PC.squeezed_problem(cid, N, K, **_spec_kw(spec))
    counts = np.bincount(np.argmax(p["instance_per_point"], 1), minlength=K)
    assert all(counts[j] == m for j, m in spec[4].items()), (spec, counts)
    da, db = PC.replay_draws(SEED0 + cid, counts, NA, NB)
    return c, p, da, db


def _solve(dev, c, p, K, da, db):
    from articulated_pose_amd.pose import PoseSolver
    sol = PoseSolver(K, 0.1, NA, NB, dev, lm_schedule="throughput").solve(
        c["P"][None], p["nocs_per_point"][None], p["instance_per_point"][None], p["joint_axis_per_point"][None],
        p["joint_cls_gt"][None], da[None], db[None])
    return sol


NP_KEYS = ("baseline", "nonlinear", "best_a", "best_b", "score_b", "inliers_a", "inliers_b", "off", "tie_a", "tie_b", "record")


@pytest.fixture(scope="module")
def solved(dev):
    """Every SPEC solved by the HIP path (B = 1 each, draws replayed) and by the reference arithmetic (12 CPU workers at most)."""
    from oracle import cpu_layout, pose_compare as PC
    refs = PC.reference_fits([s[0] for s in SPECS], [s[1] for s in SPECS], [s[2] for s in SPECS], NA, NB, seed0=SEED0,
                             workers=max(1, min(12, cpu_layout.usable_cpus() - 2)), specs=[_spec_kw(s) for s in SPECS])
    out = []
    for spec, ref in zip(SPECS, refs):
        c, p, da, db = _inputs(spec)
        sol = _solve(dev, c, p, spec[2], da, db)
        out.append(dict(spec=spec, c=c, p=p, da=da, db=db, sol=sol, np={k: sol[k].cpu().numpy() for k in NP_KEYS}, ref=ref))
    return out


def test_tiny_parts_match_the_reference_arithmetic(solved):
    from oracle import pose_compare as PC
    fits = thin = 0
    for s in solved:
        K = s["spec"][2]
        rows = PC.compare_cloud(s["np"], 0, s["ref"], K, draws=(s["da"], s["db"]), problem_data=(s["c"], s["p"]))
        n, _ = PC.check_rows(rows)          # unchanged bars: same set 1e-5 / 1e-4, other sets their bounds + the own-mask refit
        assert n == 2 * K, s["spec"]
        # a fit that ended on another consensus set than the reference's (and is not thin) carries the float64 refit of its own mask
        for r in rows:
            if PC.flipped(r) and not PC.thin(r) and not r.get("gpu_thin"):
                assert "own_mask_err" in r, (s["spec"], r)
        fits += n
        thin += sum(1 for r in rows if PC.thin(r))
        rec = s["np"]["record"]
        assert np.array_equal(rec[:, :, :13], s["np"]["baseline"], equal_nan=True), s["spec"]
        assert np.array_equal(rec[:, :, 13:], s["np"]["nonlinear"], equal_nan=True), s["spec"]
    assert fits == sum(2 * s[2] for s in SPECS)
    assert 0 < thin < fits                  # the 1- and 2-point parts and the unrelated ones are thin; most fits are compared


def _stage_a(dev, sol, K, da, scalar_points):
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW, ransac_single_batch
    return ransac_single_batch(sol["off"], sol["_src"], sol["_tgt"], 0.1, NA, draws=da.reshape(-1, NA, 3), max_n=sol["_max_n"],
                               scalar_points=scalar_points, tie_window=TIE_WINDOW)


def test_stage_a_tie_count_is_exact_in_sign_and_bounded(dev, solved):
    from oracle import pose_compare as PC
    n_overflow = n_degenerate_winner = 0
    for s in solved:
        K, sol, da = s["spec"][2], s["sol"], s["da"]
        runs = {}
        for sp in (True, False):
            a = _stage_a(dev, sol, K, da, sp)
            again = _stage_a(dev, sol, K, da, sp)
            for k in ("tie", "best", "scores", "inliers"):
                assert torch.equal(a[k], again[k]), (s["spec"], sp, k)           # a second call gives the same bytes
            assert torch.equal(a["model"].view(torch.int64), again["model"].view(torch.int64)), (s["spec"], sp)
            runs[sp] = {k: a[k].cpu().numpy() for k in ("tie", "best", "scores")}
        assert np.array_equal(runs[True]["tie"], runs[False]["tie"]), s["spec"]   # scalar-register and LDS scoring: identical
        assert np.array_equal(runs[True]["scores"], runs[False]["scores"]) and np.array_equal(runs[True]["best"], runs[False]["best"])
        tie, best, scores = runs[True]["tie"], runs[True]["best"], runs[True]["scores"]
        assert np.array_equal(tie, s["np"]["tie_a"][0]) and np.array_equal(best, s["np"]["best_a"][0]), s["spec"]   # == solve()'s
        for j in range(K):
            lo, hi, sign = PC.stage_a_tie_bounds(scores[j], da[j], best[j, 0])
            t = int(tie[j, 1])
            where = (s["spec"], j, int(best[j, 0]), int(best[j, 1]), t, lo, hi)
            assert (t < 0) == (sign < 0), where                                     # the sign: no tolerance
            assert lo <= abs(t) <= hi, where
            _, others = PC.stage_a_contenders(scores[j], da[j], best[j, 0])
            n_overflow += int(len(others) > PC.TIE_MAX_CAND)
            n_degenerate_winner += int(sign < 0)
    # the cases this file exists for: more contenders than slots (the unrelated parts), degenerate winners
    assert n_overflow >= 3 and n_degenerate_winner >= 2, (n_overflow, n_degenerate_winner)


def test_late_degenerate_winner_keeps_its_sign(dev):
    """A hand-made stage-A problem whose winner is a degenerate sample behind hundreds of degenerate contenders: part 0 holds three
    points, the first two identical.  Hypotheses 0..499 draw a single distinct point, 500 is (0, 0, 2) -- the copy and the third point
    -- and outscores all of them; the rest are random.  The sign must come out negative however many contenders precede the winner.
    The 16 examined contenders (the lowest-numbered) score below the winner, so their masks differ from its mask and all count:
    tie[1] is exactly -(1 + every other contender).  Part 1 is empty: tie 0, best (-1, 0), NaN model."""
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW, ransac_single_batch
    from oracle import pose_compare as PC
    src = np.array([[0.2, 0.3, 0.4], [0.2, 0.3, 0.4], [0.7, 0.1, 0.6]], np.float32)
    tgt = (0.8 * src[:, [1, 2, 0]] + np.array([0.1, -0.2, 0.3])).astype(np.float32)      # a similarity: 0.8 x a permutation + t
    rng = np.random.RandomState(1)
    draws = rng.randint(3, size=(NA, 3)).astype(np.int32)
    draws[:500] = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 1], [1, 0, 0], [0, 1, 0]], np.int32)[rng.randint(0, 5, 500)]
    draws[500] = [0, 0, 2]
    off = torch.tensor([0, 3, 3], dtype=torch.int32, device=dev)
    S, G = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    D = np.concatenate([draws, np.zeros((NA, 3), np.int32)])
    for sp in (True, False):
        a = ransac_single_batch(off, S, G, 0.1, NA, draws=D.reshape(2, NA, 3), max_n=3, scalar_points=sp, tie_window=TIE_WINDOW)
        tie, best, scores = a["tie"].cpu().numpy(), a["best"].cpu().numpy(), a["scores"].cpu().numpy()
        assert int(best[0, 0]) == 500 and (scores[0, :500] < best[0, 1]).all(), (best[0], np.unique(scores[0, :500]))
        wd, others = PC.stage_a_contenders(scores[0], draws, 500)
        assert wd and (others < 500).sum() >= 100, (sp, len(others))
        assert (scores[0, others[:PC.TIE_MAX_CAND]] != best[0, 1]).all()
        assert int(tie[0, 1]) == -(1 + len(others)), (sp, tie[0], len(others))
        assert tie[1].tolist() == [0, 0] and best[1].tolist() == [-1, 0] and np.isnan(a["model"][1].cpu().numpy()).all()


def test_stage_b_tie_count_equals_the_host_recount(dev, solved):
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW, ransac_joint_batch
    from oracle import pose_compare as PC
    for s in solved:
        K, sol, db = s["spec"][2], s["sol"], s["db"]
        rng0, rng1 = sol["_rng"]
        b = ransac_joint_batch(rng0, rng1, sol["_src"], sol["_tgt"], sol["joint_direction"].reshape(-1, 3), 0.1, NB,
                               draws=db.reshape(-1, NB, 6), max_n=sol["_max_n"], tie_window=TIE_WINDOW)
        tie, best, score = b["tie"].cpu().numpy(), b["best"].cpu().numpy(), b["score"].cpu().numpy()
        hyp = b["hyp_scores"].view(K - 1, NB).cpu().numpy()
        assert np.array_equal(tie, s["np"]["tie_b"][0]) and np.array_equal(best, s["np"]["best_b"][0]), s["spec"]   # == solve()'s
        for q in range(K - 1):
            want = PC.stage_b_contenders(hyp[q], db[q], score[q])
            assert int(tie[q, 1]) == want, (s["spec"], q, int(tie[q, 1]), want)
            if best[q] >= 0 and (PC.repeated_index(db[q, best[q], :3]) or PC.repeated_index(db[q, best[q], 3:])):
                assert int(tie[q, 1]) >= 1, (s["spec"], q)


def test_empty_part_gives_nan_rows(dev):
    """A part without predicted points: NaN baseline and nonlinear rows for it, best = (-1, 0), tie = 0 -- the reference raises."""
    from articulated_pose_amd.pose import PoseSolver
    from oracle import pose_compare as PC
    K = 3
    c, p = PC.squeezed_problem(52, 512, K, keep={2: 0})
    assert np.bincount(np.argmax(p["instance_per_point"], 1), minlength=K)[2] == 0
    sol = PoseSolver(K, 0.1, NA, NB, dev).solve(c["P"][None], p["nocs_per_point"][None], p["instance_per_point"][None],
                                                p["joint_axis_per_point"][None], p["joint_cls_gt"][None], seed=5)
    rec = sol["record"].cpu().numpy()[0]
    assert np.isnan(rec[2]).all() and np.isfinite(rec[:2]).all()
    assert sol["best_a"].cpu().numpy()[0, 2].tolist() == [-1, 0]
    assert sol["tie_a"].cpu().numpy()[0, 2].tolist() == [0, 0] and sol["tie_b"].cpu().numpy()[0, 1].tolist() == [0, 0]
    assert int(sol["best_b"][0, 1]) == -1


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t      # NaN-safe exact comparison


def test_device_drawn_tiny_parts_whole_sharded_repeated(dev):
    """A batch of tiny-part clouds on the on-device generator: whole with seed_dev, and as two shards with key_dev (cloud_base = the
    shard's first cloud), twice each -- records, winners, masks and both tie arrays byte-equal."""
    from articulated_pose_amd.dataset import stream_key_words
    from articulated_pose_amd.pose import PoseSolver
    from oracle import pose_compare as PC
    K, N = 3, 512
    specs = [({1: 4, 2: 12}, "unrelated"), ({1: 2, 2: 5}, "plain"), ({2: 7}, "coincident"), ({1: 4}, "collinear"), ({1: 1, 2: 3}, "plain")]
    cl = [PC.squeezed_problem(60 + b, N, K, keep=keep, kind=kind) for b, (keep, kind) in enumerate(specs)]
    inputs = [np.stack([c["P"] for c, _ in cl])] + [np.stack([p[k] for _, p in cl]) for k in ("nocs_per_point", "instance_per_point",
                                                                                              "joint_axis_per_point", "joint_cls_gt")]
    solver = PoseSolver(K, 0.1, NA, NB, dev)
    names = ("record", "best_a", "best_b", "inliers_a", "inliers_b", "tie_a", "tie_b", "score_b")
    s = 11
    seed_dev = torch.tensor([s], dtype=torch.int64, device=dev)
    key = lambda base: torch.from_numpy(stream_key_words(s, base)).to(dev)
    whole = solver.solve(*inputs, seed_dev=seed_dev)
    again = solver.solve(*inputs, seed_dev=seed_dev)
    for n in names:
        assert torch.equal(_bits(again[n]), _bits(whole[n])), n
    for _ in range(2):
        for lo, hi in ((0, 2), (2, 5)):
            part = solver.solve(*[x[lo:hi] for x in inputs], key_dev=key(lo))
            for n in names:
                assert torch.equal(_bits(part[n]), _bits(whole[n][lo:hi])), (lo, hi, n)
    # the batch does reach the fragile regime on the device generator too: contenders past the slots
    assert int((whole["tie_a"][..., 1].abs() > 0).sum()) > 0
