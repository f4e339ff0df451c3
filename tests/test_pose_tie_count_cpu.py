"""CPU tests (no GPU): the host recounts of the pose fit's degenerate contenders (oracle/pose_compare.py: stage_a_contenders,
stage_a_tie_bounds, stage_b_contenders) on small hand-built score arrays and sample streams.  tests/test_pose_tiny_parts_gpu.py holds
the finish kernels' tie[..., 1] to these recounts, so they are pinned here by hand."""
import numpy as np

from oracle import pose_compare as PC

REG, DEG = [0, 1, 2], [3, 3, 1]          # a regular 3-point sample and one that repeats an index


def _a(rows):
    return np.array(rows, np.int32).reshape(-1, 3)


def test_stage_a_ties_at_best_and_best_minus_one():
    scores = np.array([7, 9, 8, 9, 6, 8, 9])
    draws = _a([DEG, REG, DEG, [4, 4, 4], DEG, [2, 5, 2], REG])
    wd, others = PC.stage_a_contenders(scores, draws, 1)
    assert wd is False
    # h = 0 (7 < 8) and 4 (6) are too far; 2 and 5 are degenerate at best - 1, 3 at best; 6 ties at best but is regular
    np.testing.assert_array_equal(others, [2, 3, 5])
    assert others.dtype == np.int64
    assert PC.stage_a_tie_bounds(scores, draws, 1) == (0, 3, 1)


def test_stage_a_degenerate_winner_is_counted_once_and_never_listed():
    scores = np.array([5, 5, 4, 3])
    draws = _a([[1, 0, 1], DEG, REG, DEG])
    wd, others = PC.stage_a_contenders(scores, draws, 0)
    assert wd is True
    np.testing.assert_array_equal(others, [1])
    assert PC.stage_a_tie_bounds(scores, draws, 0) == (1, 2, -1)
    # a degenerate winner alone: |tie| is exactly 1, negative
    wd, others = PC.stage_a_contenders(np.array([5, 1, 1]), _a([[2, 2, 0], DEG, DEG]), 0)
    assert wd is True and others.size == 0
    assert PC.stage_a_tie_bounds(np.array([5, 1, 1]), _a([[2, 2, 0], DEG, DEG]), 0) == (1, 1, -1)


def test_stage_a_more_contenders_than_slots():
    n = 40
    scores = np.full(n, 3)
    scores[17] = 4                                        # the winner
    draws = _a([DEG] * n)
    draws[5] = REG                                        # one regular tie: not a contender
    wd, others = PC.stage_a_contenders(scores, draws, 17)
    assert wd is True
    np.testing.assert_array_equal(others, [h for h in range(n) if h not in (5, 17)])      # ascending, winner excluded
    c = n - 2
    assert PC.stage_a_tie_bounds(scores, draws, 17) == (1 + c - PC.TIE_MAX_CAND, 1 + c, -1)
    # exactly TIE_MAX_CAND others: no overflow, the lower bound is the winner alone
    s2, d2 = np.full(PC.TIE_MAX_CAND + 1, 2), _a([DEG] * (PC.TIE_MAX_CAND + 1))
    d2[0] = REG
    assert PC.stage_a_tie_bounds(s2, d2, 0) == (0, PC.TIE_MAX_CAND, 1)


def test_stage_a_empty_part():
    assert PC.stage_a_contenders(np.zeros(0, np.int32), np.zeros((0, 3), np.int32), -1)[0] is False
    assert PC.stage_a_contenders(np.zeros(0, np.int32), np.zeros((0, 3), np.int32), -1)[1].size == 0
    assert PC.stage_a_tie_bounds(np.zeros(5, np.int32), _a([DEG] * 5), -1) == (0, 0, 1)       # best = -1: no fit, nothing counted


def test_stage_a_recount_matches_brute_force():
    rng = np.random.RandomState(3)
    for trial in range(50):
        n_pts, niter = int(rng.choice([1, 2, 3, 4, 7])), int(rng.choice([1, 5, 300]))
        scores = rng.randint(0, 4, niter)
        draws = rng.randint(n_pts, size=(niter, 3))
        best = int(np.argmax(scores))                     # earliest maximum, as the kernel's arg-max
        wd, others = PC.stage_a_contenders(scores, draws, best)
        want = [h for h in range(niter) if h != best and scores[h] >= scores[best] - 1 and PC.repeated_index(draws[h])]
        assert wd == PC.repeated_index(draws[best]) and others.tolist() == want, trial


def _b(rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def test_stage_b_window_is_one_sixth():
    best = 10.0 / 6.0
    sc = np.array([best, best - 1.0 / 6.0, best - 1.0 / 6.0 - 1e-8, best - 1.0 / 6.0 + 1e-12, best, 0.0])
    draws = _b([DEG + REG, REG + DEG, DEG + DEG, REG + [5, 6, 5], REG + REG, DEG + DEG])
    # h = 0 (the winner, degenerate: counted), 1 (at best - 1/6), 3 (inside); 2 is 1e-8 below the window, 4 regular, 5 far
    assert PC.stage_b_contenders(sc, draws, best) == 3
    assert PC.stage_b_contenders(sc[[4]], draws[[4]], best) == 0           # a regular winner alone


def test_stage_b_more_than_sixteen_and_empty():
    sc = np.full(50, 2.0)
    draws = _b([REG + DEG] * 50)
    assert PC.stage_b_contenders(sc, draws, 2.0) == 50                       # no cap: every contender is counted
    assert PC.stage_b_contenders(np.zeros(0), np.zeros((0, 6), np.int32), -1.0) == 0
    assert PC.stage_b_contenders(sc, draws, -1.0) == 0                       # the finish kernel's "no fit"


def test_stage_b_recount_matches_brute_force():
    rng = np.random.RandomState(4)
    for trial in range(50):
        niter = int(rng.choice([1, 8, 200]))
        sc = rng.randint(0, 12, niter) / 6.0
        draws = np.concatenate([rng.randint(int(rng.choice([1, 3, 5])), size=(niter, 3)),
                                rng.randint(int(rng.choice([1, 2, 12])), size=(niter, 3))], 1)
        best = float(sc.max())
        want = sum(1 for h in range(niter) if sc[h] >= best - (1.0 / 6.0 + 1e-9)
                   and (PC.repeated_index(draws[h, :3]) or PC.repeated_index(draws[h, 3:])))
        assert PC.stage_b_contenders(sc, draws, best) == want, trial
