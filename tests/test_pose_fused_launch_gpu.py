"""GPU: the whole pose fit in one call (ancsh_pose_fit_rec*, pose.parallel_ancsh_pose.pose_fit_batch): stage B's LM fits and stage A's
refit in ONE launch (csrc/pose.hip, pose_lm_finish_a_kernel) against the two existing entries (ancsh_ransac_joint_rec* then
ancsh_ransac_single_rec*) on the same inputs.  Bit identity, no tolerance: the (B, K, 26) record, both stages' models, inlier masks,
winners, scores and tie counts, every hypothesis' LM result and MINPACK status.

niter_a = 512, niter_b = 72: 72 is not a multiple of the 64-hypothesis chunk, so every problem's last chunk is ragged, and a problem
has two chunks, so the chunk count of an odd number of problems is not a multiple of the four chunks an LM block takes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NA, NB = 512, 72


def _bits(t):
    """a tensor's bytes as integers (NaN-safe equality)"""
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _problem(K, B, N, first_id=60, joint_type="revolute", edit=None):
    """B synthetic clouds + predictions; edit(b, W) may rewrite cloud b's (N, K) part scores in place (tiny / empty / huge parts)"""
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    cl = [make_cloud(first_id + b, N=N, K=K, joint_type=joint_type) for b in range(B)]
    pr = [make_predictions(c, K, seed=b) for b, c in enumerate(cl)]
    if edit is not None:
        for b, p in enumerate(pr):
            edit(b, p["instance_per_point"])
    st = lambda k, src: np.stack([s[k] for s in src])
    return dict(P=st("P", cl), nocs=st("nocs_per_point", pr), W=st("instance_per_point", pr), axis=st("joint_axis_per_point", pr),
                jcls=st("joint_cls_gt", pr))


def _keep_only(W, part, m):
    """leave `part` with its first m points; the others go to part 0"""
    idx = np.nonzero(np.argmax(W, 1) == part)[0][m:]
    W[idx] = 0.0
    W[idx, 0] = 1.0


def _inputs(dev, d, K, joint_types=None, nb=NB):
    """partition + joint directions of the batch: what both forms of the fit read"""
    from articulated_pose_amd.pose import PoseSolver
    solver = PoseSolver(K, 0.1, NA, nb, dev, lm_schedule="throughput", joint_types=joint_types)
    out = solver._partition(d["P"], d["nocs"], d["W"])
    jdir = solver._joint_directions(out, d["axis"], d["jcls"], None) if K > 1 else None
    return solver, out, jdir


def _key_args(dev, mode, seed=7):
    if mode == "seed":
        return dict(seed=seed)
    if mode == "dseed":
        return dict(seed_dev=torch.tensor([seed], dtype=torch.int64, device=dev))
    from articulated_pose_amd.dataset import stream_key_words
    return dict(key_dev=torch.tensor(stream_key_words(seed, 3), dtype=torch.int32, device=dev))


def _run_both(dev, d, K, mode="seed", joint_types=None, nb=NB):
    """-> (fused a, fused b, record), (two-call a, two-call b, record), the solver's partition"""
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW, pose_fit_batch, ransac_joint_batch, ransac_single_batch
    solver, out, jdir = _inputs(dev, d, K, joint_types, nb)
    B = d["P"].shape[0]
    rng0, rng1 = out["_rng"]
    kind = solver.prepare(B)
    key = _key_args(dev, mode)
    rec_f = torch.full((B, K, 26), 7.0, dtype=torch.float64, device=dev)
    rec_t = torch.full((B, K, 26), 7.0, dtype=torch.float64, device=dev)
    a_f, b_f = pose_fit_batch(out["off"], rng0, rng1, out["_src"], out["_tgt"], jdir.view(-1, 3), 0.1, NA, nb, max_n=out["_max_n"],
                              want_lm_stat=True, lm_schedule="throughput", record=rec_f, K=K, tie_window=TIE_WINDOW, joint_kind=kind, **key)
    kb = dict(key)
    if "seed" in kb:
        kb["seed"] += 1                                 # stage B's by-value key, as PoseSolver.solve passes it
    b_t = ransac_joint_batch(rng0, rng1, out["_src"], out["_tgt"], jdir.view(-1, 3), 0.1, nb, max_n=out["_max_n"], want_lm_stat=True,
                             lm_schedule="throughput", record=rec_t, K=K, tie_window=TIE_WINDOW, joint_kind=kind, **kb)
    a_t = ransac_single_batch(out["off"], out["_src"], out["_tgt"], 0.1, NA, max_n=out["_max_n"], record=rec_t, K=K,
                              tie_window=TIE_WINDOW, **key)
    torch.cuda.synchronize()
    return (a_f, b_f, rec_f), (a_t, b_t, rec_t), out


def _assert_same(fused, two, out, K, where):
    (a_f, b_f, rec_f), (a_t, b_t, rec_t) = fused, two
    counts = out["counts"].reshape(-1)                                  # (B * K) points per part
    live_a = counts > 0
    B = out["counts"].shape[0]
    live_b = ((out["counts"][:, :1] > 0) & (out["counts"][:, 1:] > 0)).reshape(-1)      # joint problems with both parts present
    assert torch.equal(_bits(rec_f), _bits(rec_t)), where
    assert not bool((rec_f == 7.0).any()), where                        # every column of every row was written
    for k in ("model", "inliers", "best", "tie"):
        assert torch.equal(_bits(a_f[k]), _bits(a_t[k])), (where, "stage A", k)
    assert torch.equal(a_f["scores"][live_a], a_t["scores"][live_a]), (where, "stage A scores")
    for k in ("model", "inliers", "best", "score", "tie", "hyp_models", "hyp_scores"):
        assert torch.equal(_bits(b_f[k]), _bits(b_t[k])), (where, "stage B", k)
    assert torch.equal(b_f["lm_stat"][live_b], b_t["lm_stat"][live_b]), (where, "lm_stat")      # an absent problem runs no fit
    return int(live_a.sum()), int(live_b.sum())


@pytest.mark.parametrize("K,B,N", [(2, 1, 256), (3, 2, 256)])
def test_fused_launch_equals_the_two_calls(dev, K, B, N):
    """K = 2, B = 1: one joint problem = two chunks, one LM block with two idle waves, two parts."""
    d = _problem(K, B, N)
    fused, two, out = _run_both(dev, d, K)
    na, nb = _assert_same(fused, two, out, K, (K, B, N))
    assert (na, nb) == (B * K, B * (K - 1))
    assert bool(torch.isfinite(fused[2]).all())


def test_fused_launch_with_the_large_chunk(dev):
    """29 joint problems x 300 fits = 8700 > 8192: the launch size at which a wave takes 256 hypotheses instead of 64 (the bench step's
    chunk).  300 = 256 + 44, so every problem has a full and a ragged chunk, and 58 chunks are not a multiple of the four an LM block
    takes: block 14 ends with two idle waves, and chunk_id -> (problem, chunk in problem) is checked across all problems."""
    K, B, N, nb = 2, 29, 256, 300
    d = _problem(K, B, N, first_id=100)
    fused, two, out = _run_both(dev, d, K, nb=nb)
    assert B * (K - 1) * nb > 8192
    assert _assert_same(fused, two, out, K, "large chunk") == (B * K, B * (K - 1))
    assert bool(torch.isfinite(fused[2]).all())


@pytest.mark.parametrize("mode", ["seed", "dseed", "dkey"])
@pytest.mark.parametrize("joint_types", [None, ("revolute", "prismatic", "revolute"), "prismatic"])
def test_fused_launch_every_key_mode_and_kind(dev, mode, joint_types):
    """K = 4, B = 3, N = 512: 9 joint problems = 18 chunks, not a multiple of 4; 12 parts; no kind array, mixed kinds, all prismatic."""
    K, B, N = 4, 3, 512
    d = _problem(K, B, N, first_id=70, joint_type="prismatic" if joint_types == "prismatic" else "revolute")
    fused, two, out = _run_both(dev, d, K, mode=mode, joint_types=joint_types)
    assert _assert_same(fused, two, out, K, (mode, joint_types)) == (12, 9)


def test_fused_launch_empty_and_two_point_parts(dev):
    """Cloud 0 loses part 1 altogether (stage A's NaN path and the LM blocks' early return in one launch), cloud 1 keeps two points of
    part 2."""
    K, B, N = 3, 2, 256

    def edit(b, W):
        _keep_only(W, 1, 0) if b == 0 else _keep_only(W, 2, 2)
    d = _problem(K, B, N, first_id=80, edit=edit)
    fused, two, out = _run_both(dev, d, K)
    counts = out["counts"].cpu().numpy()
    assert counts[0, 1] == 0 and counts[1, 2] == 2
    assert _assert_same(fused, two, out, K, "tiny parts") == (5, 3)
    rec = fused[2].cpu().numpy()
    assert np.isnan(rec[0, 1]).all() and np.isnan(rec[0, 0, 13:]).all()      # the empty part, and part 0's nonlinear pose (joint 1's fit)
    assert np.isfinite(rec[0, 2]).all() and np.isfinite(rec[0, 0, :13]).all()
    assert fused[0]["best"].cpu().numpy()[1].tolist() == [-1, 0]


def test_fused_launch_large_part_takes_more_than_48k_of_lds(dev):
    """One cloud of 2304 points with more than 2040 of them in part 0: the refit's dynamic LDS (24 bytes per point of max_n = 2304, 55.8 KB)
    exceeds the 48 KB a kernel gets without asking, on the fused kernel."""
    K, B, N = 2, 1, 2304
    d = _problem(K, B, N, first_id=90, edit=lambda b, W: _keep_only(W, 1, 200))
    fused, two, out = _run_both(dev, d, K)
    counts = out["counts"].cpu().numpy()
    assert counts[0, 0] > 2040 and counts[0, 1] == 200 and out["_max_n"] == N
    assert _assert_same(fused, two, out, K, "large part") == (2, 1)
    assert bool(torch.isfinite(fused[2]).all())
    assert int(fused[0]["best"][0, 1]) > 1024                             # the winner's inliers reach beyond 48 KB worth of points / 2


def _call_fit(dev, npa, npb, out, jdir, K, rec):
    """ancsh_pose_fit_rec with nprob_a / nprob_b overridden (0 = that stage absent)"""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    rows, max_n = out["_src"].shape[0], out["_max_n"]
    rng0, rng1 = out["_rng"]
    r = dict(model_a=E((max(npa, 1), 13), torch.float64), inl_a=torch.zeros(rows, dtype=torch.uint8, device=dev), best_a=E((max(npa, 1), 2), torch.int32),
             tie_a=E((max(npa, 1), 2), torch.int32), model_b=E((max(npb, 1), 26), torch.float64), inl_b=E((max(npb, 1), 2, max_n), torch.uint8),
             best_b=E((max(npb, 1),), torch.int32), score_b=E((max(npb, 1),), torch.float64), tie_b=E((max(npb, 1), 2), torch.int32))
    keep = [E((max(npa, 1) * NA,), torch.int32), E((_lib.lib().ancsh_ransac_single_quads_floats(rows, max(npa, 1)),), torch.float32),
            E((max(npb, 1) * NB,), torch.float64), E((max(npb, 1) * NB, 26), torch.float64)]
    _lib.call("ancsh_pose_fit_rec", npa, _lib.ptr(out["off"]), _lib.ptr(out["_src"]), _lib.ptr(out["_tgt"]), 0.1, NA, None, 7, max_n,
              _lib.ptr(r["model_a"]), _lib.ptr(r["inl_a"]), _lib.ptr(r["best_a"]), _lib.ptr(keep[0]), _lib.ptr(keep[1]), rows, _lib.ptr(r["tie_a"]),
              TIE_WINDOW, npb, _lib.ptr(rng0), _lib.ptr(rng1), _lib.ptr(jdir), 0.1, NB, None, 8, _lib.ptr(r["model_b"]), _lib.ptr(r["inl_b"]),
              _lib.ptr(r["best_b"]), _lib.ptr(r["score_b"]), _lib.ptr(keep[2]), _lib.ptr(keep[3]), None, 1, _lib.ptr(r["tie_b"]), TIE_WINDOW,
              _lib.ptr(rec), K)
    torch.cuda.synchronize()
    return r


def test_one_stage_absent_degrades_to_the_other_stages_launches(dev):
    """nprob_b = 0 (what a K = 1 caller passes) runs stage A alone, nprob_a = 0 stage B alone; each half equals the full call's."""
    K, B, N = 3, 2, 256
    d = _problem(K, B, N)
    solver, out, jdir = _inputs(dev, d, K)
    rec = [torch.full((B, K, 26), 7.0, dtype=torch.float64, device=dev) for _ in range(3)]
    full = _call_fit(dev, B * K, B * (K - 1), out, jdir, K, rec[0])
    only_a = _call_fit(dev, B * K, 0, out, jdir, K, rec[1])
    only_b = _call_fit(dev, 0, B * (K - 1), out, jdir, K, rec[2])
    for k in ("model_a", "inl_a", "best_a", "tie_a"):
        assert torch.equal(_bits(full[k]), _bits(only_a[k])), k
    for k in ("model_b", "inl_b", "best_b", "score_b", "tie_b"):
        assert torch.equal(_bits(full[k]), _bits(only_b[k])), k
    assert torch.equal(_bits(rec[0][:, :, :13]), _bits(rec[1][:, :, :13])) and bool((rec[1][:, :, 13:] == 7.0).all())
    assert torch.equal(_bits(rec[0][:, :, 13:]), _bits(rec[2][:, :, 13:])) and bool((rec[2][:, :, :13] == 7.0).all())
    # and the full call is the two entries' (the first test's comparison, through the raw entry)
    fused, two, _ = _run_both(dev, d, K)
    assert torch.equal(_bits(rec[0]), _bits(two[2]))


def _pipe(K, N, B, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.weights import synthetic_weights
    return AncshPipeline(K, synthetic_weights(K, mixed_pred=True, early_split_nocs=True, seed=3),
                         synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=4), B, N, "cuda:0",
                         couple=True, niter_a=NA, niter_b=NB, seed=5, lm_schedule="throughput", **kw)


def _pipe_records(K, N, B, fused, monkeypatch, count_calls=False):
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.synthetic import make_batch
    monkeypatch.setattr(PoseSolver, "fused_launch", fused)
    d = make_batch(7, B, N=N, K=K)
    pipe = _pipe(K, N, B, slots=2, use_graph=not count_calls)
    pipe.load_inputs(d["P"], d["cls_gt"])
    if count_calls:
        pipe.step()
        pipe.synchronize()
        _lib.profile_start()
        pipe.step()
        return [name for name, _, _ in _lib.profile_stop()]
    pipe.prepare()
    recs = []
    for _ in range(3):                                   # both slots, and the first one again
        sl, out = pipe.step()
        sl.stream.synchronize()
        recs.append(out["record"].clone())
    return recs


def test_pipeline_records_equal_the_two_call_path(dev, monkeypatch):
    """AncshPipeline, B = 2, N = 256, two slots, captured graph: the records of the fused step, byte for byte those of a pipeline forced
    onto the two calls."""
    K, N, B = 3, 256, 2
    fused = _pipe_records(K, N, B, True, monkeypatch)
    two = _pipe_records(K, N, B, False, monkeypatch)
    assert len(fused) == len(two) == 3
    for f, t in zip(fused, two):
        assert torch.equal(_bits(f), _bits(t))
    assert bool(torch.isfinite(fused[0]).any())


def test_a_step_issues_one_abi_call_fewer(dev, monkeypatch):
    """_lib.call bookkeeping of one eager step: the fused path replaces the stage-B and stage-A calls by one; everything else in place."""
    K, N, B = 3, 256, 2
    fused = _pipe_records(K, N, B, True, monkeypatch, count_calls=True)
    two = _pipe_records(K, N, B, False, monkeypatch, count_calls=True)
    assert len(fused) == len(two) - 1
    fit = [n for n in fused if n.startswith("ancsh_pose_fit_rec")]
    assert len(fit) == 1 and not any(n.startswith("ancsh_ransac_") for n in fused)
    ib = next(i for i, n in enumerate(two) if n.startswith("ancsh_ransac_joint_rec"))
    ia = next(i for i, n in enumerate(two) if n.startswith("ancsh_ransac_single_rec"))
    assert ia == ib + 1 and fit[0] == two[ib].replace("ancsh_ransac_joint_rec", "ancsh_pose_fit_rec")
    assert two[:ib] + fit + two[ia + 1:] == fused
