"""Counterpart of evaluation/parallel_ancsh_pose.py on the MI355X.

Reference: per cloud, K x ransac(single_*, niter=10000) + (K-1) x ransac(joint_*, niter=200), each
hypothesis a numpy Kabsch fit (+ a scipy LM for joints), ~10 s/cloud/core.  Here a whole batch of clouds
is solved by five kernel launches (partition, joint-direction medians, stage A score + finish, stage B
hypotheses + finish); hypotheses are the parallel axis.

Randomness: the reference samples inside the estimators from numpy's unseeded global RNG.  Here the
3-point samples are an explicit input (`draws_*`, int32) so a run can replay numpy's stream exactly
(`draws_from_seed`), or -- draws None -- come from the on-device counter-based generator (`seed`).
"""
import os
import pickle

import numpy as np
import torch

from .. import _lib
from .d3_utils import rot_diff_degree


def _i32(t, dev):
    if torch.is_tensor(t):
        return t.to(dev, torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(t, np.int32)).to(dev)


def _f32(t, dev):
    if torch.is_tensor(t):
        return t.to(dev, torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(dev)


TIE_WINDOW = 32 * 2.0 ** -27      # default half-width of the tie window on the residual norm: 32 ulp of the float32 threshold 0.1 (2.4e-7)


def _fit_entry(base, seed, seed_dev=None, key_dev=None, joint_kind=None, nprob_b=0):
    """The entry of one family (`base`: ancsh_ransac_single_rec, ancsh_ransac_joint_rec, ancsh_pose_fit_rec) for a key mode and a joint
    kind: key_dev -> base_dkey, seed_dev -> base_dseed, neither -> base with `seed` by value; a joint_kind array (one entry per joint
    problem, nprob_b of them) -> ..._kind, with the array as the last argument.  -> (entry name, key argument, trailing arguments)."""
    if key_dev is not None:
        name, key = base + "_dkey", _lib.ptr(key_dev)
    elif seed_dev is not None:
        name, key = base + "_dseed", _lib.ptr(seed_dev)
    else:
        name, key = base, int(seed)
    if joint_kind is None:
        return name, key, []
    if joint_kind.dtype != torch.int32 or joint_kind.numel() != nprob_b or not joint_kind.is_contiguous():
        raise ValueError("joint_kind must be a contiguous int32 tensor of %d entries (one per problem)" % nprob_b)
    return name + "_kind", key, [_lib.ptr(joint_kind)]


def ransac_single_batch(off, src, tgt, inlier_th, niter, draws=None, seed=0, max_n=None, scalar_points=True, record=None, K=0,
                        tie_window=None, seed_dev=None, key_dev=None):
    """Batched ransac(dataset, single_transformation_estimator, single_transformation_verifier, th, niter).
    off (nprob+1) int32 row offsets into src/tgt (rows,3) float32 device tensors.
    scalar_points: score the hypotheses with the parts' points in scalar registers (ancsh_ransac_single_ex: a padded quad copy of
    the parts in scratch memory, no LDS) instead of the LDS-staged kernel of ancsh_ransac_single; identical results.
    record: optional (B, K, 26) float64 pose record -- every fit is ALSO written into columns 0..12 of its row by the finish kernel
    (ancsh_ransac_single_rec); tie_window: not None -> `tie` (nprob, 2) int32 [borderline points of the winner, degenerate
    contenders] (see include/ancsh_hip.h).  seed_dev: optional one-element int64 device tensor holding the generator key (its
    uint64 bits), read when the kernels run (ancsh_ransac_single_rec_dseed) -- `seed` is then unused.
    key_dev: optional 16-byte device key block (ancsh_stream_key: seed, cloud_base; e.g. four int32 words) instead of seed_dev
    (ancsh_ransac_single_rec_dkey): the generator keys problem p as p + cloud_base * K, so it needs K.
    -> dict(model (nprob,13) f64 [R(9) s t(3)], inliers (rows) uint8, best (nprob,2) int32 [iter, score])."""
    dev = src.device
    nprob = off.numel() - 1
    rows = src.shape[0]
    max_n = int(max_n or rows)
    model = torch.empty((nprob, 13), dtype=torch.float64, device=dev)
    inl = torch.empty((rows,), dtype=torch.uint8, device=dev)      # every row inside off[0]..off[-1] is written by the finish kernel
    best = torch.empty((nprob, 2), dtype=torch.int32, device=dev)
    scores = torch.empty((nprob * niter,), dtype=torch.int32, device=dev)
    d = None if draws is None else _i32(draws, dev)
    if d is not None and d.numel() != nprob * niter * 3:
        raise ValueError("draws must have shape (nprob, niter, 3)")
    tie = torch.empty((nprob, 2), dtype=torch.int32, device=dev) if tie_window is not None else None
    quads = torch.empty((_lib.lib().ancsh_ransac_single_quads_floats(rows, nprob),), dtype=torch.float32, device=dev) if scalar_points else None
    # the record entries take everything; without a record, a tie window or a device key the two older entries are called
    rec = key_dev is not None or seed_dev is not None or record is not None or tie_window is not None
    name, key, _ = _fit_entry("ancsh_ransac_single_rec", seed, seed_dev, key_dev) if rec else \
        ("ancsh_ransac_single_ex" if scalar_points else "ancsh_ransac_single", int(seed), [])
    args = [nprob, _lib.ptr(off), _lib.ptr(src), _lib.ptr(tgt), float(inlier_th), int(niter), _lib.ptr(d), key, max_n, _lib.ptr(model),
            _lib.ptr(inl), _lib.ptr(best), _lib.ptr(scores)]
    if rec or scalar_points:
        args += [_lib.ptr(quads), rows]
    if rec:
        args += [_lib.ptr(record), int(K), _lib.ptr(tie), float(tie_window or 0.0)]
    _lib.call(name, *args)
    return dict(model=model, inliers=inl, best=best, scores=scores.view(nprob, niter), tie=tie, _keep=(d, scores, quads))


LM_SCHEDULES = {"auto": 0, "throughput": 1, "latency": 2}     # ANCSH_LM_* of include/ancsh_hip.h
JOINT_KINDS = {"revolute": 0, "prismatic": 1}                 # ANCSH_JOINT_* of include/ancsh_hip.h


def check_joint_types(joint_types, num_parts):
    """Validate a joint_types argument for an object of num_parts parts, on the host, before anything touches the GPU.
    None -> None (every joint revolute: the entries without a kind array); one string -> that kind for all K - 1 joints; a sequence of
    K - 1 strings -> joint j = 1..K-1 in order.  -> a tuple of K - 1 kind codes (JOINT_KINDS), or None.  ValueError names the
    offending entry."""
    if joint_types is None:
        return None
    nj = max(int(num_parts) - 1, 0)
    if isinstance(joint_types, str):
        if joint_types not in JOINT_KINDS:
            raise ValueError("joint_types must be one of %s, got %r" % (tuple(JOINT_KINDS), joint_types))
        return (JOINT_KINDS[joint_types],) * nj
    if not isinstance(joint_types, (list, tuple)):
        raise ValueError("joint_types must be None, one of %s, or a sequence of %d of them (one per joint), got %r"
                         % (tuple(JOINT_KINDS), nj, joint_types))
    if len(joint_types) != nj:
        raise ValueError("joint_types must name the %d joints of a %d-part object, got %d entries: %r"
                         % (nj, num_parts, len(joint_types), list(joint_types)))
    for j, t in enumerate(joint_types):
        if not isinstance(t, str) or t not in JOINT_KINDS:
            raise ValueError("joint_types[%d] (joint %d) must be one of %s, got %r" % (j, j + 1, tuple(JOINT_KINDS), t))
    return tuple(JOINT_KINDS[t] for t in joint_types)


def joint_kind_tensor(kinds, B, device):
    """The (B * (K - 1)) int32 device array of the *_kind entries for B clouds of one object class (problem p = b * (K - 1) + q);
    kinds: check_joint_types' tuple, or None -> None."""
    if kinds is None:
        return None
    return torch.tensor(list(kinds) * int(B), dtype=torch.int32).to(device)


def ransac_joint_batch(rng0, rng1, src, tgt, joint_dir, inlier_th, niter, draws=None, seed=0, max_n=None, want_lm_stat=False,
                       lm_schedule="auto", record=None, K=0, tie_window=None, seed_dev=None, key_dev=None, joint_kind=None):
    """Batched ransac(dataset, joint_transformation_estimator, joint_transformation_verifier, th, niter).
    rng0/rng1 (nprob,2) int32 [start,end) rows of part 0 / part j; joint_dir (nprob,3) float32.
    seed_dev: optional one-element int64 device tensor; the kernels use its value + 1 (ancsh_ransac_joint_rec_dseed: stage B of the
    key that stage A reads there) and `seed` is unused.
    key_dev: optional 16-byte device key block (ancsh_stream_key) instead of seed_dev (ancsh_ransac_joint_rec_dkey: its seed + 1, problem
    p keyed as p + cloud_base * (K - 1); needs K).
    joint_kind: optional (nprob) int32 device tensor, 0 revolute / 1 prismatic per problem (the ancsh_ransac_joint_rec*_kind entries:
    a prismatic problem minimises objective_eval_r, :70-81, and never reads its joint_dir row); None = every problem revolute, the
    launches of the entries without it.
    -> dict(model (nprob,26) f64 [R0 s0 t0 R1 s1 t1], inliers (nprob,2,max_n) uint8, best (nprob), score (nprob))."""
    dev = src.device
    nprob = rng0.shape[0]
    max_n = int(max_n or src.shape[0])
    model = torch.empty((nprob, 26), dtype=torch.float64, device=dev)
    inl = torch.empty((nprob, 2, max_n), dtype=torch.uint8, device=dev)   # fully written (flags + zero tail) by the finish kernel
    best = torch.empty((nprob,), dtype=torch.int32, device=dev)
    score = torch.empty((nprob,), dtype=torch.float64, device=dev)
    sc = torch.empty((nprob * niter,), dtype=torch.float64, device=dev)
    mo = torch.empty((nprob * niter, 26), dtype=torch.float64, device=dev)
    stat = torch.empty((nprob, niter, 2), dtype=torch.int32, device=dev) if want_lm_stat else None
    d = None if draws is None else _i32(draws, dev)
    if d is not None and d.numel() != nprob * niter * 6:
        raise ValueError("draws must have shape (nprob, niter, 6)")
    tie = torch.empty((nprob, 2), dtype=torch.int32, device=dev) if tie_window is not None else None
    # the record entries: their finish kernel also fills the record's nonlinear columns / the tie counts
    rec = joint_kind is not None or key_dev is not None or seed_dev is not None or record is not None or tie_window is not None
    name, key, kind = _fit_entry("ancsh_ransac_joint_rec", seed, seed_dev, key_dev, joint_kind, nprob) if rec else ("ancsh_ransac_joint_ex", int(seed), [])
    args = [nprob, _lib.ptr(rng0), _lib.ptr(rng1), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(joint_dir), float(inlier_th), int(niter), _lib.ptr(d),
            key, max_n, _lib.ptr(model), _lib.ptr(inl), _lib.ptr(best), _lib.ptr(score), _lib.ptr(sc), _lib.ptr(mo), _lib.ptr(stat),
            LM_SCHEDULES[lm_schedule]]
    if rec:
        args += [_lib.ptr(record), int(K), _lib.ptr(tie), float(tie_window or 0.0)] + kind
    _lib.call(name, *args)
    return dict(model=model, inliers=inl, best=best, score=score, lm_stat=stat, hyp_models=mo, hyp_scores=sc, tie=tie, _keep=(d, joint_kind))


def pose_fit_batch(off, rng0, rng1, src, tgt, joint_dir, inlier_th, niter_a, niter_b, draws_a=None, draws_b=None, seed=0, max_n=None,
                   want_lm_stat=False, lm_schedule="auto", record=None, K=0, tie_window=None, seed_dev=None, key_dev=None, joint_kind=None):
    """ransac_joint_batch + ransac_single_batch of one batch in ONE ABI call (ancsh_pose_fit_rec*, include/ancsh_hip.h): stage B's LM
    fits and stage A's refit share a launch, seven launches instead of eight, every output byte the same.  Arguments as the two
    functions'; `seed` is stage A's key (stage B takes seed + 1, as PoseSolver.solve passes it).  -> (a, b): the two functions' dicts."""
    dev = src.device
    npa, npb = off.numel() - 1, rng0.shape[0]
    rows = src.shape[0]
    max_n = int(max_n or rows)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    model_a, inl_a, best_a, scores_a = E((npa, 13), torch.float64), E((rows,), torch.uint8), E((npa, 2), torch.int32), E((npa * niter_a,), torch.int32)
    quads = E((_lib.lib().ancsh_ransac_single_quads_floats(rows, npa),), torch.float32)
    model_b, inl_b, best_b, score_b = E((npb, 26), torch.float64), E((npb, 2, max_n), torch.uint8), E((npb,), torch.int32), E((npb,), torch.float64)
    sc_b, mo_b = E((npb * niter_b,), torch.float64), E((npb * niter_b, 26), torch.float64)
    stat = E((npb, niter_b, 2), torch.int32) if want_lm_stat else None
    tie_a = E((npa, 2), torch.int32) if tie_window is not None else None
    tie_b = E((npb, 2), torch.int32) if tie_window is not None else None
    da = None if draws_a is None else _i32(draws_a, dev)
    db = None if draws_b is None else _i32(draws_b, dev)
    if da is not None and da.numel() != npa * niter_a * 3:
        raise ValueError("draws_a must have shape (nprob_a, niter_a, 3)")
    if db is not None and db.numel() != npb * niter_b * 6:
        raise ValueError("draws_b must have shape (nprob_b, niter_b, 6)")
    name, key_a, kind = _fit_entry("ancsh_pose_fit_rec", seed, seed_dev, key_dev, joint_kind, npb)
    key_b = key_a + 1 if key_dev is None and seed_dev is None else key_a      # by value stage B takes seed + 1; on the device the kernels add it
    _lib.call(name, npa, _lib.ptr(off), _lib.ptr(src), _lib.ptr(tgt), float(inlier_th), int(niter_a), _lib.ptr(da), key_a, max_n,
              _lib.ptr(model_a), _lib.ptr(inl_a), _lib.ptr(best_a), _lib.ptr(scores_a), _lib.ptr(quads), rows, _lib.ptr(tie_a),
              float(tie_window or 0.0), npb, _lib.ptr(rng0), _lib.ptr(rng1), _lib.ptr(joint_dir), float(inlier_th), int(niter_b), _lib.ptr(db),
              key_b, _lib.ptr(model_b), _lib.ptr(inl_b), _lib.ptr(best_b), _lib.ptr(score_b), _lib.ptr(sc_b), _lib.ptr(mo_b), _lib.ptr(stat),
              LM_SCHEDULES[lm_schedule], _lib.ptr(tie_b), float(tie_window or 0.0), _lib.ptr(record), int(K), *kind)
    return (dict(model=model_a, inliers=inl_a, best=best_a, scores=scores_a.view(npa, niter_a), tie=tie_a, _keep=(da, scores_a, quads)),
            dict(model=model_b, inliers=inl_b, best=best_b, score=score_b, lm_stat=stat, hyp_models=mo_b, hyp_scores=sc_b, tie=tie_b,
                 _keep=(db, joint_kind)))


def draws_from_seed(seed, counts, niter_a, niter_b):
    """Replay np.random.seed(seed) + the reference's randint call order for ONE cloud
    (stage A parts 0..K-1, then joints 1..K-1: evaluation/parallel_ancsh_pose.py:38,110-111).
    counts: points per predicted part.  -> (draws_a (K,niter_a,3), draws_b (K-1,niter_b,6)) int32."""
    rs = np.random.RandomState(seed)
    K = len(counts)
    da = np.zeros((K, niter_a, 3), np.int32)
    for j in range(K):
        for i in range(niter_a):
            da[j, i] = rs.randint(counts[j], size=3)
    db = np.zeros((max(K - 1, 0), niter_b, 6), np.int32)
    for j in range(1, K):
        for i in range(niter_b):
            db[j - 1, i, :3] = rs.randint(counts[0], size=3)
            db[j - 1, i, 3:] = rs.randint(counts[j], size=3)
    return da, db


class PoseSolver(object):
    """solve(...) = the per-cloud body of solver_ransac_nonlinear (:238-341) for a batch of clouds.

    Inputs per cloud (device tensors or arrays): P (B,N,3); nocs_pred (B,N,3K) and mask_pred (B,N,K) (from
    the part-NOCS/baseline network when USE_BASELINE, :232-237); joint_axis_per_point (B,N,3) and
    joint_cls (B,N) int (from the ANCSH record, :295).  Returns device tensors:
        record    (B,K,26) float64  [baseline | nonlinear]: the per-part pose record (:330-353), written by the two finish kernels
        baseline  (B,K,13) float64  [R(9) row-major, scale, translation(3)]   -- stage A   (= record[:, :, :13], a view)
        nonlinear (B,K,13) float64                                             -- stage B (part 0 from joint 1; record[:, :, 13:])
        counts (B,K) int32 points per predicted part; best_a (B,K,2); best_b (B,K-1)
        tie_a (B,K,2), tie_b (B,K-1,2) int32: how implementation-sensitive each fit is -- [points within `tie_window` of the inlier
        threshold under the winning hypothesis, DEGENERATE contenders = hypotheses within one inlier of the winning score whose 3-point
        sample repeats an index (their rotation is implementation-defined in the reference itself); stage A counts only those that would
        change the consensus set and makes the count NEGATIVE exactly when the winner's own sample is degenerate -- the sharp per-fit
        warning, read from the winner's sample itself; of the OTHER contenders it examines the 16 lowest-numbered hypotheses and counts
        any beyond them as changing, so the count is deterministic]
        (include/ancsh_hip.h, ancsh_ransac_single_rec; what the counts did and did not predict: profiles/r06_pose_tie_rate_K3.txt)
    A part with no predicted points gives NaN rows (the reference raises inside randint)."""

    fused_launch = True       # solve(): both stages in one ABI call, LM fits and stage A's refit in one launch (False: the two calls)

    def __init__(self, num_parts, inlier_th=0.1, niter_a=10000, niter_b=200, device="cuda:0", want_lm_stat=False,
                 max_part_points=None, lm_schedule="auto", tie_window=TIE_WINDOW, joint_types=None):
        # joint_types: None (every joint revolute, objective_eval :56-68), "revolute" / "prismatic" for all joints, or K - 1 of them
        # for joints 1..K-1 -- a prismatic joint is fitted with objective_eval_r (:70-81): its part does not turn against part 0.
        # Checked here, on the host; "revolute" everywhere is None (the same launches as without the argument).
        kinds = check_joint_types(joint_types, num_parts)
        self.joint_kinds = kinds if kinds is not None and any(kinds) else None
        self._kind_dev = {}                    # B -> the (B * (K - 1)) device array, built once per batch size (prepare())
        self.K, self.th, self.niter_a, self.niter_b = num_parts, inlier_th, niter_a, niter_b
        self.tie_window = tie_window           # None: no tie counts
        self.device = torch.device(device)
        # Upper bound on the points of ONE predicted part (sizes the LDS-resident refits: <= 6144 for stage A, <= 3072 for the
        # joint fit).  Default: the whole cloud N, which needs no host synchronisation (graph capture) and covers N <= 3072;
        # for larger clouds whose parts are known to be smaller, pass the bound here.
        self.max_part_points = max_part_points
        if lm_schedule not in LM_SCHEDULES:
            raise ValueError("lm_schedule must be one of %s" % sorted(LM_SCHEDULES))
        self.lm_schedule = lm_schedule         # "latency": eight lanes per LM fit (a lone batch finishes sooner); "throughput": one
        self.want_lm_stat = want_lm_stat       # also return per-hypothesis (status, nfev) of the stage-B LM fits

    def prepare(self, B):
        """Build the per-problem joint-kind array of a B-cloud batch ahead of time (a host-to-device copy: call it before a step is
        captured; solve() calls it itself otherwise).  -> the (B * (K - 1)) int32 device tensor, or None when every joint is revolute."""
        if self.joint_kinds is None or self.K < 2:
            return None
        if B not in self._kind_dev:
            self._kind_dev[B] = joint_kind_tensor(self.joint_kinds, B, self.device)
        return self._kind_dev[B]

    def solve(self, P, nocs_pred, mask_pred, joint_axis_per_point, joint_cls=None, draws_a=None, draws_b=None, seed=0, seed_dev=None,
              key_dev=None, joint_index=None, fit_quality=False, ground_truth=None):
        """Both stages of a batch.  The joint fit (stage B) only needs the partition, not the per-part fits, and its LM kernel is the
        latency-bound launch (64 waves for 1.6 ms: MINPACK's longest trajectory, all but one wave gone after a fifth of it).  With
        the lane-per-fit LM schedule both stages go out in ONE call (pose_fit_batch, ancsh_pose_fit_rec*): stage A's scoring first,
        then stage A's refit INSIDE the LM launch -- on an in-order hardware queue nothing else can overlap the LM tail -- and the
        batch ends with stage B's model / verify / refit launches.  With the eight-lane schedule ("latency"), or K = 1, or
        PoseSolver.fused_launch = False, the two calls of before: stage B issued first, then stage A.  Same bytes either way: the
        stages share nothing but the partition.
        seed_dev: a one-element int64 device tensor holding the generator key (its uint64 bits) instead of `seed`: the kernels read
        it when they run, so a captured step draws a fresh sample stream per batch from whatever was written there last; the
        bytes equal those of seed=<that value>.
        key_dev: a 16-byte device key block (include/ancsh_hip.h, ancsh_stream_key; dataset.stream_key_words) instead of either: its
        seed is read as seed_dev's, and cloud b is keyed as global cloud cloud_base + b -- so a shard of clouds [lo, hi) solved with
        cloud_base = lo gives the bytes of rows [lo, hi) of the whole batch's solve(seed=<that seed>).
        joint_cls / joint_index -- exactly one of them: the joint association of stage B's directions.  joint_cls (B,N) int = a label
        per point (the ANCSH record's joint_cls_gt, :295); joint_index (B,N,C) float32 = the ANCSH network's index_per_point head, whose
        np.argmax per point is the label (lib/parallel_ancsh_pose.py:339-343,366; ancsh_pose_joint_direction_pred, which takes it while
        compacting, and ancsh_pose_poison_records_pred, which also poisons a cloud with a non-finite index value).  The records then
        equal those of joint_cls = np.argmax(joint_index, -1); a joint no point selects has a NaN direction (certain when K - 1 >= C).
        Fitted as a revolute joint it gets no joint fit: every evaluation of the objective is NaN, MINPACK accepts no step, and the row
        holds the unrefined Kabsch start of the winning sample (finite, not NaN: tests/test_prismatic_gpu.py).  A prismatic joint
        (joint_types) does not read its direction and is fitted like any other.
        fit_quality=True: one more launch behind the poison (pose.quality.fit_quality_batch) adds "record_wide", float64 -- the record's
        columns bit for bit, then per part its points, both winners' scores and the inliers / mean / RMS / median / max residual of the
        baseline and of the nonlinear pose over all points of the part.  Without it nothing changes.
        ground_truth=gt ((B, K, 19) float64 on the device, pose.gt_errors.pack_ground_truth's rows): one more launch behind those
        (pose.gt_errors.gt_error_batch, on P and the nocs_pred / mask_pred the fit read) adds "record_gt", float64 -- the record so far
        (the wide one with fit_quality=True) bit for bit, then rpy_err / xyz_err / scale_err / 3-D IoU / relative rotation error of both
        poses, the nonlinear pose's relative translation error and the part's points.  "record" and "record_wide" are unchanged.
        pose.record.BLOCKS is the table of these blocks and their columns."""
        _one_association(joint_cls, joint_index)
        if fit_quality:
            from .quality import check_fit_quality
            check_fit_quality(True, self.th)
        out = self._partition(P, nocs_pred, mask_pred)
        if self.fused_launch and self.K > 1 and self.lm_schedule != "latency":
            self._fused_fits(out, joint_axis_per_point, joint_cls, draws_a, draws_b, seed, seed_dev, key_dev, joint_index)
        else:
            self._stage_b_fits(out, joint_axis_per_point, joint_cls, draws_b, seed, seed_dev, key_dev, joint_index)
            self._stage_a_fits(out, draws_a, seed, seed_dev, key_dev)
        out = self._poison(out)
        if fit_quality:
            from .quality import fit_quality_batch
            out["record_wide"] = fit_quality_batch(out, self.th)
        if ground_truth is not None:
            from .gt_errors import gt_error_batch
            from .record import layout_for
            P32, nocs32, mask32 = out["_inputs"]          # the contiguous float32 tensors the partition read
            carried = layout_for(bool(fit_quality), True).carried("gt_errors")[0]
            out["record_gt"] = gt_error_batch(P32, nocs32, mask32, out[carried], ground_truth)
        return out

    def solve_stage_a(self, P, nocs_pred, mask_pred, draws_a=None, seed=0):
        """Part labels + per-part RANSAC / Kabsch (stage A, :238-272): needs only the part-NOCS network's outputs."""
        out = self._partition(P, nocs_pred, mask_pred)
        if self.K > 1:
            out["record"][:, :, 13:] = float("nan")      # stage B never runs on this path: "not fitted", never stale memory
        return self._poison(self._stage_a_fits(out, draws_a, seed))

    def _poison(self, out):
        """A cloud with a NaN / +-Inf anywhere in the fit's inputs gets an all-NaN record (include/ancsh_hip.h,
        ancsh_pose_poison_records): the reference raises LinAlgError on such a cloud; here the batch goes on and the cloud says so."""
        B, N = out["_shape"]
        P, nocs, W = out["_inputs"]
        axis = out.get("_axis")                   # stage B's joint-axis field (K > 1 and stage B ran)
        index = out.get("_index")                 # stage B's index head (joint_index given): scanned too, by the one poison launch
        if index is not None:
            _lib.call("ancsh_pose_poison_records_pred", B, N, self.K, _lib.ptr(P), _lib.ptr(nocs), _lib.ptr(W), _lib.ptr(axis),
                      int(index.shape[2]), _lib.ptr(index), _lib.ptr(out["record"]))
        else:
            _lib.call("ancsh_pose_poison_records", B, N, self.K, _lib.ptr(P), _lib.ptr(nocs), _lib.ptr(W), _lib.ptr(axis),
                      _lib.ptr(out["record"]))
        return out

    def _partition(self, P, nocs_pred, mask_pred):
        dev, K = self.device, self.K
        P, nocs, W = _f32(P, dev), _f32(nocs_pred, dev), _f32(mask_pred, dev)
        B, N, _ = P.shape
        if nocs.shape != (B, N, 3 * K) or W.shape != (B, N, K):
            raise ValueError("nocs_pred must be (B,N,3K) and mask_pred (B,N,K)")
        max_n = min(N, self.max_part_points or N)
        labels = torch.empty((B, N), dtype=torch.int32, device=dev)
        pidx = torch.empty((B, N), dtype=torch.int32, device=dev)
        off = torch.empty((B * K + 1,), dtype=torch.int32, device=dev)
        src = torch.empty((B * N, 3), dtype=torch.float32, device=dev)
        tgt = torch.empty((B * N, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((B, K), dtype=torch.int32, device=dev)
        rng0 = torch.empty((B * max(K - 1, 1), 2), dtype=torch.int32, device=dev) if K > 1 else None
        rng1 = torch.empty((B * max(K - 1, 1), 2), dtype=torch.int32, device=dev) if K > 1 else None
        _lib.call("ancsh_pose_partition", B, N, K, _lib.ptr(W), _lib.ptr(P), _lib.ptr(nocs), _lib.ptr(labels), _lib.ptr(pidx),
                  _lib.ptr(off), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(counts), _lib.ptr(rng0), _lib.ptr(rng1))
        # stage A's finish kernel writes columns 0..12 of every row, stage B's 13..25 (K == 1: stage A writes both): solve() runs both, so
        # nothing is filled here (no aten launch in the captured step); solve_stage_a() marks the half it leaves unwritten
        record = torch.empty((B, K, 26), dtype=torch.float64, device=dev)
        return dict(labels=labels, part_index=pidx, off=off, counts=counts, record=record, _src=src, _tgt=tgt, _max_n=max_n, _shape=(B, N),
                    _rng=(rng0, rng1), _inputs=(P, nocs, W))

    def _stage_a_fits(self, out, draws_a=None, seed=0, seed_dev=None, key_dev=None):
        dev, K = self.device, self.K
        B, N = out["_shape"]
        a = ransac_single_batch(out["off"], out["_src"], out["_tgt"], self.th, self.niter_a,
                                None if draws_a is None else _i32(draws_a, dev).reshape(B * K, self.niter_a, 3), seed, out["_max_n"],
                                record=out["record"], K=K, tie_window=self.tie_window, seed_dev=seed_dev, key_dev=key_dev)
        return self._publish_a(out, a)

    def _publish_a(self, out, a):
        K = self.K
        B, N = out["_shape"]
        out.update(baseline=out["record"][:, :, :13], best_a=a["best"].view(B, K, 2), inliers_a=a["inliers"].view(B, N))
        if a["tie"] is not None:
            out["tie_a"] = a["tie"].view(B, K, 2)
        if K == 1:
            out["nonlinear"] = out["record"][:, :, 13:]           # a one-part object: the finish kernel wrote the baseline there too
        return out

    def solve_stage_b(self, out, joint_axis_per_point, joint_cls=None, draws_b=None, seed=0, seed_dev=None, key_dev=None,
                      joint_index=None):
        """Articulated joint fit (stage B, :274-341) on top of a solve_stage_a result (key seed + 1, or *seed_dev + 1 / the key block's
        seed + 1 read on the device).  The records are poisoned again afterwards, now with the joint-axis field among the inputs: a
        cloud with a non-finite value there gets an all-NaN record on this path too.  joint_cls / joint_index: exactly one, as in solve()
        (with joint_index the index head is among the poison's inputs as well)."""
        _one_association(joint_cls, joint_index)
        return self._poison(self._stage_b_fits(out, joint_axis_per_point, joint_cls, draws_b, seed, seed_dev, key_dev, joint_index))

    def _stage_b_fits(self, out, joint_axis_per_point, joint_cls, draws_b=None, seed=0, seed_dev=None, key_dev=None, joint_index=None):
        dev, K = self.device, self.K
        B, N = out["_shape"]
        src, tgt, max_n = out["_src"], out["_tgt"], out["_max_n"]
        rng0, rng1 = out["_rng"]                                   # written by the partition kernel
        if K > 1:
            jdir = self._joint_directions(out, joint_axis_per_point, joint_cls, joint_index)
            b = ransac_joint_batch(rng0, rng1, src, tgt, jdir.view(-1, 3), self.th, self.niter_b,
                                   None if draws_b is None else _i32(draws_b, dev).reshape(B * (K - 1), self.niter_b, 6),
                                   seed + 1, max_n, want_lm_stat=self.want_lm_stat, lm_schedule=self.lm_schedule,
                                   record=out["record"], K=K, tie_window=self.tie_window, seed_dev=seed_dev, key_dev=key_dev,
                                   joint_kind=self.prepare(B))
            self._publish_b(out, b, jdir)
        else:
            out["nonlinear"] = out["record"][:, :, 13:]          # K = 1: filled by _stage_a_fits' finish kernel
        return out

    def _joint_directions(self, out, joint_axis_per_point, joint_cls, joint_index):
        """Stage B's joint directions (K > 1): the per-joint median of the axis field under the given association -> (B, K - 1, 3)."""
        dev, K = self.device, self.K
        B, N = out["_shape"]
        axis = _f32(joint_axis_per_point, dev)
        out["_axis"] = axis
        jdir = torch.empty((B, K - 1, 3), dtype=torch.float32, device=dev)
        if joint_index is not None:            # the network's association: argmax of the index head, taken by the direction kernel
            index = _f32(joint_index, dev)
            if index.dim() != 3 or tuple(index.shape[:2]) != (B, N):
                raise ValueError("joint_index must be (B, N, C) for %d clouds of %d points, got %s" % (B, N, tuple(index.shape)))
            out["_index"] = index
            _lib.call("ancsh_pose_joint_direction_pred", B, N, K, int(index.shape[2]), _lib.ptr(axis), _lib.ptr(index), _lib.ptr(jdir))
        else:
            jcls = _i32(joint_cls, dev)
            _lib.call("ancsh_pose_joint_direction", B, N, K, _lib.ptr(axis), _lib.ptr(jcls), _lib.ptr(jdir))
        return jdir

    def _fused_fits(self, out, joint_axis_per_point, joint_cls, draws_a=None, draws_b=None, seed=0, seed_dev=None, key_dev=None,
                    joint_index=None):
        """Both stages in one ABI call (K > 1, lane-per-fit LM schedule): pose_fit_batch; the same `out` entries as the two calls."""
        dev, K = self.device, self.K
        B, N = out["_shape"]
        rng0, rng1 = out["_rng"]
        jdir = self._joint_directions(out, joint_axis_per_point, joint_cls, joint_index)
        a, b = pose_fit_batch(out["off"], rng0, rng1, out["_src"], out["_tgt"], jdir.view(-1, 3), self.th, self.niter_a, self.niter_b,
                              None if draws_a is None else _i32(draws_a, dev).reshape(B * K, self.niter_a, 3),
                              None if draws_b is None else _i32(draws_b, dev).reshape(B * (K - 1), self.niter_b, 6),
                              seed, out["_max_n"], want_lm_stat=self.want_lm_stat, lm_schedule=self.lm_schedule, record=out["record"], K=K,
                              tie_window=self.tie_window, seed_dev=seed_dev, key_dev=key_dev, joint_kind=self.prepare(B))
        self._publish_b(out, b, jdir)
        return self._publish_a(out, a)

    def _publish_b(self, out, b, jdir):
        K, max_n = self.K, out["_max_n"]
        B, N = out["_shape"]
        if self.want_lm_stat:
            out["lm_stat"] = b["lm_stat"].view(B, K - 1, self.niter_b, 2)
        out["nonlinear"] = out["record"][:, :, 13:]
        if b["tie"] is not None:
            out["tie_b"] = b["tie"].view(B, K - 1, 2)
        out["best_b"] = b["best"].view(B, K - 1)
        out["score_b"] = b["score"].view(B, K - 1)          # the winning hypothesis's verifier score (:186-194)
        out["joint_direction"] = jdir
        out["inliers_b"] = b["inliers"].view(B, K - 1, 2, max_n)
        return out


def _one_association(joint_cls, joint_index):
    """Stage B's joint association: ground-truth labels or the network's index head, exactly one of them."""
    if (joint_cls is None) == (joint_index is None):
        raise ValueError("give exactly one of joint_cls (a label per point) and joint_index (the index_per_point head), got %s"
                         % ("both" if joint_cls is not None else "neither"))


def _model_to_rst(m):
    return m[:9].reshape(3, 3), m[9], m[10:13]


def records_from_solution(sol, rts_list=None):
    """Per-cloud dicts with the reference's pickle schema (:346-352): scale / rotation / translation with
    'baseline' and 'nonlinear' lists of length K (+ 'gt' and the error entries when GT is supplied as
    rts_list[b] = {'scale': {'gt': [...]}, 'rt': {'gt': [4x4...]}} from compute_gt_pose.py)."""
    base = sol["baseline"].cpu().numpy()
    nonl = sol["nonlinear"].cpu().numpy()
    B, K, _ = base.shape
    recs = []
    for b in range(B):
        scale_dict = {'gt': [], 'baseline': [], 'nonlinear': []}
        r_dict = {'gt': [], 'baseline': [], 'nonlinear': []}
        t_dict = {'gt': [], 'baseline': [], 'nonlinear': []}
        xyz_err = {'baseline': [], 'nonlinear': []}
        rpy_err = {'baseline': [], 'nonlinear': []}
        scale_err = {'baseline': [], 'nonlinear': []}
        for j in range(K):
            for kind, arr in (('baseline', base), ('nonlinear', nonl)):
                R, s, t = _model_to_rst(arr[b, j])
                scale_dict[kind].append(s)
                r_dict[kind].append(R)
                t_dict[kind].append(t)
                if rts_list is not None:
                    rt_gt, s_gt = rts_list[b]['rt']['gt'][j], rts_list[b]['scale']['gt'][j]
                    rpy_err[kind].append(rot_diff_degree(R, rt_gt[:3, :3]))
                    xyz_err[kind].append(np.linalg.norm(t - rt_gt[:3, 3]))
                    scale_err[kind].append(np.linalg.norm(s - s_gt[0]))
            if rts_list is not None:
                scale_dict['gt'].append(rts_list[b]['scale']['gt'][j][0])
                r_dict['gt'].append(rts_list[b]['rt']['gt'][j][:3, :3])
                t_dict['gt'].append(rts_list[b]['rt']['gt'][j][:3, 3])
        recs.append({'scale': scale_dict, 'rotation': r_dict, 'translation': t_dict, 'xyz_err': xyz_err,
                     'rpy_err': rpy_err, 'scale_err': scale_err})
    return recs


JOINT_SOURCES = ("gt", "predicted")


def solver_ransac_nonlinear(s_ind, e_ind, test_exp, baseline_exp, choose_threshold, num_parts, test_group, problem_ins,
                            rts_all, file_name, base_path=None, batch_size=32, seed=0, device="cuda:0", joint_source="gt",
                            joint_types=None):
    """Same positional signature as the reference entry point (:196): solves test_group[s_ind:e_ind] and
    pickles {basename: record}.  Records are read with prediction_io.load_record from
    <base_path>/results/test_pred/<exp>/<basename>.{h5,npz} (USE_BASELINE: NOCS + mask from baseline_exp).
    joint_source: "gt" = stage B associates points to joints by the record's joint_cls_gt (:295); "predicted" = by the argmax of the
    record's index_per_point head (lib/parallel_ancsh_pose.py:339-343,366) -- what the ground-truth association is worth.
    joint_types: None (revolute, what the reference's evaluation script runs: its ransac() never forwards joint_type), one kind for all
    joints or one per joint (PoseSolver); a trailing keyword, so the positional signature of the reference's callers does not move."""
    if joint_source not in JOINT_SOURCES:
        raise ValueError("joint_source must be one of %s, got %r" % (JOINT_SOURCES, joint_source))
    check_joint_types(joint_types, num_parts)
    from .. import prediction_io
    base_path = base_path or os.environ.get("ANCSH_BASE_PATH", ".")
    solver = PoseSolver(num_parts, choose_threshold, device=device, joint_types=joint_types)
    names = [test_group[i].split('.')[0] for i in range(s_ind, e_ind) if test_group[i].split('_')[0] not in problem_ins]
    all_rts = {}
    for c0 in range(0, len(names), batch_size):
        chunk = names[c0:c0 + batch_size]
        f = [prediction_io.load_record(os.path.join(base_path, 'results/test_pred', str(test_exp)), n) for n in chunk]
        fb = [prediction_io.load_record(os.path.join(base_path, 'results/test_pred', str(baseline_exp)), n) for n in chunk]
        sol = solver.solve(np.stack([r['P'][:, :3] for r in f]), np.stack([r['nocs_per_point'] for r in fb]),
                           np.stack([r['instance_per_point'] for r in fb]), np.stack([r['joint_axis_per_point'] for r in f]),
                           **({"joint_index": np.stack([r['index_per_point'] for r in f])} if joint_source == "predicted" else
                              {"joint_cls": np.stack([r['joint_cls_gt'] for r in f])}), seed=seed + c0)
        gts = [rts_all[n] for n in chunk] if rts_all is not None else None
        for n, rec in zip(chunk, records_from_solution(sol, gts)):
            all_rts[n] = rec
    with open(file_name, 'wb') as fh:
        pickle.dump(all_rts, fh)
    return all_rts
