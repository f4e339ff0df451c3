"""GPU: the ground-truth poses of a streamed batch (ancsh_gt_pose_build, pose.gt_pose.gt_pose_batch, AncshPipeline / ShardedPipeline
build_gt_pose=True): bit-equal to ancsh_umeyama on the gathered rows under compose_rt / pack_ground_truth / pack_joint_frame, against the
reference's own poses (tests/golden/gt_pose.npz) at tests/test_entry_gpu.py's bar, against the float64 oracle at
tests/test_pose_sweep_gpu.py's bar, the NaN rules cloud by cloud, and through the captured stream -- plain, annotated clouds, annotated
depth frames, the range guard and two gloo ranks -- where the records equal those of a pipeline fed host-built tables, byte for byte."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import passthrough_pose_problem
from redzone import guarded
from test_point_gt_gpu import B_, K_, N_, PAYLOAD, _batches, _dev, _pipe, _same, random_channels, widen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gt_pose.npz")
POSE, NAOCS_T = slice(0, 13), slice(16, 19)            # a gt row: the part-NOCS fit | (13..15: the extent) | the NAOCS fit's translation


# ---- the host's way to the same tables: compute_gt_pose.py's arithmetic on gathered rows ------------------------------------------------
def gathered(rows, off, perm, c):
    """Cloud c's sampled ground-truth rows: raw row offsets[c] + perm[c][i] % n_raw for sample i."""
    cloud = rows[off[c]:off[c + 1]]
    return cloud[perm[c] % cloud.shape[0]]


def host_tables(rows, off, perm, P, extents, K, rule=True):
    """ancsh_umeyama per (cloud, part) on the gathered rows -- one launch for nocs_p, one for nocs_g, as compute_gt_pose.gt_pose_records
    issues them --, compose_rt, then pack_ground_truth / pack_joint_frame.  A cloud with an empty part is skipped as gt_pose_records skips
    it (its rows keep their extents, as on the device).  rule: a fit with a non-finite number is NaN throughout, the header's rule (the
    reference's SVD raises there and the record is skipped).  -> (gt (n, K, 19), frame (n, 13), the points per (cloud, part))."""
    from articulated_pose_amd.compute_gt_pose import compose_rt
    from articulated_pose_amd.pose.aligning import umeyama_batch
    from articulated_pose_amd.pose.gt_errors import pack_ground_truth
    from articulated_pose_amd.pose.point_gt import pack_joint_frame
    n = len(off) - 1
    counts = np.zeros((n, K), np.int64)
    src_p, src_g, tgt, owner = [], [], [], []
    for c in range(n):
        g = gathered(rows, off, perm, c)
        parts = [np.flatnonzero(g[:, 3].astype(np.int32) == j) for j in range(K)]
        counts[c] = [len(p) for p in parts]
        if (counts[c] == 0).any():
            continue
        owner.append(c)
        for p in parts:
            src_p.append(g[p, 4:7]), src_g.append(g[p, 7:10]), tgt.append(P[c][p, :3])
    rt, sc, rt_g, sc_g = [[None] * n for _ in range(4)]
    if owner:
        fits_p, fits_g = umeyama_batch(src_p, tgt, "cuda:0"), umeyama_batch(src_g, tgt, "cuda:0")
        for i, c in enumerate(owner):
            for fits, rts, scs in ((fits_p, rt, sc), (fits_g, rt_g, sc_g)):
                rts[c], scs[c] = [], []
                for j in range(K):
                    s, r, t, _ = fits[i * K + j]
                    m = compose_rt(r, t)
                    if rule and not (np.isfinite(m).all() and np.isfinite(s[0])):
                        m, s = np.full((4, 4), np.nan, np.float32), np.full(3, np.nan)
                    rts[c].append(m), scs[c].append(s)
    ext = [None if extents is None else extents[c] for c in range(n)]
    boxes = [np.full((K, 3), np.nan) if e is None else e for e in ext]
    if owner:
        gt = pack_ground_truth([r if r is not None else [np.full((4, 4), np.nan)] * K for r in rt],
                               [s if s is not None else [np.full(3, np.nan)] * K for s in sc], boxes,
                               [r if r is not None else [np.full((4, 4), np.nan)] * K for r in rt_g])
    else:
        gt = np.full((n, K, 19), np.nan)
        gt[:, :, 13:16] = np.stack(boxes)
    return gt, pack_joint_frame(rt_g, sc_g), counts


# ---- the kernel against ancsh_umeyama ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, K):
    """B = 3 ragged clouds (n_raw = N - 7 so that perm wraps, N + 9, 3N + 5), random cls (a tenth -1), random NOCS, a random perm with entries
    >= n_raw, random P and extents, one of them a NaN with a payload."""
    from articulated_pose_amd.dataset import tiled_size
    rs = np.random.RandomState(100 * K + N)
    clouds = [np.concatenate([rs.uniform(-1, 1, (n_raw, 3)).astype(np.float32), random_channels(rs, n_raw, K)], 1)
              for n_raw in (N - 7, N + 9, 3 * N + 5)]
    perms = [rs.randint(0, tiled_size(c.shape[0], N), N).astype(np.int32) for c in clouds]
    assert (perms[0] >= N - 7).any() and any((np.diff(p) < 0).any() for p in perms)
    P = rs.normal(size=(3, N, 3)).astype(np.float32)
    extent = rs.uniform(0.2, 1.0, (3, K, 3))
    extent[1, K - 1, 1] = PAYLOAD
    return dict(clouds=clouds, perms=perms, P=P, extent=extent, N=N, K=K)


def _tensors(p, order=(0, 1, 2), clouds=None, P=None):
    order = list(order)
    clouds = [(clouds or p["clouds"])[c] for c in order]
    off = np.zeros(len(order) + 1, np.int32)
    off[1:] = np.cumsum([c.shape[0] for c in clouds])
    return np.concatenate(clouds), off, np.stack([p["perms"][c] for c in order]), (p["P"] if P is None else P)[order], p["extent"][order]


def _launch(p, order=(0, 1, 2), clouds=None, P=None, extent=True, off=None, skip=None):
    """gt_pose_batch on problem p with its clouds in `order` -> (gt, frame) on the host; skip: "gt" or "frame" is passed as NULL."""
    from articulated_pose_amd.pose.gt_pose import gt_pose_batch
    rows, off0, perm, P, ext = _tensors(p, order, clouds, P)
    off = off0 if off is None else off
    with guarded():                                                 # both outputs inside red zones (tests/redzone.py)
        out = None
        if skip:
            out = (None if skip == "gt" else torch.empty((len(order), p["K"], 19), dtype=torch.float64, device="cuda:0"),
                   None if skip == "frame" else torch.empty((len(order), 13), dtype=torch.float64, device="cuda:0"))
        gt, frame = gt_pose_batch(_dev(rows), _dev(off, torch.int32), _dev(perm, torch.int32), _dev(P),
                                  _dev(ext, torch.float64) if extent else None, num_parts=p["K"], out=out)
        torch.cuda.synchronize()
        got = None if gt is None else gt.cpu().numpy(), None if frame is None else frame.cpu().numpy()
    return got


SHAPES = [(64, 1), (64, 3), (257, 2), (300, 4), (1000, 8)]


@pytest.mark.parametrize("N,K", SHAPES, ids=lambda v: str(v))
def test_bit_equal_to_umeyama_on_the_gathered_rows(dev, N, K):
    p = _problem(N, K)
    rows, off, perm, P, ext = _tensors(p)
    want_gt, want_frame, counts = host_tables(rows, off, perm, P, ext, K, rule=False)
    assert (counts > 0).all(), counts                               # random cls: the empty-part rule must not silently remove a case
    assert (counts.sum(1) < N).all()                                # some sampled rows are -1: no part
    gt, frame = _launch(p)
    assert gt.shape == (3, K, 19) and frame.shape == (3, 13) and gt.dtype == frame.dtype == np.float64
    assert np.isfinite(want_gt[:, :, POSE]).all() and np.isfinite(want_frame).all()
    assert _same(gt, want_gt), np.abs(gt - want_gt).max()
    assert _same(frame, want_frame)
    assert _same(gt[:, :, 13:16], p["extent"]) and gt[1, K - 1, 14].view(np.uint64) == 0x7ff8000000000abc      # bit for bit, the payload too
    assert _same(frame[:, 10:], gt[:, 0, NAOCS_T])
    # the extent through a column slice of a (B, K, 19) table, as the pipeline passes it
    from articulated_pose_amd.pose.gt_pose import gt_pose_batch
    table = np.full((3, K, 19), 7.0)
    table[:, :, 13:16] = p["extent"]
    g2, f2 = gt_pose_batch(_dev(rows), _dev(off, torch.int32), _dev(perm, torch.int32), _dev(P), _dev(table, torch.float64)[:, :, 13:16])
    assert _same(g2.cpu().numpy(), gt) and _same(f2.cpu().numpy(), frame)


# ---- against the reference's own numbers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,K,N", [(0, 3, 1024), (1, 4, 2048)])
def test_against_the_reference_numbers(dev, i, K, N):
    from articulated_pose_amd.pose.gt_pose import gt_pose_batch
    g = np.load(GOLDEN)
    P, nocs, cls = g["P%d" % i], g["nocs_gt%d" % i], g["cls_gt%d" % i]
    assert P.shape == (N, 3) and g["rt%d" % i].shape == (K, 4, 4)
    rows = np.zeros((N, 18), np.float32)
    rows[:, :3], rows[:, 3], rows[:, 4:7], rows[:, 7:10] = P, cls, nocs, nocs
    gt, frame = gt_pose_batch(_dev(rows), _dev(np.array([0, N]), torch.int32), _dev(np.arange(N)[None], torch.int32), _dev(P[None]), num_parts=K)
    gt, frame = gt.cpu().numpy()[0], frame.cpu().numpy()[0]
    rt, scale = g["rt%d" % i].astype(np.float64), g["scale%d" % i].astype(np.float64).reshape(K, -1)[:, 0]
    for name, a, b in (("R", gt[:, 0:9], rt[:, :3, :3].reshape(K, 9)), ("t", gt[:, 10:13], rt[:, :3, 3]), ("s", gt[:, 9], scale)):
        print("gt_pose golden %d %s: max |kernel - reference| = %.3g" % (i, name, np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-4)
    assert np.isnan(gt[:, 13:16]).all() and _same(frame[10:], gt[0, NAOCS_T]) and _same(gt[:, NAOCS_T], gt[:, 10:13])      # nocs_g = nocs_p here


# ---- against the float64 oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES, ids=lambda v: str(v))
def test_against_the_float64_oracle(dev, N, K):
    """The scale within 1e-9 * max(1, |w|), tests/test_pose_sweep_gpu.py's bound for ancsh_umeyama; R and t are float32(oracle) up to one
    float32 ulp: the kernel rounds its float64 value once, and a float64 error far below the float32 spacing moves that rounding by at most
    one step."""
    from oracle import pose_oracle as PO
    p = _problem(N, K)
    rows, off, perm, P, _ = _tensors(p)
    gt, frame = _launch(p)
    hom = lambda a: np.vstack([a.T.astype(np.float64), np.ones((1, a.shape[0]))])
    worst_s = worst_ulp = 0.0

    def ulps(got, want):
        w32 = np.asarray(want, np.float64).astype(np.float32)
        return float(np.max(np.abs(got - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)))
    for c in range(3):
        g = gathered(rows, off, perm, c)
        for j in range(K):
            at = np.flatnonzero(g[:, 3].astype(np.int32) == j)
            Sp, Rp, Tp, _ = PO.estimateSimilarityUmeyama(hom(g[at, 4:7]), hom(P[c][at]))
            Sg, Rg, Tg, _ = PO.estimateSimilarityUmeyama(hom(g[at, 7:10]), hom(P[c][at]))
            err = abs(gt[c, j, 9] - Sp[0]) / max(1.0, abs(Sp[0]))
            worst_s = max(worst_s, err)
            assert err <= 1e-9, (c, j, gt[c, j, 9], Sp[0])
            pairs = [(gt[c, j, 0:9], Rp.T.reshape(9)), (gt[c, j, 10:13], Tp), (gt[c, j, NAOCS_T], Tg)]
            if j == 0:
                pairs += [(frame[c, 0:9], Rg.T.reshape(9)), (frame[c, 10:13], Tg)]
                err = abs(frame[c, 9] - Sg[0]) / max(1.0, abs(Sg[0]))
                worst_s = max(worst_s, err)
                assert err <= 1e-9, (c, frame[c, 9], Sg[0])
            for got, want in pairs:
                u = ulps(got, want)
                worst_ulp = max(worst_ulp, u)
                assert u <= 1.0, (c, j, got, want)
    print("gt_pose oracle (%d, %d): worst scale error %.3g (relative to max(1, |w|)), worst R / t difference %.3g float32 ulp" % (N, K, worst_s, worst_ulp))


# ---- the NaN rules ------------------------------------------------------------------------------------------------------------------------
def _nan_problem():
    """(257, 3): four clouds whose perms draw distinct raw rows (n_raw >= N), so that one raw row is one sampled point."""
    rs = np.random.RandomState(77)
    N, K = 257, 3
    clouds = [np.concatenate([rs.uniform(-1, 1, (n_raw, 3)).astype(np.float32), random_channels(rs, n_raw, K)], 1) for n_raw in (300, 257, 700, 411)]
    perms = [rs.permutation(c.shape[0])[:N].astype(np.int32) + (c.shape[0] if k == 2 else 0) for k, c in enumerate(clouds)]
    extent = rs.uniform(0.2, 1.0, (4, K, 3))
    return dict(clouds=clouds, perms=perms, P=rs.normal(size=(4, N, 3)).astype(np.float32), extent=extent, N=N, K=K)


def test_nan_rules_leave_the_neighbours_alone(dev):
    p = _nan_problem()
    K, order = p["K"], (0, 1, 2, 3)
    base_gt, base_fr = _launch(p, order)
    assert np.isfinite(base_gt).all() and np.isfinite(base_fr).all()
    again = _launch(p, order)
    assert _same(again[0], base_gt) and _same(again[1], base_fr)                      # the same batch twice
    moved = _launch(p, (3, 1, 0, 2))
    assert _same(moved[0], base_gt[[3, 1, 0, 2]]) and _same(moved[1], base_fr[[3, 1, 0, 2]])      # wherever the cloud lies
    alone = _launch(p, (1,))
    assert _same(alone[0][0], base_gt[1]) and _same(alone[1][0], base_fr[1])
    bad, ok = 1, [0, 2, 3]
    cloud = p["clouds"][bad]
    sampled = p["perms"][bad] % cloud.shape[0]                                        # distinct raw rows
    part1 = sampled[cloud[sampled, 3] == 1.0]

    def run(cloud_b=None, P=None, **kw):
        clouds = list(p["clouds"])
        if cloud_b is not None:
            clouds[bad] = cloud_b
        gt, fr = _launch(p, order, clouds=clouds, P=P, **kw)
        assert _same(gt[ok], base_gt[ok]) and _same(fr[ok], base_fr[ok])              # a cloud never changes a neighbour's bytes
        return gt[bad], fr[bad]
    # a part with no point: the whole cloud and its frame are NaN, the extents stay
    c = cloud.copy()
    c[c[:, 3] == 2.0, 3] = 0.0
    gt, fr = run(c)
    assert np.isnan(gt[:, POSE]).all() and np.isnan(gt[:, NAOCS_T]).all() and np.isnan(fr).all() and _same(gt[:, 13:16], p["extent"][bad])
    # a part of one point: that row alone is NaN (the other rows' points are unchanged: part 1's other rows belong to no part now)
    for none in (-1.0, float(K), 100.0):
        c = cloud.copy()
        c[part1[1:], 3] = none
        gt, fr = run(c)
        assert np.isnan(gt[1, POSE]).all() and np.isnan(gt[1, NAOCS_T]).all() and _same(gt[1, 13:16], p["extent"][bad, 1])
        assert _same(gt[[0, 2]], base_gt[bad][[0, 2]]) and _same(fr, base_fr[bad])
    # all NOCS of a part equal: varP == 0.  nocs_p alone: the part-NOCS fit's 13 columns; the NAOCS fit keeps its bytes
    c = cloud.copy()
    c[part1, 4:7] = 0.5
    gt, fr = run(c)
    assert np.isnan(gt[1, POSE]).all() and _same(gt[1, 13:], base_gt[bad, 1, 13:]) and _same(gt[[0, 2]], base_gt[bad][[0, 2]]) and _same(fr, base_fr[bad])
    c[part1, 7:10] = 0.25
    gt, fr = run(c)
    assert np.isnan(gt[1, POSE]).all() and np.isnan(gt[1, NAOCS_T]).all() and _same(gt[[0, 2]], base_gt[bad][[0, 2]]) and _same(fr, base_fr[bad])
    c = cloud.copy()
    c[sampled[cloud[sampled, 3] == 0.0], 7:10] = 0.25                                 # part 0's NAOCS: its translation and the frame
    gt, fr = run(c)
    assert np.isnan(fr).all() and np.isnan(gt[0, NAOCS_T]).all() and _same(gt[:, :16], base_gt[bad][:, :16]) and _same(gt[1:], base_gt[bad][1:])
    # a NaN point in P, in part 1
    P = p["P"].copy()
    at = int(np.flatnonzero(cloud[sampled, 3] == 1.0)[3])
    P[bad, at, 1] = np.nan
    gt, fr = run(P=P)
    assert np.isnan(gt[1, POSE]).all() and np.isnan(gt[1, NAOCS_T]).all() and _same(gt[[0, 2]], base_gt[bad][[0, 2]]) and _same(fr, base_fr[bad])
    P[bad, at, 1] = np.inf
    gt, fr = run(P=P)
    assert np.isnan(gt[1, POSE]).all() and np.isnan(gt[1, NAOCS_T]).all() and _same(gt[[0, 2]], base_gt[bad][[0, 2]])
    # cls = -1 rows are ignored: what they hold changes nothing
    c = cloud.copy()
    c[c[:, 3] == -1.0, 4:10] = np.nan
    assert (c[sampled, 3] == -1.0).any()
    gt, fr = run(c)
    assert _same(gt, base_gt[bad]) and _same(fr, base_fr[bad])
    # an empty cloud (the host refuses it): NaN throughout, the extents too
    _, off, *_ = _tensors(p, order)
    empty = off.copy()
    empty[1] = empty[2]                                                               # cloud 0 grows over cloud 1's rows, cloud 1 is [off[2], off[2])
    gt_e, fr_e = _launch(p, order, off=empty)
    assert np.isnan(gt_e[1]).all() and np.isnan(fr_e[1]).all() and _same(gt_e[[2, 3]], base_gt[[2, 3]]) and _same(fr_e[[2, 3]], base_fr[[2, 3]])
    # extent NULL: NaN extents, every other byte as before
    gt_n, fr_n = _launch(p, order, extent=False)
    assert np.isnan(gt_n[:, :, 13:16]).all() and _same(gt_n[:, :, POSE], base_gt[:, :, POSE]) and _same(gt_n[:, :, NAOCS_T], base_gt[:, :, NAOCS_T])
    assert _same(fr_n, base_fr)
    # gt NULL and frame NULL, each on its own
    none, fr_only = _launch(p, order, skip="gt")
    gt_only, none2 = _launch(p, order, skip="frame")
    assert none is None and none2 is None and _same(fr_only, base_fr) and _same(gt_only, base_gt)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
def slot_tables(pipe, sl, extents, n):
    """The host's tables for the batch slot sl holds, from the slot's own rows, offsets, perm and P; and the step's tables equal
    gt_pose_batch on the same tensors."""
    from articulated_pose_amd.pose.gt_pose import gt_pose_batch
    sl.stream.synchronize()
    off_d = sl.header(pipe.B)[1]
    want = gt_pose_batch(sl.raw_rows, off_d, sl.perm, sl.P, None if sl.gt is None else sl.gt[:, :, 13:16], num_parts=pipe.K)
    torch.cuda.synchronize()
    assert _same(sl.out["gt_pose"].cpu().numpy(), want[0].cpu().numpy()) and _same(sl.out["gt_frame"].cpu().numpy(), want[1].cpu().numpy())
    assert sl.out["gt_pose"].shape == (pipe.B, pipe.K, 19) and sl.out["gt_frame"].shape == (pipe.B, 13) and sl.frame is None
    off = off_d.cpu().numpy()[:n + 1]
    gt, frame, counts = host_tables(sl.raw_rows.cpu().numpy(), off, sl.perm.cpu().numpy(), sl.P.cpu().numpy(), extents, pipe.K)
    assert _same(sl.out["gt_pose"].cpu().numpy()[:n], gt) and _same(sl.out["gt_frame"].cpu().numpy()[:n], frame)      # ancsh_umeyama's bits
    return gt, frame, counts


@pytest.mark.parametrize("fit_quality", [False, True], ids=["record", "wide"])
def test_stream_equals_the_pipeline_fed_host_tables(dev, fit_quality):
    """Pipeline A fits the tables in the captured step; pipeline B is the parent's, fed the tables compute_gt_pose.py's arithmetic gives for
    the very points A sampled (same seeds, so it samples them again).  Records equal byte for byte."""
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 6, np.random.RandomState(2))               # a short batch at k = 0, a NaN cloud in batch 5
    rs = np.random.RandomState(17)
    wide = widen(plain, rs)
    extents = [rs.uniform(0.2, 1.0, (len(b[0]), K_, 3)) for b in plain]
    extents[3] = None                                               # a batch without boxes: gt=None
    kw = dict(fit_quality=fit_quality, ground_truth=True, point_ground_truth=True)
    ld = (39 if fit_quality else 26) + 12
    A = _pipe(pb, build_gt_pose=True, **kw).prepare()
    assert A.slots[0].gt_built.shape == (B_, K_, 19) and A.slots[0].frame_built.shape == (B_, 13) and A.slots[0].frame is None
    assert [i.name for i in A.opts.inputs] == ["gt"] and A.slots[0].outputs["record"].host[0].shape == (B_, K_, ld + 21)
    feed = [(c, nf, None if e is None else pack_box_extents(list(e))) for (c, nf), e in zip(wide, extents)]
    got_a, tables = [], []
    for k, (tag, seed, rec) in enumerate(A.stream_batches(feed)):
        assert (tag, seed) == (k, 11 + 2 * k) and rec.shape == (len(wide[k][0]), K_, ld + 21)
        gt, frame, counts = slot_tables(A, A.slots[k % 2], extents[k], len(rec))
        if k == 5:                                                  # the NaN cloud: every fit is non-finite -- an all-NaN gt / frame
            assert np.isnan(gt[1][:, POSE]).all() and np.isnan(gt[1][:, NAOCS_T]).all() and np.isnan(frame[1]).all()
            gt[1] = np.nan
        assert (counts > 0).all() and np.isfinite(gt[0][:, POSE]).all()
        got_a.append(rec)
        tables.append((gt, frame))
    assert len(got_a) == 6
    B = _pipe(pb, **kw)
    got_b = list(B.stream_batches([(c, nf, gt, frame) for (c, nf), (gt, frame) in zip(wide, tables)]))
    for k, (rec, (_, seed, want)) in enumerate(zip(got_a, got_b)):
        assert seed == 11 + 2 * k and _same(rec, want), k
        assert np.isfinite(rec[0, :, ld - 12:ld - 9]).all() and np.isfinite(rec[0, 1:, ld:ld + 8]).any(), k      # errors against the fitted poses
        iou = rec[:, :, [ld - 12 + 3, ld - 12 + 8]]
        assert np.isnan(iou).all() == (extents[k] is None), k       # without boxes only the two IoU columns are missing
    assert np.isnan(got_a[5][1][:, ld - 12:ld - 9]).all()           # the NaN cloud: B read an all-NaN gt / frame for it, and streamed the same bytes
    with pytest.raises(ValueError, match="the device builds it"):
        A.submit(wide[1][0], wide[1][1], frame=np.zeros((len(wide[1][0]), 13)))
    assert not A._inflight


def test_launch_budget(dev):
    """The option adds ancsh_gt_pose_build -- one ABI call -- directly behind the sampler; the rest of the step is the same list."""
    from test_fit_quality_gpu import _launch_names
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    for kw in (dict(joint_states=True, fit_quality=True, ground_truth=True, dense=True, build_point_gt=True), dict(ground_truth=True),
               dict(joint_source="predicted")):
        kw = dict(kw, slots=1, point_ground_truth=True)
        off = _launch_names(_pipe(pb, **kw).prepare())
        again = _launch_names(_pipe(pb, build_gt_pose=False, **kw).prepare())
        on = _launch_names(_pipe(pb, build_gt_pose=True, **kw).prepare())
        at = on.index("ancsh_gt_pose_build")
        assert on[at - 1].startswith("ancsh_input_sample_stream") and on[:at] + on[at + 1:] == off and again == off
        assert "ancsh_gt_pose_build" not in off


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
def test_with_rows_built_on_the_device(dev):
    """build_point_gt=True: annotated clouds and rigs in, the rows built in front of the sampler, the poses fitted behind it."""
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    from test_point_gt_build_gpu import annotate
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    rs = np.random.RandomState(21)
    batches = annotate(_batches(pb, 3, np.random.RandomState(4)), rs)
    extents = [rs.uniform(0.2, 1.0, (len(b[0]), K_, 3)) for b in batches]
    kw = dict(ground_truth=True, point_ground_truth=True, build_point_gt=True, keyed=True, joint_states=True)
    A, B = _pipe(pb, build_gt_pose=True, **kw), _pipe(pb, **kw)
    assert [i.name for i in A.opts.inputs] == ["gt", "rig"]
    for k, ((clouds7, nf, rigs), e) in enumerate(zip(batches, extents)):
        A.submit(clouds7, nf, gt=pack_box_extents(list(e)), rig=rigs, cloud_base=5 * k)
        _, sa, ra = A.retire()
        gt, frame, counts = slot_tables(A, A.slots[k % 2], e, len(ra))
        B.submit(clouds7, nf, gt=gt, frame=frame, rig=rigs, cloud_base=5 * k)
        _, sb, rb = B.retire()
        assert sa == sb and _same(ra, rb) and ra.shape[2] == 26 + 12 + 21, k
        assert np.isfinite(ra[:, :, 26:29]).all() and (counts > 0).all()


def test_with_annotated_depth_frames(dev):
    """Rendered depth frame + scene + rig in, every table out: the annotated depth stream's records equal those of the xyz build_point_gt
    pipeline fed depth.annotate_depth_batch's rows, both with build_gt_pose=True, and the fitted poses are the host's."""
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    from test_depth_annotate_gpu import K_ as K, _batch, _bytes, _clouds, _pipes, _weights
    pb = _weights()
    rs = np.random.RandomState(33)
    batches = [_batch(rs, "uint16", n) for n in (2, 1)]
    A, X = _pipes(pb, "uint16", ground_truth=True, build_gt_pose=True)
    assert [i.name for i in A.opts.inputs] == ["scene", "gt", "rig"] and [i.name for i in X.opts.inputs] == ["gt", "rig"]
    for k, (frames, nf, tables, rigs, _) in enumerate(batches):
        clouds, cnt, lc = _clouds(frames, tables, "uint16")
        e = rs.uniform(0.2, 1.0, (len(frames), K, 3))
        A.submit_depth(frames, nf, scene=tables, rig=rigs, gt=pack_box_extents(list(e)))
        X.submit(clouds, nf, rig=rigs, gt=pack_box_extents(list(e)))
        ga, gx = A.retire(), X.retire()
        assert ga[:2] == gx[:2] and ga[2].shape == (len(frames), K, 26 + 12 + 21) and _bytes(ga[2], gx[2]) and np.array_equal(ga[3], cnt), k
        gt, frame, counts = slot_tables(A, A.slots[k % 2], e, len(frames))
        for name in ("gt_pose", "gt_frame"):
            assert _bytes(A.slots[k % 2].out[name].cpu().numpy(), X.slots[k % 2].out[name].cpu().numpy()), (k, name)
        assert (counts > 0).all() and np.isfinite(gt).all() and np.isfinite(frame).all()
        assert np.isfinite(ga[2][:, :, 26:30]).any()                # rpy / xyz / scale errors and the IoU against the fitted poses
    with pytest.raises(ValueError, match="the device builds it"):
        A.submit_depth(frames, nf, scene=tables, rig=rigs, frame=np.zeros((len(frames), 13)))


def test_range_guard_refit_rows_carry_the_same_poses(dev):
    """One cloud forced over f16's range by its norm factor: its row is the f32 graph's, which fits the same ground-truth poses -- the fits
    read no network output --, so the guarded stream equals a guarded parent pipeline fed the host tables."""
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 2, np.random.RandomState(9))
    plain[1][1][0] = 1e6
    rs = np.random.RandomState(6)
    wide = widen(plain, rs)
    extents = [rs.uniform(0.2, 1.0, (len(b[0]), K_, 3)) for b in plain]
    kw = dict(arithmetic="f16x2", range_guard=True, ground_truth=True, point_ground_truth=True)
    A, B = _pipe(pb, build_gt_pose=True, **kw), _pipe(pb, **kw)
    for k, ((clouds, nf), e) in enumerate(zip(wide, extents)):
        A.submit(clouds, nf, gt=pack_box_extents(list(e)))
        _, _, ra, wa = A.retire(flags=True)
        sl = A.slots[k % 2]
        gt, frame, _ = slot_tables(A, sl, e, len(ra))
        if k == 1:                                                  # the refit ran: the f32 graph left the same tables in the slot
            assert wa[0] != 0 and _same(sl.out32["gt_pose"].cpu().numpy()[:len(ra)], gt) and sl.out32["gt_pose"] is sl.out["gt_pose"]
        B.submit(clouds, nf, gt=gt, frame=frame)
        _, _, rb, wb = B.retire(flags=True)
        assert _same(ra, rb) and _same(wa, wb), k
    assert A.f32_reruns == B.f32_reruns == 1


def sharded_gt_pose_problem():
    """tests/test_point_gt_gpu.py's sharded batches with box extents in the frames' place."""
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    from test_point_gt_gpu import sharded_point_gt_problem
    pb, batches, K, G, N, kw = sharded_point_gt_problem()
    rs = np.random.RandomState(47)
    return pb, [(c, nf, None if k == 2 else pack_box_extents(list(rs.uniform(0.2, 1.0, (len(c), K, 3)))), tag)
                for k, (c, nf, _, tag) in enumerate(batches)], K, G, N, kw


_SHARDED = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import articulated_pose_amd  # noqa: F401
from articulated_pose_amd import dist as D
sys.path.insert(0, sys.argv[1] + "/tests")
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=300))
import torch.distributed as dist
from test_gt_pose_gpu import sharded_gt_pose_problem
pb, batches, K, G, N, kw = sharded_gt_pose_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, articulation=True, ground_truth=True,
                       point_ground_truth=True, build_gt_pose=True, **kw)
got = list(sp.stream_batches(batches))
if dist.get_rank() != 0:
    assert all(r is None for _, _, r in got)
    got = None
dist.barrier()
dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _ in got]), counts=np.array([len(r) for _, _, r in got]), records=np.concatenate([r for _, _, r in got]))
'''


def test_sharded_rows_equal_one_pipeline(dev, tmp_path):
    """Two self-launched gloo ranks on one GPU (as tests/test_point_gt_gpu.py runs them): every rank fits its shard's poses and gets its
    shard's extents, and rank 0's gathered (n_valid, K, 59) rows equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    pb, batches, K, G, N, kw = sharded_gt_pose_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, articulation=True, ground_truth=True,
                         point_ground_truth=True, build_gt_pose=True, **kw)
    one = list(pipe.stream_batches(batches))
    del pipe
    script = tmp_path / "sharded_gt_pose.py"
    script.write_text(_SHARDED)
    out = tmp_path / "gtp2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r in one]
    assert two["records"].shape[1:] == (K, 59) and _same(two["records"], np.concatenate([r for _, _, r in one]))
    recs = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isfinite(recs[1][:, :, 26:30]).any() and np.isnan(recs[2][:, :, [29, 34]]).all() and np.isfinite(recs[2][:, :, 26:29]).any()
