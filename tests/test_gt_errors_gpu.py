"""GPU: the errors against ground truth (ancsh_gt_error_rec, pose.gt_errors.gt_error_batch, AncshPipeline / ShardedPipeline
ground_truth=True) against the numpy mirror (tests/gt_errors_mirror.py, pinned against the oracle by tests/test_gt_errors_cpu.py),
against the offline product path (metrics.amodal_boxes + iou_3d_batch, rot_diff_degree_batch, ancsh_part_extents,
ancsh_joint_state_rec) and through the captured stream, the depth front end, the fit-quality wide record, the range guard and two gloo
ranks.

Against the mirror: the carried columns, the point count and the IoU (a quotient of two integer counts, on inputs whose grid keeps
1e-9 clear of every face) are byte-equal; the float columns agree to 1e-9 absolute, the bound tests/test_gt_errors_cpu.py derives (the
test prints the largest difference per launch)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gt_errors_mirror as GM
from helpers import check_record_layout, passthrough_pose_problem
from redzone import guarded
from test_gt_errors_cpu import _rotation, make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOAD = np.frombuffer(np.array([0x7ff8000000000abc], np.uint64).tobytes(), np.float64)[0]       # a NaN with a payload
# b in {1, 3}, K in {1, 2, 3}, n in {1, 65, 300} (one point; one more than a wave; more than the part pass's 256 threads), nres = 50 (2500
# columns: three trips of the 1024 threads, the last one partial) and once 7 (49 columns: fewer than a wave's worth of threads busy)
LAUNCHES = {"b1-K1-n1": dict(seed=1, B=1, K=1, n=1, ld=26, nres=50),
            "b3-K2-n65-wide": dict(seed=2, B=3, K=2, n=65, ld=39, nres=50, exact=(1, 1, 1)),
            "b3-K3-n300": dict(seed=3, B=3, K=3, n=300, ld=26, nres=50, empty=(2, 1), nan_pose=(1, 2, 0, 11)),
            "b1-K3-n65-nres7": dict(seed=4, B=1, K=3, n=65, ld=26, nres=7),
            "nan-rules": dict(seed=7, B=2, K=3, n=40, ld=39, nres=7)}
FLOAT = (0, 1, 2, 4, 5, 6, 7, 9, 10)
EXACT = (3, 8, 11)


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a, dt):
    return torch.as_tensor(np.array(a)).to("cuda:0", dt).contiguous()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Seeded clouds, heads, records and ground truth (host arrays, never modified) and the mirror's block for them."""
    kw = dict(LAUNCHES[name])
    nres = kw.pop("nres")
    P, nocs, mask, rec, gt = make_case(**kw)
    if name == "nan-rules":                                              # tests/test_gt_errors_cpu.py's hand-made batch
        gt[0, :, 16:] = np.nan                                           # cloud 0: no NAOCS translations
        gt[1, 2] = np.nan                                                # cloud 1: part 2 has no ground truth
        rec[1, 0, 13 + 9] = np.nan                                       # cloud 1: a NaN in part 0's nonlinear pose
        rec[0, 1, 30] = PAYLOAD                                          # a NaN payload in the carried row
    want, counts = GM.gt_error_reference(P, nocs, mask, rec, gt, nres, return_counts=True)
    clear = min([v[2] for v in counts.values()] or [np.inf])
    assert clear > 1e-9, (name, clear)                                   # the counts below do not depend on the last bit of a projection
    for a in (P, nocs, mask, rec, gt, want):
        a.setflags(write=False)
    return dict(P=P, nocs=nocs, mask=mask, rec=rec, gt=gt, nres=nres, want=want, counts=counts, ld=kw["ld"])


def _launch(p, sel=slice(None)):
    """gt_error_batch on problem p (sel: some of its clouds), its output carved out of a guarded allocation -> the block on the host."""
    from articulated_pose_amd.pose.gt_errors import gt_error_batch
    with guarded():
        wide = gt_error_batch(_dev(p["P"][sel], torch.float32), _dev(p["nocs"][sel], torch.float32), _dev(p["mask"][sel], torch.float32),
                              _dev(p["rec"][sel], torch.float64), _dev(p["gt"][sel], torch.float64), p["nres"])
        torch.cuda.synchronize()
        out = wide.cpu().numpy()
    return out


def _agree(got, want, ld, what):
    """got, want (..., ld + 12): byte-equal in the carried columns, the IoU and the point count; the float columns within 1e-9."""
    assert got.shape == want.shape and _same(got[..., :ld], want[..., :ld]), what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert _same(got[..., [ld + c for c in EXACT]], want[..., [ld + c for c in EXACT]]), what
    g, w = got[..., [ld + c for c in FLOAT]], want[..., [ld + c for c in FLOAT]]
    fin = np.isfinite(w)
    worst = np.abs(g[fin] - w[fin]).max() if fin.any() else 0.0
    print("gt_errors %s: max |kernel - mirror| over the float columns = %.3g" % (what, worst))
    assert worst <= 1e-9, (what, worst)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_kernel_against_mirror(dev, name):
    p = _problem(name)
    ld, want = p["ld"], p["want"]
    got = _launch(p)                                                     # inside red zones around wide (tests/redzone.py)
    _agree(got, want, ld, name)
    assert _same(_launch(p), got)                                        # two runs, identical bytes
    if name == "b3-K3-n300":
        # an empty part: no box, no boundary; its pose errors stand.  A NaN in a baseline pose: that pose's five columns only
        assert got[2, 1, ld + 11] == 0 and np.isnan(got[2, 1, [ld + 3, ld + 8, ld + 10]]).all() and np.isfinite(got[2, 1, [ld, ld + 1, ld + 2, ld + 4]]).all()
        assert np.isnan(got[1, 2, ld:ld + 5]).all() and np.isfinite(got[1, 2, ld + 5:ld + 12]).all() and np.isfinite(got[1, 1, ld:ld + 12]).all()
        assert np.isnan(got[:, 0, [ld + 4, ld + 9, ld + 10]]).all() and np.isfinite(got[0, 1:, ld:ld + 12]).all()
        assert (got[0, :, ld + 3] > 0).all() and (got[0, :, ld + 8] < 1).all()            # boxes 0.01 .. 30 degrees and <= 0.1 apart overlap
    if name == "b3-K2-n65-wide":
        assert got[1, 1, ld + 6] == 0.0 and got[1, 1, ld + 7] == 0.0 and got[1, 1, ld + 8] > 0      # the exact pose
    if name == "b1-K1-n1":
        assert got.shape == (1, 1, 38) and np.isnan(got[0, 0, [30, 35, 36]]).all() and got[0, 0, 37] == 1 and np.isfinite(got[0, 0, [29, 34]]).all()
    if name == "nan-rules":
        assert got[0, 1, 30].view(np.uint64) == 0x7ff8000000000abc
        assert np.isnan(got[0, :, 49]).all() and np.isfinite(got[0, :, 39:43]).all() and np.isfinite(got[0, 1:, [43, 48]]).all()
        assert np.isnan(got[1, 2, 39:50]).all() and got[1, 2, 50] > 0
        assert np.isnan(got[1, 0, 44:50]).all() and np.isfinite(got[1, 0, 39:43]).all()
        assert np.isnan(got[1, 1, [48, 49]]).all() and np.isfinite(got[1, 1, 39:48]).all()


def test_same_bytes_wherever_the_cloud_lies(dev):
    """Cloud 0 again as cloud 2 of the batch, and alone: the same bytes."""
    p = _problem("b3-K3-n300")
    twice = {k: np.concatenate([p[k][:2], p[k][:1]]) for k in ("P", "nocs", "mask", "rec", "gt")}
    got = _launch(dict(p, **twice))
    assert _same(got[0], got[2]) and _same(got[:2], _launch(p)[:2]) and _same(_launch(p, slice(0, 1))[0], got[2])


def test_kernel_against_the_offline_product_path(dev):
    """The same inputs through what the offline scripts call: ancsh_part_extents, metrics.amodal_boxes + iou_3d_batch (counts equal on
    these clear inputs, so the quotient is the same double), rot_diff_degree_batch, and ancsh_joint_state_rec's boundary slide."""
    from articulated_pose_amd.pose import metrics as M
    from articulated_pose_amd.pose.evaluation import part_extents
    from articulated_pose_amd.pose.joint_params import joint_state_batch
    for name in ("b3-K3-n300", "b3-K2-n65-wide"):
        p = _problem(name)
        ld, rec, gt, got = p["ld"], p["rec"], p["gt"], _launch(p)
        B, K = rec.shape[:2]
        f64 = lambda a: _dev(a, torch.float64)
        nocs, mask, P = _dev(p["nocs"], torch.float32), _dev(p["mask"], torch.float32), _dev(p["P"], torch.float32)
        sc, dy, cnt = part_extents(nocs, mask, P, rec[:, 0, 13:22].reshape(B, 3, 3), rec[:, 0, 23:26])
        assert np.array_equal(got[:, :, ld + 11], cnt.cpu().numpy())
        box_gt = M.amodal_boxes(f64(gt[:, :, 13:16]), f64(gt[:, :, 9]), f64(gt[:, :, :9].reshape(B, K, 3, 3)), f64(gt[:, :, 10:13]))
        full = (cnt.cpu().numpy() > 0)
        for q in range(2):
            m = rec[:, :, 13 * q:13 * q + 13]
            ok = full & ~np.isnan(m).any(2)
            R32 = f64(m[:, :, :9].reshape(B, K, 3, 3)).float().double()
            box_pr = M.amodal_boxes(sc.double(), f64(m[:, :, 9]), R32, f64(m[:, :, 10:13]).float().double())
            iou = M.iou_3d_batch(box_gt.reshape(B * K, 8, 3), box_pr.reshape(B * K, 8, 3), nres=p["nres"]).reshape(B, K).cpu().numpy()
            assert ok.sum() >= B * K - 2 and _same(got[:, :, ld + 3 + 5 * q][ok], iou[ok]), (name, q)
            rpy = M.rot_diff_degree_batch(f64(m[:, :, :9].reshape(B, K, 3, 3)), f64(gt[:, :, :9].reshape(B, K, 3, 3))).cpu().numpy()
            fin = ~np.isnan(m).any(2) & np.isfinite(rpy)
            assert np.abs(got[:, :, ld + 5 * q][fin] - rpy[fin]).max() <= 1e-9
    # the boundary slide: with R_0 = I and equal NAOCS translations the relative translation error IS |dynam - canon|, bit for bit
    p = _problem("b3-K3-n300")
    rec, gt = np.array(p["rec"]), np.array(p["gt"])
    rec[:, 0, 13:22] = np.eye(3).reshape(9)
    gt[:, :, 16:19] = 0.25
    got = _launch(dict(p, rec=rec, gt=gt))
    js = joint_state_batch(_dev(p["P"], torch.float32), dict(nocs_per_point=_dev(p["nocs"], torch.float32), W=_dev(p["mask"], torch.float32)),
                           _dev(rec, torch.float64), torch.zeros((3, 3, 12), dtype=torch.float64, device=dev)).cpu().numpy()
    assert np.isfinite(js[[0, 1], 1:, 18]).all() and np.isnan(js[2, 1, 18])
    assert np.array_equal(got[:, 1:, 36], np.abs(js[:, 1:, 18]), equal_nan=True) and np.array_equal(got[:, :, 37], js[:, :, 19])


def test_solver_option_and_capture(dev):
    """PoseSolver.solve(ground_truth=gt) adds "record_gt" next to "record" (and "record_wide"); the launch replays from a captured graph
    with changed inputs behind the same pointers."""
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.gt_errors import gt_error_batch
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    K, N = 3, 300
    cl = [make_cloud(50 + i, N=N, K=K) for i in range(2)]
    pr = [make_predictions(c, K, seed=i) for i, c in enumerate(cl)]
    st = lambda k: np.stack([q[k] for q in pr])
    args = (np.stack([c["P"] for c in cl]), st("nocs_per_point"), st("instance_per_point"), st("joint_axis_per_point"), st("joint_cls_gt"))
    gt = _dev(_random_gt(np.random.RandomState(0), 2, K), torch.float64)
    solver = PoseSolver(K, 0.1, 64, 8, "cuda:0", lm_schedule="throughput")
    plain = solver.solve(*args, seed=5)
    assert "record_gt" not in plain
    sol = solver.solve(*args, seed=5, ground_truth=gt)
    both = solver.solve(*args, seed=5, ground_truth=gt, fit_quality=True)
    torch.cuda.synchronize()
    r38, r51 = sol["record_gt"].cpu().numpy(), both["record_gt"].cpu().numpy()
    assert r38.shape == (2, K, 38) and r51.shape == (2, K, 51) and sol["record"].shape == (2, K, 26) and "record_wide" not in sol
    assert _same(r38[:, :, :26], plain["record"].cpu().numpy()) and _same(r51[:, :, :39], both["record_wide"].cpu().numpy())
    assert _same(r38[:, :, 26:], r51[:, :, 39:])
    # captured: the same bytes, and new ones after the ground truth changed behind the same pointer
    P, nocs, mask = (_dev(a, torch.float32) for a in args[:3])
    rec = sol["record"].clone()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        eager = gt_error_batch(P, nocs, mask, rec, gt)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = gt_error_batch(P, nocs, mask, rec, gt)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), eager.cpu().numpy()) and _same(out.cpu().numpy(), r38)
    gt.copy_(_dev(_random_gt(np.random.RandomState(1), 2, K), torch.float64))
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not _same(got, r38) and _same(got, gt_error_batch(P, nocs, mask, rec, gt).cpu().numpy())


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
K_, B_, N_ = 3, 4, 512                                             # the set-up of tests/test_fit_quality_gpu.py's stream tests


def _random_gt(rs, n, K):
    """(n, K, 19) ground truth near the passthrough problem's clouds: any finite rows serve a byte comparison."""
    gt = np.zeros((n, K, 19))
    for c in range(n):
        for j in range(K):
            gt[c, j] = np.concatenate([_rotation(rs).reshape(9), [rs.uniform(0.5, 1.5)], rs.uniform(-0.3, 0.3, 3), rs.uniform(0.3, 0.9, 3),
                                       rs.uniform(-0.3, 0.3, 3)])
    return gt


def _with_gt(batches, rs, none_at=()):
    """(clouds, norm factors) -> (clouds, norm factors, gt): random ground truth, None for the batches in none_at."""
    return [(c, nf, None if k in none_at else _random_gt(rs, len(c), K_)) for k, (c, nf) in enumerate(batches)]


def _batches(pb, count, rs):
    from test_articulation_gpu import _stream_batches
    return _stream_batches(pb, K_, B_, N_, count, rs)              # a short batch at k = 0, a NaN cloud in batch 5


def _pipe(pb, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", raw_capacity=B_ * 3 * N_), **kw)
    return AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **kw)


def _check_against_batch_call(pipe, k, rows, gt):
    """rows = batch k's retired records; its slot (k mod slots: a slot is reused only by a later submit) still holds that batch's P,
    NPCS heads, record and ground truth: gt_error_batch on them gives the streamed rows, byte for byte."""
    from articulated_pose_amd.pose.gt_errors import gt_error_batch
    sl = pipe.slots[k % len(pipe.slots)]
    sl.stream.synchronize()
    out = sl.out
    carried = out["record_wide"] if pipe.fit_quality else out["record"]
    ld = carried.shape[2]
    L = pipe.record_layout
    assert out[L.carried("gt_errors")[0]] is carried and L.carried("gt_errors")[1] == ld and L.key == "record_gt" and L.width == rows.shape[2]
    assert out["record"].shape == (pipe.B, pipe.K, 26) and out["record_gt"].shape == (pipe.B, pipe.K, ld + 12) == (pipe.B, pipe.K, rows.shape[2])
    n = len(rows)
    dev_gt = sl.gt.cpu().numpy()
    assert np.isnan(dev_gt[n:]).all() and (_same(dev_gt[:n], gt) if gt is not None else np.isnan(dev_gt).all())
    want = gt_error_batch(sl.P, out["npcs"]["nocs_per_point"].contiguous(), out["npcs"]["W"].contiguous(), carried, sl.gt)
    torch.cuda.synchronize()
    assert _same(rows, want.cpu().numpy()[:n]) and _same(rows, out["record_gt"].cpu().numpy()[:n])
    return ld


@pytest.mark.parametrize("fit_quality", [False, True], ids=["record", "wide"])
def test_stream_keeps_the_record_and_adds_the_errors(dev, fit_quality):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 6, np.random.RandomState(2))
    batches = _with_gt(plain, np.random.RandomState(5), none_at=(3,))
    base = list(_pipe(pb, fit_quality=fit_quality).stream_batches(plain))
    pipe = _pipe(pb, fit_quality=fit_quality, ground_truth=True).prepare()
    ld = 39 if fit_quality else 26
    assert pipe.slots[0].outputs["record"].host[0].shape == (B_, K_, ld + 12) and pipe.slots[0].gt.shape == (B_, K_, 19)
    L = check_record_layout(pipe, ["pose"] + ["fit_quality"] * fit_quality + ["gt_errors"])
    n = 0
    for k, ((t0, s0, r0), (t1, s1, r1)) in enumerate(zip(base, pipe.stream_batches(batches))):
        clouds, _, gt = batches[k]
        assert (t0, s0) == (t1, s1) == (k, 11 + 2 * k) and r1.shape == (len(clouds), K_, ld + 12)
        assert _same(r0, r1[..., :ld])                               # the record (and the fit quality) of the pipeline without the option
        assert L.width == r1.shape[2] and _same(L.block(r1, "gt_errors"), r1[..., ld:]) and _same(L.block(r1, "pose"), r0[..., :26])
        assert _check_against_batch_call(pipe, k, r1, gt) == ld
        assert (r1[:, :, ld + 11].sum(1) == N_).all()
        if gt is None:
            assert np.isnan(r1[:, :, ld:ld + 11]).all()
        elif k == 5:                                                 # the NaN cloud: a poisoned record has no errors
            assert np.isnan(r1[1, :, ld:ld + 11]).all()
        else:
            assert np.isfinite(r1[:, :, ld:ld + 3]).any() and not np.isnan(r1[:, :, ld + 11]).any()
        n += 1
    assert n == 6
    # (clouds, norm factors, gt, tag) items; a gt of the wrong shape is refused and the stream goes on
    with pytest.raises(ValueError, match=r"gt must be \(%d, 3, 19\)" % len(plain[1][0])):
        pipe.submit(plain[1][0], plain[1][1], gt=np.zeros((len(plain[1][0]) + 1, K_, 19)))
    tagged = list(pipe.stream_batches([b + ("t%d" % k,) for k, b in enumerate(batches[:2])]))
    assert [t[0] for t in tagged] == ["t0", "t1"] and tagged[0][2].shape == (len(plain[0][0]), K_, ld + 12)


def test_launch_budget(dev):
    """Exactly one ABI call more with the option, the last of the fit: behind the record poison and the fit-quality launch."""
    from test_fit_quality_gpu import _launch_names
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    for kw in (dict(fit_quality=True, articulation=True), dict()):
        plain = _launch_names(_pipe(pb, slots=1, **kw).prepare())
        on = _launch_names(_pipe(pb, slots=1, ground_truth=True, **kw).prepare())
        at = on.index("ancsh_gt_error_rec")
        assert "ancsh_gt_error_rec" not in plain and on[:at] + on[at + 1:] == plain
        assert on[at - 1] == ("ancsh_fit_quality_rec" if kw else "ancsh_pose_poison_records")
        if kw:
            assert on[at + 1] == "ancsh_articulation_rec"


def test_depth_stream_carries_the_errors(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_depth_gpu import SIDE, _camera, _depth_batches, _scale
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _depth_batches(pb, 3, 2, np.random.RandomState(4), "uint16", short_last=False)        # two small crops a batch
    rs = np.random.RandomState(8)
    gts = [_random_gt(rs, 2, K_), None, _random_gt(rs, 2, K_)]
    batches = [(f, nf) + ((dict(gt=g),) if g is not None else ()) for (f, nf), g in zip(plain, gts)]
    mk = lambda **kw: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], 2, N_, "cuda:0", couple=True, slots=2, niter_a=64, niter_b=8, seed=11,
                                    lm_schedule="throughput", depth_capacity=2 * SIDE * SIDE, joint_source="predicted", **kw)
    base = list(mk().stream_depth_batches(plain, _camera(), _scale("uint16")))
    pipe = mk(ground_truth=True)
    n = 0
    for k, ((t0, s0, r0, c0), (t1, s1, r1, c1)) in enumerate(zip(base, pipe.stream_depth_batches(batches, _camera(), _scale("uint16")))):
        assert (t0, s0) == (t1, s1) and r1.shape == (2, K_, 38) and _same(r0, r1[..., :26]) and _same(c0, c1)
        _check_against_batch_call(pipe, k, r1, gts[k])
        assert np.isnan(r1[:, :, 26:37]).all() == (gts[k] is None)
        n += 1
    assert n == 3


def test_range_guard_takes_the_f32_rows(dev):
    """One cloud forced over f16's range by its norm factor, as tests/test_fit_quality_gpu.py does: its 38 columns are the f32 graph's."""
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 4, np.random.RandomState(9))
    hot = []
    for k, (clouds, nf) in enumerate(plain):
        h = np.zeros(len(clouds), bool)
        if k % 2 == 1:
            nf[0] = 1e6
            h[0] = True
        hot.append(h)
    batches = _with_gt(plain, np.random.RandomState(6))
    mk = lambda arith, guard: _pipe(pb, arithmetic=arith, range_guard=guard, ground_truth=True)
    f32 = list(mk("f32", False).stream_batches(batches))
    f16 = list(mk("f16x2", False).stream_batches(batches))
    guarded_pipe = mk("f16x2", True)
    assert guarded_pipe.slots[0].outputs["record"].host32[0].shape == (B_, K_, 38)
    got = list(guarded_pipe.stream_batches(batches, flags=True))
    assert guarded_pipe.f32_reruns == 2
    for (tag, _, rec, words), (_, _, r32), (_, _, r16), h in zip(got, f32, f16, hot):
        assert ((words != 0) == h).all() and rec.shape[2] == 38, tag
        assert _same(rec[h], r32[h]) and _same(rec[~h], r16[~h]), tag


def sharded_gt_problem():
    """tests/test_joint_states_gpu.py's global batches with ground truth in front of the tag; batch 2 travels without."""
    from test_joint_states_gpu import sharded_problem
    pb, batches, K, G, N, kw = sharded_problem()
    rs = np.random.RandomState(31)
    return pb, [(c, nf, None if k == 2 else _random_gt(rs, len(c), K), tag) for k, (c, nf, tag) in enumerate(batches)], K, G, N, kw


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
from test_gt_errors_gpu import sharded_gt_problem
pb, batches, K, G, N, kw = sharded_gt_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, ground_truth=True, **kw)
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
    """Two self-launched gloo ranks on one GPU (as tests/test_fit_quality_gpu.py runs them): every rank gets its shard's rows of the
    ground truth, and rank 0's gathered (n_valid, K, 38) rows equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    pb, batches, K, G, N, kw = sharded_gt_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, ground_truth=True, **kw)
    one = list(pipe.stream_batches(batches))
    del pipe
    script = tmp_path / "sharded_gt_errors.py"
    script.write_text(_SHARDED)
    out = tmp_path / "gt2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r in one]
    assert two["records"].shape[1:] == (K, 38) and _same(two["records"], np.concatenate([r for _, _, r in one]))
    recs = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(recs[2][:, :, 26:37]).all() and np.isfinite(recs[3][2, :, 26:29]).all() and np.isnan(recs[3][3, :, 26:37]).all()
