"""GPU: the fit quality (ancsh_fit_quality_rec, pose.quality.fit_quality_batch, AncshPipeline / ShardedPipeline fit_quality=True) against
the numpy mirror (tests/fit_quality_mirror.py) and through the captured stream, the depth front end, prismatic joints, a keyed stream, the
range guard and two gloo ranks.

Against the mirror: the record's columns, the point count, both winners' scores, the inlier counts, the medians and the maxima are
byte-equal (the residual norm is evaluated in the mirror's order without contraction, and division and square root are correctly
rounded); mean and RMS agree within n 2^-52 relative, n the points of the part: only the order of the sums differs, and every term is
non-negative (the test prints the largest difference in that unit per launch)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fit_quality_mirror import MAX_N, WIDTH, fit_quality_reference, partition, residual_norms
from helpers import check_record_layout, passthrough_pose_problem
from test_joint_states_cpu import _rotation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 0.1
EXACT = [c for c in range(WIDTH) if c not in (29, 30, 35, 36)]          # everything but the two means and the two RMS
SUMS = (29, 30, 35, 36)
PAYLOAD = np.frombuffer(np.array([0x7ff8000000000abc], np.uint64).tobytes(), np.float64)[0]       # a NaN with a payload
# (b, K, part sizes): every size at which the kernel takes another path -- an empty part, fewer points than a wave, than the block, one
# more and one fewer than either, several trips of the block, the whole buffer, and one beyond it (the clamp)
LAUNCHES = {"K3": (3, 3, (0, 257, 64, 3, 63, 65, 1024, 1, 255)),
            "K1": (4, 1, (8192, 8193, 2, 256)),
            "K8": (2, 8, (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 100, 7, 8193, 5, 4096))}


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a, dt):
    return None if a is None else torch.as_tensor(np.array(a)).to("cuda:0", dt).contiguous()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Seeded packed rows, records and winners' scores (host arrays, never modified) and the mirror's block for them.  K3: cloud 0's part 2
    has a NaN in its nonlinear pose only, cloud 1 is poisoned throughout (NaNs with a payload) between clean neighbours, cloud 2's part 2
    has a NaN in its baseline only.  K1 is launched without either winner's score."""
    b, K, sizes = LAUNCHES[name]
    rs = np.random.RandomState(len(name) * 100 + K)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    src = rs.uniform(0, 1, (off[-1], 3)).astype(np.float32)
    tgt = np.empty_like(src)
    rec = np.empty((b, K, 26))
    for p, n in enumerate(sizes):
        R, s, t = _rotation(rs), rs.uniform(0.6, 1.2), rs.uniform(-0.3, 0.3, 3)
        a = off[p]
        tgt[a:a + n] = (s * src[a:a + n].astype(np.float64) @ R.T + t + 0.06 * rs.normal(size=(n, 3))).astype(np.float32)
        R2 = R @ _rotation(rs, 0.02)
        rec[p // K, p % K] = np.concatenate([R.ravel(), [s], t, R2.ravel(), [s * 1.01], t + rs.normal(size=3) * 0.01])
    best = rs.randint(0, 9000, (b * K, 2)).astype(np.int32) if K > 1 else None
    score = rs.uniform(0, 1, b * (K - 1)) if K > 1 else None
    if name == "K3":
        rec[0, 2, 22] = np.nan
        rec[1] = PAYLOAD
        rec[2, 2, 4] = np.nan
    # the mirror's norms keep clear of the threshold: the inlier counts below do not depend on the last bit
    clear = np.inf
    for p, n in enumerate(sizes):
        for q in (0, 1):
            pose = rec[p // K, p % K, 13 * q:13 * q + 13]
            if 1 <= n <= MAX_N and not np.isnan(pose).any():
                clear = min(clear, np.abs(residual_norms(src[off[p]:off[p + 1]], tgt[off[p]:off[p + 1]], pose) - TH).min())
    assert clear > 1e-9, clear
    want = fit_quality_reference(off, src, tgt, rec, TH, best, score)
    for a in (off, src, tgt, rec, want):
        a.setflags(write=False)
    return dict(b=b, K=K, sizes=sizes, off=off, src=src, tgt=tgt, rec=rec, best=best, score=score, want=want)


def _launch(p, rec=None, clouds=None, red=4):
    """One call of the entry on problem p (clouds: a slice of its clouds, the rows re-based) -> the (rows + red, 39) buffer, sentinel-filled
    before the call: the last `red` rows are the red zone behind `wide`."""
    from articulated_pose_amd import _lib
    b, K = p["b"], p["K"]
    lo, hi = clouds or (0, b)
    off = p["off"][lo * K:hi * K + 1]
    a, e = int(off[0]), int(off[-1])
    t = dict(off=_dev(off - off[0], torch.int32), src=_dev(p["src"][a:e] if e > a else np.zeros((1, 3)), torch.float32),
             tgt=_dev(p["tgt"][a:e] if e > a else np.zeros((1, 3)), torch.float32),
             rec=_dev((p["rec"] if rec is None else rec)[lo:hi], torch.float64),
             best=_dev(None if p["best"] is None else p["best"][lo * K:hi * K], torch.int32),
             score=_dev(None if p["score"] is None else p["score"][lo * (K - 1):hi * (K - 1)], torch.float64))
    wide = torch.full(((hi - lo) * K + red, WIDTH), -7.0, dtype=torch.float64, device="cuda:0")
    _lib.call("ancsh_fit_quality_rec", hi - lo, K, _lib.ptr(t["off"]), _lib.ptr(t["src"]), _lib.ptr(t["tgt"]), _lib.ptr(t["rec"]), TH,
              _lib.ptr(t["best"]), _lib.ptr(t["score"]), _lib.ptr(wide))
    torch.cuda.synchronize()
    return wide.cpu().numpy()


def _agree(got, want, what):
    """got, want (..., 39): byte-equal outside the sums, the sums within n 2^-52 relative."""
    got, want = got.reshape(-1, WIDTH), want.reshape(-1, WIDTH)
    assert _same(got[:, EXACT], want[:, EXACT]), what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    worst = 0.0
    for col in SUMS:
        fin = np.isfinite(want[:, col])
        rel = np.abs(got[fin, col] - want[fin, col]) / (np.abs(want[fin, col]) * want[fin, 26] * 2.0 ** -52)
        worst = max(worst, rel.max() if rel.size else 0.0)
    print("fit_quality %s: max |kernel - mirror| of mean / RMS = %.3g x n 2^-52 relative" % (what, worst))
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_kernel_against_mirror(dev, name):
    p = _problem(name)
    b, K, want = p["b"], p["K"], p["want"]
    full = _launch(p)
    got = full[:b * K].reshape(b, K, WIDTH)
    assert (full[b * K:] == -7.0).all()                                 # the red zone behind wide
    _agree(got, want, name)
    assert _same(_launch(p), full)                                      # two runs, identical bytes
    sizes = np.asarray(p["sizes"]).reshape(b, K)
    dead = (sizes == 0) | (sizes > MAX_N)
    assert np.array_equal(got[:, :, 26], sizes)
    if name == "K3":
        nanb, nann = dead.copy(), dead.copy()
        nanb[1], nann[1] = True, True
        nann[0, 2], nanb[2, 2] = True, True
        assert np.array_equal(np.isnan(got[:, :, 28:33]).all(2), nanb) and np.array_equal(np.isnan(got[:, :, 28:33]).any(2), nanb)
        assert np.array_equal(np.isnan(got[:, :, 34:39]).all(2), nann) and np.array_equal(np.isnan(got[:, :, 34:39]).any(2), nann)
        assert _same(got[1, :, :26], p["rec"][1]) and (got[1, :, :26].view(np.uint64) == 0x7ff8000000000abc).all()
        assert np.array_equal(got[:, :, 27].ravel(), p["best"][:, 1]) and np.array_equal(got[:, :, 33], p["score"].reshape(b, 2)[:, [0, 0, 1]])
        assert 0 < got[2, 0, 28] < 1024 and got[2, 0, 32] > TH > got[2, 0, 31] * 0 and got[2, 0, 29] <= got[2, 0, 30] <= got[2, 0, 32]
        # cloud 2 alone, its rows re-based: the bytes it has as cloud 2 of 3
        alone = _launch(p, clouds=(2, 3))
        assert (alone[K:] == -7.0).all() and _same(alone[:K], got[2])
    if name == "K1":
        assert np.isnan(got[:, 0, 27]).all() and np.isnan(got[:, 0, 33]).all()             # neither winner's score was passed
        assert np.isnan(got[1, 0, 28:33]).all() and np.isnan(got[1, 0, 34:39]).all() and got[1, 0, 26] == 8193      # the clamp
        assert np.isfinite(got[[0, 2, 3], 0, 28:33]).all() and np.isfinite(got[[0, 2, 3], 0, 34:39]).all()
    if name == "K8":
        assert np.array_equal(np.isnan(got[:, :, 28:33]).all(2), dead) and np.array_equal(np.isnan(got[:, :, 34:39]).any(2), dead)
        assert np.array_equal(got[:, :, 33], p["score"].reshape(b, 7)[:, [0, 0, 1, 2, 3, 4, 5, 6]])


def test_batch_wrapper_and_solver_option(dev):
    """pose.quality.fit_quality_batch on a solve() result is the block PoseSolver.solve(fit_quality=True) returns, and the mirror's."""
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.quality import fit_quality_batch
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    K, N = 3, 512
    cl = [make_cloud(50 + i, N=N, K=K) for i in range(2)]
    pr = [make_predictions(c, K, seed=i) for i, c in enumerate(cl)]
    st = lambda k: np.stack([q[k] for q in pr])
    args = (np.stack([c["P"] for c in cl]), st("nocs_per_point"), st("instance_per_point"), st("joint_axis_per_point"), st("joint_cls_gt"))
    solver = PoseSolver(K, TH, 64, 8, "cuda:0", lm_schedule="throughput")
    plain = solver.solve(*args, seed=5)
    assert "record_wide" not in plain
    sol = solver.solve(*args, seed=5, fit_quality=True)
    torch.cuda.synchronize()
    wide = sol["record_wide"].cpu().numpy()
    assert wide.shape == (2, K, WIDTH) and _same(wide[:, :, :26], plain["record"].cpu().numpy())
    assert _same(fit_quality_batch(sol, TH).cpu().numpy(), wide)
    off, src, tgt = partition(args[0], args[1], args[2])
    assert np.array_equal(off, sol["off"].cpu().numpy()) and _same(src, sol["_src"].cpu().numpy()) and _same(tgt, sol["_tgt"].cpu().numpy())
    _agree(wide, fit_quality_reference(off, src, tgt, wide[:, :, :26], TH, sol["best_a"].cpu().numpy().reshape(-1, 2),
                                       sol["score_b"].cpu().numpy()), "solve()")
    assert (wide[:, :, 26].sum(1) == N).all() and (wide[:, :, 28] <= wide[:, :, 26]).all() and (wide[:, :, 34] <= wide[:, :, 26]).all()


def test_launch_is_capturable(dev):
    from articulated_pose_amd import _lib
    p = _problem("K3")
    b, K = p["b"], p["K"]
    t = dict(off=_dev(p["off"], torch.int32), src=_dev(p["src"], torch.float32), tgt=_dev(p["tgt"], torch.float32),
             rec=_dev(p["rec"], torch.float64), best=_dev(p["best"], torch.int32), score=_dev(p["score"], torch.float64))
    wide = torch.zeros((b, K, WIDTH), dtype=torch.float64, device=dev)
    launch = lambda: _lib.call("ancsh_fit_quality_rec", b, K, _lib.ptr(t["off"]), _lib.ptr(t["src"]), _lib.ptr(t["tgt"]), _lib.ptr(t["rec"]),
                               TH, _lib.ptr(t["best"]), _lib.ptr(t["score"]), _lib.ptr(wide))
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        launch()
    st.synchronize()
    eager = wide.cpu().numpy()
    assert _same(eager.reshape(-1, WIDTH), _launch(p)[:b * K])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        launch()
    wide.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same(wide.cpu().numpy(), eager)
    # changed inputs behind the same pointers: clouds 0 and 2 trade their records, the winners' scores change
    rec2 = np.array(p["rec"])
    rec2[[0, 2]] = rec2[[2, 0]]
    t["rec"].copy_(torch.as_tensor(rec2))
    t["best"].add_(1)
    g.replay()
    torch.cuda.synchronize()
    got = wide.cpu().numpy()
    assert _same(got.reshape(-1, WIDTH), _launch(dict(p, best=p["best"] + 1), rec=rec2)[:b * K]) and not _same(got, eager)
    _agree(got, fit_quality_reference(p["off"], p["src"], p["tgt"], rec2, TH, p["best"] + 1, p["score"]), "replay")


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
K_, B_, N_ = 3, 4, 512                                             # the set-up of tests/test_joint_states_gpu.py's stream tests


def _batches(pb, count, rs):
    from test_articulation_gpu import _stream_batches
    return _stream_batches(pb, K_, B_, N_, count, rs)              # short batches at k = 0, a NaN cloud in batch 5


def _pipe(pb, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=1, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", raw_capacity=B_ * 3 * N_), **kw)
    return AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **kw)


def _check_against_mirror(pipe, wide, f32=False):
    """`wide` was just retired from a one-slot pipeline: the slot still holds that batch's P, NPCS heads, record and winners' scores."""
    sl = pipe.slots[0]
    sl.stream.synchronize()
    out = sl.out32 if f32 else sl.out
    P, n, sol = sl.P.cpu().numpy(), out["npcs"], out["pose"]
    assert out["record"].shape == (pipe.B, pipe.K, 26) and out["record_wide"].shape == (pipe.B, pipe.K, WIDTH)
    nocs, mask = n["nocs_per_point"].cpu().numpy(), n["W"].cpu().numpy()
    if np.isfinite(mask).all():
        off, src, tgt = partition(P, nocs, mask)
        assert np.array_equal(off, sol["off"].cpu().numpy())
    else:          # a NaN cloud in the batch: the label of a NaN mask row is not defined here; the solver's own rows (its record is NaN anyway)
        off, src, tgt = (sol[k].cpu().numpy() for k in ("off", "_src", "_tgt"))
    score = sol["score_b"].cpu().numpy() if pipe.K > 1 else None
    want = fit_quality_reference(off, src, tgt, out["record"].cpu().numpy(), TH, sol["best_a"].cpu().numpy().reshape(-1, 2), score)
    _agree(wide, want[:len(wide)], "stream")


def _launch_names(pipe):
    """The ABI calls of one eager step on slot 0, in order."""
    from articulated_pose_amd import _lib
    names, real = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        with torch.cuda.stream(pipe.slots[0].stream):
            pipe._run(pipe.slots[0])
        pipe.synchronize()
    finally:
        _lib.call = real
    return names


@pytest.mark.parametrize("slots", [1, 4])
def test_stream_keeps_the_record_and_adds_the_quality(dev, slots):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _batches(pb, 12, np.random.RandomState(slots))
    kw = dict(slots=slots, articulation=True, joint_states=True)
    base = list(_pipe(pb, **kw).stream_batches(batches, articulation=True))
    pipe = _pipe(pb, fit_quality=True, **kw).prepare()
    assert pipe.slots[0].outputs["record"].host[0].shape == (B_, K_, WIDTH) and pipe.slots[0].outputs["record"].host32 is None
    L = check_record_layout(pipe, ["pose", "fit_quality"])
    assert (L.width, L.key, L.carried("fit_quality")) == (WIDTH, "record_wide", ("record", 26))
    graphs = [sl.graph for sl in pipe.slots]
    got = []
    for item in pipe.stream_batches(batches, articulation=True):
        got.append(item)
        if slots == 1:
            _check_against_mirror(pipe, item[2])
    assert all(g is not None and g is sl.graph for g, sl in zip(graphs, pipe.slots))       # one graph per slot served every batch
    assert len(got) == len(base) == 12
    for (t0, s0, r0, a0), (t1, s1, r1, a1), (clouds, _) in zip(base, got, batches):
        assert (t0, s0) == (t1, s1) and r0.shape == (len(clouds), K_, 26) and r1.shape == (len(clouds), K_, WIDTH)
        assert _same(r0, r1[..., :26]) and _same(a0, a1), t0                                # the record and the articulation / joint-state block
        assert _same(L.block(r1, "pose"), r1[..., :26]) and _same(L.block(r1, "fit_quality"), r1[..., 26:])
    w5 = got[5][2]
    assert np.isnan(w5[1, :, :26]).all() and np.isnan(w5[1, :, 28:33]).all() and np.isnan(w5[1, :, 34:39]).all()
    assert (w5[:, :, 26].sum(1) == N_).all() and np.isfinite(w5[0, :, 28:39]).all()
    if slots == 4:                                                  # equal bytes for equal lm_schedule, whatever the slots
        one = list(_pipe(pb, fit_quality=True, slots=1).stream_batches(batches))
        assert all(len(x) == 3 for x in one) and all(_same(a[2], b[2]) for a, b in zip(one, got))


def test_launch_budget(dev):
    """Exactly one ABI call more with the option, behind the record poison and in front of the articulation launch; none more without."""
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    for kw in (dict(articulation=True), dict()):
        plain = _launch_names(_pipe(pb, **kw).prepare())
        off = _launch_names(_pipe(pb, fit_quality=False, **kw).prepare())
        on = _launch_names(_pipe(pb, fit_quality=True, **kw).prepare())
        assert off == plain and "ancsh_fit_quality_rec" not in plain
        at = on.index("ancsh_fit_quality_rec")
        assert on[:at] + on[at + 1:] == plain and on[at - 1] == "ancsh_pose_poison_records"
        if kw:
            assert on[at + 1] == "ancsh_articulation_rec"
    # couple=False: the fit reads the caller's predictions, and the quality the solver's own packed rows
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    cl = [make_cloud(60 + i, N=N_, K=K_) for i in range(2)]
    pr = [make_predictions(c, K_, seed=i) for i, c in enumerate(cl)]
    P, cls = np.stack([c["P"] for c in cl]), np.stack([q["joint_cls_gt"] for q in pr])
    pred = {k: np.stack([q[k] for q in pr]) for k in ("nocs_per_point", "instance_per_point", "joint_axis_per_point")}
    pipe = AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], 2, N_, "cuda:0", couple=False, niter_a=64, niter_b=8, seed=11, fit_quality=True)
    pipe.load_inputs(P, cls, pred)
    pipe.prepare()
    sl, out = pipe.step()
    sl.stream.synchronize()
    off, src, tgt = partition(P, pred["nocs_per_point"], pred["instance_per_point"])
    sol = out["pose"]
    _agree(out["record_wide"].cpu().numpy(), fit_quality_reference(off, src, tgt, out["record"].cpu().numpy(), TH,
                                                                   sol["best_a"].cpu().numpy().reshape(-1, 2), sol["score_b"].cpu().numpy()),
           "couple=False")


def test_depth_stream_carries_the_quality(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_depth_gpu import SIDE, _camera, _depth_batches, _scale
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _depth_batches(pb, 2, 2, np.random.RandomState(4), "uint16", short_last=False)        # two small crops a batch
    mk = lambda **kw: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], 2, N_, "cuda:0", couple=True, slots=1, niter_a=64, niter_b=8, seed=11,
                                    lm_schedule="throughput", articulation=True, depth_capacity=2 * SIDE * SIDE, joint_source="predicted", **kw)
    base = list(mk().stream_depth_batches(batches, _camera(), _scale("uint16"), articulation=True))
    pipe = mk(fit_quality=True)
    n = 0
    for (t0, s0, r0, a0, c0), item in zip(base, pipe.stream_depth_batches(batches, _camera(), _scale("uint16"), articulation=True)):
        t1, s1, r1, a1, c1 = item
        assert (t0, s0) == (t1, s1) and r1.shape == (2, K_, WIDTH) and _same(r0, r1[..., :26]) and _same(a0, a1) and _same(c0, c1)
        _check_against_mirror(pipe, r1)
        n += 1
    assert n == 2


def test_prismatic_and_keyed_streams_carry_the_quality(dev):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _batches(pb, 3, np.random.RandomState(6))
    base = list(_pipe(pb, joint_types="prismatic").stream_batches(batches))
    pipe = _pipe(pb, joint_types="prismatic", fit_quality=True)
    for (t0, s0, r0), (t1, s1, r1) in zip(base, pipe.stream_batches(batches)):
        assert (t0, s0) == (t1, s1) and _same(r0, r1[..., :26])
        _check_against_mirror(pipe, r1)
    # keyed, at a cloud_base other than 0: the graph of cloud_base 0 serves it
    plain, wide = _pipe(pb, keyed=True), _pipe(pb, keyed=True, fit_quality=True)
    for k, (clouds, nf) in enumerate(batches):
        for p in (plain, wide):
            p.submit(clouds, nf, seed=40 + k, tag=k, cloud_base=7 * k + 5)
        (t0, s0, r0), (t1, s1, r1) = plain.retire(), wide.retire()
        assert (t0, s0) == (t1, s1) == (k, 40 + k) and r1.shape == (len(clouds), K_, WIDTH) and _same(r0, r1[..., :26])
        _check_against_mirror(wide, r1)


def test_range_guard_takes_the_f32_wide_rows(dev):
    """One cloud forced over f16's range by its norm factor, as tests/test_joint_states_gpu.py and tests/test_range_guard_gpu.py do."""
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _batches(pb, 4, np.random.RandomState(9))
    hot = []
    for k, (clouds, nf) in enumerate(batches):
        h = np.zeros(len(clouds), bool)
        if k % 2 == 1:
            nf[0] = 1e6
            h[0] = True
        hot.append(h)
    mk = lambda arith, guard, **kw: _pipe(pb, slots=2, arithmetic=arith, range_guard=guard, **kw)
    f32 = list(mk("f32", False, fit_quality=True).stream_batches(batches))
    f16 = list(mk("f16x2", False, fit_quality=True).stream_batches(batches))
    plain = list(mk("f16x2", True).stream_batches(batches, flags=True))
    guarded = mk("f16x2", True, fit_quality=True)
    assert guarded.slots[0].outputs["record"].host32[0].shape == (B_, K_, WIDTH)
    got = list(guarded.stream_batches(batches, flags=True))
    assert guarded.f32_reruns == 2
    for (tag, _, rec, words), (_, _, r32), (_, _, r16), (_, _, r26, w26), h in zip(got, f32, f16, plain, hot):
        assert ((words != 0) == h).all() and rec.shape[2] == WIDTH and _same(words, w26) and _same(rec[..., :26], r26), tag
        assert _same(rec[h], r32[h]) and _same(rec[~h], r16[~h]), tag


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
from test_joint_states_gpu import sharded_problem
pb, batches, K, G, N, kw = sharded_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, articulation=True, fit_quality=True, **kw)
got = list(sp.stream_batches(batches, articulation=True))
if dist.get_rank() != 0:
    assert all(r is None and a is None for _, _, r, a in got)
    got = None
dist.barrier()
dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _, _ in got]), counts=np.array([len(r) for _, _, r, _ in got]),
             records=np.concatenate([r for _, _, r, _ in got]), blocks=np.concatenate([a for _, _, _, a in got]))
'''


def test_sharded_wide_records_equal_one_pipeline(dev, tmp_path):
    """Two self-launched gloo ranks on one GPU (as tests/test_dist_gpu.py runs them): rank 0's gathered (n_valid, K, 39) records and the
    articulation blocks behind them in the same gather equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_joint_states_gpu import sharded_problem
    pb, batches, K, G, N, kw = sharded_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, articulation=True, fit_quality=True, **kw)
    one = list(pipe.stream_batches(batches, articulation=True))
    del pipe
    script = tmp_path / "sharded_fit_quality.py"
    script.write_text(_SHARDED)
    out = tmp_path / "wide2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r, _ in one]
    assert two["records"].shape[1:] == (K, WIDTH) and two["blocks"].shape[1:] == (K, 12)
    assert _same(two["records"], np.concatenate([r for _, _, r, _ in one]))
    assert _same(two["blocks"], np.concatenate([a for _, _, _, a in one]))
    recs = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(recs[3][3, :, 28:33]).all() and np.isfinite(recs[3][2, :, 28:39]).all() and (recs[3][:, :, 26].sum(1) == N).all()
