"""Streaming pipeline on the MI355X: the graph-capturable sampler of raw clouds (ancsh_input_sample_stream), the pose fit keyed from
device memory (ancsh_ransac_*_rec_dseed) and AncshPipeline(raw_capacity=...).submit / retire / stream, each against an eager pass."""
import numpy as np
import pytest
import torch

from helpers import passthrough_pose_problem
from stream_mirror import sample_perm

pytestmark = pytest.mark.gpu


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int64)      # NaN-safe exact comparison of float64 records


def _raw18(rs, n, K):
    """(n, 18) pack_cloud rows: random xyz / channels, integer part class (col 3) and joint class (col 17)."""
    r = rs.uniform(-1, 1, (n, 18)).astype(np.float32)
    r[:, 3] = rs.randint(0, K, n)
    r[:, 17] = rs.randint(0, K, n)
    return r


@pytest.mark.parametrize("N", [512, 1024])
def test_sampler_matches_mirror_and_create_unit_data_batch(dev, N):
    from articulated_pose_amd.dataset import create_unit_data_batch, sample_raw_batch
    K = 3
    rs = np.random.RandomState(N)
    sizes = [1, 7, N - 1, N, 3 * N, 200]
    raw = [_raw18(rs, n, K) for n in sizes]
    nf = rs.uniform(0.5, 2.0, len(sizes)).astype(np.float32)
    for seed in (0, 12345, 2 ** 64 - 3):
        got = sample_raw_batch([r[:, [0, 1, 2, 17]] for r in raw], N, nf, seed, dev, return_perm=True)
        perm = got["perm"].cpu().numpy()
        for b, n in enumerate(sizes):
            assert np.array_equal(perm[b], sample_perm(seed, b, n, N)), (seed, b, n)
        want = create_unit_data_batch(raw, N, nf, K, perms=list(perm), device=dev)
        assert torch.equal(got["P"], want["P"])
        assert torch.equal(got["joint_cls"], want["joint_cls_gt"].to(torch.int32))


def test_captured_sampler_follows_device_buffers(dev):
    """One capture, then new sizes and a new seed written into the device buffers: the replay samples the new clouds."""
    from articulated_pose_amd import _lib
    B, N, cap = 3, 256, 4000
    rows = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    nf = torch.ones(B, dtype=torch.float32, device=dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    P = torch.zeros((B, N, 3), dtype=torch.float32, device=dev)
    jc = torch.zeros((B, N), dtype=torch.int32, device=dev)
    perm = torch.zeros((B, N), dtype=torch.int32, device=dev)

    def launch():
        _lib.call("ancsh_input_sample_stream", B, N, 4, _lib.ptr(rows), cap, _lib.ptr(off), _lib.ptr(nf), 3, _lib.ptr(seed), _lib.ptr(P),
                  _lib.ptr(jc), _lib.ptr(perm))
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        launch()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    rs = np.random.RandomState(0)
    for sizes, sd in (([10, 300, 256], 5), ([1000, 3, 2000], 2 ** 63 + 9)):
        r = rs.uniform(-1, 1, (sum(sizes), 4)).astype(np.float32)
        rows[:len(r)] = torch.from_numpy(r).to(dev)
        off.copy_(torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)))
        seed.fill_(int(np.uint64(sd).view(np.int64)))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        o = np.concatenate([[0], np.cumsum(sizes)])
        for b, n in enumerate(sizes):
            want = sample_perm(sd, b, n, N)
            assert np.array_equal(perm[b].cpu().numpy(), want)
            assert torch.equal(P[b].cpu(), torch.from_numpy(r[o[b] + want % n, :3]))


def _net_inputs(dev, K, B, N, seed):
    from articulated_pose_amd.network import Network
    pb = passthrough_pose_problem(K, B, N, seed=seed)
    a = Network(K, pb["w_ancsh"], "ancsh", dev).predict(pb["P"])
    n = Network(K, pb["w_npcs"], "npcs", dev).predict(pb["P"])
    return pb, (torch.from_numpy(pb["P"]).to(dev), n["nocs_per_point"], n["W"], a["joint_axis_per_point"],
                torch.from_numpy(pb["cls"].astype(np.int32)).to(dev))


@pytest.mark.parametrize("K", [2, 3, 4])
def test_device_seed_equals_by_value_seed(dev, K):
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.d3_utils import rot_diff_degree
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW
    B, N = 2, 1024
    pb, inputs = _net_inputs(dev, K, B, N, seed=K)
    solver = PoseSolver(K, 0.1, 400, 32, dev, tie_window=TIE_WINDOW)
    keys = ("record", "best_a", "best_b", "inliers_a", "inliers_b", "tie_a", "tie_b", "score_b")
    best = []
    for s in (7, 2 ** 64 - 2):
        by_value = solver.solve(*inputs, seed=s)
        sd = torch.tensor([int(np.uint64(s).view(np.int64))], dtype=torch.int64, device=dev)
        by_dev = solver.solve(*inputs, seed_dev=sd)
        for k in keys:
            assert torch.equal(_bits(by_value[k]) if by_value[k].dtype == torch.float64 else by_value[k],
                               _bits(by_dev[k]) if by_dev[k].dtype == torch.float64 else by_dev[k]), (s, k)
        rec = by_dev["record"].cpu().numpy()
        for b in range(B):
            for j in range(K):
                assert rot_diff_degree(rec[b, j, 13:22].reshape(3, 3), pb["R"][j]) < 1.0
                assert abs(rec[b, j, 22] / pb["s"][j] - 1) < 0.02
    # another key, another sample stream: on noisy predictions with outliers (where the winning iteration is not simply the first
    # hypothesis, as on the clean passthrough problem) the winners move
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    cl = [make_cloud(40 + b, N=N, K=K) for b in range(B)]
    pr = [make_predictions(c, K, seed=b) for b, c in enumerate(cl)]
    noisy = [np.stack([c["P"] for c in cl])] + [np.stack([p[k] for p in pr]) for k in ("nocs_per_point", "instance_per_point",
                                                                                            "joint_axis_per_point", "joint_cls_gt")]
    for s in (7, 8):
        sd = torch.tensor([s], dtype=torch.int64, device=dev)
        by_dev = solver.solve(*noisy, seed_dev=sd)
        assert torch.equal(_bits(by_dev["record"]), _bits(solver.solve(*noisy, seed=s)["record"]))
        best.append(by_dev["best_a"][..., 0].clone())
    assert not torch.equal(best[0], best[1])


# ---- the streaming pipeline ---------------------------------------------------------------------------------------------------
def _raw_batches(pb, count, B, rs, short_last=True):
    """Ragged raw clouds cut from the passthrough problem's clouds: (clouds [(n, 4)], norm factors) per batch."""
    Pn, cls = pb["P"], pb["cls"]
    N = Pn.shape[1]
    out = []
    for k in range(count):
        nb = B if not (short_last and k == count - 1) else max(1, B // 2)
        clouds = []
        for _ in range(nb):
            src = rs.randint(Pn.shape[0])
            n = int(rs.randint(N // 3, 3 * N))
            idx = rs.randint(0, N, n)
            c = np.concatenate([Pn[src][idx] + rs.normal(0, 2e-3, (n, 3)).astype(np.float32), cls[src][idx, None]], 1)
            clouds.append(c.astype(np.float32))
        out.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32)))
    return out


def _eager(pipe, clouds, nf, seed):
    """sample_raw_batch -> both networks -> PoseSolver.solve(seed=...) on the padded batch -> records of the valid clouds."""
    from articulated_pose_amd.dataset import sample_raw_batch
    from articulated_pose_amd.pose import PoseSolver
    n = len(clouds)
    padded = list(clouds) + [clouds[0]] * (pipe.B - n)
    nfp = np.concatenate([nf, np.repeat(nf[:1], pipe.B - n)])
    s = sample_raw_batch(padded, pipe.N, nfp, seed, pipe.device)
    a, m = pipe.ancsh.predict(s["P"]), pipe.npcs.predict(s["P"])
    solver = PoseSolver(pipe.K, pipe.solver.th, pipe.solver.niter_a, pipe.solver.niter_b, pipe.device, lm_schedule=pipe.solver.lm_schedule,
                        tie_window=None)
    sol = solver.solve(s["P"], m["nocs_per_point"], m["W"], a["joint_axis_per_point"], s["joint_cls"], seed=seed)
    return sol["record"][:n].cpu().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("slots", [1, 4])
def test_stream_equals_eager(dev, slots):
    from articulated_pose_amd.pipeline import AncshPipeline
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=1)
    rs = np.random.RandomState(slots)
    batches = _raw_batches(pb, 200, B, rs)
    nan_batch = 37                                       # cloud 1 of this batch: every row NaN -> its record only is poisoned
    batches[nan_batch][0][1][:, :3] = np.nan
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, couple=True, slots=slots, niter_a=64, niter_b=8, seed=100,
                         raw_capacity=B * 3 * N)
    got = list(pipe.stream_batches([(c, nf, "b%d" % k) for k, (c, nf) in enumerate(batches)]))
    assert [g[0] for g in got] == ["b%d" % k for k in range(len(batches))]
    for k, ((tag, seed, rec), (clouds, nf)) in enumerate(zip(got, batches)):
        assert seed == 100 + 2 * k and rec.shape == (len(clouds), K, 26) and rec.dtype == np.float64
        assert _same(rec, _eager(pipe, clouds, nf, seed)), k
    assert len(got[-1][2]) == B // 2                      # the short last batch: its valid records only
    rec = got[nan_batch][2]
    assert np.isnan(rec[1]).all() and not np.isnan(rec[0, :, :13]).all()
    assert np.isfinite(got[0][2]).all()                   # the passthrough clouds' fits are all defined


def test_stream_full_size_batch(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    K, B, N = 3, 32, 1024
    pb = passthrough_pose_problem(K, 8, N, seed=2)
    batches = _raw_batches(pb, 2, B, np.random.RandomState(3), short_last=False)
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, couple=True, slots=2, raw_capacity=B * 3 * N)
    for (tag, seed, rec), (clouds, nf) in zip(pipe.stream_batches(batches), batches):
        assert _same(rec, _eager(pipe, clouds, nf, seed)), tag


def test_stream_misuse_raises_and_pipeline_stays_usable(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    K, B, N = 3, 2, 512
    pb = passthrough_pose_problem(K, 4, N, seed=4)
    with pytest.raises(ValueError):
        AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, couple=False, raw_capacity=4096)
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, couple=True, slots=2, niter_a=64, niter_b=8, raw_capacity=3000)
    rs = np.random.RandomState(5)
    (good, nf), = _raw_batches(pb, 1, B, rs, short_last=False)
    good = [c[:1000] for c in good]
    big = [np.zeros((2000, 4), np.float32), np.zeros((1500, 4), np.float32)]
    with pytest.raises(ValueError):
        pipe.submit(big, [1.0, 1.0])                      # 3500 rows > raw_capacity
    with pytest.raises(ValueError):
        pipe.submit([np.concatenate([good[0]] * 10)[:1600]], [1.0])     # padded with itself: 3200 rows
    with pytest.raises(ValueError):
        pipe.submit([good[0], np.zeros((0, 4), np.float32)], [1.0, 1.0])
    with pytest.raises(ValueError):
        pipe.submit(good, [1.0, float("inf")])
    with pytest.raises(RuntimeError):
        pipe.retire()
    pipe.submit(good, nf, tag="a")
    pipe.submit(good, nf, seed=77, tag="b")
    with pytest.raises(RuntimeError):
        pipe.submit(good, nf)                             # both slots hold unretired batches
    ta, sa, ra = pipe.retire()
    pipe.submit(good, nf, tag="c")
    tb, sb, rb = pipe.retire()
    tc, sc, rc = pipe.retire()
    assert (ta, sa, tb, sb, tc, sc) == ("a", 0, "b", 77, "c", 4)
    for seed, rec in ((sa, ra), (sb, rb), (sc, rc)):
        assert _same(rec, _eager(pipe, good, nf, seed))
