"""GPU: the joint association from the ANCSH network's index head (joint_source="predicted") -- the direction kernel against the
ground-truth-label kernel and numpy, the solver against solve(joint_cls=argmax), the xyz sampler against the 4-column one, the stream
against its eager composition (plain, (n, 4) rows, articulation, dense, range guard, slots 1 and 4), the launch budget, the sharded
stream and the offline entry."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_stream_gpu import _raw_batches, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    """NaN-safe exact comparison: floats by their bits."""
    return {torch.float64: lambda x: x.view(torch.int64), torch.float32: lambda x: x.view(torch.int32)}.get(t.dtype, lambda x: x)(t.contiguous())


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _index_head(rs, B, N, jc, jcls=None):
    """(B, N, jc) float32 rows: random, the labelled channel lifted when jcls is given, with exact ties and NaN rows mixed in."""
    idx = rs.uniform(0, 1, (B, N, jc)).astype(np.float32)
    if jcls is not None:
        b, i = np.nonzero(jcls < jc)
        idx[b, i, jcls[b, i]] += 1.0
    m = rs.uniform(size=(B, N))
    tie = m < 0.08                                                       # exact ties between two channels
    c0, c1 = rs.randint(0, jc, (B, N)), rs.randint(0, jc, (B, N))
    bb, ii = np.nonzero(tie)
    idx[bb, ii, c1[bb, ii]] = idx[bb, ii, c0[bb, ii]]
    full = (m >= 0.08) & (m < 0.1)                                       # a whole row equal: channel 0 wins
    idx[full] = 0.5
    return idx


def _with_nans(rs, idx):
    x = idx.copy()
    B, N, jc = x.shape
    m = rs.uniform(size=(B, N)) < 0.03
    bb, ii = np.nonzero(m)
    x[bb, ii, rs.randint(0, jc, bb.size)] = np.nan                       # np.argmax: the first NaN of the row
    return x


@pytest.mark.parametrize("jc", [3, 5])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_direction_kernel_equals_label_kernel_and_numpy(dev, K, jc):
    from articulated_pose_amd import _lib
    rs = np.random.RandomState(10 * K + jc)
    for n in (1, 777, 1024, 2048, 3000):
        B = 3
        axis = rs.normal(size=(B, n, 3)).astype(np.float32)
        axis[:, : n // 3] = np.round(axis[:, : n // 3], 1)               # repeated values inside a joint's selection
        idx = _with_nans(rs, _index_head(rs, B, n, jc))
        idx[2, :, 1:] = -1.0                                             # cloud 2: every point selects channel 0 -> no joint has a point
        lab = np.argmax(idx, -1).astype(np.int32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        got = torch.full((B, K - 1, 3), 7.0, device=dev)
        old = torch.full((B, K - 1, 3), 7.0, device=dev)
        da, di, dl = d(axis), d(idx), d(lab)                             # held until the kernels have run
        _lib.call("ancsh_pose_joint_direction_pred", B, n, K, jc, _lib.ptr(da), _lib.ptr(di), _lib.ptr(got))
        _lib.call("ancsh_pose_joint_direction", B, n, K, _lib.ptr(da), _lib.ptr(dl), _lib.ptr(old))
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(old)), (K, jc, n)
        want = np.full((B, K - 1, 3), np.nan, np.float32)
        for b in range(B):
            for j in range(1, K):
                sel = axis[b][lab[b] == j]
                if len(sel):
                    want[b, j - 1] = np.median(sel, 0)
        g = got.cpu().numpy()
        assert np.array_equal(g.view(np.int32), want.view(np.int32)) or np.array_equal(g, want, equal_nan=True), (K, jc, n)
        assert np.isnan(g[2]).all()                                      # no point selects a joint
        if K - 1 >= jc:
            assert np.isnan(g[:, jc - 1:]).all()                         # a head jc wide never selects joint >= jc


def _noisy_inputs(K, B, N, seed):
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    cl = [make_cloud(80 + seed + b, N=N, K=K) for b in range(B)]
    pr = [make_predictions(c, K, seed=b) for b, c in enumerate(cl)]
    base = [np.stack([c["P"] for c in cl])] + [np.stack([p[k] for p in pr]) for k in ("nocs_per_point", "instance_per_point",
                                                                                      "joint_axis_per_point")]
    return base, np.stack([p["joint_cls_gt"] for p in pr])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_solver_index_equals_argmax_labels(dev, K):
    from articulated_pose_amd.dataset import stream_key_words
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW
    B, N = 4, 1024
    base, jcls = _noisy_inputs(K, B, N, K)
    rs = np.random.RandomState(K)
    idx = _index_head(rs, B, N, 3, jcls)
    lab = np.argmax(idx, -1).astype(np.int32)
    solver = PoseSolver(K, 0.1, 300, 16, dev, tie_window=TIE_WINDOW)
    names = ("record", "best_a", "best_b", "inliers_a", "inliers_b", "tie_a", "tie_b", "score_b", "joint_direction")
    key = torch.from_numpy(stream_key_words(9, 3)).to(dev)
    sd = torch.tensor([9], dtype=torch.int64, device=dev)
    for kw in (dict(seed=9), dict(seed_dev=sd), dict(key_dev=key)):
        a = solver.solve(*base, joint_index=idx, **kw)
        b = solver.solve(*base, lab, **kw)
        for n in names:
            assert torch.equal(_bits(a[n]), _bits(b[n])), (K, kw.keys(), n)
    jd = a["joint_direction"].cpu().numpy()
    assert np.isfinite(jd[:, :min(K - 1, 2)]).all()
    if K == 4:
        assert np.isnan(jd[:, 2]).all()                                  # the 3-wide head never selects joint 3: no direction for it
    # a NaN in one cloud's index head poisons that cloud's record only
    bad = idx.copy()
    bad[1, 17, 2] = np.nan
    p = solver.solve(*base, joint_index=bad, seed=9)["record"].cpu().numpy()
    ref = solver.solve(*base, np.argmax(bad, -1).astype(np.int32), seed=9)["record"].cpu().numpy()
    assert np.isnan(p[1]).all() and not np.isnan(ref[1]).all()
    keep = [0, 2, 3]
    assert _same(p[keep], ref[keep])
    inf = idx.copy()
    inf[3, 0, 0] = np.inf
    assert np.isnan(solver.solve(*base, joint_index=inf, seed=9)["record"][3].cpu().numpy()).all()
    # stage B on its own: the same bytes as the one-call form
    out = solver.solve_stage_a(*base[:3], seed=9)
    sb = solver.solve_stage_b(out, base[3], joint_index=idx, seed=9)
    assert _same(sb["record"].cpu().numpy(), solver.solve(*base, joint_index=idx, seed=9)["record"].cpu().numpy())


@pytest.mark.parametrize("nchan", [3, 5])
def test_xyz_sampler_equals_four_column_sampler(dev, nchan):
    from articulated_pose_amd import _lib
    from articulated_pose_amd.dataset import sample_raw_batch, stream_key_words
    N = 512
    rs = np.random.RandomState(nchan)
    sizes = [1, 7, N - 1, N, 3 * N, 200, 900]
    wide = [rs.uniform(-1, 1, (n, max(nchan, 4))).astype(np.float32) for n in sizes]
    nf = rs.uniform(0.5, 2.0, len(sizes)).astype(np.float32)
    B = len(sizes)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    rows4 = torch.from_numpy(np.concatenate(wide)).to(dev)                               # the 4-column entry: column 3 is joint_cls
    rowsx = torch.from_numpy(np.ascontiguousarray(np.concatenate(wide)[:, :nchan])).to(dev)
    nfd = torch.from_numpy(nf).to(dev)
    cap = rows4.shape[0]
    for seed in (0, 2 ** 64 - 3):
        for base in (None, 0, 3, 1000):
            if base is None:
                s = torch.tensor([int(np.uint64(seed).view(np.int64))], dtype=torch.int64, device=dev)
            else:
                s = torch.from_numpy(stream_key_words(seed, base)).to(dev)
            e4, ex = ("ancsh_input_sample_stream", "ancsh_input_sample_stream_xyz") if base is None else \
                ("ancsh_input_sample_stream_keyed", "ancsh_input_sample_stream_xyz_keyed")
            P4, Px = (torch.full((B, N, 3), 9.0, device=dev) for _ in range(2))
            m4, mx = (torch.full((B, N), -5, dtype=torch.int32, device=dev) for _ in range(2))
            jc = torch.empty((B, N), dtype=torch.int32, device=dev)
            _lib.call(e4, B, N, rows4.shape[1], _lib.ptr(rows4), cap, _lib.ptr(off), _lib.ptr(nfd), 3, _lib.ptr(s), _lib.ptr(P4),
                      _lib.ptr(jc), _lib.ptr(m4))
            _lib.call(ex, B, N, nchan, _lib.ptr(rowsx), cap, _lib.ptr(off), _lib.ptr(nfd), _lib.ptr(s), _lib.ptr(Px), _lib.ptr(mx))
            torch.cuda.synchronize()
            assert torch.equal(_bits(P4), _bits(Px)) and torch.equal(m4, mx), (seed, base)
    # the eager wrapper: (n, 3) and (n, 4) clouds give the 4-column sampler's P and perm
    clouds4 = [w[:, :4] for w in wide]
    ref = sample_raw_batch(clouds4, N, nf, 5, dev, return_perm=True, cloud_base=2)
    for cl in (clouds4, [c[:, :3] for c in clouds4]):
        got = sample_raw_batch(cl, N, nf, 5, dev, return_perm=True, cloud_base=2, xyz_only=True)
        assert set(got) == {"P", "perm"} and torch.equal(got["P"], ref["P"]) and torch.equal(got["perm"], ref["perm"])


# ---- the stream -----------------------------------------------------------------------------------------------------------------
def _pipe(pb, K, B, N, slots, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput", raw_capacity=B * 3 * N), **kw)
    return AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, "cuda:0", slots=slots, joint_source="predicted", **kw)


def _eager_predicted(pipe, clouds, nf, seed):
    """xyz sampler -> both networks -> PoseSolver.solve(joint_index=ancsh['index_per_point']) on the padded batch."""
    from articulated_pose_amd.dataset import sample_raw_batch
    from articulated_pose_amd.pose import PoseSolver
    n = len(clouds)
    padded = list(clouds) + [clouds[0]] * (pipe.B - n)
    nfp = np.concatenate([nf, np.repeat(nf[:1], pipe.B - n)])
    s = sample_raw_batch(padded, pipe.N, nfp, seed, pipe.device, xyz_only=True)
    a, m = pipe.ancsh.predict(s["P"]), pipe.npcs.predict(s["P"])
    solver = PoseSolver(pipe.K, pipe.solver.th, pipe.solver.niter_a, pipe.solver.niter_b, pipe.device, lm_schedule=pipe.solver.lm_schedule,
                        tie_window=None)
    sol = solver.solve(s["P"], m["nocs_per_point"], m["W"], a["joint_axis_per_point"], joint_index=a["index_per_point"], seed=seed)
    return sol["record"][:n].cpu().numpy()


@pytest.mark.parametrize("slots", [1, 4])
def test_stream_equals_eager_composition(dev, slots):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=1)
    batches = _raw_batches(pb, 24, B, np.random.RandomState(slots))
    batches[5][0][1][:, :3] = np.nan                                     # one all-NaN cloud: its record alone is poisoned
    xyz = [([c[:, :3].copy() for c in cl], nf) for cl, nf in batches]
    rs = np.random.RandomState(50 + slots)
    four = [([np.concatenate([c, rs.uniform(-9, 9, (len(c), 1)).astype(np.float32)], 1) for c in cl], nf) for cl, nf in xyz]
    pipe = _pipe(pb, K, B, N, slots)
    assert pipe.slots[0].raw_rows.shape == (B * 3 * N, 3)
    got = list(pipe.stream_batches(xyz))
    for k, ((tag, seed, rec), (clouds, nf)) in enumerate(zip(got, xyz)):
        assert seed == 100 + 2 * k and rec.shape == (len(clouds), K, 26)
        assert _same(rec, _eager_predicted(pipe, clouds, nf, seed)), k
    assert np.isnan(got[5][2][1]).all() and not np.isnan(got[5][2][0]).all()
    assert pipe.slots[0].graph is not None
    got4 = list(_pipe(pb, K, B, N, slots).stream_batches(four))          # a random 4th column is ignored
    assert len(got4) == len(got) and all(_same(a[2], b[2]) for a, b in zip(got, got4))


def test_stream_articulation_and_dense_equal_eager_ops(dev):
    from articulated_pose_amd.dataset import raw_point_labels
    from articulated_pose_amd.pose.joint_params import articulation_batch
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches = [([c[:, :3].copy() for c in cl], nf) for cl, nf in _raw_batches(pb, 8, B, np.random.RandomState(4))]
    plain = list(_pipe(pb, K, B, N, 2).stream_batches(batches))
    pipe = _pipe(pb, K, B, N, 2, articulation=True, dense=True)
    for k, item in enumerate(pipe.stream_batches(batches, articulation=True, dense=True)):
        tag, seed, rec, art, (labels, values, off) = item
        assert _same(rec, plain[k][2]), k
        sl = pipe.slots[k % 2]                                           # still holds batch k (the next submit follows this yield)
        with torch.cuda.stream(sl.stream):
            _, doff, dnf = sl.header(B)
            el, ev = raw_point_labels(sl.raw_rows, doff, dnf, sl.P, sl.out["npcs"], sl.out["ancsh"])
            ea = articulation_batch(sl.out["ancsh"], sl.out["npcs"], sl.out["record"])
        sl.stream.synchronize()
        assert _bytes(labels, el[:off[-1]].cpu().numpy()) and _bytes(values, ev[:off[-1]].cpu().numpy()), k
        assert _same(art, ea[:len(batches[k][0])].cpu().numpy()), k


def test_range_guard_refits_in_f32(dev):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches = [([c[:, :3].copy() for c in cl], nf) for cl, nf in _raw_batches(pb, 4, B, np.random.RandomState(9), short_last=False)]
    batches[1][1][0] = 1e6                                               # cloud 0 of batch 1: beyond f16's range
    f32 = list(_pipe(pb, K, B, N, 2, arithmetic="f32").stream_batches(batches))
    f16 = list(_pipe(pb, K, B, N, 2, arithmetic="f16x2").stream_batches(batches))
    guard = _pipe(pb, K, B, N, 2, arithmetic="f16x2", range_guard=True)
    got = list(guard.stream_batches(batches, flags=True))
    assert guard.f32_reruns == 1
    for k, (tag, seed, rec, words) in enumerate(got):
        for c in range(len(words)):
            hot = k == 1 and c == 0
            assert (words[c] != 0) == hot
            assert _same(rec[c], (f32 if hot else f16)[k][2][c]), (k, c)


def test_launch_budget_matches_ground_truth_mode(dev):
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 4, N, seed=2)
    calls = {}
    for src in ("gt", "predicted"):
        pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, "cuda:0", couple=True, niter_a=64, niter_b=8, use_graph=False,
                             joint_source=src)
        pipe.load_inputs(pb["P"], pb["cls"] if src == "gt" else None)
        pipe.step()
        pipe.synchronize()
        _lib.profile_start()
        pipe.step()
        calls[src] = [name for name, _, _ in _lib.profile_stop()]
        del pipe
    gt, pr = calls["gt"], calls["predicted"]
    assert len(gt) == len(pr)
    swap = {"ancsh_pose_joint_direction": "ancsh_pose_joint_direction_pred", "ancsh_pose_poison_records": "ancsh_pose_poison_records_pred"}
    assert [swap.get(n, n) for n in gt] == pr
    assert "ancsh_pose_joint_direction" not in pr and "ancsh_pose_poison_records" not in pr


_SHARDED = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import articulated_pose_amd  # noqa: F401
from articulated_pose_amd import dist as D
from articulated_pose_amd.synthetic import passthrough_pose_problem
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=500))
K, G, N, count = 3, 5, 512, 12
pb = passthrough_pose_problem(K, 6, N, seed=3)
rs = np.random.RandomState(19)
sizes = [G] * count
sizes[4], sizes[-1] = 4, 1
batches = []
for k, nb in enumerate(sizes):
    clouds = []
    for _ in range(nb):
        src, n = rs.randint(6), int(rs.randint(N // 3, 3 * N))
        idx = rs.randint(0, N, n)
        clouds.append((pb["P"][src][idx] + rs.normal(0, 2e-3, (n, 3))).astype(np.float32))
    batches.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32), "b%d" % k))
kw = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput", joint_source="predicted")
if world == 1:
    from articulated_pose_amd.pipeline import AncshPipeline
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, **kw)
    got = list(pipe.stream_batches(batches))
else:
    import torch.distributed as dist
    group, note = D.init_groups("gloo", "cuda:0")
    sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, **kw)
    got = list(sp.stream_batches(batches))
    if dist.get_rank() != 0:
        got = None
    dist.barrier()
    dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _ in got]), seeds=np.array([s for _, s, _ in got]),
             counts=np.array([len(r) for _, _, r in got]), records=np.concatenate([r for _, _, r in got]))
'''


def test_sharded_predicted_stream_equals_single_process(dev, tmp_path):
    script = tmp_path / "sharded_predicted.py"
    script.write_text(_SHARDED)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    outs = []
    for world in (1, 2):
        out = tmp_path / ("pred%d.npz" % world)
        r = subprocess.run([sys.executable, str(script), ROOT, str(world), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (world, r.returncode, r.stderr[-3000:])
        outs.append(np.load(out))
    one, two = outs
    assert list(one["tags"]) == list(two["tags"]) and list(one["seeds"]) == list(two["seeds"])
    assert list(one["counts"]) == list(two["counts"]) and one["counts"][-1] == 1
    assert _same(one["records"], two["records"])


def test_offline_solver_predicted_equals_pose_solver(dev, tmp_path):
    from articulated_pose_amd.pose import PoseSolver, solver_ransac_nonlinear
    K, B, N = 3, 3, 512
    base, jcls = _noisy_inputs(K, B, N, 7)
    idx = _index_head(np.random.RandomState(7), B, N, 3, jcls)
    names = ["obj_%d_0" % b for b in range(B)]
    for exp in ("ancsh", "npcs"):
        d = tmp_path / "results" / "test_pred" / exp
        d.mkdir(parents=True)
        for b, n in enumerate(names):
            np.savez(str(d / (n + ".npz")), P=base[0][b], nocs_per_point=base[1][b], instance_per_point=base[2][b],
                     joint_axis_per_point=base[3][b], joint_cls_gt=jcls[b], index_per_point=idx[b])
    got = solver_ransac_nonlinear(0, B, "ancsh", "npcs", 0.1, K, [n + ".h5" for n in names], [], None, str(tmp_path / "p.pkl"),
                                  base_path=str(tmp_path), batch_size=B, seed=4, joint_source="predicted")
    want = PoseSolver(K, 0.1, device=dev).solve(*base, joint_index=idx, seed=4)["nonlinear"].cpu().numpy()
    gt = PoseSolver(K, 0.1, device=dev).solve(*base, jcls, seed=4)["nonlinear"].cpu().numpy()
    for b, n in enumerate(names):
        for j in range(K):
            R, s, t = got[n]["rotation"]["nonlinear"][j], got[n]["scale"]["nonlinear"][j], got[n]["translation"]["nonlinear"][j]
            assert _same(np.concatenate([R.reshape(-1), [s], t]), want[b, j]), (n, j)
    assert not _same(want, gt)                                           # the association moved the fit
