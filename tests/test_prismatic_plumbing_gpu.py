"""GPU: joint_types on every path that reaches stage B -- streamed records against the existing one-batch mirrors (wrapped, not copied:
the mirrors build their own PoseSolver, which is given the pipeline's joint_types while they run), keyed streams, couple=False
steps, articulation + dense streams, two ShardedPipeline ranks on one GPU -- and the joint_kind contract of the ABI 14 entries."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_joint_source_gpu as JS
import test_stream_gpu as TS
from helpers import passthrough_pose_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = ["revolute", "prismatic"]


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


@contextlib.contextmanager
def mirror_joint_types(joint_types):
    """The one-batch mirrors (test_stream_gpu._eager, test_joint_source_gpu._eager_predicted) import PoseSolver when they run: inside
    this context the solver they build fits the given joint kinds; everything else of the mirror is what it is."""
    import articulated_pose_amd.pose as pose
    real = pose.PoseSolver
    pose.PoseSolver = functools.partial(real, joint_types=joint_types)
    try:
        yield
    finally:
        pose.PoseSolver = real


@pytest.mark.parametrize("keyed", [False, True])
def test_gt_stream_equals_mirror(dev, keyed):
    """joint_source="gt", K = 3 with a revolute and a prismatic joint, captured step on 4 slots, plain and keyed header: every streamed
    record equals test_stream_gpu._eager run with the same joint_types, and is not the all-revolute record."""
    from articulated_pose_amd.pipeline import AncshPipeline
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=1)
    batches = TS._raw_batches(pb, 12, B, np.random.RandomState(7))
    kw = dict(couple=True, slots=4, niter_a=64, niter_b=8, seed=100, raw_capacity=B * 3 * N, keyed=keyed)
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, joint_types=MIXED, **kw)
    got = list(pipe.stream_batches(batches))
    assert pipe.slots[0].graph is not None
    plain = list(AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, **kw).stream_batches(batches))
    for k, ((tag, seed, rec), (clouds, nf)) in enumerate(zip(got, batches)):
        with mirror_joint_types(MIXED):
            want = TS._eager(pipe, clouds, nf, seed)
        assert TS._same(rec, want), k
        assert TS._same(rec[:, :2], plain[k][2][:, :2]) and not TS._same(rec[:, 2, 13:], plain[k][2][:, 2, 13:]), k   # the kind is per joint


def test_stream_articulation_and_dense_with_joint_types(dev):
    """articulation=True and dense=True on top of joint_types (predicted association, all prismatic): the records are those of the
    plain joint_types stream and of the mirror, the articulation block and the raw-row labels those of the eager ops on the slot."""
    from articulated_pose_amd.dataset import raw_point_labels
    from articulated_pose_amd.pose.joint_params import articulation_batch
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches = [([c[:, :3].copy() for c in cl], nf) for cl, nf in TS._raw_batches(pb, 8, B, np.random.RandomState(4))]
    plain = list(JS._pipe(pb, K, B, N, 2, joint_types="prismatic").stream_batches(batches))
    pipe = JS._pipe(pb, K, B, N, 2, articulation=True, dense=True, joint_types="prismatic")
    for k, item in enumerate(pipe.stream_batches(batches, articulation=True, dense=True)):
        tag, seed, rec, art, (labels, values, off) = item
        assert TS._same(rec, plain[k][2]), k
        with mirror_joint_types("prismatic"):
            assert TS._same(rec, JS._eager_predicted(pipe, batches[k][0], batches[k][1], seed)), k
        sl = pipe.slots[k % 2]
        with torch.cuda.stream(sl.stream):
            _, doff, dnf = sl.header(B)
            el, ev = raw_point_labels(sl.raw_rows, doff, dnf, sl.P, sl.out["npcs"], sl.out["ancsh"])
            ea = articulation_batch(sl.out["ancsh"], sl.out["npcs"], sl.out["record"])
        sl.stream.synchronize()
        assert JS._bytes(labels, el[:off[-1]].cpu().numpy()) and JS._bytes(values, ev[:off[-1]].cpu().numpy()), k
        assert TS._same(art, ea[:len(batches[k][0])].cpu().numpy()), k


@pytest.mark.parametrize("use_graph", [False, True])
def test_couple_false_step_equals_solve(dev, use_graph):
    """couple=False (the pose stage fed by load_inputs' predictions), 4 slots, eager and captured: every slot's record is the bytes of
    PoseSolver(joint_types=...).solve on the same inputs and seed."""
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    from articulated_pose_amd.weights import synthetic_weights
    K, B, N = 3, 4, 512
    cl = [make_cloud(320 + b, N=N, K=K) for b in range(B)]
    pr = [make_predictions(c, K, seed=b) for b, c in enumerate(cl)]
    P, jc = np.stack([c["P"] for c in cl]), np.stack([p["joint_cls_gt"] for p in pr])
    pred = {k: np.stack([p[k] for p in pr]) for k in ("nocs_per_point", "instance_per_point", "joint_axis_per_point")}
    w = synthetic_weights(K)
    pipe = AncshPipeline(K, w, w, B, N, dev, couple=False, use_graph=use_graph, slots=4, seed=5, niter_a=500, niter_b=64, joint_types=MIXED)
    pipe.load_inputs(P, jc, pred)
    pipe.prepare()
    solver = PoseSolver(K, pipe.solver.th, 500, 64, dev, lm_schedule=pipe.solver.lm_schedule, tie_window=None, joint_types=MIXED)
    want = solver.solve(P, pred["nocs_per_point"], pred["instance_per_point"], pred["joint_axis_per_point"], jc, seed=5)["record"]
    rev = PoseSolver(K, pipe.solver.th, 500, 64, dev, lm_schedule=pipe.solver.lm_schedule, tie_window=None).solve(
        P, pred["nocs_per_point"], pred["instance_per_point"], pred["joint_axis_per_point"], jc, seed=5)["record"]
    for _ in range(5):
        sl, out = pipe.step()
        sl.stream.synchronize()
        assert torch.equal(_bits(out["record"]), _bits(want))
    assert torch.equal(_bits(want[:, :2]), _bits(rev[:, :2])) and not torch.equal(_bits(want[:, 2, 13:]), _bits(rev[:, 2, 13:]))


_SHARDED = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import articulated_pose_amd  # noqa: F401
from articulated_pose_amd import dist as D
from articulated_pose_amd.synthetic import passthrough_pose_problem
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=500))
K, G, N, count = 3, 5, 512, 12
pb = passthrough_pose_problem(K, 6, N, seed=3)
rs = np.random.RandomState(29)
sizes = [G] * count
sizes[5], sizes[-1] = 4, 1
batches = []
for k, nb in enumerate(sizes):
    clouds = []
    for _ in range(nb):
        src, n = rs.randint(6), int(rs.randint(N // 3, 3 * N))
        idx = rs.randint(0, N, n)
        clouds.append(np.concatenate([pb["P"][src][idx], pb["cls"][src][idx, None]], 1).astype(np.float32))
    batches.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32), "b%d" % k))
kw = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput", articulation=True, dense=True)
if sys.argv[4] != "none":
    kw["joint_types"] = sys.argv[4].split(",")
if world == 1:
    from articulated_pose_amd.pipeline import AncshPipeline
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, **kw)
    got = list(pipe.stream_batches(batches, articulation=True, dense=True))
else:
    import torch.distributed as dist
    group, note = D.init_groups("gloo", "cuda:0")
    sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, **kw)
    got = list(sp.stream_batches(batches, articulation=True, dense=True))
    if dist.get_rank() != 0:
        got = None
    dist.barrier()
    dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([g[0] for g in got]), records=np.concatenate([g[2] for g in got]),
             articulation=np.concatenate([g[3] for g in got]), labels=np.concatenate([g[4][0] for g in got]),
             values=np.concatenate([g[4][1] for g in got]), offsets=np.concatenate([g[4][2] for g in got]))
'''


def test_sharded_stream_with_joint_types_equals_single_process(dev, tmp_path):
    """Two self-launched gloo ranks sharing the GPU, articulation=True and dense=True on, joint 1 revolute and joint 2 prismatic: rank 0's
    records, articulation blocks and raw-row labels equal the one-GPU stream's byte for byte -- and the records are not the all-revolute
    stream's (the kinds did reach both ranks' kernels)."""
    script = tmp_path / "sharded_kinds.py"
    script.write_text(_SHARDED)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    outs = {}
    for world, kinds in ((1, "revolute,prismatic"), (2, "revolute,prismatic"), (1, "none")):
        out = tmp_path / ("kinds%d%s.npz" % (world, kinds[:3]))
        r = subprocess.run([sys.executable, str(script), ROOT, str(world), str(out), kinds], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (world, kinds, r.returncode, r.stderr[-3000:])
        outs[(world, kinds)] = np.load(out)
    one, two, rev = outs[(1, "revolute,prismatic")], outs[(2, "revolute,prismatic")], outs[(1, "none")]
    assert list(one["tags"]) == list(two["tags"])
    for key in ("records", "articulation", "labels", "values", "offsets"):
        assert one[key].shape == two[key].shape and one[key].tobytes() == two[key].tobytes(), key
    assert TS._same(one["records"][:, :2], rev["records"][:, :2]) and not TS._same(one["records"][:, 2, 13:], rev["records"][:, 2, 13:])


# ---- the joint_kind contract of the ABI 14 entries (include/ancsh_hip.h) -----------------------------------------------------------
def _stage_b_problem(dev):
    """Two stage-B problems (a K = 3 cloud) from PoseSolver's own partition, with every buffer an entry needs."""
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    K, N = 3, 512
    c = make_cloud(310, N=N, K=K, joint_type="prismatic")
    p = make_predictions(c, K, seed=1)
    sol = PoseSolver(K, 0.1, 64, 50, dev).solve(c["P"][None], p["nocs_per_point"][None], p["instance_per_point"][None],
                                                p["joint_axis_per_point"][None], p["joint_cls_gt"][None], seed=3)
    return sol, K


def _call_entry(name, sol, K, dev, kind_ptr=None):
    from articulated_pose_amd import _lib
    nprob, niter, max_n = K - 1, 50, sol["_max_n"]
    o = dict(model=torch.empty((nprob, 26), dtype=torch.float64, device=dev), inl=torch.empty((nprob, 2, max_n), dtype=torch.uint8, device=dev),
             best=torch.empty((nprob,), dtype=torch.int32, device=dev), score=torch.empty((nprob,), dtype=torch.float64, device=dev),
             sc=torch.empty((nprob * niter,), dtype=torch.float64, device=dev), mo=torch.empty((nprob * niter, 26), dtype=torch.float64, device=dev),
             stat=torch.empty((nprob, niter, 2), dtype=torch.int32, device=dev), rec=torch.zeros((1, K, 26), dtype=torch.float64, device=dev),
             tie=torch.empty((nprob, 2), dtype=torch.int32, device=dev))
    rng0, rng1 = sol["_rng"]
    args = [nprob, _lib.ptr(rng0), _lib.ptr(rng1), _lib.ptr(sol["_src"]), _lib.ptr(sol["_tgt"]), _lib.ptr(sol["joint_direction"]), 0.1, niter,
            None, 4, max_n, _lib.ptr(o["model"]), _lib.ptr(o["inl"]), _lib.ptr(o["best"]), _lib.ptr(o["score"]), _lib.ptr(o["sc"]),
            _lib.ptr(o["mo"]), _lib.ptr(o["stat"]), 1, _lib.ptr(o["rec"]), K, _lib.ptr(o["tie"]), 2.0 ** -22]
    if name.endswith("_kind"):
        args.append(kind_ptr)
    _lib.call(name, *args)
    torch.cuda.synchronize()
    return o


def test_joint_kind_contract(dev):
    """NULL through ancsh_ransac_joint_rec_kind = the bytes of ancsh_ransac_joint_rec; a device array [0, 7] = the bytes of [0, 1] (any
    non-zero entry is prismatic; nothing traps) and not those of [0, 0]; a pinned host array [0, 2] is refused before any launch with
    ANCSH_EINVAL and a message naming entry 1; a pinned [0, 1] is accepted and gives the device array's bytes."""
    from articulated_pose_amd import _lib
    sol, K = _stage_b_problem(dev)
    base = _call_entry("ancsh_ransac_joint_rec", sol, K, dev)
    null = _call_entry("ancsh_ransac_joint_rec_kind", sol, K, dev, None)
    for k in base:
        assert torch.equal(_bits(base[k]), _bits(null[k])), k
    dk = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    k01, k07, k00, km1 = (dk(0, 1), dk(0, 7), dk(0, 0), dk(0, -1))
    o01, o07, o00, om1 = (_call_entry("ancsh_ransac_joint_rec_kind", sol, K, dev, _lib.ptr(t)) for t in (k01, k07, k00, km1))
    for k in o01:
        assert torch.equal(_bits(o01[k]), _bits(o07[k])) and torch.equal(_bits(o01[k]), _bits(om1[k])), k
        assert torch.equal(_bits(o00[k]), _bits(base[k])), k
    assert not torch.equal(_bits(o01["model"][1]), _bits(base["model"][1])) and torch.equal(_bits(o01["model"][0]), _bits(base["model"][0]))
    bad = torch.tensor([0, 2], dtype=torch.int32).pin_memory()
    with pytest.raises(ValueError, match=r"joint_kind\[1\] = 2"):
        _call_entry("ancsh_ransac_joint_rec_kind", sol, K, dev, bad.data_ptr())
    L = _lib.lib()
    assert b"joint_kind[1]" in L.ancsh_last_error()
    good = torch.tensor([0, 1], dtype=torch.int32).pin_memory()
    og = _call_entry("ancsh_ransac_joint_rec_kind", sol, K, dev, good.data_ptr())
    for k in o01:
        assert torch.equal(_bits(o01[k]), _bits(og[k])), k
