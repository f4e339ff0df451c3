"""Sharded streaming on the MI355X: the key block (ancsh_stream_key) makes a cloud's samples and pose draws follow its GLOBAL index,
so the keyed sampler / pose fit of a shard with cloud_base = lo equal rows [lo, hi) of the whole batch, a captured keyed slot follows
the base written into its header, and dist.ShardedPipeline.stream_batches over two ranks gives the records of one
AncshPipeline.stream_batches byte for byte."""
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
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t      # NaN-safe exact comparison


def test_keyed_sampler_is_shard_invariant(dev):
    from articulated_pose_amd.dataset import sample_raw_batch
    N = 512
    rs = np.random.RandomState(7)
    sizes = [1, 7, N - 1, N, 3 * N, 200, 900]
    clouds = []
    for n in sizes:
        c = rs.uniform(-1, 1, (n, 4)).astype(np.float32)
        c[:, 3] = rs.randint(0, 3, n)
        clouds.append(c)
    nf = rs.uniform(0.5, 2.0, len(sizes)).astype(np.float32)
    keys = ("P", "joint_cls", "perm")
    for seed in (0, 12345, 2 ** 64 - 3):
        plain = sample_raw_batch(clouds, N, nf, seed, dev, return_perm=True)
        full = sample_raw_batch(clouds, N, nf, seed, dev, return_perm=True, cloud_base=0)
        for k in keys:
            assert torch.equal(full[k], plain[k]), (seed, k)                 # base 0 keyed = the plain entry, byte for byte
        for lo, hi in ((0, 3), (3, 7), (2, 5), (6, 7)):
            part = sample_raw_batch(clouds[lo:hi], N, nf[lo:hi], seed, dev, return_perm=True, cloud_base=lo)
            for k in keys:
                assert torch.equal(part[k], full[k][lo:hi]), (seed, lo, hi, k)
    # the base is what moves the sample: cloud 4 keyed as global cloud 0 draws another permutation than as cloud 4
    as0 = sample_raw_batch(clouds[4:5], N, nf[4:5], 5, dev, return_perm=True, cloud_base=0)["perm"]
    as4 = sample_raw_batch(clouds[4:5], N, nf[4:5], 5, dev, return_perm=True, cloud_base=4)["perm"]
    assert not torch.equal(as0, as4)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_keyed_pose_fit_is_shard_invariant(dev, K):
    """Stages A and B of clouds [lo, hi) with the key block (seed s, cloud_base lo) give rows [lo, hi) of the whole batch's by-value
    solve(seed=s): records, winners, inlier masks, joint scores and tie counts (the stage-B finish kernel's tie pass re-draws too)."""
    from articulated_pose_amd.dataset import stream_key_words
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.parallel_ancsh_pose import TIE_WINDOW
    from articulated_pose_amd.synthetic import make_cloud, make_predictions
    B, N = 5, 1024
    cl = [make_cloud(60 + b, N=N, K=K) for b in range(B)]
    pr = [make_predictions(c, K, seed=b) for b, c in enumerate(cl)]
    inputs = [np.stack([c["P"] for c in cl])] + [np.stack([p[k] for p in pr]) for k in ("nocs_per_point", "instance_per_point",
                                                                                      "joint_axis_per_point", "joint_cls_gt")]
    solver = PoseSolver(K, 0.1, 400, 32, dev, tie_window=TIE_WINDOW)
    names = ("record", "best_a", "best_b", "inliers_a", "inliers_b", "tie_a", "tie_b", "score_b")
    key = lambda s, base: torch.from_numpy(stream_key_words(s, base)).to(dev)
    for s in (7, 2 ** 64 - 2):
        full = solver.solve(*inputs, seed=s)
        base0 = solver.solve(*inputs, key_dev=key(s, 0))
        for n in names:
            assert torch.equal(_bits(base0[n]), _bits(full[n])), (s, n)
        for lo, hi in ((0, 2), (2, 5), (4, 5)):
            part = solver.solve(*[x[lo:hi] for x in inputs], key_dev=key(s, lo))
            for n in names:
                assert torch.equal(_bits(part[n]), _bits(full[n][lo:hi])), (s, lo, hi, n)
    # without the base, a shard draws other samples: the winners move
    unbased = solver.solve(*[x[2:5] for x in inputs], key_dev=key(7, 0))
    assert not torch.equal(unbased["best_a"], solver.solve(*inputs, seed=7)["best_a"][2:5])


def test_captured_keyed_slot_follows_the_header_base(dev):
    """One captured keyed slot, its header's base rewritten between replays (2, 0, 2): base 2 gives rows 2..5 of a six-cloud keyed
    pipeline's batch both times, base 0 gives the unkeyed pipeline's record.  Misuse of cloud_base is refused."""
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, N = 3, 512
    pb = passthrough_pose_problem(K, 6, N, seed=1)
    (clouds, nf), = _raw_batches(pb, 1, 6, np.random.RandomState(11), short_last=False)
    kw = dict(couple=True, slots=1, niter_a=64, niter_b=8, raw_capacity=6 * 3 * N, lm_schedule="throughput")
    p6 = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], 6, N, dev, keyed=True, **kw)
    p6.submit(clouds, nf, seed=21)
    r6 = p6.retire()[2]
    del p6
    p4 = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], 4, N, dev, keyed=True, **kw)
    got = {}
    for i, base in enumerate((2, 0, 2)):
        p4.submit(clouds[2:6], nf[2:6], seed=21, cloud_base=base)
        got[i] = p4.retire()[2]
    assert p4.slots[0].graph is not None
    assert _same(got[0], r6[2:6]) and _same(got[2], r6[2:6])
    assert not _same(got[1], r6[2:6])
    with pytest.raises(ValueError):
        p4.submit(clouds[2:6], nf[2:6], cloud_base=-1)
    with pytest.raises(ValueError):
        p4.submit(clouds[2:6], nf[2:6], cloud_base=(1 << 20) // K)
    del p4
    pu = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], 4, N, dev, keyed=False, **kw)
    with pytest.raises(ValueError):
        pu.submit(clouds[2:6], nf[2:6], cloud_base=2)
    pu.submit(clouds[2:6], nf[2:6], seed=21)
    assert _same(pu.retire()[2], got[1])


_STREAM_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import articulated_pose_amd
from articulated_pose_amd import dist as D
from articulated_pose_amd.synthetic import passthrough_pose_problem
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=500))
K, G, N, count = 3, 5, 512, 52
pb = passthrough_pose_problem(K, 6, N, seed=3)
rs = np.random.RandomState(17)
sizes = [G] * count
sizes[10], sizes[20], sizes[-1] = 4, 3, 1          # short batches: rank 1 (clouds 3, 4) holds one cloud, none, none
batches = []
for k, nb in enumerate(sizes):
    clouds = []
    for _ in range(nb):
        src, n = rs.randint(6), int(rs.randint(N // 3, 3 * N))
        idx = rs.randint(0, N, n)
        c = np.concatenate([pb["P"][src][idx] + rs.normal(0, 2e-3, (n, 3)).astype(np.float32), pb["cls"][src][idx, None]], 1)
        clouds.append(c.astype(np.float32))
    batches.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32), "b%d" % k))
batches[30][0][3][:, :3] = np.nan                   # an all-NaN cloud in rank 1's shard
kw = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput")
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
        assert all(r is None for _, _, r in got) and [t for t, _, _ in got] == [b[2] for b in batches]
        got = None
    dist.barrier()
    dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _ in got]), seeds=np.array([s for _, s, _ in got]),
             counts=np.array([len(r) for _, _, r in got]), records=np.concatenate([r for _, _, r in got]))
'''


def test_sharded_stream_equals_single_process(dev, tmp_path):
    """Two self-launched ranks share the GPU (gloo): ShardedPipeline.stream_batches over 52 ragged global batches of 5 clouds (a 3 + 2
    split; short batches of 4, 3 and 1 clouds leave rank 1 one cloud or none; an all-NaN cloud in rank 1's shard) gives on rank 0 the
    tags, seeds and records of one AncshPipeline.stream_batches over the same batches, byte for byte."""
    script = tmp_path / "sharded_stream.py"
    script.write_text(_STREAM_SCRIPT)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    outs = []
    for world in (1, 2):
        out = tmp_path / ("stream%d.npz" % world)
        r = subprocess.run([sys.executable, str(script), ROOT, str(world), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (world, r.returncode, r.stderr[-3000:])
        outs.append(np.load(out))
    one, two = outs
    assert list(one["tags"]) == list(two["tags"]) == ["b%d" % k for k in range(52)]
    assert list(one["seeds"]) == list(two["seeds"]) == [100 + 2 * k for k in range(52)]
    assert list(one["counts"]) == list(two["counts"]) and one["counts"][-1] == 1 and one["counts"][20] == 3
    assert _same(one["records"], two["records"])
    rec = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(rec[30][3]).all() and not any(np.isnan(rec[30][i]).all() for i in (0, 1, 2, 4))
    assert sum(np.isnan(r).all(axis=(1, 2)).sum() for r in rec) == 1          # the NaN cloud's record alone is poisoned
