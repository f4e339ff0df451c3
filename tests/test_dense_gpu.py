"""GPU: the per-raw-point labels (ancsh_raw_point_labels, dataset.raw_point_labels, AncshPipeline / ShardedPipeline dense=True) against
the existing three_nn_weights + three_interpolate operators (bit for bit), against the CPU oracle, on the rows the sampler picked, and
through the captured stream, non-finite input, the range guard and two gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0", dt).contiguous()


def _heads(rs, B, N, K, G):
    """Random heads: W positive rows summing to ~1 (some points with channels 0 and 1 equal), nocs (3K), gocs (G)."""
    W = rs.uniform(0.01, 1.0, (B, N, K)).astype(np.float32)
    if K > 1:
        W[:, ::7, 1] = W[:, ::7, 0]                                       # exact ties: the first maximum wins
    W /= W.sum(2, keepdims=True)
    return {"W": W.astype(np.float32), "nocs_per_point": rs.uniform(0, 1, (B, N, 3 * K)).astype(np.float32)}, \
        {"gocs_per_point": rs.uniform(-1, 1, (B, N, G)).astype(np.float32)}


def _clouds(rs, sizes):
    return [np.concatenate([rs.uniform(-0.5, 0.5, (n, 3)), rs.randint(0, 3, (n, 1))], 1).astype(np.float32) for n in sizes]


def _pack(clouds, cap=None):
    rows = np.concatenate(clouds, 0)
    if cap is not None:
        rows = np.concatenate([rows, np.zeros((cap - rows.shape[0], rows.shape[1]), np.float32)], 0)
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([c.shape[0] for c in clouds], out=off[1:])
    return rows, off


def _select(Wi, Ni, Gi, q, K, G):
    """The definition's selection from interpolated heads (numpy): -> labels, values."""
    R = Wi.shape[0]
    ok = np.isfinite(q).all(1) & np.isfinite(Wi).all(1)
    lab = np.where(ok, Wi.argmax(1), -1).astype(np.int32)
    l = np.maximum(lab, 0)
    r = np.arange(R)
    vals = np.empty((R, 7), np.float32)
    vals[:, 0] = Wi[r, l]
    for c in range(3):
        vals[:, 1 + c] = Ni[r, 3 * l + c]
        vals[:, 4 + c] = Gi[r, (0 if G == 3 else 3 * l) + c]
    vals[~ok] = np.nan
    return lab, vals


def _existing_ops(q, P, heads):
    """Per cloud: ancsh_three_nn_weights on (q, P) then ancsh_three_interpolate of each head -> (idx, interpolated heads) on the host."""
    from articulated_pose_amd import _lib
    n, N = q.shape[0], P.shape[0]
    qd, Pd = _dev(q[None]), _dev(P[None])
    dist = torch.empty((1, n, 3), dtype=torch.float32, device="cuda:0")
    idx = torch.empty((1, n, 3), dtype=torch.int32, device="cuda:0")
    w = torch.empty((1, n, 3), dtype=torch.float32, device="cuda:0")
    _lib.call("ancsh_three_nn_weights", 1, n, N, _lib.ptr(qd), _lib.ptr(Pd), _lib.ptr(dist), _lib.ptr(idx), _lib.ptr(w))
    out = []
    for h in heads:
        hd = _dev(h[None])
        o = torch.empty((1, n, h.shape[1]), dtype=torch.float32, device="cuda:0")
        _lib.call("ancsh_three_interpolate", 1, N, h.shape[1], n, _lib.ptr(hd), _lib.ptr(idx), _lib.ptr(w), _lib.ptr(o))
        out.append(o[0].cpu().numpy())
    return idx[0].cpu().numpy(), out


def _batch_case(K, N, G, seed):
    from articulated_pose_amd.dataset import sample_raw_batch
    rs = np.random.RandomState(seed)
    clouds = _clouds(rs, [1, N // 3, 20000, 777])                        # one row, a tiled cloud (duplicate points), large, medium
    nf = rs.uniform(0.5, 2.0, len(clouds)).astype(np.float32)
    s = sample_raw_batch(clouds, N, nf, seed=seed, return_perm=True)
    npcs, ancsh = _heads(rs, len(clouds), N, K, G)
    return clouds, nf, s, npcs, ancsh


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_equals_the_existing_operators_bit_for_bit(dev, K, N):
    from articulated_pose_amd.dataset import raw_point_labels
    G = 3 if K == 2 else 3 * K
    clouds, nf, s, npcs, ancsh = _batch_case(K, N, G, 10 * K + N // 1024)
    rows, off = _pack(clouds, cap=sum(c.shape[0] for c in clouds) + 50)
    lab, val = raw_point_labels(_dev(rows), _dev(off, torch.int32), _dev(nf), s["P"], {k: _dev(v) for k, v in npcs.items()},
                                {k: _dev(v) for k, v in ancsh.items()})
    lab, val = lab.cpu().numpy(), val.cpu().numpy()
    P = s["P"].cpu().numpy()
    for b, c in enumerate(clouds):
        q = c[:, :3] * nf[b]                                              # numpy float32 products: the sampler's bits
        _, (Wi, Ni, Gi) = _existing_ops(q, P[b], [npcs["W"][b], npcs["nocs_per_point"][b], ancsh["gocs_per_point"][b]])
        want_l, want_v = _select(Wi, Ni, Gi, q, K, G)
        a, e = off[b], off[b + 1]
        assert _same(lab[a:e], want_l), (b, np.flatnonzero(lab[a:e] != want_l)[:5])
        assert _same(val[a:e], want_v), b
    assert (lab[off[-1]:] == -1).all() and np.isnan(val[off[-1]:]).all()      # rows beyond the batch: untouched


def test_against_the_cpu_oracle(dev, oracle):
    from articulated_pose_amd.dataset import raw_point_labels
    K, N, G = 3, 1024, 9
    clouds, nf, s, npcs, ancsh = _batch_case(K, N, G, 7)
    rows, off = _pack(clouds)
    lab, val = raw_point_labels(_dev(rows), _dev(off, torch.int32), _dev(nf), s["P"], {k: _dev(v) for k, v in npcs.items()},
                                {k: _dev(v) for k, v in ancsh.items()})
    lab, val = lab.cpu().numpy(), val.cpu().numpy()
    P = s["P"].cpu().numpy()
    for b, c in enumerate(clouds):
        q = c[:, :3] * nf[b]
        d, i = oracle.three_nn(q[None], P[b][None])
        w = oracle.three_weights(d)[0].astype(np.float64)
        i = i[0]
        gpu_idx, _ = _existing_ops(q, P[b], [])
        assert np.array_equal(i, gpu_idx), b                                # 3-NN indices exact (the operator the labels equal bit for bit)
        interp = lambda h: (h[i] * w[:, :, None]).sum(1)
        Wi, Ni, Gi = interp(npcs["W"][b]), interp(npcs["nocs_per_point"][b]), interp(ancsh["gocs_per_point"][b])
        want_l, want_v = _select(Wi, Ni, Gi, q, K, G)
        a, e = off[b], off[b + 1]
        top2 = np.sort(Wi, 1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-6
        assert np.array_equal(lab[a:e][clear], want_l[clear]), b
        same = lab[a:e] == want_l
        np.testing.assert_allclose(val[a:e][same], want_v[same], rtol=0, atol=1e-6)


def test_sampled_rows_carry_their_own_head_values(dev):
    """A raw row the sampler picked sits at distance 0 from its copy in P: its labels and values are that point's own heads.  Points on a
    jittered grid (no two closer than ~0.03) keep the other two neighbours' weights below 1e-7."""
    from articulated_pose_amd.dataset import raw_point_labels, sample_raw_batch
    K, N, G = 4, 1024, 12
    rs = np.random.RandomState(5)
    clouds = []
    for n in (3000, 1500):
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)[rs.permutation(4096)[:n]]
        xyz = (g * 0.05 + rs.uniform(-0.01, 0.01, g.shape) - 0.4).astype(np.float32)
        clouds.append(np.concatenate([xyz, np.zeros((n, 1), np.float32)], 1))
    nf = np.array([1.0, 1.7], np.float32)
    s = sample_raw_batch(clouds, N, nf, seed=3, return_perm=True)
    npcs, ancsh = _heads(rs, 2, N, K, G)
    rows, off = _pack(clouds)
    lab, val = raw_point_labels(_dev(rows), _dev(off, torch.int32), _dev(nf), s["P"], {k: _dev(v) for k, v in npcs.items()},
                                {k: _dev(v) for k, v in ancsh.items()})
    lab, val, perm = lab.cpu().numpy(), val.cpu().numpy(), s["perm"].cpu().numpy()
    for b, c in enumerate(clouds):
        raw = off[b] + perm[b] % c.shape[0]                                 # raw row of sampled point i
        W = npcs["W"][b]
        top2 = np.sort(W, 1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-5
        l = W.argmax(1)
        assert np.array_equal(lab[raw][clear], l[clear]), b
        i = np.arange(N)
        own = np.concatenate([W[i, l][:, None], npcs["nocs_per_point"][b].reshape(N, K, 3)[i, l],
                              ancsh["gocs_per_point"][b].reshape(N, K, 3)[i, l]], 1)
        np.testing.assert_allclose(val[raw][clear], own[clear], rtol=0, atol=1e-6)


# ---- the stream ---------------------------------------------------------------------------------------------------------------
def _stream_batches(pb, B, N, count, rs, cap=None):
    out = []
    for k in range(count):
        nb = B if k % 4 else max(1, B - 1 - k % 3)                       # short batches now and then
        clouds = []
        for _ in range(nb):
            src, n = rs.randint(pb["P"].shape[0]), int(rs.randint(1, 3 * N))
            idx = rs.randint(0, N, n)
            clouds.append(np.concatenate([pb["P"][src][idx], pb["cls"][src][idx, None]], 1).astype(np.float32))
        out.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32)))
    if cap is not None:                                                   # the last batch fills raw_capacity exactly
        clouds = [c.copy() for c in out[1][0]]
        assert len(clouds) == B
        extra = cap - sum(c.shape[0] for c in clouds[:-1])
        clouds[-1] = np.concatenate([clouds[-1]] * (extra // clouds[-1].shape[0] + 1), 0)[:extra]
        out.append((clouds, out[1][1]))
    return out


def _pipe(pb, K, B, N, slots, cap, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    return AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, "cuda:0", couple=True, slots=slots, niter_a=64, niter_b=8, seed=11,
                         lm_schedule="throughput", raw_capacity=cap, **kw)


@pytest.mark.parametrize("slots,articulation", [(1, False), (3, True)])
def test_stream_equals_the_eager_op_and_records_unchanged(dev, slots, articulation):
    from articulated_pose_amd.dataset import raw_point_labels
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    cap = B * 3 * N
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches = _stream_batches(pb, B, N, 14, np.random.RandomState(slots), cap=cap)
    plain = list(_pipe(pb, K, B, N, slots, cap, articulation=articulation).stream_batches(batches, articulation=articulation))
    pipe = _pipe(pb, K, B, N, slots, cap, articulation=articulation, dense=True)
    n = 0
    for k, item in enumerate(pipe.stream_batches(batches, articulation=articulation, dense=True)):
        clouds = batches[k][0]
        assert len(item) == (5 if articulation else 4)
        labels, values, off = item[-1]
        assert _same(item[2], plain[k][2]), k                            # records unchanged by the extra launch
        if articulation:
            assert _same(item[3], plain[k][3]), k
        assert list(off) == list(np.cumsum([0] + [c.shape[0] for c in clouds])) and labels.shape == (off[-1],)
        # the slot of batch k still holds it (the generator submits the next batch after this yield): the eager op on its tensors
        sl = pipe.slots[k % slots]
        with torch.cuda.stream(sl.stream):
            _, doff, dnf = sl.header(B)
            el, ev = raw_point_labels(sl.raw_rows, doff, dnf, sl.P, sl.out["npcs"], sl.out["ancsh"])
        sl.stream.synchronize()
        assert _same(labels, el[:off[-1]].cpu().numpy()) and _same(values, ev[:off[-1]].cpu().numpy()), k
        assert (labels >= 0).mean() > 0.99, k
        n += 1
    assert n == len(batches)
    assert sum(c.shape[0] for c in batches[-1][0]) == cap
    assert all(len(x) == 3 for x in _pipe(pb, K, B, N, 1, cap, dense=True).stream_batches(batches[:2]))      # default: 3-tuples
    with pytest.raises(RuntimeError, match="dense=True"):
        next(_pipe(pb, K, B, N, 1, cap).stream_batches(batches[:1], dense=True))


def test_nonfinite_rows_are_isolated(dev):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    cap = B * 3 * N
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    clean = _stream_batches(pb, B, N, 4, np.random.RandomState(2))
    dirty = [([c.copy() for c in cl], nf) for cl, nf in clean]
    bad = []
    for k, (cl, _) in enumerate(dirty):
        j = (k + 1) % len(cl)
        r = np.random.RandomState(k).choice(cl[j].shape[0], min(5, cl[j].shape[0]), replace=False)
        cl[j][r[0], 0] = np.nan
        cl[j][r[1:], 1 + k % 2] = np.inf if k % 2 else -np.inf
        bad.append((j, r))
    got_c = list(_pipe(pb, K, B, N, 2, cap, dense=True).stream_batches(clean, dense=True))
    got_d = list(_pipe(pb, K, B, N, 2, cap, dense=True).stream_batches(dirty, dense=True))
    for k, ((_, _, _, (lc, vc, oc)), (_, _, _, (ld, vd, od)), (j, r)) in enumerate(zip(got_c, got_d, bad)):
        assert list(oc) == list(od)
        a, e = od[j], od[j + 1]
        assert (ld[a + r] == -1).all() and np.isnan(vd[a + r]).all(), k
        assert _same(ld[:a], lc[:a]) and _same(ld[e:], lc[e:]), k
        assert _same(vd[:a], vc[:a]) and _same(vd[e:], vc[e:]), k


def test_range_guard_takes_the_f32_rows(dev):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    cap = B * 3 * N
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches = _stream_batches(pb, B, N, 8, np.random.RandomState(9))
    hot = []
    for k, (clouds, nf) in enumerate(batches):
        h = np.zeros(len(clouds), bool)
        if k % 3 == 1:
            nf[0] = 1e6
            h[0] = True
        hot.append(h)
    mk = lambda arith, guard: _pipe(pb, K, B, N, 2, cap, arithmetic=arith, range_guard=guard, dense=True)
    f32 = list(mk("f32", False).stream_batches(batches, dense=True))
    f16 = list(mk("f16x2", False).stream_batches(batches, dense=True))
    got = list(mk("f16x2", True).stream_batches(batches, flags=True, dense=True))
    for (tag, _, rec, words, (lab, val, off)), x32, x16, h in zip(got, f32, f16, hot):
        assert ((words != 0) == h).all(), tag
        for c in range(len(h)):
            a, e = off[c], off[c + 1]
            ref = x32 if h[c] else x16
            assert _same(lab[a:e], ref[3][0][a:e]) and _same(val[a:e], ref[3][1][a:e]), (tag, c)


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
K, G, N, count = 3, 5, 512, 16
pb = passthrough_pose_problem(K, 6, N, seed=3)
rs = np.random.RandomState(23)
sizes = [G] * count
sizes[7], sizes[-1] = 4, 1
batches = []
for k, nb in enumerate(sizes):
    clouds = []
    for _ in range(nb):
        src, n = rs.randint(6), int(rs.randint(1, 3 * N))
        idx = rs.randint(0, N, n)
        clouds.append(np.concatenate([pb["P"][src][idx], pb["cls"][src][idx, None]], 1).astype(np.float32))
    batches.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32), "b%d" % k))
batches[12][0][3][:7, :3] = np.nan
kw = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput")
if world == 1:
    from articulated_pose_amd.pipeline import AncshPipeline
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, dense=True, **kw)
    got = list(pipe.stream_batches(batches, dense=True))
else:
    import torch.distributed as dist
    group, note = D.init_groups("gloo", "cuda:0")
    sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, dense=True, **kw)
    got = list(sp.stream_batches(batches, dense=True))
    if dist.get_rank() != 0:
        assert all(r is None and d is None for _, _, r, d in got)
        got = None
    dist.barrier()
    dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _, _ in got]), records=np.concatenate([r for _, _, r, _ in got]),
             labels=np.concatenate([d[0] for _, _, _, d in got]), values=np.concatenate([d[1] for _, _, _, d in got]),
             offsets=np.concatenate([d[2] for _, _, _, d in got]))
'''


def test_sharded_rows_equal_single_process(dev, tmp_path):
    """Two self-launched gloo ranks on one GPU: rank 0's raw-row labels and values (and records) equal one AncshPipeline stream's, byte
    for byte."""
    script = tmp_path / "sharded_dense.py"
    script.write_text(_SHARDED)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    outs = []
    for world in (1, 2):
        out = tmp_path / ("dense%d.npz" % world)
        r = subprocess.run([sys.executable, str(script), ROOT, str(world), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (world, r.returncode, r.stderr[-3000:])
        outs.append(np.load(out))
    one, two = outs
    assert list(one["tags"]) == list(two["tags"])
    for key in ("records", "labels", "values", "offsets"):
        assert _same(one[key], two[key]), key
    assert (two["labels"] == -1).sum() >= 1                             # the NaN rows of batch 12
