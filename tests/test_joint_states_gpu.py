"""GPU: the joint states (ancsh_joint_state_rec, pose.joint_params.joint_state_batch, AncshPipeline / ShardedPipeline joint_states=True)
against the numpy mirror (tests/joint_state_mirror.py), against ancsh_part_extents on the same heads, and through the captured stream, the
depth front end, the range guard and two gloo ranks.

Columns 12, 13 and 17 against the mirror, absolute 1e-9 (degrees / record units): O(1) float64 inputs through three-term dot products, a
square root and one atan2, a few ulp each -- the margin of the CPU check of the angle (tests/test_joint_states_cpu.py).  Largest
differences measured on an MI355X over the four shapes below (the test prints them per shape): column 12 2.84e-14 degrees, column 13
2.84e-14 degrees, column 17 4.44e-16 -- all below the 1e-12 a few ulp of a value up to 180 lets one expect."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import passthrough_pose_problem
from joint_state_mirror import joint_state_reference
from test_joint_states_cpu import _rotation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 100, 3), (2, 64, 2), (1, 7, 1), (2, 257, 4)]          # (b, n, K): n no multiple of 64; one wave; K = 1; two trips of the block
TOL = 1e-9


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.array(a)).to("cuda:0", dt).contiguous()


@functools.lru_cache(maxsize=None)
def _problem(b, n, K):
    """Seeded random heads, records and articulation blocks (host arrays, never modified) and the mirror's block for them.  K = 3: cloud 0
    has R_1 = R_0 and no point in part 2, cloud 1 a NaN axis for joint 2, cloud 2 a NaN in part 0's pose; K = 4: P rows of 4 floats, cloud 1
    a NaN in part 2's pose and a zero axis for joint 3."""
    rs = np.random.RandomState(1000 * b + 10 * n + K)
    ldp = 4 if K == 4 else 3
    P = rs.uniform(-1, 1, (b, n, ldp)).astype(np.float32)
    nocs = rs.uniform(0, 1, (b, n, 3 * K)).astype(np.float32)
    mask = rs.uniform(0, 1, (b, n, K)).astype(np.float32)
    rec = rs.normal(size=(b, K, 26))
    for c in range(b):
        rec[c, :, 13:22] = np.stack([_rotation(rs) for _ in range(K)]).reshape(K, 9)
    art = rs.normal(size=(b, K, 12))
    art[:, 0, 6:] = np.nan
    if K == 3:
        rec[0, 1, 13:22] = rec[0, 0, 13:22]
        mask[0, :, 2] = -1.0
        art[0, 2, :3] = np.nan                                      # as ancsh_articulation_rec leaves an empty part's box
        art[1, 2, 9:12] = np.nan
        rec[2, 0, 17] = np.nan
        art[2] = np.frombuffer(np.array([0x7ff8000000000abc], np.uint64).tobytes(), np.float64)[0]       # NaNs with a payload
    if K == 4:
        rec[1, 2, 25] = np.nan
        art[1, 3, 9:12] = 0.0
    want = joint_state_reference(P, nocs, mask, rec, art)
    for a in (P, nocs, mask, rec, art, want):
        a.setflags(write=False)
    return dict(P=P, nocs=nocs, mask=mask, rec=rec, art=art, want=want, ldp=ldp)


def _run(p):
    from articulated_pose_amd.pose.joint_params import joint_state_batch
    return joint_state_batch(_dev(p["P"]), {"nocs_per_point": _dev(p["nocs"]), "W": _dev(p["mask"])}, _dev(p["rec"], torch.float64),
                             _dev(p["art"], torch.float64))


@pytest.mark.parametrize("b,n,K", SHAPES)
def test_kernel_against_mirror_and_part_extents(dev, b, n, K):
    from articulated_pose_amd import _lib
    p = _problem(b, n, K)
    wide = _run(p)
    assert wide.shape == (b, K, 20) and wide.dtype == torch.float64
    art = _dev(p["art"], torch.float64)
    assert torch.equal(wide[..., :12].contiguous().view(torch.int64), art.view(torch.int64))          # bit patterns, NaN payloads included
    got, want = wide.cpu().numpy(), p["want"]
    assert _same(_run(p).cpu().numpy(), got)                                                          # two runs, identical bytes
    # ancsh_part_extents with the record's part-0 pose: dynam, canon and the count behind columns 18 and 19
    rec = _dev(p["rec"], torch.float64)
    scale = torch.empty((b, K, 3), dtype=torch.float32, device=dev)
    dyn = torch.empty((b, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((b, K), dtype=torch.int32, device=dev)
    pose0 = torch.cat([rec[:, 0, 13:22], rec[:, 0, 23:26]], 1).contiguous()
    nocs, mask, P = _dev(p["nocs"]), _dev(p["mask"]), _dev(p["P"])
    _lib.call("ancsh_part_extents", b, n, K, 3 * K, _lib.ptr(nocs), _lib.ptr(mask), _lib.ptr(P), p["ldp"], _lib.ptr(pose0), _lib.ptr(scale),
              _lib.ptr(dyn), _lib.ptr(cnt))
    canon = -scale.cpu().numpy()[:, :, 0] / np.float32(2) + np.float32(0.5)
    d = dyn.cpu().numpy() - canon.astype(np.float64)
    nan_pose = np.isnan(p["rec"][:, :, 13:26]).any(2)
    dead = nan_pose | nan_pose[:, :1]
    d[dead] = np.nan
    assert np.array_equal(got[:, :, 19], cnt.cpu().numpy().astype(np.float64))
    assert np.array_equal(got[:, :, 18], d, equal_nan=True) and np.array_equal(np.isnan(d), dead | (cnt.cpu().numpy() == 0))
    # the mirror: exact where the arithmetic is a difference or a count, 1e-9 behind the dot products, the square root and the atan2
    assert np.array_equal(got[:, :, 14:17], want[:, :, 14:17], equal_nan=True) and np.array_equal(got[:, :, 19], want[:, :, 19])
    assert np.array_equal(got[:, :, 18], want[:, :, 18], equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for col in (12, 13, 17):
        fin = np.isfinite(want[:, :, col])
        diff = np.abs(got[:, :, col][fin] - want[:, :, col][fin]).max() if fin.any() else 0.0
        print("joint_state (b, n, K) = %s column %d: max |kernel - mirror| = %.3g" % ((b, n, K), col, diff))
        assert diff <= TOL, (col, diff)
    # the rows that must be NaN, and only those
    nan = np.isnan(got[:, :, 12:19])
    must = np.zeros((b, K, 7), bool)
    must[:, 0, :6] = True                                           # row 0: no relative pose
    must[dead] = True                                               # a poisoned part 0: the cloud; a poisoned part: its row
    must[:, :, 6] |= cnt.cpu().numpy() == 0                         # a part without points: no boundary
    no_axis = ~(np.linalg.norm(p["art"][:, :, 9:12], axis=2) > 0)   # NaN or zero axis: no signed angle, no slide along it
    must[:, :, 1] |= no_axis
    must[:, :, 5] |= no_axis
    assert np.array_equal(nan, must)
    if K == 3:
        assert got[0, 1, 12] == 0.0 and got[0, 2, 19] == 0 and np.isnan(got[2, :, 12:19]).all() and np.isfinite(got[1, 2, 12])
        assert np.isfinite(got[0, 0, 18]) and np.isnan(got[1, 2, 13]) and np.isnan(got[1, 2, 17])
    if K == 4:
        assert np.isnan(got[1, 2, 12:19]).all() and np.isfinite(got[1, 1, 12:19]).all() and np.isfinite(got[1, 0, 18])
    assert got[:, :, 19].sum() == b * n


def test_launch_is_capturable(dev):
    from articulated_pose_amd import _lib
    b, n, K = SHAPES[0]
    p = _problem(b, n, K)
    P, nocs, mask = _dev(p["P"]), _dev(p["nocs"]), _dev(p["mask"])
    rec, art = _dev(p["rec"], torch.float64), _dev(p["art"], torch.float64)
    wide = torch.zeros((b, K, 20), dtype=torch.float64, device=dev)
    launch = lambda: _lib.call("ancsh_joint_state_rec", b, n, K, _lib.ptr(P), p["ldp"], _lib.ptr(nocs), _lib.ptr(mask), _lib.ptr(rec),
                               _lib.ptr(art), _lib.ptr(wide))
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        launch()
    st.synchronize()
    eager = wide.cpu().numpy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        launch()
    runs = []
    for _ in range(2):
        wide.zero_()
        g.replay()
        torch.cuda.synchronize()
        runs.append(wide.cpu().numpy())
    assert _same(runs[0], eager) and _same(runs[1], eager)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
K_, B_, N_ = 3, 4, 512                                             # the set-up of tests/test_articulation_gpu.py's stream tests


def _batches(pb, count, rs):
    from test_articulation_gpu import _stream_batches
    return _stream_batches(pb, K_, B_, N_, count, rs)              # short batches at k = 0, a NaN cloud in batch 5


def _pipe(pb, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=1, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", raw_capacity=B_ * 3 * N_,
                   articulation=True), **kw)
    return AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **kw)


def _check_against_eager(pipe, block):
    """`block` was just retired from a one-slot pipeline: the slot still holds that batch's P, heads, record and block."""
    from articulated_pose_amd.pose.joint_params import joint_state_batch
    sl = pipe.slots[0]
    sl.stream.synchronize()
    out = sl.out
    eager = joint_state_batch(sl.P, out["npcs"], out["record"], out["articulation"][..., :12].contiguous())
    assert _same(eager.cpu().numpy()[:len(block)], block)


@pytest.mark.parametrize("slots", [1, 4])
def test_stream_keeps_records_and_block_and_adds_the_state(dev, slots):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _batches(pb, 12, np.random.RandomState(slots))
    base = list(_pipe(pb, slots=slots).stream_batches(batches, articulation=True))
    pipe = _pipe(pb, slots=slots, joint_states=True)
    assert pipe.slots[0].outputs["articulation"].host[0].shape == (B_, K_, 20)
    got = []
    for item in pipe.stream_batches(batches, articulation=True):
        got.append(item)
        if slots == 1:
            _check_against_eager(pipe, item[3])
    assert len(got) == len(base) == 12
    for (t0, s0, r0, a0), (t1, s1, r1, a1), (clouds, _) in zip(base, got, batches):
        assert (t0, s0) == (t1, s1) and _same(r0, r1)
        assert a0.shape == (len(clouds), K_, 12) and a1.shape == (len(clouds), K_, 20) and _same(a0, a1[..., :12]), t0
    w5 = got[5][3]
    assert np.isnan(w5[1, :, :19]).all() and np.isfinite(w5[0, 1:, 12]).all() and (w5[:, :, 19].sum(1) == N_).all()
    assert all(len(x) == 3 for x in _pipe(pb, joint_states=True).stream_batches(batches[:1]))       # the default keeps 3-tuples


def test_depth_stream_carries_the_state(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_depth_gpu import SIDE, _camera, _depth_batches, _scale
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _depth_batches(pb, 2, 2, np.random.RandomState(4), "uint16", short_last=False)        # two small crops a batch
    mk = lambda **kw: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], 2, N_, "cuda:0", couple=True, slots=1, niter_a=64, niter_b=8, seed=11,
                                    lm_schedule="throughput", articulation=True, depth_capacity=2 * SIDE * SIDE, joint_source="predicted", **kw)
    base = list(mk().stream_depth_batches(batches, _camera(), _scale("uint16"), articulation=True))
    pipe = mk(joint_states=True)
    n = 0
    for (t0, s0, r0, a0, c0), item in zip(base, pipe.stream_depth_batches(batches, _camera(), _scale("uint16"), articulation=True)):
        t1, s1, r1, a1, c1 = item
        assert (t0, s0) == (t1, s1) and _same(r0, r1) and _same(c0, c1) and a1.shape == (2, K_, 20) and _same(a0, a1[..., :12])
        _check_against_eager(pipe, a1)
        n += 1
    assert n == 2


def test_range_guard_takes_the_f32_wide_rows(dev):
    """One cloud forced over f16's range by its norm factor, as tests/test_articulation_gpu.py and tests/test_range_guard_gpu.py do."""
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    batches = _batches(pb, 4, np.random.RandomState(9))
    hot = []
    for k, (clouds, nf) in enumerate(batches):
        h = np.zeros(len(clouds), bool)
        if k % 2 == 1:
            nf[0] = 1e6
            h[0] = True
        hot.append(h)
    mk = lambda arith, guard: _pipe(pb, slots=2, arithmetic=arith, range_guard=guard, joint_states=True)
    f32 = list(mk("f32", False).stream_batches(batches, articulation=True))
    f16 = list(mk("f16x2", False).stream_batches(batches, articulation=True))
    guarded = mk("f16x2", True)
    assert guarded.slots[0].outputs["articulation"].host32[0].shape == (B_, K_, 20)
    got = list(guarded.stream_batches(batches, flags=True, articulation=True))
    assert guarded.f32_reruns == 2
    for (tag, _, rec, words, wide), (_, _, r32, w32), (_, _, r16, w16), h in zip(got, f32, f16, hot):
        assert ((words != 0) == h).all() and wide.shape[2] == 20, tag
        assert _same(wide[h], w32[h]) and _same(rec[h], r32[h]), tag
        assert _same(wide[~h], w16[~h]) and _same(rec[~h], r16[~h]), tag


_SHARDED = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import articulated_pose_amd  # noqa: F401
from articulated_pose_amd import dist as D
sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import passthrough_pose_problem
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=300))
import torch.distributed as dist
from test_joint_states_gpu import sharded_problem
pb, batches, K, G, N, kw = sharded_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, articulation=True, joint_states=True, **kw)
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


def sharded_problem():
    """The global batches the two ranks and the single pipeline stream: 5 clouds a batch (shards of 3 and 2), one short batch, a NaN cloud."""
    K, G, N = 3, 5, 512
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    rs = np.random.RandomState(23)
    batches = []
    for k, nb in enumerate([G, G, 4, G, G, 1]):
        clouds = []
        for _ in range(nb):
            src, n = rs.randint(6), int(rs.randint(N // 3, 3 * N))
            idx = rs.randint(0, N, n)
            clouds.append(np.concatenate([pb["P"][src][idx], pb["cls"][src][idx, None]], 1).astype(np.float32))
        batches.append((clouds, rs.uniform(0.9, 1.1, nb).astype(np.float32), "b%d" % k))
    batches[3][0][3][:, :3] = np.nan
    return pb, batches, K, G, N, dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput")


def test_sharded_wide_blocks_equal_one_pipeline(dev, tmp_path):
    """Two self-launched gloo ranks on one GPU (as tests/test_dist_gpu.py runs them): rank 0's gathered (n_valid, K, 20) blocks and records
    equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    pb, batches, K, G, N, kw = sharded_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, articulation=True, joint_states=True, **kw)
    one = list(pipe.stream_batches(batches, articulation=True))
    del pipe
    script = tmp_path / "sharded_joint_states.py"
    script.write_text(_SHARDED)
    out = tmp_path / "wide2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r, _ in one]
    assert two["blocks"].shape[1:] == (K, 20)
    assert _same(two["records"], np.concatenate([r for _, _, r, _ in one]))
    assert _same(two["blocks"], np.concatenate([a for _, _, _, a in one]))
    blocks = np.split(two["blocks"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(blocks[3][3, :, :19]).all() and np.isfinite(blocks[3][2, 1:, 12]).all()
