"""GPU: the per-point ground truth built on the device (ancsh_point_gt_build, dataset.build_point_gt_rows, AncshPipeline / ShardedPipeline
build_point_gt=True) against the reference's own rows (tests/golden/point_gt_build.npz: x y z, cls and joint_cls bit-exact, every other
column within one float32 ulp -- both sides round one float64 result once, and those results differ by evaluation order only), against the
float64 mirror at ragged shapes, and through the sampler, the captured stream, the range guard and two gloo ranks, where a pipeline fed
7-column clouds and rigs must stream the bytes of one fed the 18-column rows the eager op made of them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import passthrough_pose_problem
from point_gt_build_mirror import build_batch, rig_width
from redzone import guarded
from test_point_gt_build_cpu import CASES, check_rows, golden_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_rows_nan(got, want, what):
    """check_rows where the expectation holds NaN: the same elements are NaN, every other one meets check_rows' bars."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    check_rows(np.nan_to_num(got, nan=1.0), np.nan_to_num(want, nan=1.0), what)


# ---- the eager op against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_eager_rows_equal_the_reference(dev, name):
    from articulated_pose_amd.dataset import build_point_gt_rows
    c, src, rig, _, K = golden_case(name)
    with guarded():
        rows, off = build_point_gt_rows([src], [rig], dev)
        torch.cuda.synchronize()
        got = rows.cpu().numpy()
    assert off.cpu().tolist() == [0, src.shape[0]] and got.shape == (src.shape[0], 18)
    check_rows(got, c["rows"], "eager, case " + name)


@pytest.mark.parametrize("names,misalign", [(("b", "e", "b"), 0), (("a", "c", "a"), 4), (("e", "b", "e"), 8)], ids=["K3", "K2-misaligned", "K3-misaligned"])
def test_three_clouds_in_one_launch_with_spare_capacity(dev, names, misalign):
    """Shape2motion and sapien rigs side by side in one launch; the buffers hold 300 rows more than the batch and sit inside red zones, at
    the allocator's alignment and 4 / 8 bytes off it (the 16-byte body of the tile copies then starts elsewhere)."""
    from articulated_pose_amd.dataset import build_point_gt_rows
    cases = [golden_case(n) for n in names]
    n_total = sum(c[1].shape[0] for c in cases)
    with guarded(misalign=misalign):
        rows, off = build_point_gt_rows([c[1] for c in cases], [c[2] for c in cases], dev, capacity=n_total + 300)
        torch.cuda.synchronize()
        got = rows.cpu().numpy()
    assert got.shape == (n_total + 300, 18) and off.cpu().tolist() == np.cumsum([0] + [c[1].shape[0] for c in cases]).tolist()
    check_rows(got[:n_total], np.concatenate([c[0]["rows"] for c in cases]), "batch " + "".join(names))
    assert (got[n_total:].view(np.uint8) == 0xFF).all()                  # rows beyond offsets[B]: the allocation's fill, untouched


# ---- ragged batches against the mirror ----------------------------------------------------------------------------------------------------
def random_rig(rs, K, sapien):
    """A rig of K single-link parts with random boxes: shape2motion -- a chain 0 <- 1 <- 2 ... plus every third joint hanging off part 0 --
    or sapien -- prismatic, revolute and fixed joints on the last part, a random base rotation and a rotated relabelling."""
    from articulated_pose_amd.dataset import pack_joint_rig
    corners = np.zeros((K + 1, 2, 3))
    corners[:, 0], corners[:, 1] = rs.uniform(-0.6, -0.3, (K + 1, 3)), rs.uniform(0.3, 0.6, (K + 1, 3))
    factors = 1.0 / np.linalg.norm(corners[:, 1] - corners[:, 0], axis=1)
    xyz = [list(rs.uniform(-0.15, 0.15, 3)) for _ in range(K + 1)]
    axis = [list(rs.normal(size=3)) for _ in range(K)]
    parts_map = [[j] for j in range(K)]
    if not sapien:
        joints = {"link": {"xyz": xyz[:K]}, "joint": {"axis": axis, "parent": [-1] + [0 if j % 3 == 0 else j - 1 for j in range(1, K)]}}
        return pack_joint_rig(corners, factors, joints, parts_map)[0]
    kinds = [("prismatic", "revolute", "fixed")[j % 3] for j in range(K - 1)] + ["fixed"]
    joints = {"link": {"xyz": [[x] for x in xyz]},
              "joint": {"axis": axis, "parent": [K] * (K - 1) + [0], "type": kinds, "rpy": [list(rs.uniform(-1.5, 1.5, 3)) for _ in range(K)]}}
    return pack_joint_rig(corners, factors, joints, parts_map, "sapien", target_order=[(j + K - 1) % K for j in range(K)])[0]


def ragged_problem(K):
    """Five clouds of 1, 63, 64, 65 and 700 rows, sorted by part as pack_annotated_cloud leaves them, and an empty cloud between them; in
    the largest, one row with part = K, one with part = 0.5 and one with NaN coordinates."""
    rs = np.random.RandomState(60 + K)
    sizes = [1, 63, 0, 64, 65, 700]
    clouds, rigs = [], []
    for b, n in enumerate(sizes):
        src = np.concatenate([rs.uniform(-1, 1, (n, 3)), rs.uniform(-0.3, 0.3, (n, 3)), np.sort(rs.randint(0, K, (n, 1)), axis=0)], 1).astype(np.float32)
        clouds.append(src)
        rigs.append(random_rig(rs, K, sapien=K >= 3 and b % 2 == 1))
    clouds[5][300, 6], clouds[5][301, 6], clouds[5][430, 3:6] = K, 0.5, np.nan
    return clouds, np.stack(rigs)


def launch(clouds, rigs, K, capacity=None, fill=None):
    """dataset.point_gt_build on a batch that may hold empty clouds -> the rows on the host (fill: what the buffer holds before the launch)."""
    from articulated_pose_amd.dataset import point_gt_build
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([c.shape[0] for c in clouds])
    cap = int(off[-1]) if capacity is None else capacity
    dev = "cuda:0"
    src = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    src[:off[-1]].copy_(torch.from_numpy(np.concatenate(clouds)))
    rows = torch.empty((cap, 18), dtype=torch.float32, device=dev)
    if fill is not None:
        rows.copy_(torch.from_numpy(fill))
    point_gt_build(src, torch.from_numpy(off).to(dev), torch.from_numpy(np.ascontiguousarray(rigs)).to(dev), K, rows)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


@pytest.mark.parametrize("K", [1, 4, 8])
def test_ragged_batch_equals_the_mirror(dev, K):
    clouds, rigs = ragged_problem(K)
    want = build_batch([c for c in clouds if c.shape[0]], [r for c, r in zip(clouds, rigs) if c.shape[0]], K)
    with guarded():
        got = launch(clouds, rigs, K)
    check_rows_nan(got, want, "ragged, K = %d" % K)
    base = sum(c.shape[0] for c in clouds[:5])
    for r in (300, 301):                                                 # not a part of the rig: -1 labels, NaN between, x y z kept
        row = got[base + r]
        assert row[3] == row[17] == -1 and np.isnan(row[4:17]).all() and np.array_equal(row[:3], clouds[5][r, :3])
    row = got[base + 430]                                                # NaN coordinates: its own NOCS only
    assert np.isnan(row[4:10]).all() and row[3] >= 0 and not np.isnan(got[base + 429]).any() and not np.isnan(got[base + 431]).any()
    if K == 1:
        assert (got[np.isfinite(got[:, 4]), 10:] == 0).all() and (got[:, 3] <= 0).all()      # no joints: no heat-map, label 0
    else:
        assert (got[:, 10] > 0).any() and (got[:, 10] == 0).any()
    # byte for byte the same on a second launch, and a batch's bytes do not depend on what the buffer held
    again = launch(clouds, rigs, K, fill=np.full(got.shape, 7.0, np.float32))
    assert _same(got, again)


def test_clouds_outside_the_buffer_and_other_rows_are_left_alone(dev):
    """Offsets that start behind row 0: rows in front of offsets[0] and behind offsets[B] keep their bytes; a cloud reaching past capacity
    writes nothing (the host refuses it; this is the ABI's own guard)."""
    from articulated_pose_amd.dataset import point_gt_build
    c, src, rig, _, K = golden_case("a")
    n, cap = src.shape[0], src.shape[0] + 40
    s = torch.zeros((cap, 7), dtype=torch.float32, device=dev)
    s[10:10 + n].copy_(torch.from_numpy(src))
    with guarded():
        rows = torch.empty((cap, 18), dtype=torch.float32, device=dev)
        rigs = torch.from_numpy(np.stack([rig, rig])).to(dev)
        point_gt_build(s, torch.tensor([10, 10 + n, cap + 5], dtype=torch.int32, device=dev), rigs, K, rows)
        torch.cuda.synchronize()
        got = rows.cpu().numpy()
    check_rows(got[10:10 + n], c["rows"], "offset cloud")
    assert (got[:10].view(np.uint8) == 0xFF).all() and (got[10 + n:].view(np.uint8) == 0xFF).all()


# ---- the sampler behind the build --------------------------------------------------------------------------------------------------------------
def test_sampled_record_equals_the_reference(dev):
    """Case d end to end: build the rows, sample them with the permutation numpy drew for the reference's 128-point record -- the
    relabelling (:697-699), the rotation (:371-379) and the sampling (:346-368) in the reference's own output."""
    from articulated_pose_amd.dataset import build_point_gt_rows, create_unit_data_batch
    from test_point_gt_build_cpu import within_one_ulp
    c, src, rig, _, K = golden_case("d")
    rows, _ = build_point_gt_rows([src], [rig], dev)
    N = int(c["num_points"])
    rec = create_unit_data_batch([rows.cpu().numpy()], N, [np.float32(c["factors"][0])], K, perms=[c["perm"]], device=dev)
    got = {k: v.cpu().numpy()[0] for k, v in rec.items()}
    for k in ("cls_gt", "joint_cls_gt", "mask_array", "joint_cls_mask"):
        assert np.array_equal(got[k], np.asarray(c["rec_" + k], np.float32)), k
    for k in ("nocs_gt", "nocs_gt_g", "heatmap_gt", "unitvec_gt", "orient_gt"):
        worst = within_one_ulp(got[k], c["rec_" + k])
        print("sampled %s: worst difference %.3g ulp" % (k, worst))
        assert worst <= 1.0, (k, worst)
    # P = xyz * norm_factors[0]: the sampler multiplies in float32 by the float32 factor, the reference by the float64 one -- half an ulp for
    # the factor's rounding, half for the product's, and (where the reference returned float64) half for rounding its value here
    np.testing.assert_allclose(got["P"], np.asarray(c["rec_P"], np.float64), rtol=1.5 * 2.0 ** -23, atol=0)
    assert (got["cls_gt"] == got["joint_cls_gt"]).all() and set(np.unique(got["cls_gt"])) <= {0.0, 1.0, 2.0, 3.0}


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
K_, B_, N_ = 3, 4, 512


def _pipe(pb, **kw):
    from test_point_gt_gpu import _pipe as pipe
    return pipe(pb, point_ground_truth=True, **kw)


def stream_rig():
    """Golden case b's rig: two revolute joints on part 0, whose tubes cross inside it."""
    return golden_case("b")[2]


def annotate(batches, rs):
    """(n, 4) clouds [x y z label] -> (n, 7) annotated clouds [x y z | random canonical coordinates | label as the part], one rig per cloud."""
    out = []
    for b in batches:
        clouds = [np.concatenate([c[:, :3], rs.uniform(-0.3, 0.3, (c.shape[0], 3)), c[:, 3:]], 1).astype(np.float32) for c in b[0]]
        out.append((clouds, b[1], np.tile(stream_rig(), (len(clouds), 1))))
    return out


def eager_rows(clouds7, rigs):
    """-> the eager op's 18-column rows of a batch, one host array per cloud."""
    from articulated_pose_amd.dataset import build_point_gt_rows
    rows, off = build_point_gt_rows(clouds7, rigs, "cuda:0")
    rows, off = rows.cpu().numpy(), off.cpu().numpy()
    return [np.ascontiguousarray(rows[off[b]:off[b + 1]]) for b in range(len(clouds7))]


@pytest.mark.parametrize("wide", [False, True], ids=["plain", "keyed-widest"])
def test_stream_equals_the_pipeline_fed_built_rows(dev, wide):
    """Pipeline A builds its rows in the captured step from 7-column clouds and rigs; pipeline B is the existing point_ground_truth pipeline
    fed the eager op's rows.  Same seeds: records and articulation blocks are equal byte for byte, and A's slot holds the eager rows."""
    from test_gt_errors_gpu import _random_gt
    from test_point_gt_gpu import _batches, random_frames
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    rs = np.random.RandomState(12)
    plain = _batches(pb, 6, np.random.RandomState(2))                   # a short batch at k = 0, a NaN cloud in batch 5
    batches = annotate(plain, rs)
    kw = dict(keyed=True, fit_quality=True, ground_truth=True) if wide else {}
    A, B = _pipe(pb, build_point_gt=True, **kw).prepare(), _pipe(pb, **kw).prepare()
    sl = A.slots[0]
    assert sl.src_rows.shape == (B_ * 3 * N_, 7) and sl.h_rows.shape == (B_ * 3 * N_, 7) and sl.raw_rows.shape == (B_ * 3 * N_, 18)
    assert sl.rig.shape == sl.h_rig.shape == (B_, rig_width(K_)) and B.slots[0].rig is None and B.slots[0].h_rows.shape[1] == 18
    for k, (clouds7, nf, rigs) in enumerate(batches):
        built = eager_rows(clouds7, rigs)
        more = dict(frame=random_frames(rs, len(clouds7)))
        if wide:
            more.update(gt=_random_gt(rs, len(clouds7), K_), cloud_base=7 * k)
        A.submit(clouds7, nf, rig=rigs, **more)
        B.submit(built, nf, **more)
        (ta, sa, ra, aa), (tb, sb, rb, ab) = A.retire(articulation=True), B.retire(articulation=True)
        assert (ta, sa) == (tb, sb) and ra.shape == (len(clouds7), K_, (51 if wide else 26) + 21)
        assert _same(ra, rb) and _same(aa, ab), k
        sl = A.slots[k % 2]
        n = sum(c.shape[0] for c in clouds7)
        assert _same(sl.raw_rows[:n].cpu().numpy(), np.concatenate(built)), k
        assert _same(sl.rig.cpu().numpy()[:len(clouds7)], rigs) and _same(sl.rig.cpu().numpy()[len(clouds7):], np.tile(rigs[0], (B_ - len(clouds7), 1)))
        assert np.isfinite(ra[:, :, 26 + 8:]).any()
    # refused before anything is enqueued, and the pipelines stay usable
    clouds7, nf, rigs = batches[1]
    with pytest.raises(ValueError, match=r"\(n_raw, 7\)"):
        A.submit(eager_rows(clouds7, rigs), nf, rig=rigs)
    with pytest.raises(ValueError, match="rig="):
        A.submit(clouds7, nf)
    with pytest.raises(ValueError, match="rig needs AncshPipeline"):
        B.submit(eager_rows(clouds7, rigs), nf, rig=rigs)
    assert not A._inflight and not B._inflight
    got = list(A.stream_batches([(c, f) + ((None,) if wide else ()) + (None, r, "t%d" % k) for k, (c, f, r) in enumerate(batches[:2])]))
    assert [g[0] for g in got] == ["t0", "t1"]


def test_range_guard_takes_the_f32_rows(dev):
    """One cloud forced over f16's range by its norm factor: both pipelines refit it from the slot's rows -- A's f32 graph builds them again
    -- and stream the same bytes."""
    from test_point_gt_gpu import _batches, random_frames
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 4, np.random.RandomState(9))
    for k, (clouds, nf) in enumerate(plain):
        if k % 2 == 1:
            nf[0] = 1e6
    rs = np.random.RandomState(6)
    batches = annotate(plain, rs)
    frames = [random_frames(rs, len(b[0])) for b in batches]
    kw = dict(arithmetic="f16x2", range_guard=True)
    A, B = _pipe(pb, build_point_gt=True, **kw), _pipe(pb, **kw)
    got_a = list(A.stream_batches([(c, nf, f, r) for (c, nf, r), f in zip(batches, frames)], flags=True))
    got_b = list(B.stream_batches([(eager_rows(c, r), nf, f) for (c, nf, r), f in zip(batches, frames)], flags=True))
    assert A.f32_reruns == B.f32_reruns == 2
    for k, ((_, _, ra, wa), (_, _, rb, wb)) in enumerate(zip(got_a, got_b)):
        assert _same(ra, rb) and _same(wa, wb) and (wa[0] != 0) == (k % 2 == 1), k


def test_launch_budget(dev):
    """The option adds ancsh_point_gt_build -- one ABI call -- in front of the sampler; the rest of the step is pipeline B's."""
    from test_fit_quality_gpu import _launch_names
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    for kw in (dict(joint_states=True, fit_quality=True, ground_truth=True, dense=True), dict()):
        off = _launch_names(_pipe(pb, slots=1, **kw).prepare())
        on = _launch_names(_pipe(pb, slots=1, build_point_gt=True, **kw).prepare())
        assert on == ["ancsh_point_gt_build"] + off and on[1].startswith("ancsh_input_sample_stream")


# ---- two gloo ranks --------------------------------------------------------------------------------------------------------------------------
def sharded_build_problem():
    """tests/test_joint_states_gpu.py's global batches as annotated clouds, with frames and rigs in front of the tag; batch 2 travels without
    frames."""
    from test_joint_states_gpu import sharded_problem
    from test_point_gt_gpu import random_frames
    pb, batches, K, G, N, kw = sharded_problem()
    rs = np.random.RandomState(43)
    ann = annotate(batches, rs)
    return pb, [(c, nf, None if k == 2 else random_frames(rs, len(c)), rigs, batches[k][2]) for k, (c, nf, rigs) in enumerate(ann)], K, G, N, kw


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
from test_point_gt_build_gpu import sharded_build_problem
pb, batches, K, G, N, kw = sharded_build_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, articulation=True, point_ground_truth=True,
                       build_point_gt=True, **kw)
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
    """Two self-launched gloo ranks on one GPU (as tests/test_point_gt_gpu.py runs them): every rank gets its shard's annotated clouds, frames
    and rigs, and rank 0's gathered (n_valid, K, 47) rows equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    pb, batches, K, G, N, kw = sharded_build_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, articulation=True, point_ground_truth=True,
                         build_point_gt=True, **kw)
    one = list(pipe.stream_batches(batches))
    del pipe
    script = tmp_path / "sharded_point_gt_build.py"
    script.write_text(_SHARDED)
    out = tmp_path / "pgb2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r in one]
    assert two["records"].shape[1:] == (K, 47) and _same(two["records"], np.concatenate([r for _, _, r in one]))
    recs = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(recs[2][:, :, 26:34]).all() and np.isfinite(recs[1][:, 1:, 28:34]).any() and np.isfinite(recs[2][:, :, 34:38]).all()
