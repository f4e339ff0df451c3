"""GPU: the streamed side inputs (gt, frame, rig, scene) and the row kinds, held to bytes.  Five small streams -- three batches of 2, 2 and 1
clouds through two slots, so the last batch is padded, with the ground truth or the frames left out of one batch -- return, byte for byte, what
the commit before the side-input table returned (tests/golden/stream_inputs_unchanged.npz): every element of every retired tuple, the
slots' headers after the last batch and the ABI calls of one eager step."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_, B_, N_, CAP_ = 3, 2, 64, 8192
SIZES = (2, 2, 1)
STREAMS = ("a", "b", "c", "d", "e")
KW = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput")


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _raw_batches(rs):
    """[(clouds (m, 4) [x y z joint_cls], norm factors)] of SIZES clouds, 40..900 rows each."""
    out = []
    for n in SIZES:
        clouds = []
        for _ in range(n):
            m = int(rs.randint(40, 900))
            clouds.append(np.concatenate([rs.uniform(-0.5, 0.5, (m, 3)), rs.randint(0, K_, (m, 1))], 1).astype(np.float32))
        out.append((clouds, rs.uniform(0.9, 1.1, n).astype(np.float32)))
    return out


def _feed(name):
    """-> (the stream's batches as stream_batches / stream_depth_batches takes them, its pipeline keywords)."""
    from test_gt_errors_gpu import _random_gt
    from test_point_gt_gpu import random_channels
    rs = np.random.RandomState(71)
    raw = _raw_batches(rs)
    if name == "a":
        return raw, dict(raw_capacity=CAP_)
    if name == "b":                                                      # the ground truth on batches 0 and 2 only
        return ([(c, nf, None if k == 1 else _random_gt(rs, len(c), K_)) for k, (c, nf) in enumerate(raw)],
                dict(raw_capacity=CAP_, ground_truth=True, fit_quality=True))
    if name in ("c", "d"):                                               # 18-column clouds; no frame on batch 1
        wide = [[np.concatenate([c[:, :3], random_channels(rs, c.shape[0], K_, jcls=c[:, 3])], 1).astype(np.float32) for c in cl] for cl, _ in raw]
        return ([(cl, nf, _random_gt(rs, len(cl), K_), None if k == 1 else rs.normal(size=(len(cl), 13)), "t%d" % k)
                 for k, (cl, (_, nf)) in enumerate(zip(wide, raw))],
                dict(raw_capacity=CAP_, point_ground_truth=True, articulation=True, joint_states=True, ground_truth=True))
    from test_depth_annotate_gpu import _batch                           # e: annotated depth frames
    return ([(f, nf, dict(scene=t, rig=r, frame=jf)) for f, nf, t, r, jf in (_batch(rs, "uint16", n) for n in SIZES)],
            dict(depth_capacity=CAP_, depth_dtype="uint16", joint_source="predicted", articulation=True, point_ground_truth=True,
                 build_point_gt=True))


def recorded_stream(name):
    """Stream `name` (a: a plain joint_source="gt" raw stream; b: with ground_truth and fit_quality; c: point_ground_truth, articulation,
    joint_states and ground_truth on 18-column clouds; d: c keyed, through a world-1 ShardedPipeline; e: annotated depth frames with
    link_counts) from seeded generators only -> {key: array}: the retired tuples' elements, both slots' headers, the ABI calls."""
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_depth_annotate_gpu import _weights
    from test_fit_quality_gpu import _launch_names
    pb = _weights()
    feed, kw = _feed(name)
    art = bool(kw.get("articulation"))
    if name == "d":
        top = ShardedPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(KW, **kw))
        pipe, got = top.pipe, list(top.stream_batches(feed, articulation=True))
        assert pipe.keyed
    else:
        pipe = AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(KW, **kw))
        got = list(pipe.stream_depth_batches(feed, articulation=True, link_counts=True) if name == "e" else
                   pipe.stream_batches(feed, articulation=art))
    out = {}
    for k, g in enumerate(got):
        for i, v in enumerate(g):
            out["%s_batch%d_%d" % (name, k, i)] = np.asarray(v)
    for i, sl in enumerate(pipe.slots):
        out["%s_hdr%d" % (name, i)] = sl.hdr.cpu().numpy()
    out["%s_launches" % name] = np.array(_launch_names(pipe))
    return out


@pytest.mark.parametrize("name", STREAMS)
def test_stream_returns_the_parent_commits_bytes(dev, name):
    golden = np.load(os.path.join(HERE, "golden", "stream_inputs_unchanged.npz"))
    want = {k: golden[k] for k in golden.files if k.startswith(name + "_")}
    got = recorded_stream(name)
    assert sorted(got) == sorted(want) and len(want) == 3 * {"a": 3, "b": 3, "c": 4, "d": 4, "e": 6}[name] + 3
    for key in sorted(want):
        if key.endswith("_launches"):
            assert got[key].tolist() == want[key].tolist(), key
        else:
            assert _bytes(got[key], want[key]), key
    width = {"a": 26, "b": 51, "c": 59, "d": 59, "e": 47}[name]
    assert [got["%s_batch%d_2" % (name, k)].shape for k in range(3)] == [(n, K_, width) for n in SIZES]
    assert np.isfinite(got[name + "_batch2_2"][:, :, :26]).any()
    if name == "b":                                                      # no ground truth on batch 1: its error columns are NaN
        assert np.isnan(got["b_batch1_2"][:, :, 39:50]).all() and np.isfinite(got["b_batch0_2"][:, :, 39:50]).any()
    if name in ("c", "d"):
        assert got[name + "_batch0_3"].shape == (2, K_, 20) and got[name + "_batch0_0"].tolist() == "t0"
    if name == "e":
        assert got["e_batch2_4"].shape == (1,) and got["e_batch2_5"].shape == (1, 16) and got["e_batch2_5"].dtype == np.int32
