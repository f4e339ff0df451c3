"""CPU (no GPU): the ground-truth pose entry (ancsh_gt_pose_build) is declared, exported and bound without a new ABI number and checks its
arguments before any launch; build_gt_pose=True is one rule of stream.check_options -- it needs point_ground_truth, takes `frame` out of
the side inputs and changes no width --; pose.gt_errors.pack_box_extents is pack_ground_truth's extent columns and NaN elsewhere; and a
frame handed to such a pipeline is refused before anything touches a device."""
import ctypes

import numpy as np
import pytest

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_entry_is_declared_exported_and_bound_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    L = _lib.lib()
    assert "ancsh_gt_pose_build" in declared_symbols() and hasattr(L, "ancsh_gt_pose_build")
    assert len(_lib.SIGNATURES["ancsh_gt_pose_build"]) == 15
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def call(b=1, n=64, K=3, nchan=18, rows=P8, cap=100, off=P8, perm=P8, P=P8, ldp=3, extent=P8, ld_extent=19, gt=P8, frame=P8):
        return L.ancsh_gt_pose_build(b, n, K, nchan, rows, cap, off, perm, P, ldp, extent, ld_extent, gt, frame, None)
    for kw, word in ((dict(b=-1), b"b=-1"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(nchan=17), b"nchan=17"), (dict(nchan=4), b"nchan=4"),
                     (dict(n=0), b"n=0"), (dict(n=4097), b"n=4097"), (dict(ldp=2), b"ldp=2"), (dict(ld_extent=2), b"ld_extent=2"),
                     (dict(cap=-1), b"capacity=-1"), (dict(cap=1 << 30), b"capacity="), (dict(rows=None), b"null pointer"),
                     (dict(off=None), b"null pointer"), (dict(perm=None), b"null pointer"), (dict(P=None), b"null pointer"),
                     (dict(gt=None, frame=None), b"gt and frame are both NULL")):
        assert call(**kw) == -1 and word in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    # ld_extent is only read with an extent; nothing to do: nothing enqueued
    assert call(b=0, extent=None, ld_extent=0) == 0
    assert L.ancsh_gt_pose_build(0, 64, 3, 18, None, 0, None, None, None, 3, None, 0, None, None, None) == 0
    assert call(b=0, K=1) == 0 and call(b=0, K=8, n=4096) == 0


def test_the_option_is_one_rule_of_check_options():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import OPTION_FLAGS, SIDE_INPUTS, check_options
    assert "build_gt_pose" in OPTION_FLAGS and [i.name for i in SIDE_INPUTS] == ["scene", "gt", "frame", "rig"]
    with pytest.raises(ValueError, match="build_gt_pose=True .* point_ground_truth=True"):
        check_options(raw_capacity=1000, articulation=True, build_gt_pose=True)
    # the constructors check before they build a network or touch a device ("cpu" never reaches a kernel)
    with pytest.raises(ValueError, match="build_gt_pose=True .* point_ground_truth=True"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, articulation=True, ground_truth=True, build_gt_pose=True)
    with pytest.raises(ValueError, match="build_gt_pose=True .* point_ground_truth=True"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, articulation=True, build_gt_pose=True)
    names = lambda o: [i.name for i in o.inputs]
    for kw in (dict(raw_capacity=1000), dict(raw_capacity=1000, ground_truth=True), dict(raw_capacity=1000, ground_truth=True, fit_quality=True),
               dict(raw_capacity=1000, build_point_gt=True, joint_states=True, keyed=True, range_guard=True),
               dict(raw_capacity=1000, joint_source="predicted", ground_truth=True),
               dict(depth_capacity=4096, joint_source="predicted", build_point_gt=True, ground_truth=True)):
        kw = dict(kw, articulation=True, point_ground_truth=True)
        off, on = check_options(**kw), check_options(build_gt_pose=True, **kw)
        assert not off.build_gt_pose and on.build_gt_pose
        assert "frame" in names(off) and names(on) == [n for n in names(off) if n != "frame"]      # only the existing side inputs, frame gone
        assert (on.record_width, on.record_key, on.art_width, on.rows) == (off.record_width, off.record_key, off.art_width, off.rows)
        assert on._replace(build_gt_pose=False, inputs=()) == off._replace(inputs=())


def test_pack_box_extents_is_pack_ground_truths_extent_columns():
    from articulated_pose_amd.pose.gt_errors import GT_EXTENT, check_ground_truth, pack_box_extents, pack_ground_truth
    rs = np.random.RandomState(0)
    n, K = 4, 3
    rt = [[np.vstack([rs.normal(size=(3, 4)), [0, 0, 0, 1]]).astype(np.float32) for _ in range(K)] for _ in range(n)]
    sc = [[np.array([rs.uniform(0.5, 2)], np.float32) for _ in range(K)] for _ in range(n)]
    lo = rs.uniform(-1, 0, (n, K, 3))
    corners = [[[[lo[f, j]], [lo[f, j] + rs.uniform(0.1, 1, 3)]] for j in range(K)] for f in range(n)]      # bbox3d_all's [[min], [max]] tables
    extents = [rs.uniform(0.1, 1, (K, 3)) for _ in range(n)]
    for boxes in (corners, extents):
        boxes = list(boxes)
        boxes[2] = None                                                  # a frame without boxes
        want, got = pack_ground_truth(rt, sc, boxes), pack_box_extents(boxes)
        assert got.shape == (n, K, 19) and got.dtype == np.float64
        assert np.array_equal(got[..., GT_EXTENT], want[..., 13:16], equal_nan=True) and np.isnan(got[2]).all()
        assert np.isfinite(got[[0, 1, 3]][..., 13:16]).all() and np.isnan(got[..., :13]).all() and np.isnan(got[..., 16:]).all()
        assert check_ground_truth(got, n, K) is not None                 # what submit(gt=...) accepts
    with pytest.raises(ValueError, match="does not hold 3 parts"):
        pack_box_extents([extents[0], extents[1][:2]])


def test_a_frame_is_refused_before_a_device_is_touched():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    cloud = [np.zeros((7, 18), np.float32)]
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.B, pipe.K = check_options(raw_capacity=1000, articulation=True, ground_truth=True, point_ground_truth=True, build_gt_pose=True), 2, 3
    with pytest.raises(ValueError, match="frame.*build_gt_pose=True.*the device builds it"):
        pipe.submit(cloud, [1.0], frame=np.zeros((1, 13)))
    with pytest.raises(ValueError, match=r"gt must be \(1, 3, 19\)"):      # gt still travels in and is still checked
        pipe._enqueue(lambda: (1, np.ones(1, np.float32), None), None, None, 0, gt=np.zeros((2, 3, 19)))
    pipe.opts = check_options(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True,
                              build_gt_pose=True)
    with pytest.raises(ValueError, match="frame.*the device builds it"):
        pipe.submit_depth([], [], frame=np.zeros((1, 13)))
    sp = ShardedPipeline.__new__(ShardedPipeline)
    sp.opts, sp.raw_capacity = check_options(raw_capacity=1000, articulation=True, point_ground_truth=True, build_gt_pose=True), 1000
    with pytest.raises(ValueError, match="frame.*ShardedPipeline built with build_gt_pose=True.*the device builds it"):
        sp.submit(cloud, [1.0], frame=np.zeros((1, 13)))
    # a stream_batches item of such a pipeline: (clouds, norm_factors[, gt][, rig][, tag])
    from articulated_pose_amd.stream import split_item
    o = check_options(raw_capacity=1000, articulation=True, ground_truth=True, point_ground_truth=True, build_point_gt=True, build_gt_pose=True)
    assert split_item(("c", "nf", "g", "r", "t"), o.inputs, 0) == ("c", "nf", dict(gt="g", rig="r"), "t")
