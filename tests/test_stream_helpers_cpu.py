"""CPU tests of stream.py's host-side helpers (no GPU): the slot header's layout, the names and order of retire()'s tuple, the
"not built with it" guard, the submit / retire loop, the options check, the table of side inputs and the stream_batches item splitter."""
import collections
import itertools

import numpy as np
import pytest


def test_header_layout_is_the_kernels_layout():
    from articulated_pose_amd.depth import CAM_WORDS, GEOM_WORDS
    from articulated_pose_amd.stream import header_layout
    for B in (1, 4, 32):
        for keyed in (False, True):
            lead = 4 if keyed else 2
            lay = header_layout(B, keyed)
            assert lay.key == slice(0, lead) and lay.seed == slice(0, 2) and lay.base == (slice(2, 3) if keyed else None)
            assert lay.off == slice(lead, lead + B + 1) and lay.nf == slice(lead + B + 1, lead + 2 * B + 1)
            assert lay.geom is None and lay.cam is None and lay.dest is None and lay.words == lead + 2 * B + 1
            d = header_layout(B, keyed, depth=True)
            g0 = lead + 2 * B + 1
            assert (d.key, d.off, d.nf) == (lay.key, lay.off, lay.nf)
            assert d.geom == slice(g0, g0 + GEOM_WORDS * B) and d.cam == slice(d.geom.stop, d.geom.stop + CAM_WORDS * B)
            assert d.dest is None and d.words == d.cam.stop
            i = header_layout(B, keyed, depth=True, label_images=True)
            assert i[:-2] == d[:-2] and i.dest == slice(d.words, d.words + B) and i.words == d.words + B


def test_results_pack_in_the_documented_order_and_unpack_by_name():
    from articulated_pose_amd.stream import RESULT_ORDER, pack_results, unpack_results
    assert RESULT_ORDER == ("tag", "seed", "record", "flags", "articulation", "dense", "label_images", "counts", "link_counts")
    named = {k: k.upper() for k in RESULT_ORDER}
    assert pack_results(named) == ("TAG", "SEED", "RECORD")
    assert pack_results(named, flags=True) == ("TAG", "SEED", "RECORD", "FLAGS")
    assert pack_results(named, articulation=True, dense=True) == ("TAG", "SEED", "RECORD", "ARTICULATION", "DENSE")
    assert pack_results(named, flags=False, label_images=True, counts=True) == ("TAG", "SEED", "RECORD", "LABEL_IMAGES", "COUNTS")
    for asked in (dict(), dict(flags=True), dict(dense=True, flags=True), dict(articulation=True, label_images=True, counts=True)):
        got = unpack_results(pack_results(named, **asked), **asked)
        assert got == {k: named[k] for k in RESULT_ORDER[:3] + tuple(k for k in RESULT_ORDER[3:] if asked.get(k))}


def test_guard_names_the_method_the_class_and_the_option():
    from articulated_pose_amd.stream import check_built_with, only_asked
    owner = collections.namedtuple("Owner", "articulation dense label_images")(False, True, False)
    check_built_with(owner, "retire", "AncshPipeline", articulation=False, dense=True, label_images=False)
    with pytest.raises(RuntimeError) as e:
        check_built_with(owner, "retire", "AncshPipeline", articulation=True, dense=True, label_images=True)      # the first one wins
    assert str(e.value) == "retire(articulation=True) needs AncshPipeline(..., articulation=True)"
    with pytest.raises(RuntimeError) as e:
        check_built_with(owner, "stream_depth_batches", "AncshPipeline", label_images=True)
    assert str(e.value) == "stream_depth_batches(label_images=True) needs AncshPipeline(..., depth_capacity=<pixels>, label_images=True)"
    assert only_asked(articulation=False, dense=True) == {"dense": True} and only_asked(dense=False) == {}


def test_pump_keeps_the_window_full_and_drains_in_order():
    from articulated_pose_amd.stream import pump
    inflight, log = collections.deque(), []

    def submit(k, item):
        assert len(inflight) < 2
        inflight.append(item)
        log.append(("submit", k, item))

    def retire():
        log.append(("retire", inflight[0]))
        return inflight.popleft()
    assert list(pump("abcd", inflight, 2, submit, retire)) == list("abcd") and not inflight
    assert [e[0] for e in log] == ["submit", "submit", "retire", "submit", "retire", "submit", "retire", "retire"]
    assert [e[1] for e in log if e[0] == "submit"] == [0, 1, 2, 3]
    assert list(pump([], inflight, 2, submit, retire)) == []


def test_options_give_the_record_width_and_key_and_every_refusal():
    from articulated_pose_amd.pose.point_gt import CARRIED_WIDTHS, POINT_GT_WIDTH
    from articulated_pose_amd.stream import ROW_KINDS, check_options
    assert CARRIED_WIDTHS == (26, 39, 38, 51) and POINT_GT_WIDTH == 21
    want = {(False, False): (26, "record"), (True, False): (39, "record_wide"), (False, True): (38, "record_gt"), (True, True): (51, "record_gt")}
    for fq, gt, pgt in itertools.product((False, True), repeat=3):
        o = check_options(raw_capacity=1000, articulation=True, fit_quality=fq, ground_truth=gt, point_ground_truth=pgt)
        width, key = want[fq, gt]
        assert width in CARRIED_WIDTHS and (o.record_width, o.record_key) == ((width + 21, "record_point_gt") if pgt else (width, key)), (fq, gt, pgt)
        assert (o.fit_quality, o.ground_truth, o.point_ground_truth) == (fq, gt, pgt) and o.art_width == 12
        assert [i.name for i in o.inputs] == ["gt"] * gt + ["frame"] * pgt and o.rows is ROW_KINDS["point_gt" if pgt else "labelled"]
    assert check_options(raw_capacity=8, articulation=True, joint_states=True).art_width == 20
    # the row kinds: the joint source, the per-point ground truth, the annotated rows; a depth pipeline's slots hold its pixel capacity of rows
    pg = dict(articulation=True, point_ground_truth=True)
    assert check_options(raw_capacity=8, joint_source="predicted").rows is ROW_KINDS["xyz"] and check_options().rows is None
    o = check_options(raw_capacity=8, build_point_gt=True, **pg)
    assert o.rows is ROW_KINDS["annotated"] and (o.rows.nchan, o.rows.staged) == (18, 7) and [i.name for i in o.inputs] == ["frame", "rig"]
    assert [(k.name, k.nchan, k.staged) for k in ROW_KINDS.values()] == [("labelled", 4, 4), ("xyz", 3, 3), ("point_gt", 18, 18), ("annotated", 18, 7)]
    depth = dict(depth_capacity=4096, joint_source="predicted")
    o = check_options(batch_size=2, **depth)
    assert (o.raw_capacity, o.depth_capacity, o.depth_dtype, o.rows, o.link_counts, o.inputs) == (4096, 4096, "uint16", ROW_KINDS["xyz"], False, ())
    o = check_options(batch_size=2, build_point_gt=True, ground_truth=True, **dict(depth, **pg))
    assert o.link_counts and [i.name for i in o.inputs] == ["scene", "gt", "frame", "rig"] and o.record_width == 26 + 12 + 21
    assert check_options(ground_truth=True, **depth).inputs[0].name == "gt" and not check_options(raw_capacity=8).keyed
    # every refusal the constructors' CPU tests match
    annotated = dict(depth, build_point_gt=True, **pg)
    for kw, msg in ((dict(joint_source="nonsense"), "joint_source"), (dict(couple=False, articulation=True), "couple=True"),
                    (dict(num_points=4097, articulation=True), "num_points"), (dict(joint_states=True), "joint_states=True .* needs articulation=True"),
                    (dict(inlier_th=0.0, fit_quality=True), "fit_quality=True .* inlier_th"),
                    (dict(ground_truth=True), "ground_truth=True .* raw_capacity or depth_capacity"),
                    (dict(raw_capacity=1000, point_ground_truth=True), "point_ground_truth=True .* articulation=True"),
                    (dict(depth, **pg), "point_ground_truth=True .* depth.*build_point_gt=True"), (pg, "point_ground_truth=True .* raw_capacity"),
                    (dict(raw_capacity=1000, coord_regress_loss="Soft_L1", **pg), "coord_regress_loss"),
                    (dict(raw_capacity=1000, articulation=True, build_point_gt=True), "build_point_gt=True .* needs point_ground_truth=True"),
                    (dict(depth, joint_source="gt"), "predicted"), (dict(depth, couple=False), "couple=True"), (dict(depth, dense=True), "dense.*label_images=True"),
                    (dict(depth, raw_capacity=100), "raw_capacity"), (dict(depth, depth_dtype="float64"), "depth_dtype"),
                    (dict(depth, batch_size=2, depth_capacity=1), "depth_capacity"), (dict(depth, depth_capacity=1 << 30), "depth_capacity"),
                    (dict(label_images=True), "label_images=True .* depth_capacity"), (dict(raw_capacity=4096, label_images=True), "label_images=True .* depth_capacity"),
                    (dict(annotated, label_images=True), "label_images"), (dict(annotated, articulation=False), "articulation=True"),
                    (dict(keyed=True), "raw_capacity"), (dict(dense=True), "raw_capacity"), (dict(raw_capacity=0), "raw_capacity"),
                    (dict(range_guard=True, arithmetic="f32"), "range_guard"), (dict(range_guard=True, arithmetic=None), "range_guard")):
        with pytest.raises(ValueError, match=msg):
            check_options(**kw)


def test_side_input_table_shapes_fills_padding_and_refusals():
    from articulated_pose_amd.dataset import RIG_WIDTH, identity_rig
    from articulated_pose_amd.depth import SCENE_HEAD, SCENE_WIDTH
    from articulated_pose_amd.stream import (SIDE_INPUTS, check_side_inputs, refuse_side_inputs, require_side_inputs, side_host, stage_side_input,
                                             unit_scene)
    K, B, n = 3, 2, 1
    assert [i.name for i in SIDE_INPUTS] == ["scene", "gt", "frame", "rig"]
    unit = (0.125, 0.0, -0.5, 0.0, 0.25, -0.5, 1.0 / 65535.0)
    shapes = dict(gt=(K, 19), frame=(13,), rig=(RIG_WIDTH(K),), scene=(SCENE_WIDTH,))
    scene = np.zeros(SCENE_WIDTH)                                       # the slot's first scene: one link, the identity map, that camera
    scene[0:6], scene[6], scene[7:13], scene[13], scene[14] = unit[:6], unit[6], unit[:6], 10, 1
    scene[SCENE_HEAD + 2:SCENE_HEAD + 14] = np.eye(4)[:3].reshape(12)
    fills = dict(gt=np.full((K, 19), np.nan), frame=np.full(13, np.nan), rig=identity_rig(K), scene=scene)
    text = dict(gt="ground_truth=True", frame="point_ground_truth=True", rig="point_ground_truth=True, build_point_gt=True",
                scene="depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True")
    assert np.array_equal(unit_scene(K, unit), scene)
    rs = np.random.RandomState(3)
    for inp in SIDE_INPUTS:
        host = side_host(inp, B, K, unit, pin=False)
        view = host.numpy()
        assert view.shape == (B,) + shapes[inp.name] == (B,) + inp.shape(K) and view.dtype == np.float64
        assert all(np.array_equal(view[b], fills[inp.name], equal_nan=True) for b in range(B)), inp.name
        value = rs.normal(size=(n,) + shapes[inp.name])
        stage_side_input(inp, view, value, n)                            # one valid cloud, one padding cloud
        assert np.array_equal(view[:n], value) and inp.pad == ("nan" if inp.name in ("gt", "frame") else "first")
        assert np.isnan(view[n:]).all() if inp.pad == "nan" else np.array_equal(view[n], value[0]), inp.name
        if inp.pad == "nan":                                             # a batch without the input: NaN everywhere
            stage_side_input(inp, view, None, n)
            assert np.isnan(view).all()
        for cls in ("AncshPipeline", "ShardedPipeline"):
            refuse_side_inputs((inp,), {inp.name: value}, cls)
            refuse_side_inputs((), {inp.name: None}, cls)
            for refuse in (lambda: refuse_side_inputs((), {inp.name: value}, cls), lambda: check_side_inputs((), {inp.name: value}, n, K, cls)):
                with pytest.raises(ValueError) as e:
                    refuse()
                assert str(e.value) == "%s needs %s(..., %s)" % (inp.name, cls, text[inp.name])
        # a submit must carry rig and scene
        assert (inp.missing is not None) == (inp.name in ("rig", "scene"))
        if inp.missing:
            with pytest.raises(ValueError, match="annotated frames" if inp.name == "scene" else "rig=.* needs one dataset.pack_joint_rig table per cloud"):
                require_side_inputs((inp,), {})
        require_side_inputs((inp,), {inp.name: value})
    # checked in the table's order, by the entry's own checker; scenes arrive checked
    built = tuple(i for i in SIDE_INPUTS if i.name != "scene")
    good = dict(gt=np.zeros((n, K, 19)), frame=np.zeros((n, 13)), rig=np.tile(identity_rig(K), (n, 1)))
    out = check_side_inputs(built, dict(good, frame=None), n, K, "AncshPipeline")
    assert list(out) == ["gt", "frame", "rig"] and out["frame"] is None and out["gt"].shape == (n, K, 19) and out["rig"].dtype == np.float64
    for name, msg in (("gt", r"gt must be \(1, 3, 19\)"), ("frame", r"frame must be \(1, 13\)"), ("rig", r"rig must be \(1, %d\)" % RIG_WIDTH(K))):
        with pytest.raises(ValueError, match=msg):
            check_side_inputs(built, dict(good, **{name: np.zeros((n + 1,) + shapes[name])}), n, K, "AncshPipeline")
    with pytest.raises(ValueError, match="gt must be"):                  # the ground truth before the frames
        check_side_inputs(built, dict(good, gt=np.zeros(3), frame=np.zeros(3)), n, K, "AncshPipeline")


def test_item_splitter_follows_the_positional_order():
    from articulated_pose_amd.stream import SIDE, split_item
    values = dict(gt="GT", frame="FRAME", rig="RIG")
    for g, f, r in itertools.product((0, 1), repeat=3):
        built = tuple(SIDE[name] for name, on in (("gt", g), ("frame", f), ("rig", r)) if on)
        for tagged in (False, True):
            item = ("clouds", "nf") + tuple(values[i.name] for i in built) + (("tag",) if tagged else ())
            # the arithmetic the two stream_batches used to carry, restated
            more = dict(gt=item[2] if len(item) > 2 else None) if g else {}
            if f:
                more["frame"] = item[2 + g] if len(item) > 2 + g else None
            if r:
                more["rig"] = item[2 + g + f] if len(item) > 2 + g + f else None
            tag = item[2 + g + f + r] if len(item) > 2 + g + f + r else 7
            assert split_item(item, built, 7) == ("clouds", "nf", more, tag), (g, f, r, tagged)
            assert more == {i.name: values[i.name] for i in built} and tag == ("tag" if tagged else 7)
        # a shorter item: the inputs it leaves out are None and the tag is the batch's index
        assert split_item(("clouds", "nf"), built, 5) == ("clouds", "nf", {i.name: None for i in built}, 5)
