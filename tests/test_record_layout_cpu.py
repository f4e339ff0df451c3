"""CPU (no GPU): pose.record, the one table of the streamed record's blocks.  For every combination of the five flags check_options accepts
the layout agrees with check_options and with the "which record do I carry" expressions the step used to write out by hand; a record with
every block is cut where the blocks lie; the table functions read their block through a layout from a record of any width; a block that
is not built is refused by the name of its option."""
import itertools

import numpy as np
import pytest

from test_render_cpu import box_mesh

FLAGS = ("fit_quality", "ground_truth", "point_ground_truth", "reprojection", "refine")
# an independent statement of the table: (fq, gt) fastest, then point_gt, then (reprojection, refine)
WIDTHS = [26, 38, 39, 51, 47, 59, 60, 72, 62, 74, 75, 87, 83, 95, 96, 108, 98, 110, 111, 123]


def accepted():
    """[(flags dict, Options)] of every combination check_options accepts, with what each needs besides: a stream for ground_truth, the
    articulation block for point_ground_truth, annotated depth frames and a mesh for reprojection and refine."""
    from articulated_pose_amd.depth import pack_mesh
    from articulated_pose_amd.pose.refinement import pack_refine
    from articulated_pose_amd.stream import check_options
    mesh, table = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])]), pack_refine()
    annotated = dict(depth_capacity=4096, joint_source="predicted", build_point_gt=True, render_mesh=mesh)
    out, refused = [], 0
    for rf, rp, pgt, fq, gt in itertools.product((False, True), repeat=5):
        flags = dict(fit_quality=fq, ground_truth=gt, point_ground_truth=pgt, reprojection=rp, refine=rf)
        kw = dict(flags, batch_size=2, articulation=True, refine=table if rf else None, **(annotated if rp or rf else dict(raw_capacity=1000)))
        try:
            out.append((flags, check_options(**kw)))
        except ValueError:
            assert (rp or rf) and not pgt                                # a mesh is held by annotated frames only
            refused += 1
    assert len(out) == 20 and refused == 12
    return out


def test_every_accepted_combination_agrees_with_check_options():
    from articulated_pose_amd.pose.record import BLOCKS, OPTIONS, RecordLayout
    assert OPTIONS == FLAGS and [b.width for b in BLOCKS] == [26, 13, 12, 21, 15, 36]
    assert [b.key for b in BLOCKS] == ["record", "record_wide", "record_gt", "record_point_gt", "record_reproj", "record_refined"]
    widths = []
    for flags, o in accepted():
        L = RecordLayout(**flags)
        assert L == o.layout == RecordLayout.of(o) and (L.width, L.key) == (o.record_width, o.record_key), flags
        spans = [L.span(name) for name in L.names]
        assert spans[0].start == 0 and spans[-1].stop == L.width and all(a.stop == b.start for a, b in zip(spans, spans[1:])), flags
        assert L.names == tuple(b.name for b in BLOCKS if b.option is None or flags[b.option])
        assert all(s.stop - s.start == b.width for s, b in zip(spans, L.blocks))
        assert len(L.columns) == L.width == len(set(L.columns)) and all(c.split(".")[0] in L.names for c in L.columns)
        assert all(L.columns[L.column(b.name, c)] == b.name + "." + c for b in L.blocks for c in b.columns)
        widths.append(L.width)
    assert widths == WIDTHS and len(set(widths)) == 20


def test_carried_reproduces_the_hand_written_choices():
    """The four expressions PoseSolver.solve and AncshPipeline._run spelled out before the table, on every accepted combination."""
    from articulated_pose_amd.pose.point_gt import CARRIED_WIDTHS
    from articulated_pose_amd.pose.record import RecordLayout, carried_widths
    seen = set()
    for flags, o in accepted():
        L, fq, gt, rp = RecordLayout(**flags), flags["fit_quality"], flags["ground_truth"], flags["reprojection"]
        width = {"record": 26, "record_wide": 39, "record_gt": 51 if fq else 38, "record_point_gt": (39 if fq else 26) + (12 if gt else 0) + 21,
                 "record_reproj": (39 if fq else 26) + (12 if gt else 0) + 21 + 15}
        if fq:
            assert L.carried("fit_quality") == ("record", 26)
        if gt:
            key = "record_wide" if fq else "record"                      # parallel_ancsh_pose.py: out["record_wide"] if fit_quality else out["record"]
            assert L.carried("gt_errors") == (key, width[key])
        if flags["point_ground_truth"]:
            key = "record_gt" if gt else "record_wide" if fq else "record"      # pipeline.py: record_gt if ground_truth else record_wide if fit_quality else record
            assert L.carried("point_gt") == (key, width[key])
            seen.add(width[key])
        if rp:
            assert L.carried("reprojection") == ("record_point_gt", width["record_point_gt"])      # pipeline.py: out["record_point_gt"]
        if flags["refine"]:
            key = "record_reproj" if rp else "record_point_gt"           # pipeline.py: "record_reproj" if self.reprojection else "record_point_gt"
            assert L.carried("refinement") == (key, width[key])
        with pytest.raises(ValueError, match="pose block"):
            L.carried("pose")
    assert CARRIED_WIDTHS == carried_widths("point_gt") == (26, 39, 38, 51) and seen == set(CARRIED_WIDTHS)
    assert carried_widths("gt_errors") == (26, 39)


def test_the_new_names_are_the_constants_columns():
    from articulated_pose_amd.pose import gt_errors as GE, point_gt as PG, quality as Q, refinement as RF, reprojection as RP
    from articulated_pose_amd.pose.record import BLOCKS, RecordLayout
    pose, fq, err, pgt, rp, rf = (b.columns for b in BLOCKS)
    # the pose record (include/ancsh_hip.h): the baseline pose in 0..12 and the nonlinear pose in 13..25, each R (9, row-major) | s | t (3)
    assert pose[0] == "baseline_R00" and pose[5] == "baseline_R12" and pose[9] == "baseline_s" and pose[10:13] == ("baseline_tx", "baseline_ty", "baseline_tz")
    assert pose[13] == "nonlinear_R00" and pose[22] == "nonlinear_s" and pose[23:26] == ("nonlinear_tx", "nonlinear_ty", "nonlinear_tz")
    assert pose[:13] == tuple("baseline_" + c for c in RF.POSE_COLUMNS[:13])      # the refinement block names a pose the same way
    # the fit-quality block: quality.COL_* are absolute columns of the wide record
    at = lambda col: fq[col - 26]
    assert at(Q.COL_POINTS) == "points" and at(Q.COL_CONSENSUS_A) == "consensus_a" and at(Q.COL_SCORE_B) == "score_b"
    assert [at(Q.COL_BASELINE + k) for k in range(5)] == ["baseline_inliers", "baseline_mean", "baseline_rms", "baseline_median", "baseline_max"]
    assert [at(Q.COL_NONLINEAR + k) for k in range(5)] == ["nonlinear_inliers", "nonlinear_mean", "nonlinear_rms", "nonlinear_median", "nonlinear_max"]
    assert Q.FIT_QUALITY_WIDTH == 39 and Q.COL_NONLINEAR + 5 == Q.FIT_QUALITY_WIDTH
    # the error block: gt_errors.ERR_* count from the block's first column
    want = {GE.ERR_RPY: "baseline_rpy_err", GE.ERR_XYZ: "baseline_xyz_err", GE.ERR_SCALE: "baseline_scale_err", GE.ERR_IOU: "baseline_iou",
            GE.ERR_REL_ROT: "baseline_rel_rot_err", GE.ERR_NL_RPY: "nonlinear_rpy_err", GE.ERR_NL_XYZ: "nonlinear_xyz_err",
            GE.ERR_NL_SCALE: "nonlinear_scale_err", GE.ERR_NL_IOU: "nonlinear_iou", GE.ERR_NL_REL_ROT: "nonlinear_rel_rot_err",
            GE.ERR_NL_REL_TRANS: "nonlinear_rel_trans_err", GE.ERR_POINTS: "points"}
    assert err == tuple(want[k] for k in range(GE.GT_ERROR_WIDTH)) and len(want) == GE.GT_ERROR_WIDTH == 12
    # the other three take their modules' own names
    assert pgt is PG.POINT_GT_COLUMNS and rp is RP.COLUMN_NAMES and rf is RF.COLUMN_NAMES
    assert pgt[PG.PGT_ANGLE_ERR] == "angle_err" and pgt[PG.PGT_NPCS_NOCS] == "npcs_nocs_loss" and rp[RP.COL_OBSERVED] == "n_obs"
    L = RecordLayout(fit_quality=True, ground_truth=True)
    assert L.column("gt_errors", "nonlinear_iou") == 39 + GE.ERR_NL_IOU and L.column("fit_quality", "points") == Q.COL_POINTS
    assert L.column("pose", "nonlinear_s") == 22 and L.columns[39 + GE.ERR_NL_IOU] == "gt_errors.nonlinear_iou"
    with pytest.raises(ValueError, match="no column 'n_obs'"):
        L.column("gt_errors", "n_obs")


def test_a_record_with_every_block_is_cut_where_the_blocks_lie():
    import torch
    from articulated_pose_amd.pose import refinement, reprojection
    from articulated_pose_amd.pose.record import RecordLayout
    L = RecordLayout(*(True,) * 5)
    assert L.width == 123 and L.key == "record_refined"
    rec = np.arange(2 * 3 * 123, dtype=np.float64).reshape(2, 3, 123)
    at = 26 + 13 + 12 + 21
    assert L.span("reprojection") == slice(at, at + 15) and L.span("refinement") == slice(at + 15, 123)
    got = reprojection.named_columns(L.block(rec, "reprojection"))
    assert np.array_equal(got["n_obs"], rec[:, :, at]) and np.array_equal(got["nonlinear_mean_signed"], rec[:, :, at + 14])
    # the documented trap: on the whole record the trailing columns are the refinement's
    assert not np.array_equal(reprojection.named_columns(rec)["n_obs"], rec[:, :, at])
    assert np.array_equal(reprojection.named_columns(rec)["n_obs"], rec[:, :, 123 - 15])
    assert np.array_equal(refinement.named_columns(L.block(rec, "refinement"))["baseline_R00"], rec[:, :, at + 15])
    # every block, numpy and torch, is a view of the record's own columns
    t = torch.from_numpy(rec)
    for name in L.names:
        s = L.span(name)
        assert np.array_equal(L.block(rec, name), rec[:, :, s]) and np.shares_memory(L.block(rec, name), rec)
        assert torch.equal(L.block(t, name), t[:, :, s.start:s.stop]) and L.block(t, name).data_ptr() == t[:, :, s.start:].data_ptr()
    assert np.array_equal(np.concatenate([L.block(rec, name) for name in L.names], -1), rec)
    # refined_record: the block where the layout says -- here the record's last, so the call without a layout agrees -- and behind more
    want = np.concatenate([rec[:, :, at + 15:at + 28], rec[:, :, at + 33:at + 46]], -1)
    assert np.array_equal(refinement.refined_record(rec, layout=L), want) and np.array_equal(refinement.refined_record(rec), want)
    assert torch.equal(refinement.refined_record(t, layout=L), torch.from_numpy(want))
    with pytest.raises(ValueError, match="122 columns"):
        L.block(rec[:, :, :122], "pose")
    with pytest.raises(ValueError, match="122 columns"):
        refinement.refined_record(rec[:, :, :122], layout=L)


@pytest.mark.parametrize("fit_quality", [False, True])
def test_the_tables_read_their_block_through_the_layout(fit_quality):
    """A ground-truth and point-gt record, 59 or 72 columns: with layout= the table functions print what today's calls print on the hand-cut
    38- / 51-column and (ld + 21)-column rows.  Without a layout the width decides, and 59 is refused as it always was."""
    from articulated_pose_amd.pose import evaluation as EV
    from articulated_pose_amd.pose.point_gt import stream_point_tables
    from articulated_pose_amd.pose.record import RecordLayout
    from test_gt_errors_cpu import scripts_rows
    from test_point_gt_cpu import point_rows
    G, K, rows38, error_skip, _ = scripts_rows("eval_scripts.pkl")
    F = rows38.shape[0]
    L = RecordLayout(fit_quality=fit_quality, ground_truth=True, point_ground_truth=True)
    ld = 39 if fit_quality else 26
    assert L.width == ld + 12 + 21 == (72 if fit_quality else 59)
    rows = np.full((F, K, L.width), np.nan)
    rows[:, :, :26], rows[:, :, ld:ld + 12] = rows38[:, :, :26], rows38[:, :, 26:]
    if fit_quality:
        rows[:, :, 26:39] = np.random.RandomState(0).normal(size=(F, K, 13))
    rows[:, :, ld + 12:] = point_rows(26, F, K)[:, :, 26:]
    kw = dict(error_skip=error_skip)
    want = EV.stream_tables(np.ascontiguousarray(rows[:, :, :ld + 12]), K, G["item"], G["domain"], "ANCSH", **kw)      # today's call, hand-cut
    assert EV.stream_tables(rows, K, G["item"], G["domain"], "ANCSH", layout=L, **kw) == want
    assert want == EV.stream_tables(rows38, K, G["item"], G["domain"], "ANCSH", **kw) and len(want) == 24
    cut = np.concatenate([rows[:, :, :26], rows[:, :, ld + 12:]], -1)                                                 # (F, K, 26 + 21)
    for opt in (dict(), dict(is_mixed=False), dict(network="npcs")):
        assert stream_point_tables(rows, K, layout=L, **opt) == stream_point_tables(cut, K, **opt)
    if not fit_quality:                                                      # 59 = 38 + 21 is a record, yet no width the functions may guess from
        with pytest.raises(ValueError, match="rows must be"):
            EV.stream_tables(rows, K, G["item"], G["domain"])
    # a record of another width than the layout's, and a layout without the block
    with pytest.raises(ValueError, match="%d columns" % (L.width - 21)):
        EV.stream_tables(rows[:, :, :L.width - 21], K, G["item"], G["domain"], layout=L)
    with pytest.raises(ValueError, match="%d columns" % (L.width - 1)):
        stream_point_tables(rows[:, :, :L.width - 1], K, layout=L)
    with pytest.raises(ValueError, match="point_ground_truth=True"):
        stream_point_tables(rows[:, :, :ld + 12], K, layout=RecordLayout(fit_quality=fit_quality, ground_truth=True))


def test_a_block_that_is_not_built_names_its_option():
    from articulated_pose_amd.pose import evaluation as EV, refinement
    from articulated_pose_amd.pose.record import BLOCKS, RecordLayout
    L = RecordLayout()
    assert L.names == ("pose",) and (L.width, L.key) == (26, "record")
    rec = np.zeros((1, 2, 26))
    for b in BLOCKS[1:]:
        for ask in (lambda: L.span(b.name), lambda: L.carried(b.name), lambda: L.block(rec, b.name), lambda: L.column(b.name, b.columns[0])):
            with pytest.raises(ValueError, match=r"\b%s=" % b.option):
                ask()
    with pytest.raises(ValueError, match="ground_truth=True"):
        EV.stream_tables(rec, 2, "drawer", "unseen", layout=L)
    with pytest.raises(ValueError, match="refine=<pose.refinement.pack_refine"):
        refinement.refined_record(rec, layout=L)
    with pytest.raises(ValueError, match="no block 'quality'"):
        L.span("quality")


def test_both_pipelines_carry_the_layout():
    """AncshPipeline and ShardedPipeline take their layout from the one options check, so they agree wherever the sharded one has the option."""
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pose.record import RecordLayout
    from articulated_pose_amd.stream import check_options

    class Fake(object):
        def __init__(self, *a, **kw):
            self.kw = kw
    for fq, gt, pgt in itertools.product((False, True), repeat=3):
        flags = dict(fit_quality=fq, ground_truth=gt, point_ground_truth=pgt)
        sp = ShardedPipeline(3, None, None, 4, 8, "cpu", pipeline_factory=Fake, raw_capacity=64, articulation=True, **flags)
        o = check_options(batch_size=4, raw_capacity=64, keyed=True, articulation=True, **flags)
        assert sp.record_layout == o.layout == RecordLayout(**flags) and sp.record_width == sp.record_layout.width == o.record_width
