"""CPU (no GPU): the per-point ground-truth entry (ancsh_point_gt_rec) is declared, exported and bound without a new ABI number and checks
its arguments before any launch; the pipelines refuse the option where it cannot work, and clouds or frames of the wrong shape, before
anything touches a device; pose.point_gt.stream_point_tables prints the closing lines of the reference's eval_joint_params.py and the
test_loss.txt line of the oracle."""
import ctypes

import numpy as np
import pytest

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_entry_is_declared_exported_and_bound_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    L = _lib.lib()
    assert "ancsh_point_gt_rec" in declared_symbols() and hasattr(L, "ancsh_point_gt_rec")
    assert len(_lib.SIGNATURES["ancsh_point_gt_rec"]) == 28
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def call(b=1, n=64, K=3, nchan=18, cap=100, G=9, JC=3, ld_art=12, ld=26, type_l=0, rows=P8, perm=P8, frame=P8, wide=P8):
        return L.ancsh_point_gt_rec(b, n, K, nchan, rows, cap, P8, perm, G, JC, P8, P8, P8, P8, P8, P8, P8, P8, P8, P8, ld_art, frame, P8, ld,
                                    type_l, wide, None, None)
    for kw, word in ((dict(b=-1), b"b=-1"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(n=0), b"n=0"), (dict(n=4097), b"n=4097"),
                     (dict(nchan=17), b"nchan=17"), (dict(nchan=4), b"nchan=4"), (dict(ld=27), b"ld=27"), (dict(ld=47), b"ld=47"),
                     (dict(ld_art=13), b"ld_art=13"), (dict(cap=-1), b"capacity=-1"), (dict(cap=1 << 30), b"capacity="), (dict(G=6), b"gocs"),
                     (dict(JC=0), b"joint_channels=0"), (dict(type_l=2), b"type_l=2"), (dict(rows=None), b"null pointer"),
                     (dict(perm=None), b"null pointer"), (dict(frame=None), b"null pointer"), (dict(wide=None), b"null pointer")):
        assert call(**kw) == -1 and word in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for ld in (26, 39, 38, 51):                                          # every carried width, nothing to do: nothing enqueued
        assert L.ancsh_point_gt_rec(0, 64, 3, 18, None, 0, None, None, 9, 3, None, None, None, None, None, None, None, None, None, None, 20, None,
                                    None, ld, 1, None, None, None) == 0


def test_constructors_refuse_before_a_device_is_touched():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    # the constructors check before they build a network or touch a device ("cpu" never reaches a kernel)
    with pytest.raises(ValueError, match="point_ground_truth=True .* articulation=True"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, point_ground_truth=True)
    with pytest.raises(ValueError, match="point_ground_truth=True .* depth"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True)
    with pytest.raises(ValueError, match="point_ground_truth=True .* raw_capacity"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", articulation=True, point_ground_truth=True)
    with pytest.raises(ValueError, match="coord_regress_loss"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, articulation=True, point_ground_truth=True, coord_regress_loss="Soft_L1")
    with pytest.raises(ValueError, match="point_ground_truth=True .* articulation=True"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, point_ground_truth=True)


def test_clouds_and_frames_are_checked_on_the_host():
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose import point_gt as PG
    from articulated_pose_amd.stream import check_options
    assert PG.POINT_GT_WIDTH == 21 == len(PG.POINT_GT_COLUMNS) and PG.FRAME_WIDTH == 13
    assert [PG.PGT_ANGLE_ERR, PG.PGT_DIST_ERR, PG.PGT_MIOU, PG.PGT_NPCS_MIOU, PG.PGT_PART_POINTS, PG.PGT_JOINT_POINTS, PG.PGT_NOCS, PG.PGT_GOCS,
            PG.PGT_HEATMAP, PG.PGT_UNITVEC, PG.PGT_ORIENT, PG.PGT_NPCS_NOCS] == [0, 1, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20]
    good, nf = PG.check_point_clouds([np.zeros((5, 18)), np.ones((1, 18), np.float32)], [1.0, 2.0], 4)
    assert [c.dtype for c in good] == [np.float32] * 2 and all(c.flags.c_contiguous for c in good) and nf.dtype == np.float32
    # a 4-column cloud on such a pipeline: refused by the submit path before anything is enqueued, and the message names the 18 columns
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts, pipe.B, pipe.K = check_options(raw_capacity=1000, articulation=True, point_ground_truth=True), 2, 3
    with pytest.raises(ValueError, match=r"\(n_raw, 18\).*x y z \| cls \| nocs_p 3 \| nocs_g 3 \| heatmap \| unitvec 3 \| orient 3 \| joint_cls.*\(7, 4\)"):
        pipe.submit([np.zeros((7, 4), np.float32)], [1.0])
    for bad in ([np.zeros((0, 18))], [np.zeros((3, 17))], "nonsense", []):
        with pytest.raises(ValueError):
            PG.check_point_clouds(bad, [1.0] * (len(bad) if isinstance(bad, list) else 1), 4)
    with pytest.raises(ValueError, match="norm_factors"):
        PG.check_point_clouds([np.zeros((3, 18))], [np.inf], 4)
    # frames
    fr = np.zeros((2, 13))
    fr[1] = np.nan                                                       # a cloud without a ground-truth NAOCS pose is fine
    out = PG.check_frames(fr, 2)
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (2, 13)
    for bad, word in ((np.zeros((2, 12)), r"frame must be \(2, 13\)"), (np.zeros((3, 13)), r"frame must be \(2, 13\)"), ("nonsense", "frame must be"),
                      (np.where(np.arange(13) == 9, np.inf, 0.0) * np.ones((2, 1)), r"frame\[0\]\[9\] is infinite")):
        with pytest.raises(ValueError, match=word):
            PG.check_frames(bad, 2)
    # frame on a pipeline built without the option: refused right after the front end's own checks
    built, pipe.opts = pipe.opts, check_options(raw_capacity=1000)
    front = lambda: (1, np.ones(1, np.float32), None)
    with pytest.raises(ValueError, match="frame needs AncshPipeline"):
        pipe._enqueue(front, None, None, 0, frame=np.zeros((1, 13)))
    pipe.opts = built
    with pytest.raises(ValueError, match=r"frame must be \(1, 13\)"):
        pipe._enqueue(front, None, None, 0, frame=np.zeros((2, 13)))


def test_pack_joint_frame_reads_the_pickle_shapes():
    from articulated_pose_amd.pose.point_gt import pack_joint_frame
    rs = np.random.RandomState(0)
    K = 3
    rt = [[np.vstack([rs.normal(size=(3, 4)), [0, 0, 0, 1]]).astype(np.float32) for _ in range(K)] for _ in range(3)]
    sc = [[np.array([rs.uniform(0.5, 2)], np.float32) for _ in range(K)] for _ in range(3)]
    rt[1] = None
    fr = pack_joint_frame(rt, sc)
    assert fr.shape == (3, 13) and fr.dtype == np.float64 and np.isnan(fr[1]).all()
    for f in (0, 2):
        assert np.array_equal(fr[f, :9].reshape(3, 3), rt[f][0][:3, :3]) and fr[f, 9] == sc[f][0][0] and np.array_equal(fr[f, 10:], rt[f][0][:3, 3])
    with pytest.raises(ValueError, match="one entry per frame"):
        pack_joint_frame(rt, sc[:2])


def point_rows(ld, F=5, K=3):
    """Hand-made (F, K, ld + 21) streamed rows: the point-gt block behind a carried row of ld columns."""
    rs = np.random.RandomState(ld)
    rows = rs.normal(size=(F, K, ld + 21))
    rows[:, 0, ld:ld + 8] = np.nan
    rows[2, 1, ld] = np.nan                                              # a NaN angle error: counts as 0
    rows[4, 2, ld + 1] = np.nan
    rows[:, :, ld + 12:] = rows[:, :1, ld + 12:]                         # the cloud's losses: the same on every row
    return rows


@pytest.mark.parametrize("ld", [26, 51])
def test_stream_point_tables_print_the_closing_lines(ld, capsys):
    """Hand-made rows: the joint lines are the reference's closing lines (eval_joint_params.py:262-269, restated here as it prints them: a
    NaN error counts as 0), the loss line is the oracle's collect_losses under the product's formatter of lib/network.py:228-243."""
    from articulated_pose_amd.loss import format_loss_result
    from articulated_pose_amd.pose.point_gt import stream_point_tables
    from oracle import loss_oracle as LO
    F, K = 5, 3
    rows = point_rows(ld, F, K)
    # the reference's lines
    r_diff_arr, t_diff_arr = rows[:, 1:, ld].copy(), rows[:, 1:, ld + 1].copy()
    r_diff_arr[np.where(np.isnan(r_diff_arr))] = 0
    t_diff_arr[np.where(np.isnan(t_diff_arr))] = 0
    print(r_diff_arr.shape, t_diff_arr.shape, K)
    for k in range(K - 1):
        print('joint {} with mean angle error {} degrees, mean dist {}'.format(k, np.mean(np.abs(r_diff_arr[:, k])), np.mean(np.abs(t_diff_arr[:, k]))))
        print(np.mean(np.abs(r_diff_arr[:, k])), np.mean(np.abs(t_diff_arr[:, k])))
    want = capsys.readouterr().out.splitlines()
    lines, loss = stream_point_tables(rows, K)
    assert lines == want and len(lines) == 1 + 2 * (K - 1)
    assert lines[1] != 'joint 0 with mean angle error {} degrees, mean dist {}'.format(np.nanmean(np.abs(rows[:, 1, ld])), np.mean(np.abs(rows[:, 1, ld + 1])))
    ld_ = dict(nocs_loss=rows[:, 0, ld + 12], gocs_loss=rows[:, 0, ld + 13], heatmap_loss=rows[:, 0, ld + 14], unitvec_loss=rows[:, 0, ld + 15],
               orient_loss=rows[:, 0, ld + 16], index_loss=rows[:, 0, ld + 17:ld + 20], miou_loss=rows[:, :, ld + 8])
    assert loss == format_loss_result(LO.collect_losses(ld_, True), True) and loss.startswith("Total Loss: ") and "gocs Loss" in loss
    _, not_mixed = stream_point_tables(rows, K, is_mixed=False)
    assert not_mixed == format_loss_result(LO.collect_losses(ld_, False), False) and "gocs Loss" not in not_mixed
    _, npcs = stream_point_tables(rows, K, network="npcs")
    flags = dict(pred_joint=False, pred_joint_ind=False)
    assert npcs == format_loss_result(LO.collect_losses(dict(ld_, nocs_loss=rows[:, 0, ld + 20], miou_loss=rows[:, :, ld + 9]), False, **flags),
                                      False, **flags)
    with pytest.raises(ValueError, match="rows must be"):
        stream_point_tables(rows[:, :, :ld + 20], K)
