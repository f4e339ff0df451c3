"""GPU: the joint step of render-and-compare ICP.  ancsh_refine_joint_step against its mirror (tests/joint_step_mirror.py, validated on its own
in tests/test_refine_joints_cpu.py) on the GPU's OWN sums and predicted tables: xi, pose_out, best, state and obj byte for byte -- one call
behind a rendered pass, an eight-part chain fed with hand-made sums and mirror-made tables (the 48 x 48 solve), the special cases, and the
whole loop replayed pass by pass --; the CPU test's two behavioural bars against the plain loop on the same inputs; and AncshPipeline(refine=
pack_refine(joints=...)) through three posed streams against depth.refine_frames and against the same pipeline with joints=None."""
import numpy as np
import pytest
import torch

import joint_step_mirror as JS
import refinement_mirror as RF
import reprojection_mirror as RP
from helpers import check_record_layout
from test_refine_joints_cpu import (TREES, as_columns, chain_problem, hand_sums, joint_problem, joints_table, kept_gaps, moved_record, small_part_problem,
                                    tree_problem)
from test_refinement_gpu import _flat
from test_reprojection_cpu import object_links, object_mesh4, posed_object
from test_reprojection_gpu import B_, _bytes, _pipe, _stream_batches, _t

pytestmark = pytest.mark.gpu


def _where(a, b):
    return np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))[:8]


def _joint_call(dev, kin, scene, tables, nf, table, p, last, pose_in, sums, pose_out, state, obj):
    """One launch on host arrays (state and obj as they stand before it) -> (xi, pose_out, best, state, obj) read back; twice, the same bytes."""
    from articulated_pose_amd.pose.refinement import refine_joint_step
    n, K = pose_in.shape[:2]
    d = [_t(np.asarray(a, np.float64), dev) for a in (kin, scene, tables, table, pose_in, sums)]
    d_nf, first = _t(np.asarray(nf, np.float32), dev), None
    for _ in range(2):
        d_out, d_state, d_obj = (_t(np.asarray(a, np.float64), dev) for a in (pose_out, state, obj))
        d_best, d_xi = torch.full((n, K, 2, 18), -7.0, dtype=torch.float64, device=dev), torch.full((n, 2, 48), -7.0, dtype=torch.float64, device=dev)
        refine_joint_step(d[0], d[1], d[2], d_nf, d[3], p, last, d[4], d[5], d_out, d_best, d_state, d_obj, d_xi)
        got = tuple(t.cpu().numpy() for t in (d_xi, d_out, d_best, d_state, d_obj))
        assert first is None or all(_bytes(a, b) for a, b in zip(got, first))
        first = got
    return got


def _against_the_mirror(dev, kin, scene, tables, nf, table, p, last, pose_in, sums, pose_out, state=None, obj=None):
    """The launch and the mirror on the same arrays: all five outputs byte for byte.  -> the outputs."""
    n, K = pose_in.shape[:2]
    state = np.full((n, K, 2, 18), np.nan) if state is None else state
    obj = np.zeros((n, 2, 8)) if obj is None else obj
    got = _joint_call(dev, kin, scene, tables, nf, table, p, last, pose_in, sums, pose_out, state, obj)
    m_state, m_obj = state.copy(), obj.copy()
    want = JS.step_batch(kin, scene, tables, nf, table, p, last, pose_in, sums, pose_out, m_state, m_obj) + (m_state, m_obj)
    for name, g, w in zip(("xi", "pose_out", "best", "state", "obj"), got, want):
        assert _bytes(g, w), (name, _where(g, w), g.ravel()[:8], w.ravel()[:8])
    return got


# ---- one call -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(2, "uint16"), (2, "float32"), (3, "uint16"), (3, "float32")])
def test_one_call_behind_a_rendered_pass_equals_the_mirror(dev, K, dtype):
    """Three posed frames of at most 33 x 40 pixels, every part perturbed differently, a record wider than 26: the tables, the renderer,
    ancsh_refine_pass, then the joint step on the pass's own sums and tables; pass 1 (the last: nothing is solved) on pass 0's state."""
    from articulated_pose_amd.depth import mesh_to_device, render_depth
    from articulated_pose_amd.pose.refinement import refine_buffers, refine_pass
    from articulated_pose_amd.pose.reprojection import predicted_buffers, reproject_scene_build
    prob, rec, split = joint_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = joints_table()
    wide = np.concatenate([split, np.random.RandomState(1).normal(size=split.shape[:2] + (7,))], 2)
    d_mesh = mesh_to_device(mesh, dev)
    od, ol = (_t(a, dev) for a in _flat(prob, dtype))
    d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, d_par = (_t(a, dev) for a in (render, scene, rigs, nf, wide, geom, table))
    pred = predicted_buffers(cap, dtype, dev)
    tables = reproject_scene_build(d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, cap)
    render_depth(d_mesh, tables[1], tables[0], dtype, out=pred[:2], scratch=pred[2])
    bufs = refine_buffers(3, K, dev)
    w0, best, sums = bufs.work[0], bufs.best, bufs.sums
    refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, d_rec, w0, best, sums[0])
    h_tables, h_sums, h_out = tables[0].cpu().numpy(), sums[0].cpu().numpy(), w0.cpu().numpy()
    assert _bytes(h_tables, RP.scene_tables(render, scene, rigs, nf, wide, geom, cap)[0])
    xi, out, g_best, state, obj = _against_the_mirror(dev, kin, scene, h_tables, nf, table, 0, False, wide, h_sums, h_out)
    assert (obj[:, :, 5] == 1).all() and (obj[:, :, 6] == 1).all() and (obj[:, :, 3] == 1).all() and not _bytes(out, h_out)
    assert (np.abs(xi[:, :, :6 * K]).max(2) > 0).all() and (xi[:, :, 6 * K:] == 0).all() and _bytes(out[:, :, [9, 22]], split[:, :, [9, 22]])
    assert _bytes(g_best[..., :13].reshape(3, K, 26), split) and (g_best[..., 16] == 0).all() and (g_best[..., 17] == 1).all()
    x2, out2, best2, state2, obj2 = _against_the_mirror(dev, kin, scene, h_tables, nf, table, 1, True, wide, h_sums, h_out, state, obj)
    assert (x2 == 0).all() and _bytes(out2, h_out) and (obj2[:, :, 6] == 0).all() and _bytes(obj2[:, :, :3], obj[:, :, :3]) and _bytes(best2[..., :16], g_best[..., :16])
    from articulated_pose_amd.pose.refinement import refine_joint_step
    d = dict(kin=_t(kin, dev), state=torch.zeros_like(best), obj=torch.zeros((3, 2, 8), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="overlap"):
        refine_joint_step(d["kin"], d_sc, tables[0], d_nf, d_par, 0, False, w0, sums[0], w0, best, d["state"], d["obj"])
    with pytest.raises(ValueError, match="overlap"):
        refine_joint_step(d["kin"], d_sc, tables[0], d_nf, d_par, 0, False, d_rec, sums[0], w0, best, best, d["obj"])
    with pytest.raises(ValueError, match="params"):
        refine_joint_step(d["kin"], d_sc, tables[0], d_nf, d_par[:16].contiguous(), 0, False, d_rec, sums[0], w0, best, d["state"], d["obj"])


# ---- hand-made sums and mirror-made tables: no rendering ---------------------------------------------------------------------------------------
def test_eight_part_chain_solves_the_48_by_48_system_as_the_mirror_does(dev):
    """K = 8, seven joints alternately revolute and prismatic, sums of width 32 and 36, every pose moved off the exact record: the largest
    system, with and without the clamp, and a later pass that takes the object's best-of both ways."""
    K = 8
    kin, render, scene, rigs, nf, geom, cap, rec = chain_problem()
    rs = np.random.RandomState(4)
    moved = moved_record(rs, rec, 0.01)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, moved, geom, cap)
    for width, table in ((32, joints_table(max_angle_deg=90.0, max_dist=10.0)), (36, joints_table()), (36, joints_table(silhouette=(1.0, 0.05)))):
        S = np.stack([np.stack([hand_sums(rs, K, b_scale=1e-3, width=width) for v in range(2)], 1) for f in range(2)])
        if width == 36:
            S[..., 33] = 7.0
        xi, out, best, state, obj = _against_the_mirror(dev, kin, scene, tables, nf, table, 0, False, moved, S, moved[:, :, :26].copy())
        assert (obj[:, :, 5] == 7).all() and (obj[:, :, 6] == 1).all() and (np.abs(xi).reshape(2, 2, 8, 6).max(3) > 0).all()
        worse, better = S.copy(), S.copy()
        worse[..., 30] *= 2.0
        better[..., 30] *= 0.5
        for S2, kept in ((worse, 0.0), (better, 1.0)):
            o2 = _against_the_mirror(dev, kin, scene, tables, nf, table, 1, False, out, S2, out.copy(), state.copy(), obj.copy())
            assert (o2[4][:, :, 2] == kept).all() and (o2[2][..., 16] == kept).all() and _bytes(o2[2][..., :13].reshape(2, K, 26), out if kept else moved[:, :, :26])


def test_special_cases_equal_the_mirror(dev):
    """NaN poses, a zero norm factor, a part below min_pixels and one without a pixel, K = 1, a library instance with another tree, an instance
    and a parent out of range (the kernel's own checks: depth.check_kinematics refuses such a table on the host), a failed Cholesky (a sum
    that is not finite), all-zero sums."""
    name = "K3-both-two-link-part"
    K, maps = TREES[name]
    kin, render, scene, rigs, nf, geom, cap, rec = tree_problem(K, maps)
    rs = np.random.RandomState(6)
    moved = moved_record(rs, rec, 0.01)
    table = joints_table(max_angle_deg=90.0, max_dist=10.0)
    S = np.stack([np.stack([hand_sums(rs, K, b_scale=1e-3) for v in range(2)], 1) for f in range(3)])
    bad = moved.copy()
    bad[0, 2, 4] = np.nan                                                # frame 0: a NaN baseline pose of part 2
    bad[1, 1, 13 + 9] = np.inf                                           # frame 1: an infinite scale in part 1's nonlinear pose
    nf2 = nf.copy()
    nf2[2] = 0.0                                                         # frame 2: nothing is live
    tables, _ = RP.scene_tables(render, scene, rigs, nf2, bad, geom, cap)
    S2 = S.copy()
    S2[0, 1, 1, 28] = 5.0                                                # below min_pixels: its block counts as 0
    S2[1, 0, 0, 28:31] = [0.0, 0.0, np.nan]                              # no pixel: C = NaN, not counted in the object's cost
    S2[0, 2, 0], S2[1, 1, 1], S2[2] = np.nan, np.nan, np.nan             # what the pass leaves for a pose that is not usable
    S2[0, 2, 0, 31] = S2[1, 1, 1, 31] = S2[2, :, :, 31] = 0.0
    xi, out, best, state, obj = _against_the_mirror(dev, kin, scene, tables, nf2, table, 0, False, bad, S2, bad[:, :, :26].copy())
    assert obj[0, 0, 5] == 1 and obj[0, 1, 5] == 2 and obj[1, 1, 5] == 1 and (obj[2, :, 5] == 0).all() and np.isnan(obj[2, :, 4]).all()
    assert np.isnan(best[2]).all() and np.isnan(best[0, 2, 0]).all() and np.isnan(best[1, 1, 1]).all() and np.isfinite(best[0, :2]).all()
    assert (xi[2] == 0).all() and (np.abs(xi[0, 1, 6:12]).max() > 0) and (xi[0, 0, 12:18] == 0).all()
    tables, _ = RP.scene_tables(render, scene, rigs, nf, moved, geom, cap)
    fresh = lambda: moved[:, :, :26].copy()
    inf = S.copy()
    inf[1, 1, 0, 3] = np.inf                                             # frame 1, baseline: the Cholesky fails, the pass's poses stay
    zero = S.copy()
    zero[0, :, :, :28] = 0.0                                             # frame 0: all-zero sums: the damping's 1e-12 and the joints' rows still solve
    for sums in (inf, zero):
        o = _against_the_mirror(dev, kin, scene, tables, nf, table, 0, False, moved, sums, fresh())
        assert (o[4][:, :, 6] == (0 if sums is inf else 1))[1 if sums is inf else 0, 0].all()
    assert (_against_the_mirror(dev, kin, scene, tables, nf, table, 0, False, moved, inf, fresh())[0][1, 0] == 0).all()
    # an instance out of range, then a library whose instance 1 is another tree; a parent out of range
    t9 = tables.copy()
    t9[[1, 4], 9] = 1.0                                                  # frame 1, both poses
    o = _against_the_mirror(dev, kin, scene, t9, nf, table, 0, False, moved, S, fresh())
    assert (o[4][1, :, 5] == 0).all() and (o[4][0, :, 5] == 2).all() and (o[0][1] == 0).all()
    other = kin.copy()
    other[32 + 40 * 3 + 3] = 0.0                                         # instance 1: link 3's joint is fixed
    o = _against_the_mirror(dev, np.stack([kin, other]), scene, t9, nf, table, 0, False, moved, S, fresh())
    assert (o[4][1, :, 5] == 1).all() and (o[4][0, :, 5] == 2).all()
    for value in (3.0, 7.0, -1.0, 0.5, np.nan, 1e300):
        k2 = kin.copy()
        k2[32 + 40 * 3 + 2] = value
        assert (_against_the_mirror(dev, k2, scene, tables, nf, table, 0, False, moved, S, fresh())[4][:, :, 5] == 1).all(), value
    for value in (3.0, -1.0, 1.5, np.nan):
        k2 = kin.copy()
        k2[32 + 40 * 1 + 3] = value
        assert (_against_the_mirror(dev, k2, scene, tables, nf, table, 0, False, moved, S, fresh())[4][:, :, 5] == 1).all(), value
    # the instance a table names in value 9, one frame, K = 2, one revolute joint, a 16 x 16 crop: not an integer, negative, >= ninst -> no
    # joint is active and nothing is solved; 0 -> the joint is
    K2, maps2 = TREES["K2-revolute-two-link-part"]
    kin2, render2, scene2, rigs2, nf2, _, _, rec2 = tree_problem(K2, maps2)
    render2, scene2, rigs2, nf2, rec2 = (a[:1] for a in (render2, scene2, rigs2, nf2, rec2))
    moved2 = moved_record(rs, rec2, 0.01)
    t2, _ = RP.scene_tables(render2, scene2, rigs2, nf2, moved2, np.array([[0, 16, 16, 0, 0]], np.int32), 256)
    S2 = np.stack([np.stack([hand_sums(rs, K2, b_scale=1e-3) for v in range(2)], 1)])
    for value, active in ((0.0, 1), (0.5, 0), (-1.0, 0), (1.0, 0)):
        t2[:, 9] = value
        o = _against_the_mirror(dev, kin2, scene2, t2, nf2, table, 0, False, moved2, S2, moved2[:, :, :26].copy())
        assert (o[4][:, :, 5] == active).all() and (o[4][:, :, 6] == active).all() and ((o[0] == 0).all() != bool(active)), value
    # K = 1: no joint, no solve; the best-of still runs
    kin1, render1, scene1, rigs1, nf1, geom1, cap1, rec1 = tree_problem(1, [[0, 1, 2, 3]])
    t1, _ = RP.scene_tables(render1, scene1, rigs1, nf1, rec1, geom1, cap1)
    o = _against_the_mirror(dev, kin1, scene1, t1, nf1, table, 0, False, rec1, S[:, :1].copy(), rec1[:, :, :26].copy())
    assert (o[0] == 0).all() and (o[4][:, :, 5] == 0).all() and (o[4][:, :, 3] == 1).all() and _bytes(o[1], rec1[:, :, :26])


# ---- the whole loop -----------------------------------------------------------------------------------------------------------------------------
def _replay(prob, rec, table, gpu_sums, gpu_obj):
    """The loop replayed at the entry's own poses: per pass refinement_mirror's thread 0 on the ENTRY's sums (test_refinement_gpu shows that it
    IS the pass's pose_out), ancsh_reproject_scene_build's mirror (bit-exact, test_reprojection_gpu), then the joint step's mirror; every
    pass's obj rows byte for byte.  -> the 36 columns."""
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    n, K = rec.shape[:2]
    iters = int(table[0])
    pass_best, state, obj, work, best = np.full((n, K, 2, 18), np.nan), np.full((n, K, 2, 18), np.nan), np.zeros((n, 2, 8)), rec[:, :, :26].copy(), None
    for p in range(iters + 1):
        G = gpu_sums[p].copy()
        out = RF.step(G, work, pass_best, p, p == iters, table)
        assert _bytes(G[..., 31], gpu_sums[p][..., 31])
        tables, _ = RP.scene_tables(render, scene, rigs, nf, work, geom, cap)
        _, work, best = JS.step_batch(kin, scene, tables, nf, table, p, p == iters, work, gpu_sums[p], out, state, obj)
        assert _bytes(obj, gpu_obj[p]), (p, _where(obj, gpu_obj[p]), obj, gpu_obj[p])
    return best.reshape(n, K, 36)


@pytest.mark.parametrize("K,dtype,sil", [(2, "uint16", False), (3, "float32", False), (3, "uint16", True)], ids=["K2-uint16", "K3-float32", "K3-uint16-silhouette"])
def test_full_loop_replays_pass_by_pass_and_meets_the_behavioural_bars(dev, K, dtype, sil):
    """depth.refine_frames(debug=True, kinematics=) on the record whose parts are perturbed differently: the 36 columns and every pass's obj
    rows equal the replay's byte for byte; a second call gives the same bytes; with joints=None the bytes are the plain loop's.
    Bar (a): the kept poses' hinge gap is strictly lower with joints= than with the same table without it, on every frame and pose.
    Bar (b): with min_pixels above the wedge part's pixel count the plain loop keeps that part's pose (best_pass 0, the bytes unchanged); with
    joints= it moves and its hinge gap is strictly lower than at the start."""
    from articulated_pose_amd.depth import refine_frames
    prob, rec, split = joint_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    extra = dict(silhouette=dict(weight=1.0, dist=0.05, slack=1.0)) if sil else {}
    table = joints_table(**extra)
    args = (mesh, render, scene, rigs, nf, split, frames, dtype)
    columns, sums, obj = refine_frames(*args, table, debug=True, device=dev, kinematics=kin)
    assert columns.shape == (3, K, 36) and sums.shape == (4, 3, K, 2, 36 if sil else 32) and obj.shape == (4, 3, 2, 8)
    assert _bytes(columns, refine_frames(*args, table, device=dev, kinematics=kin))
    want = _replay(prob, split, table, sums, obj)
    assert _bytes(columns, want), _where(columns, want)
    assert (obj[:, :, :, 5] == 1).all() and (obj[-1, :, :, 1] <= obj[-1, :, :, 0]).all() and (obj[-1, :, :, 6] == 0).all()
    with pytest.raises(ValueError, match="kinematics=<depth.pack_kinematics"):
        refine_frames(*args, table, device=dev)
    plain = refine_frames(*args, table[:16] if sil else table[:8], device=dev)
    g_joint, g_plain, start = kept_gaps(prob, columns, K), kept_gaps(prob, plain, K), kept_gaps(prob, as_columns(split), K)
    print("hinge gap at the start", start.ravel(), "\nplain loop", g_plain.ravel(), "\nwith joints", g_joint.ravel())
    assert (g_joint < g_plain).all(), (g_joint, g_plain)                  # (a)
    if sil:
        return
    j, min_pixels, one = small_part_problem(prob, rec, split, K)           # (b)
    t2 = joints_table(min_pixels=min_pixels)
    args = (mesh, render, scene, rigs, nf, one, frames, dtype)
    p2 = refine_frames(*args, t2[:8], device=dev).reshape(3, K, 2, 18)
    assert (p2[:, j, :, 16] == 0).all() and _bytes(p2[:, j, :, :13], one[:, j].reshape(3, 2, 13))
    c2 = refine_frames(*args, t2, device=dev, kinematics=kin)
    g2, s2 = kept_gaps(prob, c2, K), kept_gaps(prob, as_columns(one), K)
    print("min_pixels", min_pixels, "gap at the start", s2.ravel(), "with joints", g2.ravel())
    assert (c2.reshape(3, K, 2, 18)[:, j, :, :13] != one[:, j].reshape(3, 2, 13)).any(axis=2).all() and (g2 < s2).all(), (g2, s2)


# ---- the streams --------------------------------------------------------------------------------------------------------------------------------
def _check_against_eager(got, off, batches, mesh, kin, dtype, K, dev, observed, table):
    """Every retired batch: the 36 columns equal depth.refine_frames(kinematics=) on the same tables and the streamed record's own leading
    columns, byte for byte; everything outside the refinement block equals the same pipeline with joints=None."""
    from articulated_pose_amd.depth import refine_frames
    assert len(got) == len(off) == len(batches)
    for k, (g, o, (crops, nf, ps, rt, sc, rigs)) in enumerate(zip(got, off, batches)):
        rec, W = g[2], g[2].shape[2] - 36
        assert rec.shape == o[2].shape == (3, K, W + 36) and g[:2] == o[:2] and len(g) == len(o)
        assert _bytes(rec[:, :, :W], o[2][:, :, :W]) and all(_bytes(a, b) for a, b in zip(g[3:], o[3:])), k
        columns = refine_frames(mesh, rt, sc, rigs, nf, rec[:, :, :W], observed(k, crops, rt, sc, g[1]), dtype, table, device=dev, kinematics=kin)
        assert _bytes(rec[:, :, W:], columns), (k, _where(rec[:, :, W:], columns))


def _both(K, dtype, table, plain, feed, **kw):
    """The pipeline with the joint step and the same one with joints=None -> ([results], [launch names], the first one's slot-0 buffers' shapes)."""
    from test_fit_quality_gpu import _launch_names
    results, names, shapes = [], [], None
    for refine in (table, plain):
        P = _pipe(K, dtype, refine=refine, **kw)
        names.append(_launch_names(P.prepare()))
        sl = P.slots[0]
        assert (sl.refine_bufs.state is not None) == (refine is table) and P.opts.refine_joints == (refine is table)
        if refine is table:
            shapes = [tuple(t.shape) for t in (sl.refine_bufs.state, sl.refine_bufs.obj)]
            assert sl.refine_bufs.xi is None and all(s.refine_bufs.state.data_ptr() != sl.refine_bufs.state.data_ptr() for s in P.slots[1:])
            assert sl.out["refine_object"].shape == (B_, 2, 8) and (sl.graph32 is None or sl.out32["refine_object"].data_ptr() == sl.out["refine_object"].data_ptr())
        else:
            assert "refine_object" not in sl.out
        check_record_layout(P)
        results.append(list(P.stream_posed_batches(feed, articulation=True, link_counts=True)))
        del P
    return results, names, shapes


def test_posed_keyed_stream_equals_the_eager_operator_and_the_plain_pipeline(dev):
    """stream_posed_batches, K = 3, uint16, keyed, two slots, three padded batches: 6 (iters + 1) + 1 launches with the option, today's 5 (iters
    + 1) + 1 without it, and nothing else in the list differs."""
    from articulated_pose_amd.depth import render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    table, plain = joints_table(iters=2), joints_table(iters=2)[:8]
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k, cloud_base=4 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names, shapes = _both(K, dtype, table, plain, feed, render_mesh=mesh, kinematics=kin, keyed=True, fit_quality=True)
    loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_refine_pass"]
    assert names[0][-13:] == (loop + ["ancsh_refine_joint_step"]) * 3 + ["ancsh_refine_rec"] and names[1][-10:] == loop * 3 + ["ancsh_refine_rec"]
    assert names[0][:-13] == names[1][:-10] and [n for n in names[0] if n != "ancsh_refine_joint_step"] == names[1]
    assert shapes == [(B_, K, 2, 18), (1, B_, 2, 8)]
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(mesh, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, mesh, kin, dtype, K, dev, observed, table)


def test_posed_stream_with_a_sensor_and_the_silhouette_term(dev):
    """K = 2, float32, a noisy sensor with holes and edge dropout, not keyed, the silhouette term and the joint step in one table: 6 (iters + 1)
    + 2 launches, the sums rows are 36 wide."""
    from articulated_pose_amd.depth import pack_sensor, render_depth_frames, sensor_frames
    K, dtype = 2, "float32"
    rs = np.random.RandomState(43)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    sensor = pack_sensor(sigma=(0.002, 0.001, 0.0), z0=1.0, p_hole=0.2, p_edge=0.5, edge_rel=0.05)
    table = joints_table(iters=1, max_dist=0.1, silhouette=dict(weight=0.5, dist=0.05, slack=1.0))
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=900 + 5 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names, shapes = _both(K, dtype, table, table[:16], feed, render_mesh=mesh, kinematics=kin, sensor=sensor)
    loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_refine_pass_sil"]
    assert names[0][-10:] == ["ancsh_silhouette_field"] + (loop + ["ancsh_refine_joint_step"]) * 2 + ["ancsh_refine_rec"]
    assert [n for n in names[0] if n != "ancsh_refine_joint_step"] == names[1]
    observed = lambda k, crops, rt, sc, seed: sensor_frames(render_depth_frames(mesh, rt, crops, dtype, dev), sc, sensor, dtype, seed=seed, device=dev)
    _check_against_eager(results[0], results[1], batches, mesh, kin, dtype, K, dev, observed, table)


def test_library_stream_under_the_range_guard(dev):
    """A two-instance library (two meshes, two kinematic tables with different joint origins) through stream_posed_batches, built under the
    F16x2 range guard, whose f32 graph of the step shares the slot's two joint buffers."""
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, pose_scene_tables, render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(47)
    kin0, _ = posed_object(rs, K, dtype)
    kin1, _ = posed_object(np.random.RandomState(48), K, dtype)
    kin1[:32] = kin0[:32]                                                # one camera
    kins = np.stack([kin0, kin1])
    mesh = object_mesh4()
    lib = pack_mesh_library([mesh, pack_mesh([(0.9 * v, f) for v, f in object_links()])])
    table = joints_table(iters=1)
    batches = []
    for k, (crops, nf, ps, rt, sc, rigs) in enumerate(_stream_batches(rs, K, dtype, kin0, mesh, dev, nbatches=2)):
        ps[:, 28] = [(k + f) % 2 for f in range(3)]
        rt, sc = pose_scene_tables(kins, ps, dev)
        batches.append((crops, nf, ps, rt, sc, rigs))
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=70 + k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names, shapes = _both(K, dtype, table, table[:8], feed, render_mesh=lib, kinematics=kins, arithmetic="f16x2", range_guard=True)
    assert [n for n in names[0] if n != "ancsh_refine_joint_step"] == names[1] and names[0].count("ancsh_refine_joint_step") == 2
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(lib, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, lib, kins, dtype, K, dev, observed, table)
