"""GPU: render-and-compare ICP.  ancsh_refine_pass against its mirror (tests/refinement_mirror.py, validated on its own in
tests/test_refinement_cpu.py): the counts and the solve flag equal, every float sum within the summation-order bound the mirror computes from
the terms themselves, and the mirror's solve and update on the entry's OWN sums equal to pose_out byte for byte -- so the whole loop is
replayed pass by pass at the entry's own poses, with no error to propagate --; the two behavioural bars of the CPU test on the GPU's output;
identical bytes on two runs and on two slots; the exact-pose and NaN rules; and AncshPipeline(refine=) through stream_posed_batches and
stream_render_batches against the eager operator depth.refine_frames and against the same pipeline built without the option."""
import numpy as np
import pytest
import torch

import refinement_mirror as RF
import reprojection_mirror as RP
from helpers import check_record_layout
from test_refinement_cpu import MAX_DIST, behavioural_bars, refine_problem, refine_table
from test_reprojection_cpu import DTYPES, object_links, object_mesh4, posed_object
from test_reprojection_gpu import B_, CAP_, _bytes, _pipe, _stream_batches, _t

pytestmark = pytest.mark.gpu
CASES = [(2, "uint16", False), (2, "float32", False), (3, "uint16", False), (3, "float32", False), (3, "uint16", True)]
IDS = ["K2-uint16", "K2-float32", "K3-uint16", "K3-float32", "K3-sapien-rotation"]


def _flat(prob, dtype):
    """The observed frames where the geometry rows say -> (depth (cap,), labels (cap,))."""
    geom, cap, frames = prob[6], prob[7], prob[8]
    od, ol = np.zeros(cap, DTYPES[dtype]), np.full(cap, 255, np.uint8)
    for (s, h, w, _, _), (d, l, _) in zip(geom, frames):
        od[s:s + h * w], ol[s:s + h * w] = d.reshape(-1), l.reshape(-1)
    return od, ol


def _check_sums(got, want, bounds, where):
    """One pass: got, want (n, K, 2, 32), bounds (n, K, 2, 30).  NaN places, n_used and n_obs equal; every float sum within its bound."""
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), where
    ok = ~np.isnan(want[..., 29])
    assert ok.any() and _bytes(got[ok][:, 28:30], want[ok][:, 28:30]), (where, got[ok][:, 28:30], want[ok][:, 28:30])
    err = np.abs(got[ok][:, :28] - want[ok][:, :28])
    assert (err <= bounds[ok][:, :28]).all(), (where, np.argwhere(err > bounds[ok][:, :28]), (err / np.maximum(bounds[ok][:, :28], 1e-300)).max())
    return float((err / np.maximum(bounds[ok][:, :28], 1e-300)).max())


def _replay(prob, rec, dtype, table, gpu_sums):
    """The loop replayed at the entry's own poses: per pass the mirror's sums at those poses against the entry's, then the mirror's thread 0 on
    the ENTRY's sums -> (best (n, K, 2, 18), poses [iters + 2], the mirror's sums per pass).  The cost and the solve flag must be the
    mirror's functions of the entry's sums, bit for bit."""
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    n, K = rec.shape[:2]
    iters = int(table[0])
    best, work, poses, mine, worst = np.full((n, K, 2, RF.BEST), np.nan), rec[:, :, :26].copy(), [rec[:, :, :26].copy()], [], 0.0
    for p in range(iters + 1):
        S, Bd = RF.evaluate(mesh, render, scene, rigs, nf, work, geom, frames, table)
        worst = max(worst, _check_sums(gpu_sums[p], S, Bd, "pass %d" % p))
        G = gpu_sums[p].copy()
        for idx in np.ndindex(n, K, 2):
            if not np.isnan(G[idx][29]):
                c = RF.cost(G[idx], table)
                assert np.array([c]).tobytes() == G[idx][30:31].tobytes() or (np.isnan(c) and np.isnan(G[idx][30])), (p, idx, c, G[idx][30])
        flags = G[..., 31].copy()
        work = RF.step(G, work, best, p, p == iters, table)
        assert _bytes(G[..., 31], flags), (p, G[..., 31], flags)
        poses.append(work.copy())
        mine.append(S)
    print("worst sum error / bound: %.3g" % worst)
    return best, poses, mine


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype,sapien", CASES, ids=IDS)
def test_one_pass_equals_the_mirror(dev, K, dtype, sapien):
    """Pass 0 on the perturbed record through the device wrappers: the tables, the renderer, ancsh_refine_pass.  n_used, n_obs and the flag
    equal the mirror's; the float sums lie within 4 n eps sum |term|; the mirror's solve and update on the GPU's own sums give pose_out byte for
    byte, and the best block is the input pose and its cost.  Twice into the same buffers: the same bytes."""
    from articulated_pose_amd.depth import mesh_to_device, render_depth
    from articulated_pose_amd.pose.refinement import refine_buffers, refine_pass
    from articulated_pose_amd.pose.reprojection import predicted_buffers, reproject_scene_build
    prob, rec, per = refine_problem(K, dtype, sapien)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    wide = np.concatenate([per, np.random.RandomState(1).normal(size=per.shape[:2] + (7,))], 2)      # a record wider than 26: ld_in = 33
    d_mesh = mesh_to_device(mesh, dev)
    od, ol = (_t(a, dev) for a in _flat(prob, dtype))
    d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, d_par = (_t(a, dev) for a in (render, scene, rigs, nf, wide, geom, table))
    pred = predicted_buffers(cap, dtype, dev)
    tables = reproject_scene_build(d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, cap)
    render_depth(d_mesh, tables[1], tables[0], dtype, out=pred[:2], scratch=pred[2])
    bufs = refine_buffers(3, K, dev)
    w0, best, sums = bufs.work[0], bufs.best, bufs.sums
    first = None
    for _ in range(2):
        for b in (w0, best, sums):
            b.fill_(-7.0)
        refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, d_rec, w0, best, sums[0])
        got = tuple(b.cpu().numpy() for b in (w0, best, sums[0]))
        assert first is None or all(_bytes(a, b) for a, b in zip(got, first))
        first = got
    pose_out, g_best, g_sums = got
    want, bounds = RF.evaluate(mesh, render, scene, rigs, nf, per, geom, frames, table)
    print("worst sum error / bound: %.3g" % _check_sums(g_sums, want, bounds, "pass 0"))
    assert (g_sums[..., 28] >= table[5]).all() and (g_sums[..., 29] >= g_sums[..., 28]).all()
    m_best = np.full((3, K, 2, RF.BEST), np.nan)
    G = g_sums.copy()
    m_out = RF.step(G, per, m_best, 0, False, table)
    assert _bytes(G[..., 31], g_sums[..., 31]) and (g_sums[..., 31] == 1).all()
    assert _bytes(pose_out, m_out), np.argwhere(pose_out.view(np.uint64) != m_out.view(np.uint64))
    assert _bytes(g_best, m_best) and _bytes(g_best[..., :13].reshape(3, K, 26), per) and (g_best[..., 15:].reshape(-1, 3) == g_sums[..., [28, 29, 31]].reshape(-1, 3) * [1, 0, 1]).all()
    assert not _bytes(pose_out, per) and _bytes(pose_out[:, :, [9, 22]], per[:, :, [9, 22]])          # the poses moved, the scales did not
    # the last pass only evaluates: the pose is copied through, the flag is 0
    w1 = torch.full_like(w0, -7.0)
    refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 1, True, d_rec, w1, best, sums[0])
    assert _bytes(w1.cpu().numpy(), per) and (sums[0][..., 31] == 0).all() and _bytes(sums[0][..., :31].cpu().numpy(), g_sums[..., :31])
    with pytest.raises(ValueError, match="pose_out"):
        refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, d_rec, d_rec, best, sums[0])
    with pytest.raises(ValueError, match="overlap"):
        refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, w0, w0, best, sums[0])


# ---- the full loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype,sapien", CASES, ids=IDS)
def test_full_loop_equals_the_mirror_and_meets_the_behavioural_bars(dev, K, dtype, sapien):
    """depth.refine_frames(debug=True) on the perturbed record.  The loop is replayed at the GPU's own poses (the first test shows that the
    mirror's thread 0 on the GPU's sums IS the GPU's pose_out): every pass's sums lie within the summation-order bound of the mirror's at those
    poses, and the 36 columns equal the replay's best block byte for byte.  Against the mirror run on its own, best_pass is equal wherever the
    mirror's costs are separated by more than the bound on the cost, and the refined poses agree to 1e-9: the sums differ by about 1e-13 of
    their size and the damped 6 x 6 solve multiplies that by at most 1 / damping = 1e3 per pass.  The CPU test's two bars hold on the GPU's
    output.  A second call gives the same bytes."""
    from articulated_pose_amd.depth import refine_frames
    from articulated_pose_amd.pose.refinement import named_columns
    prob, rec, per = refine_problem(K, dtype, sapien)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    columns, sums = refine_frames(mesh, render, scene, rigs, nf, per, frames, dtype, table, debug=True, device=dev)
    again = refine_frames(mesh, render, scene, rigs, nf, per, frames, dtype, table, device=dev)
    assert columns.shape == (3, K, 36) and sums.shape == (4, 3, K, 2, 32) and _bytes(columns, again)
    best, poses, mine = _replay(prob, per, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, K, 36)), np.argwhere(columns.view(np.uint64) != best.reshape(3, K, 36).view(np.uint64))
    behavioural_bars(columns, strict=True)
    m_cols, m_sums, m_bounds, m_poses = RF.refine(mesh, render, scene, rigs, nf, per, geom, frames, dtype, table)
    g, m = columns.reshape(3, K, 2, 18), m_cols.reshape(3, K, 2, 18)
    cost_bound = (m_bounds[..., 27] / m_sums[..., 29]).max(0) + 4 * RF.EPS * np.abs(m_sums[..., 30]).max(0)      # (3, K, 2): the sum's bound and the division
    costs = np.sort(m_sums[..., 30], 0)
    separated = (costs[1] - costs[0]) > 2 * cost_bound
    assert separated.any() and (g[..., 16] == m[..., 16])[separated].all(), (g[..., 16], m[..., 16], separated)
    same = g[..., 16] == m[..., 16]
    assert np.abs(g[..., :13] - m[..., :13])[same].max() <= 1e-9 and (g[..., 17] == m[..., 17]).all()
    c = named_columns(columns)
    print("cost_start", c["baseline_cost_start"].ravel(), "\ncost_best ", c["baseline_cost_best"].ravel(), "\nbest_pass ", c["baseline_best_pass"].ravel())


# ---- the exact-pose and NaN rules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(2, "uint16"), (3, "float32")])
def test_exact_poses_keep_their_cost_level(dev, K, dtype):
    """The exact record: cost_start equals the mirror's to the summation bound, whose level test_refinement_cpu holds to depth quantisation; the
    refinement keeps the pose (best_pass 0) or lowers the cost."""
    from articulated_pose_amd.depth import refine_frames
    prob, rec, _ = refine_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    columns, sums = refine_frames(mesh, render, scene, rigs, nf, rec, frames, dtype, table, debug=True, device=dev)
    best, _, mine = _replay(prob, rec, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, K, 36))
    behavioural_bars(columns, strict=False)
    s0 = sums[0]
    # half a quantum of 1e-3 times the largest norm factor (1.3) and ray length (under 1.05): 0.7e-3; a tenth of the pixels may be missed
    assert (s0[..., 28] >= 0.9 * s0[..., 29]).all() and (columns.reshape(3, K, 2, 18)[..., 13] <= (0.7e-3) ** 2 + MAX_DIST ** 2 * 0.1).all()


def test_nan_poses_zero_norm_factors_and_unseen_parts(dev):
    """The CPU test's edge cases on the GPU: a part with no observed pixel, a prediction that misses the crop, a NaN pose, a zero norm factor,
    min_pixels one above the first pass's n_used -- the columns equal the replay's byte for byte, so every rule the mirror was held to holds."""
    from articulated_pose_amd.depth import refine_frames
    K, dtype = 3, "uint16"
    prob, rec, per = refine_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    parts, _ = RP.link_parts(scene[0], K)
    obs = [list(fr) for fr in frames]
    obs[0][1] = np.where(np.isin(obs[0][1], np.nonzero(parts == 1)[0]), 255, obs[0][1]).astype(np.uint8)
    obs = [tuple(o) for o in obs]
    bad = per.copy()
    bad[1, 0, 13 + 10] += 10.0
    bad[1, 2, 4] = np.nan
    nf2 = nf.copy()
    nf2[2] = 0.0
    prob2 = prob[:5] + (nf2,) + prob[6:8] + (obs,)
    # (a norm factor of 0 is refused by the eager operator's host checks: the device wrappers take it)
    columns, sums = _loop_on_device(dev, prob2, bad, dtype, table)
    best, poses, _ = _replay(prob2, bad, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, K, 36))
    b = columns.reshape(3, K, 2, 18)
    assert np.isnan(b[2]).all() and np.isnan(b[1, 2, 0]).all() and np.isfinite(b[1, 2, 1]).all()
    assert np.isnan(b[0, 1, :, 13:15]).all() and (b[0, 1, :, 15:] == 0).all() and _bytes(b[0, 1, :, :13].reshape(26), bad[0, 1])
    assert (sums[:, 1, 0, 1, 28] == 0).all() and _bytes(b[1, 0, 1, :13], bad[1, 0, 13:]) and b[1, 0, 1, 13] == b[1, 0, 1, 14] and b[1, 0, 1, 17] == 0
    assert abs(b[1, 0, 1, 13] - MAX_DIST ** 2) <= 1e-18
    n0 = sums[0, 0, 0, 0, 28]
    for mp, solved in ((n0, 1.0), (n0 + 1, 0.0)):
        t2 = refine_table(iters=1, min_pixels=mp)
        c2, s2 = refine_frames(mesh, render, scene, rigs, nf, per, frames, dtype, t2, debug=True, device=dev)
        assert s2[0, 0, 0, 0, 31] == solved and c2[0, 0, 17] == solved
        assert (c2[0, 0, 16] == 0) or solved


def _loop_on_device(dev, prob, rec, dtype, table):
    """pose.refinement.refine_batch on staged device tensors (what depth.refine_frames does behind its host checks) -> (columns, sums)."""
    from articulated_pose_amd.depth import mesh_to_device
    from articulated_pose_amd.pose.refinement import refine_batch, refine_buffers
    from articulated_pose_amd.pose.reprojection import predicted_buffers
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    n, K = rec.shape[:2]
    iters = int(table[0])
    od, ol = (_t(a, dev) for a in _flat(prob, dtype))
    d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, d_par = (_t(a, dev) for a in (render, scene, rigs, nf, rec, geom, table))
    tables = (torch.zeros((2 * n, 208), dtype=torch.float64, device=dev), torch.zeros((2 * n, 5), dtype=torch.int32, device=dev))
    bufs = refine_buffers(n, K, dev, passes=iters + 1)
    wide = refine_batch(mesh_to_device(mesh, dev), d_rt, d_sc, d_rig, d_nf, d_geom, (od, ol), d_rec, dtype, tables, predicted_buffers(cap, dtype, dev),
                        d_par, iters, bufs)
    assert _bytes(wide[:, :, :rec.shape[2]].cpu().numpy(), rec)
    return wide[:, :, rec.shape[2]:].cpu().numpy(), bufs.sums.cpu().numpy()


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------
def _check_against_eager(got, off, batches, mesh, dtype, K, dev, observed, table, reproj=False, layouts=None):
    """Every retired batch: the 36 columns equal depth.refine_frames on the same tables and the streamed record's own leading columns, byte for
    byte; every earlier column and every other element of the tuple equal the pipeline built without the option.  layouts = the two
    pipelines' record_layout: the hand slices below are the layout's blocks."""
    from articulated_pose_amd.depth import refine_frames
    from articulated_pose_amd.pose.refinement import refined_record
    assert len(got) == len(off) == len(batches)
    for k, (g, o, (crops, nf, ps, rt, sc, rigs)) in enumerate(zip(got, off, batches)):
        rec, W = g[2], o[2].shape[2]
        assert rec.shape == (3, K, W + 36) and g[:2] == o[:2] and len(g) == len(o)
        assert _bytes(rec[:, :, :W], o[2]), k
        if layouts is not None:
            L, Lo = layouts
            assert L.width == rec.shape[2] and Lo.width == W == L.span("refinement").start and L.names == Lo.names + ("refinement",)
            assert _bytes(L.block(rec, "refinement"), rec[:, :, W:]) and all(_bytes(L.block(rec, n), Lo.block(o[2], n)) for n in Lo.names)
            assert _bytes(refined_record(rec, layout=L), refined_record(rec))
        assert all(_bytes(a, b) for a, b in zip(g[3:], o[3:])), k
        columns = refine_frames(mesh, rt, sc, rigs, nf, rec[:, :, :W], observed(k, crops, rt, sc, g[1]), dtype, table, device=dev)
        assert _bytes(rec[:, :, W:], columns), (k, rec[:, :, W:], columns)
        for v in range(2):                                                 # a pose that is not finite has NaN in its 18 columns
            poisoned = ~np.isfinite(rec[:, :, 13 * v:13 * v + 13]).all(2)
            assert np.isnan(rec[:, :, W + 18 * v:W + 18 * v + 18][poisoned]).all()


def test_posed_keyed_stream_equals_the_eager_operator_and_the_plain_pipeline(dev):
    """stream_posed_batches, K = 3, uint16, keyed, two slots, three padded batches, with reprojection=True as well: the step's last 5 (iters + 1) +
    1 ABI calls are the option's, behind reprojection's three; reprojection's 15 columns are unchanged; a pipeline without the option issues
    exactly the launches it issues today."""
    from articulated_pose_amd.depth import render_depth_frames
    from test_fit_quality_gpu import _launch_names
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    table = refine_table(iters=2)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k, cloud_base=4 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results = []
    for refine in (table, None):
        P = _pipe(K, dtype, render_mesh=mesh, kinematics=kin, keyed=True, fit_quality=True, reprojection=True, **(dict(refine=refine) if refine is not None else {}))
        names = _launch_names(P.prepare())
        sl = P.slots[0]
        L = check_record_layout(P, ("pose", "fit_quality", "point_gt", "reprojection") + (("refinement",) if refine is not None else ()))
        if refine is not None:
            loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_refine_pass"]
            assert names[-10:] == loop * 3 + ["ancsh_refine_rec"], names[-12:]
            assert names[-13:-10] == ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_reproject_compare_rec"]
            assert [tuple(t.shape) for t in sl.refine_bufs.work] == [(B_, K, 26)] * 2 and sl.refine_bufs.best.shape == (B_, K, 2, 18)
            assert sl.refine_bufs.sums.shape == (1, B_, K, 2, 32) and all(s.refine_bufs.best.data_ptr() != sl.refine_bufs.best.data_ptr() for s in P.slots[1:])
            assert sl.out["record"].shape == (B_, K, 26) and sl.out["record_refined"].shape == (B_, K, 39 + 21 + 15 + 36)
            assert sl.out["record_reproj"].shape == (B_, K, 39 + 21 + 15)
            assert (L.width, L.key, L.carried("refinement")) == (39 + 21 + 15 + 36, "record_refined", ("record_reproj", 39 + 21 + 15))
        else:
            assert sl.refine_bufs is None and not any("refine" in n for n in names) and "record_refined" not in sl.out
            assert names == results[0][1][:-10]
        results.append((list(P.stream_posed_batches(feed, articulation=True, link_counts=True)), names, L))
        del P
    P = _pipe(K, dtype, render_mesh=mesh, kinematics=kin, keyed=True, fit_quality=True)      # neither option: the launches of today
    plain = _launch_names(P.prepare())
    assert plain == results[1][1][:-3] and P.slots[0].reproj_pix is None
    del P
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(mesh, rt, crops, dtype, dev)
    _check_against_eager(results[0][0], results[1][0], batches, mesh, dtype, K, dev, observed, table, layouts=(results[0][2], results[1][2]))
    # reprojection's block lies in front of the refinement's: named through the layout it is the other pipeline's trailing 15 columns
    from articulated_pose_amd.pose.reprojection import named_columns
    for g, o in zip(results[0][0], results[1][0]):
        a, b = named_columns(results[0][2].block(g[2], "reprojection")), named_columns(o[2])
        assert all(_bytes(a[n], b[n]) for n in a)


def test_rendered_stream_with_a_sensor_refines_on_the_degraded_frame(dev):
    """stream_render_batches, K = 2, float32, a noisy sensor, not keyed, without reprojection (the slot makes the predicted tables and pixel
    triple for the option alone): the observed side is the degraded frame."""
    from articulated_pose_amd.depth import pack_sensor, render_depth_frames, sensor_frames
    K, dtype = 2, "float32"
    rs = np.random.RandomState(43)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    sensor = pack_sensor(sigma=(0.002, 0.001, 0.0), z0=1.0, p_hole=0.2, p_edge=0.5, edge_rel=0.05)
    table = refine_table(iters=1, max_dist=0.1)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(render=rt, scene=sc, rig=rigs, seed=900 + 5 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, layouts = [], []
    for refine in (table, None):
        P = _pipe(K, dtype, render_mesh=mesh, sensor=sensor, **(dict(refine=refine) if refine is not None else {}))
        results.append(list(P.stream_render_batches(feed, articulation=True, link_counts=True)))
        assert (P.slots[0].reproj_pix is not None) == (refine is not None)
        layouts.append(check_record_layout(P, ("pose", "point_gt") + (("refinement",) if refine is not None else ())))
        del P
    observed = lambda k, crops, rt, sc, seed: sensor_frames(render_depth_frames(mesh, rt, crops, dtype, dev), sc, sensor, dtype, seed=seed, device=dev)
    _check_against_eager(results[0], results[1], batches, mesh, dtype, K, dev, observed, table, layouts=layouts)


def test_library_stream_equals_the_eager_operator(dev):
    """A two-instance library through stream_render_batches, built under the F16x2 range guard, whose f32 graph of the step carries the option
    too: a z-buffer key names a global triangle of the library."""
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(47)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    lib = pack_mesh_library([mesh, pack_mesh([(0.9 * v, f) for v, f in object_links()])])
    table = refine_table(iters=1)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev, nbatches=2)
    for k, b in enumerate(batches):
        b[3][:, 9] = [(k + f) % 2 for f in range(3)]
    feed = [(crops, nf, dict(render=rt, scene=sc, rig=rigs, seed=70 + k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results = []
    for refine in (table, None):
        on = refine is not None
        P = _pipe(K, dtype, render_mesh=lib, arithmetic="f16x2", range_guard=True, **(dict(refine=refine) if on else {}))
        results.append(list(P.stream_render_batches(feed, articulation=True, link_counts=True)))
        sl = P.slots[0]
        assert sl.graph32 is not None and ("record_refined" in sl.out32) == on and ("record_refined" in sl.out) == on
        assert not on or sl.out32["record_refined"].shape == sl.out["record_refined"].shape == (B_, K, 26 + 21 + 36)
        assert check_record_layout(P).width == 26 + 21 + (36 if on else 0)      # the f32 graph's record too
        del P
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(lib, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, lib, dtype, K, dev, observed, table)
    # the library through the eager operator on frames that show the object: instance 1's triangles lie behind instance 0's in the arrays
    prob, rec, per = refine_problem(K, dtype)
    mesh1, kin1, render, scene, rigs, nf, geom, cap, frames = prob
    both = pack_mesh_library([pack_mesh([(0.9 * v, f) for v, f in object_links()]), mesh1])
    r1 = render.copy()
    r1[:, 9] = 1
    from articulated_pose_amd.depth import refine_frames
    single = refine_frames(mesh1, render, scene, rigs, nf, per, frames, dtype, refine_table(), device=dev)
    library = refine_frames(both, r1, scene, rigs, nf, per, frames, dtype, refine_table(), device=dev)
    assert _bytes(single, library)
