"""GPU: the coverage term of render-and-compare ICP.  ancsh_coverage_field byte for byte against the mirror's brute force
(tests/coverage_mirror.py, validated on its own in tests/test_coverage_cpu.py) on hand-made predicted pairs inside red zones;
ancsh_refine_pass_cov against the mirror -- counts equal, float sums within the summation-order bound, and the mirror's thread 0 on the
entry's OWN sums equal to pose_out and best byte for byte, so the loop is replayed pass by pass at the entry's own poses --; the edge cases;
ancsh_refine_joint_step on 40-wide sums; AncshPipeline(refine=<32-value table>) through three streams against the eager operator and the
silhouette-only pipeline; and the CPU test's lateral bars on the GPU's result."""
import numpy as np
import pytest
import torch

import coverage_mirror as CM
import joint_step_mirror as JS
import refinement_mirror as RF
import reprojection_mirror as RP
import silhouette_mirror as SM
from redzone import Arena
from test_coverage_cpu import PERTURBED, PERTURBED_IDS, coverage_table
from test_refine_joints_cpu import chain_problem, hand_sums, moved_record
from test_refine_joints_gpu import _check_against_eager, _joint_call, _where
from test_refinement_cpu import MAX_DIST, behavioural_bars, refine_table
from test_refinement_gpu import _flat
from test_reprojection_cpu import DTYPES, object_links, object_mesh4, posed_object
from test_reprojection_gpu import B_, CAP_, _bytes, _pipe, _stream_batches, _t
from test_silhouette_cpu import lateral_bar, problem, refined, silhouette_table
from test_silhouette_gpu import _field_frames, _scene

pytestmark = pytest.mark.gpu


# ---- the field --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_cover_equals_the_brute_force_inside_red_zones(dev, K, dtype):
    """test_silhouette_gpu's hand-made crops (1 x 1, 1 x 7, 7 x 1, a checkerboard, a filled crop, a far-corner pixel, random blobs with holes
    and links of no part up to 33 x 65, 3 x 300 and 140 x 2) as PREDICTED pairs: pose 1's half holds other content than pose 0's (mirrored
    left to right, the blobs drawn anew), the starts are unaligned, two padding frames have no crop, and odd frames' scene rows map the links
    to the parts in reverse, so a frame row that read another scene row would show.  The output is carved out of red zones and pre-filled:
    every word of a crop equals the mirror's, every other word keeps its fill, no guard byte changes; twice, the same bytes."""
    from articulated_pose_amd.pose.refinement import coverage_field
    npdt = DTYPES[dtype]
    halves = [_field_frames(np.random.RandomState(17), K, npdt), [(np.fliplr(d).copy(), np.fliplr(l).copy()) for d, l in _field_frames(np.random.RandomState(23), K, npdt)]]
    n = len(halves[0]) + 2
    geom, a = [], 3
    for d, l in halves[0]:
        geom.append((a, d.shape[0], d.shape[1], 5, -7))
        a += d.size + 5
    cap = a + 2
    geom = np.asarray(geom + [(0, 0, 0, 0, 0)] * 2, np.int32)
    geom_out = np.concatenate([geom, geom])
    geom_out[n:n + len(halves[1]), 0] += cap                             # pose 1's crops lie cap pixels further on; a padding row stays 0
    scene = np.stack([_scene(K, 1e-3) for _ in range(n)])
    for f in range(1, n, 2):
        for l in range(K):
            scene[f, 16 + 14 * l + 1] = K - 1 - l
    pd, pl = np.zeros(2 * cap, npdt), np.full(2 * cap, 255, np.uint8)
    frames = []
    for v in range(2):
        for f in range(n):
            if f >= len(halves[v]):
                frames.append(None)
                continue
            d, l = halves[v][f]
            s = int(geom_out[v * n + f][0])
            pd[s:s + d.size], pl[s:s + d.size] = d.reshape(-1), l.reshape(-1)
            frames.append((d, l))
    want = CM.cover_flat(frames, scene, geom_out, K, cap, fill=-1)
    assert (want != -1).any() and not _bytes(want[:, :cap], want[:, cap:]) and (want[:, :3] == -1).all() and (want[:, cap:cap + 3] == -1).all()
    arena = Arena()
    out = arena.empty((K, 2 * cap), dtype=torch.int32, device=dev)      # the body is 0xff bytes: -1
    pred = (_t(pd, dev), _t(pl, dev), None)
    args = (pred, _t(geom_out, dev), _t(scene, dev), K)
    got = coverage_field(*args, out=out).cpu().numpy()
    assert _bytes(got, want), np.argwhere(got != want)[:10]
    assert _bytes(coverage_field(*args, out=out).cpu().numpy(), want)
    assert arena.check() == 1
    assert _bytes(coverage_field(*args).cpu().numpy(), CM.cover_flat(frames, scene, geom_out, K, cap, fill=0))      # its own buffer: zeros outside
    if K == 8:                                                           # reversed parts: part 0 of an odd frame is link 7's pixels
        s, h, w = (int(v) for v in geom_out[7][:3])
        fwd = CM.cover_flat(frames, np.stack([_scene(K, 1e-3)] * n), geom_out, K, cap, fill=-1)
        assert not _bytes(got[:, s:s + h * w], fwd[:, s:s + h * w]) and _bytes(got[0, s:s + h * w], fwd[7, s:s + h * w])


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------------
COUNTS, FLOATS = [28, 29, 33, 34, 35, 37, 38, 39], list(range(28)) + [32, 36]


def _check_sums(got, want, bounds, where):
    """One pass: got, want, bounds (n, K, 2, 40).  NaN places and the counts equal; every float sum within its bound."""
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), where
    ok = ~np.isnan(want[..., 29])
    assert ok.any() and _bytes(got[ok][:, COUNTS], want[ok][:, COUNTS]), (where, got[ok][:, COUNTS], want[ok][:, COUNTS])
    err, bd = np.abs(got[ok][:, FLOATS] - want[ok][:, FLOATS]), bounds[ok][:, FLOATS]
    assert (err <= bd).all(), (where, np.argwhere(err > bd), (err / np.maximum(bd, 1e-300)).max())
    return float((err / np.maximum(bd, 1e-300)).max())


def _replay(prob, rec, dtype, table, gpu_sums, frames=None):
    """test_silhouette_gpu's replay with both terms: per pass the mirror's sums at the entry's own poses against the entry's, the cost and the
    solve flag as the mirror's functions of the ENTRY's sums bit for bit -> (best (n, K, 2, 18), poses)."""
    mesh, kin, render, scene, rigs, nf, geom, cap, own = prob
    frames = own if frames is None else frames
    n, K = rec.shape[:2]
    iters = int(table[0])
    fields = SM.field(frames, scene, K)
    best, work, poses, worst = np.full((n, K, 2, RF.BEST), np.nan), rec[:, :, :26].copy(), [rec[:, :, :26].copy()], 0.0
    for p in range(iters + 1):
        S, Bd = CM.evaluate(mesh, render, scene, rigs, nf, work, geom, frames, table, fields)
        worst = max(worst, _check_sums(gpu_sums[p], S, Bd, "pass %d" % p))
        G = gpu_sums[p].copy()
        for idx in np.ndindex(n, K, 2):
            if not np.isnan(G[idx][29]):
                c = CM.cost(G[idx], table)
                assert np.array([c]).tobytes() == G[idx][30:31].tobytes() or (np.isnan(c) and np.isnan(G[idx][30])), (p, idx, c, G[idx][30])
        flags = G[..., 31].copy()
        work = CM.step(G, work, best, p, p == iters, table)
        assert _bytes(G[..., 31], flags), (p, G[..., 31], flags)
        poses.append(work.copy())
    print("worst sum error / bound: %.3g" % worst)
    return best, poses


def _loop_on_device(dev, prob, rec, dtype, table, frames=None):
    """pose.refinement.refine_batch on staged device tensors (what depth.refine_frames does behind its host checks, which refuse a zero norm
    factor) -> (columns, sums (iters + 1, ...), the launches' names)."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import mesh_to_device
    from articulated_pose_amd.pose.refinement import has_coverage, refine_batch, refine_buffers
    from articulated_pose_amd.pose.reprojection import predicted_buffers
    mesh, kin, render, scene, rigs, nf, geom, cap, own = prob
    n, K = rec.shape[:2]
    iters = int(table[0])
    od, ol = (_t(a, dev) for a in _flat(prob[:8] + (own if frames is None else frames,), dtype))
    d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, d_par = (_t(a, dev) for a in (render, scene, rigs, nf, rec, geom, table))
    tables = (torch.zeros((2 * n, 208), dtype=torch.float64, device=dev), torch.zeros((2 * n, 5), dtype=torch.int32, device=dev))
    bufs = refine_buffers(n, K, dev, passes=iters + 1, silhouette=True, pixel_capacity=cap, coverage=has_coverage(table))
    names, real = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        wide = refine_batch(mesh_to_device(mesh, dev), d_rt, d_sc, d_rig, d_nf, d_geom, (od, ol), d_rec, dtype, tables,
                            predicted_buffers(cap, dtype, dev), d_par, iters, bufs)
    finally:
        _lib.call = real
    assert _bytes(wide[:, :, :rec.shape[2]].cpu().numpy(), rec)
    return wide[:, :, rec.shape[2]:].cpu().numpy(), bufs.sums.cpu().numpy(), names


def _cut(pd, pl, pz, geom_out):
    """The predicted buffers read back -> the 2 n crops (depth, labels, keys)."""
    out = []
    for s, h, w, _, _ in geom_out:
        out.append(tuple(a[s:s + h * w].reshape(h, w) for a in (pd, pl, pz)))
    return out


@pytest.mark.parametrize("K,dtype,sapien", PERTURBED, ids=PERTURBED_IDS)
def test_one_pass_equals_the_mirror(dev, K, dtype, sapien):
    """Pass 0 on a record shifted across the ray by two pixels (gap pixels on every part) through the device wrappers: both fields, the
    tables, the renderer, ancsh_refine_pass_cov.  The cover equals the mirror's on the renderer's own output; the counts equal the mirror's;
    the float sums lie within 4 (rows + 1) eps sum |term|; the mirror's solve and update on the GPU's own sums give pose_out and best byte
    for byte.  Twice into the same buffers: the same bytes."""
    from articulated_pose_amd.depth import mesh_to_device, render_depth
    from articulated_pose_amd.pose.refinement import coverage_field, refine_buffers, refine_pass, silhouette_field
    from articulated_pose_amd.pose.reprojection import predicted_buffers, reproject_scene_build
    prob, rec, per, cen = problem(K, dtype, sapien)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = coverage_table()
    lat = SM.lateral_record(rec, cen, 0.02)
    wide = np.concatenate([lat, np.random.RandomState(1).normal(size=lat.shape[:2] + (7,))], 2)       # ld_in = 33
    d_mesh = mesh_to_device(mesh, dev)
    od, ol = (_t(a, dev) for a in _flat(prob, dtype))
    d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, d_par = (_t(a, dev) for a in (render, scene, rigs, nf, wide, geom, table))
    bufs = refine_buffers(3, K, dev, silhouette=True, pixel_capacity=cap, coverage=True)
    field = silhouette_field(od, ol, d_geom, d_sc, K, out=bufs.field)
    pred = predicted_buffers(cap, dtype, dev)
    tables = reproject_scene_build(d_rt, d_sc, d_rig, d_nf, d_rec, d_geom, cap)
    render_depth(d_mesh, tables[1], tables[0], dtype, out=pred[:2], scratch=pred[2])
    cover = coverage_field(pred, tables[1], d_sc, K, out=bufs.cover)
    geom_out = tables[1].cpu().numpy()
    assert _bytes(geom_out[3:, 0], geom[:, 0] + cap) and _bytes(geom_out[:3], geom)
    crops = _cut(pred[0].cpu().numpy(), pred[1].cpu().numpy(), pred[2].cpu().numpy().view(np.uint64), geom_out)
    assert _bytes(cover.cpu().numpy(), CM.cover_flat(crops, scene, geom_out, K, cap))
    w0, best, sums = bufs.work[0], bufs.best, bufs.sums
    first = None
    for _ in range(2):
        for b in (w0, best, sums):
            b.fill_(-7.0)
        refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, d_rec, w0, best, sums[0], field=field, cover=cover)
        got = tuple(b.cpu().numpy() for b in (w0, best, sums[0]))
        assert first is None or all(_bytes(a, b) for a, b in zip(got, first))
        first = got
    pose_out, g_best, g_sums = got
    want, bounds = CM.evaluate(mesh, render, scene, rigs, nf, lat, geom, frames, table)
    print("worst sum error / bound: %.3g" % _check_sums(g_sums, want, bounds, "pass 0"), "n_cov", g_sums[..., 37].ravel())
    assert (g_sums[..., 37] > 0).sum() >= g_sums[..., 37].size // 2 and (g_sums[..., 38] == 0).all()
    m_best = np.full((3, K, 2, RF.BEST), np.nan)
    G = g_sums.copy()
    m_out = CM.step(G, lat, m_best, 0, False, table)
    assert _bytes(G, g_sums) and all(CM.cost(r, table) == r[30] for r in g_sums.reshape(-1, 40))
    assert _bytes(pose_out, m_out), _where(pose_out, m_out)
    assert _bytes(g_best, m_best) and (g_sums[..., 31] == 1).any()
    for bad in (dict(field=field), dict(cover=cover), {}):               # the 32-value table goes with both fields and no other entry
        with pytest.raises(ValueError, match="params|cover goes with field"):
            refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, d_par, 0, False, d_rec, w0, best, sums[0], **bad)
    with pytest.raises(ValueError, match="params"):
        refine_pass(d_mesh, od, ol, pred, d_geom, d_sc, tables[0], d_nf, _t(silhouette_table(), dev), 0, False, d_rec, w0, best, sums[0], field=field, cover=cover)


# ---- the full loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype,sapien", PERTURBED, ids=PERTURBED_IDS)
def test_full_loop_equals_the_replay_and_the_existing_perturbation_ends_lower(dev, K, dtype, sapien):
    """depth.refine_frames(debug=True) with the 32-value table on test_refinement_cpu's perturbed record: every pass's sums within the
    summation-order bound of the mirror's at the GPU's own poses, the 36 columns equal to the replay's best block byte for byte, cost_best <
    cost_start for every part and pose.  A second call gives the same bytes."""
    from articulated_pose_amd.depth import refine_frames
    prob, rec, per, cen = problem(K, dtype, sapien)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = coverage_table()
    columns, sums = refine_frames(mesh, render, scene, rigs, nf, per, frames, dtype, table, debug=True, device=dev)
    again = refine_frames(mesh, render, scene, rigs, nf, per, frames, dtype, table, device=dev)
    assert columns.shape == (3, K, 36) and sums.shape == (int(table[0]) + 1, 3, K, 2, 40) and _bytes(columns, again)
    best, poses = _replay(prob, per, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, K, 36)), _where(columns, best.reshape(3, K, 36))
    behavioural_bars(columns, strict=True)
    assert (sums[..., 37] > 0).any()


def test_the_lateral_bars_hold_on_the_gpus_result(dev):
    """The CPU test's bars on the GPU's result, K = 2, uint16, a shift of four pixels, against the silhouette term alone and the plain loop
    (also the GPU's): the lateral bar, no triple above 1.0, at least as many at or below 0.5."""
    from articulated_pose_amd.depth import refine_frames
    K, dtype, shift = 2, "uint16", 0.04
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    lat = SM.lateral_record(rec, cen, shift)
    cols, s_cols, p_cols = (refine_frames(mesh, render, scene, rigs, nf, lat, frames, dtype, t, device=dev)
                            for t in (coverage_table(), silhouette_table(), refine_table()))
    behavioural_bars(cols, strict=False)
    r_cov, r_sil, r_plain = (SM.lateral_errors(rec, refined(c), cen) / shift for c in (cols, s_cols, p_cols))
    lateral_bar(r_cov, r_plain)
    print("coverage: worst %.3f; silhouette alone: worst %.3f, at or below 0.5: %d" % (r_cov.max(), r_sil.max(), (r_sil <= 0.5).sum()))
    assert (r_cov > 1.0).sum() == 0 and (r_cov <= 0.5).sum() >= (r_sil <= 0.5).sum(), (np.sort(r_cov.ravel()), np.sort(r_sil.ravel()))


# ---- the edge cases ---------------------------------------------------------------------------------------------------------------------------
def test_nan_poses_zero_norm_factors_parts_without_a_predicted_pixel_and_the_launch_sequence(dev):
    """A part without an observed pixel, a part whose pose draws no pixel in the crop (the cover's sentinel: no row, no charge beyond the
    missed pixels', the solve threshold counts nothing), a NaN pose, a zero norm factor: the columns equal the replay's byte for byte.  The
    launches: the observed field once, then iters + 1 times the table builder, the renderer, ancsh_coverage_field and
    ancsh_refine_pass_cov, then ancsh_refine_rec.  A (frame, part, pose) without a gap pixel has ancsh_refine_pass_sil's first 36 sums."""
    K, dtype = 3, "uint16"
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = coverage_table(iters=2)
    parts, _ = RP.link_parts(scene[0], K)
    obs = [list(fr) for fr in frames]
    obs[0][1] = np.where(np.isin(obs[0][1], np.nonzero(parts == 1)[0]), 255, obs[0][1]).astype(np.uint8)
    obs = [tuple(o) for o in obs]
    bad = rec.copy()
    bad[:, 0] = SM.lateral_record(rec, cen, 0.02)[:, 0]                  # part 0 slides; the others stay where the frame has them
    bad[1, 0, 13 + 10] += 10.0
    bad[1, 2, 4] = np.nan
    nf2 = nf.copy()
    nf2[2] = 0.0
    prob2 = prob[:5] + (nf2,) + prob[6:8] + (obs,)
    columns, sums, names = _loop_on_device(dev, prob2, bad, dtype, table)
    loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_coverage_field", "ancsh_refine_pass_cov"]
    assert names == ["ancsh_silhouette_field"] + loop * 3 + ["ancsh_refine_rec"]
    best, poses = _replay(prob2, bad, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, K, 36))
    b = columns.reshape(3, K, 2, 18)
    assert np.isnan(b[2]).all() and np.isnan(b[1, 2, 0]).all() and np.isfinite(b[1, 2, 1]).all()
    assert np.isnan(sums[:, 2, :, :, :31]).all() and np.isnan(sums[:, 2, :, :, 32:35]).all() and np.isnan(sums[:, 2, :, :, 36:39]).all()
    assert (sums[:, 2, :, :, 31] == 0).all() and (sums[:, 2, :, :, 35] == 0).all() and (sums[:, 2, :, :, 39] == 0).all()
    assert (sums[:, 0, 1, :, 29] == 0).all() and (sums[:, 0, 1, :, 36:] == 0).all() and np.isnan(b[0, 1, :, 13:15]).all()
    assert (sums[:, 1, 0, 1, 28] == 0).all() and (sums[:, 1, 0, 1, 29] > 0).all() and (sums[:, 1, 0, 1, 32:] == 0).all()      # the sentinel
    assert _bytes(b[1, 0, 1, :13], bad[1, 0, 13:]) and b[1, 0, 1, 17] == 0 and abs(b[1, 0, 1, 13] - MAX_DIST ** 2) <= 1e-18
    s_cols, s_sums, _ = _loop_on_device(dev, prob2, bad, dtype, table[:16].copy())
    bare = ((sums[0, ..., 37] + sums[0, ..., 38]) == 0) & ~np.isnan(sums[0, ..., 29])
    assert bare.any() and (sums[0, 0, 0, :, 37] > 0).all() and _bytes(sums[0][bare][:, :36], s_sums[0][bare])


def test_one_part_and_a_crop_of_one_pixel(dev):
    """K = 1, and every frame cut down to one pixel of the part (a 1 x 1 crop: the pixel is a depth row, or a gap pixel whose cover is the
    sentinel or names the pixel itself -- never a row): both against the replay, byte for byte."""
    from test_refinement_cpu import centroids
    from test_reprojection_cpu import random_rigs
    dtype = "uint16"
    prob2 = problem(2, dtype)[0]                                         # the two-part object's frames at K = 1: part 1's links are in no part
    prob = prob2[:4] + (random_rigs(np.random.RandomState(3), 3, 1, False),) + prob2[5:]
    rec = RP.exact_record(prob[2], prob[3], prob[4], prob[5], prob[1], 1)
    cen = centroids(prob[3], prob[5], prob[8], 1)
    table = coverage_table(iters=1, min_pixels=1)
    lat = SM.lateral_record(rec, cen, 0.02)
    columns, sums, _ = _loop_on_device(dev, prob, lat, dtype, table)
    best, _ = _replay(prob, lat, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, 1, 36)) and (sums[0, ..., 37] > 0).all()
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    geom1, frames1, a = [], [], 3
    for f, ((s, h, w, r0, c0), (d, l, _)) in enumerate(zip(geom, frames)):
        img = RP.part_image(d, l, RP.link_parts(scene[f], 1)[0])
        ii, jj = np.nonzero(img == 0)
        i, j = int(ii[len(ii) // 2]), int(jj[len(ii) // 2])
        geom1.append((a, 1, 1, r0 + i, c0 + j))
        frames1.append((d[i:i + 1, j:j + 1].copy(), l[i:i + 1, j:j + 1].copy(), (r0 + i, c0 + j)))
        a += 4
    prob1 = prob[:6] + (np.asarray(geom1, np.int32), a + 2, frames1)
    moved = rec.copy()
    moved[1, 0, 10] += 10.0                                              # frame 1, pose 0: no predicted pixel
    columns, sums, _ = _loop_on_device(dev, prob1, moved, dtype, table)
    best, _ = _replay(prob1, moved, dtype, table, sums)
    assert _bytes(columns, best.reshape(3, 1, 36)) and (sums[..., 29] == 1).all() and (sums[..., 37] == 0).all() and (sums[:, 1, 0, 0, 28] == 0).all()
    assert (sums[:, 0, 0, :, 28] == 1).all()


# ---- the joint step ---------------------------------------------------------------------------------------------------------------------------
def test_joint_step_counts_the_coverage_rows_of_40_wide_sums(dev):
    """K = 8, seven joints, hand-made sums 40 wide and a (32,) table with joint values: xi, pose_out, best, state and obj equal the joint-step
    mirror fed n_j = (sums[28] + sums[33]) + sums[37] byte for byte.  Part 1 reaches min_pixels only through its coverage rows and part 3 only
    through both kinds together, so a rule that dropped either count would solve another system.  sums_ld = 33 is still refused."""
    from articulated_pose_amd.pose.refinement import refine_joint_step
    K = 8
    kin, render, scene, rigs, nf, geom, cap, rec = chain_problem()
    rs = np.random.RandomState(4)
    moved = moved_record(rs, rec, 0.01)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, moved, geom, cap)
    table = coverage_table(joints=dict(weight=1.0, axis_length=0.5), min_pixels=100)
    assert table.shape == (32,)
    S36 = np.stack([np.stack([hand_sums(rs, K, b_scale=1e-3, width=36) for v in range(2)], 1) for f in range(2)])
    S = np.concatenate([S36, np.zeros(S36.shape[:3] + (4,))], 3)
    S[..., 33], S[..., 37] = 7.0, 5.0
    S[:, 1, :, 28], S[:, 1, :, 33], S[:, 1, :, 37] = 60.0, 0.0, 45.0     # 60 < 100 <= 105
    S[:, 3, :, 28], S[:, 3, :, 33], S[:, 3, :, 37] = 40.0, 35.0, 30.0    # 75 < 100 <= 105
    state, obj = np.full((2, K, 2, 18), np.nan), np.zeros((2, 2, 8))
    got = _joint_call(dev, kin, scene, tables, nf, table, 0, False, moved, S, moved[:, :, :26].copy(), state, obj)
    outs = {}
    for name, fed in (("new", CM.joint_sums(S)), ("without n_cov", S[..., :36].copy())):
        m_state, m_obj = state.copy(), obj.copy()
        outs[name] = JS.step_batch(kin, scene, tables, nf, table[:24].copy(), 0, False, moved, fed, moved[:, :, :26].copy(), m_state, m_obj) + (m_state, m_obj)
    for what, g, w in zip(("xi", "pose_out", "best", "state", "obj"), got, outs["new"]):
        assert _bytes(g, w), (what, _where(g, w))
    assert not _bytes(got[0], outs["without n_cov"][0]) and (got[4][:, :, 5] == 7).all() and (got[4][:, :, 6] == 1).all()
    d = [_t(np.asarray(a, np.float64), dev) for a in (kin, scene, tables, table, moved, S)]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="sums"):
        refine_joint_step(d[0], d[1], d[2], _t(nf, dev), d[3], 0, False, d[4], z(2, K, 2, 33), z(2, K, 26), z(2, K, 2, 18), z(2, K, 2, 18), z(2, 2, 8))


# ---- the streams ------------------------------------------------------------------------------------------------------------------------------
def _both(K, dtype, table, off, stream, feed, **kw):
    """The pipeline with the coverage term and the same one with the table cut to `off` values -> ([results], [launch names])."""
    from test_fit_quality_gpu import _launch_names
    results, names = [], []
    for refine in (table, table[:off].copy()):
        on = refine is table
        P = _pipe(K, dtype, refine=refine, **kw)
        names.append(_launch_names(P.prepare()))
        sl = P.slots[0]
        assert P.opts.refine_coverage is on and (sl.refine_bufs.cover is not None) == on and sl.refine_bufs.sums.shape == (1, B_, K, 2, 40 if on else 36)
        if on:
            assert sl.refine_bufs.cover.shape == (K, 2 * CAP_) and sl.refine_bufs.cover.dtype == torch.int32 and sl.refine_bufs.field.shape == (K, CAP_)
            assert all(s.refine_bufs.cover.data_ptr() != sl.refine_bufs.cover.data_ptr() for s in P.slots[1:])
        results.append(list(getattr(P, stream)(feed, articulation=True, link_counts=True)))
        del P
    return results, names


def test_posed_keyed_stream_equals_the_eager_operator_and_the_silhouette_pipeline(dev):
    """stream_posed_batches, K = 3, uint16, keyed, two slots, three padded batches, with reprojection=True as well: the step's last 6 (iters +
    1) + 2 ABI calls are the option's; without the field launches the list is the silhouette-only pipeline's."""
    from articulated_pose_amd.depth import render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    table = coverage_table(iters=2)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k, cloud_base=4 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names = _both(K, dtype, table, 16, "stream_posed_batches", feed, render_mesh=mesh, kinematics=kin, keyed=True, fit_quality=True, reprojection=True)
    loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_coverage_field", "ancsh_refine_pass_cov"]
    assert names[0][-14:] == ["ancsh_silhouette_field"] + loop * 3 + ["ancsh_refine_rec"], names[0][-15:]
    assert names[0][-15] == "ancsh_reproject_compare_rec" and "ancsh_refine_pass_sil" not in names[0] and "ancsh_coverage_field" not in names[1]
    assert [x.replace("_cov", "_sil") for x in names[0] if x != "ancsh_coverage_field"] == names[1]
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(mesh, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, mesh, None, dtype, K, dev, observed, table)


def test_rendered_stream_with_a_sensor_equals_the_eager_operator(dev):
    """stream_render_batches, K = 2, float32, a noisy sensor with holes and edge dropout, not keyed: the gap pixels are the degraded frame's,
    holes read as background."""
    from articulated_pose_amd.depth import pack_sensor, render_depth_frames, sensor_frames
    K, dtype = 2, "float32"
    rs = np.random.RandomState(43)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    sensor = pack_sensor(sigma=(0.002, 0.001, 0.0), z0=1.0, p_hole=0.2, p_edge=0.5, edge_rel=0.05)
    table = coverage_table(iters=1, max_dist=0.1, silhouette=dict(weight=0.5, dist=0.05, slack=1.0), coverage=dict(weight=0.5, dist=0.05, slack=1.0))
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(render=rt, scene=sc, rig=rigs, seed=900 + 5 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names = _both(K, dtype, table, 16, "stream_render_batches", feed, render_mesh=mesh, sensor=sensor)
    assert names[0].count("ancsh_coverage_field") == 2 and names[0].count("ancsh_refine_pass_cov") == 2
    observed = lambda k, crops, rt, sc, seed: sensor_frames(render_depth_frames(mesh, rt, crops, dtype, dev), sc, sensor, dtype, seed=seed, device=dev)
    _check_against_eager(results[0], results[1], batches, mesh, None, dtype, K, dev, observed, table)


def test_library_stream_with_the_joint_step_under_the_range_guard(dev):
    """A two-instance library through stream_posed_batches with joint values in the (32,) table, built under the F16x2 range guard, whose f32
    graph of the step shares the slot's planes: 7 (iters + 1) + 2 launches, and the joint step reads the 40-wide sums."""
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, pose_scene_tables, render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(47)
    kin0, _ = posed_object(rs, K, dtype)
    kin1, _ = posed_object(np.random.RandomState(48), K, dtype)
    kin1[:32] = kin0[:32]                                                # one camera
    kins = np.stack([kin0, kin1])
    mesh = object_mesh4()
    lib = pack_mesh_library([mesh, pack_mesh([(0.9 * v, f) for v, f in object_links()])])
    table = coverage_table(iters=1, joints=dict(weight=1.0, axis_length=0.5))
    batches = []
    for k, (crops, nf, ps, rt, sc, rigs) in enumerate(_stream_batches(rs, K, dtype, kin0, mesh, dev, nbatches=2)):
        ps[:, 28] = [(k + f) % 2 for f in range(3)]
        rt, sc = pose_scene_tables(kins, ps, dev)
        batches.append((crops, nf, ps, rt, sc, rigs))
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=70 + k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, names = _both(K, dtype, table, 24, "stream_posed_batches", feed, render_mesh=lib, kinematics=kins, arithmetic="f16x2", range_guard=True)
    loop = ["ancsh_reproject_scene_build", "ancsh_render_depth_labels_lib", "ancsh_coverage_field", "ancsh_refine_pass_cov", "ancsh_refine_joint_step"]
    assert names[0][-12:] == ["ancsh_silhouette_field"] + loop * 2 + ["ancsh_refine_rec"], names[0][-13:]
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(lib, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, lib, kins, dtype, K, dev, observed, table)
