"""GPU: render-and-compare.  ancsh_reproject_scene_build against its numpy mirror (tests/reprojection_mirror.py, validated on its own in
tests/test_reprojection_cpu.py) bit for bit; the predicted frames against tests/render_mirror.py run on the mirror's tables, byte for byte;
ancsh_reproject_compare_rec against the mirror -- counts exact, uint16 columns bit for bit, float32 columns against math.fsum --; the exact
record, which must reproduce the frame (IoU >= 0.99, max |d| <= one quantum), and a shifted one, which must not; and AncshPipeline(
reprojection=True) through stream_posed_batches and stream_render_batches against the eager chain depth.reprojection_frames and against the same
pipeline built without the option."""
import numpy as np
import pytest
import torch

import reprojection_mirror as RP
from helpers import check_record_layout
from test_reprojection_cpu import (DTYPES, MAPS, SCALE, SIZES, crop_origins, frames_problem, object_links, object_mesh4, posed_object, poses,
                                   predicted_frames, random_rigs)

pytestmark = pytest.mark.gpu
B_, N_, CAP_ = 4, 64, 4096


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _records(rs, exact):
    """The exact record with a shifted nonlinear pose, then arbitrary finite numbers in frame 1, a NaN scale in (0, 1)'s nonlinear pose, an
    infinite entry in (2, 0)'s baseline pose and an all-NaN row."""
    rec = exact.copy()
    rec[:, :, 13 + 10] += 0.03
    rec[1] = rs.normal(size=rec[1].shape)
    rec[0, 1, 13 + 9] = np.nan
    rec[2, 0, 4] = np.inf
    rec[2, -1] = np.nan
    return rec


# ---- the table builder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,sapien", [(2, False), (3, False), (3, True)], ids=["K2", "K3", "K3-sapien-rotation"])
def test_scene_build_equals_the_mirror(dev, K, sapien):
    """Three frames, four links of which one is in no part, records that are exact, arbitrary, NaN in one pose and NaN in a whole row, norm
    factors that are no powers of two, then 0 and inf, a start that is negative, a record wider than 26: both outputs bit for bit, twice."""
    from articulated_pose_amd.pose.reprojection import reproject_scene_build
    mesh, kin, render, scene, rigs, nf, geom, cap, _ = frames_problem(K, "uint16", sapien=sapien)
    rs = np.random.RandomState(3)
    rec = _records(rs, RP.exact_record(render, scene, rigs, nf, kin, K))
    wide = np.concatenate([rec, rs.normal(size=rec.shape[:2] + (33,))], 2)
    for record, factors, g in ((rec, nf, geom), (wide, np.array([nf[0], 0.0, np.inf], np.float32), np.where(np.arange(15).reshape(3, 5) == 5, -4, geom))):
        want_t, want_g = RP.scene_tables(render, scene, rigs, factors, record, g, cap)
        args = [_t(a, dev) for a in (render, scene, rigs, factors, record, np.asarray(g, np.int32))]
        out = (torch.full((6, 208), -7.0, dtype=torch.float64, device=dev), torch.full((6, 5), -7, dtype=torch.int32, device=dev))
        for _ in range(2):
            got_t, got_g = reproject_scene_build(*args, cap, out=out)
            torch.cuda.synchronize()
            assert _bytes(got_g.cpu().numpy(), want_g)
            diff = np.flatnonzero((got_t.cpu().numpy().view(np.uint64) != want_t.view(np.uint64)).any(1))
            assert _bytes(got_t.cpu().numpy(), want_t), diff
    assert np.isnan(want_t[1, 16:64]).all() and np.isnan(want_t[5, 16:64]).all() and np.isfinite(want_t[0, 16:52]).all() and want_g[4, 0] == -4
    with pytest.raises(ValueError, match="rig"):
        reproject_scene_build(args[0], args[1], args[2][:, :-1].contiguous(), *args[3:], cap)


# ---- the predicted frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(3, "uint16"), (2, "float32")])
def test_predicted_frames_equal_the_render_mirror_and_the_columns_the_compare_mirror(dev, K, dtype):
    """depth.reprojection_frames on records with shifted, arbitrary and NaN poses: the two predicted crops per frame equal the render mirror run on
    the mirror's tables byte for byte, the counts are exact, uint16 columns bit for bit, float32 columns within n * 2^-52 of math.fsum."""
    from articulated_pose_amd.depth import reprojection_frames
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = frames_problem(K, dtype)
    rec = _records(np.random.RandomState(4), RP.exact_record(render, scene, rigs, nf, kin, K))
    columns, pred = reprojection_frames(mesh, render, scene, rigs, nf, rec, frames, dtype, dev)
    tables, _ = RP.scene_tables(render, scene, rigs, nf, rec, geom, cap)
    want_pred = predicted_frames(mesh, tables, geom, dtype)
    for f in range(3):
        for v in range(2):
            assert _bytes(pred[f][v][0], want_pred[f][v][0]) and _bytes(pred[f][v][1], want_pred[f][v][1]), (f, v)
    assert any((p[1][1] != 255).any() for p in pred) and (pred[0][1][1] != frames[0][1]).any()
    _check_columns(columns, RP.compare([(d, l) for d, l, _ in frames], want_pred, scene, rec)[:, :, 26:], dtype)
    assert np.isnan(columns[2, -1]).all() and np.isnan(columns[0, 1, 8:]).all() and np.isfinite(columns[0, 1, :3]).all()


def _check_columns(got, want, dtype):
    """Counts and NaN places exact; uint16: every column bit for bit; float32: the depth columns within n_both * 2^-52 relative of the mirror's
    math.fsum values (the maximum exact)."""
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), (got, want)
    if dtype == "uint16":
        assert _bytes(got, want), np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        return
    for cols in ([0], [1, 2, 3], [8, 9, 10], [6], [13]):                 # counts, IoU (one division of exact counts) and the maxima: exact
        assert _bytes(got[..., cols], want[..., cols]), cols
    for base in (1, 8):
        n = want[..., base + 1]
        for c in (3, 4, 6):
            g, w = got[..., base + c], want[..., base + c]
            ok = np.isnan(w) | (np.abs(g - w) <= n * 2.0 ** -52 * np.abs(w))
            assert ok.all(), (base, c, g[~ok], w[~ok], n[~ok])


# ---- the comparison on hand-made and random crops ---------------------------------------------------------------------------------------------
def _scene4(scale):
    sc = np.zeros(240)
    sc[6], sc[14] = scale, 4
    for l, (rank, part) in enumerate(((0, 0), (1, 1), (2, 2), (-1, 0))):
        sc[16 + 14 * l], sc[16 + 14 * l + 1] = rank, part
    return sc


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_compare_equals_the_mirror_on_hand_made_and_random_crops(dev, dtype):
    """Seven frames in one call at unaligned starts: the hand-made row of the CPU test (an empty intersection, a part only the prediction has,
    holes on either side, a link of no part), an all-background pair (the empty union), one pixel, and random 24 x 40 / 17 x 33 / 33 x 40 crops
    (more than 256 pixels: every thread strides) whose predicted depth lies mostly behind the observed one."""
    from articulated_pose_amd.pose.reprojection import reproject_compare
    rs = np.random.RandomState(8)
    K, npdt = 3, DTYPES[dtype]
    hand_o = (np.array([[10, 0, 20, 30, 40, 12]]).astype(npdt), np.array([[0, 0, 1, 255, 3, 0]], np.uint8))
    hand_p = (np.array([[14, 11, 21, 31, 41, 13]]).astype(npdt), np.array([[0, 0, 2, 2, 0, 255]], np.uint8))
    blank = (np.zeros((1, 6), npdt), np.full((1, 6), 255, np.uint8))
    one_o, one_p = (np.array([[7]]).astype(npdt), np.zeros((1, 1), np.uint8)), (np.array([[9]]).astype(npdt), np.zeros((1, 1), np.uint8))
    obs, pred = [hand_o, blank, one_o, hand_o], [(hand_p, hand_p), (blank, blank), (one_p, one_o), (hand_p, blank)]

    def random_pair(h, w):
        lab = rs.randint(0, 4, (h, w)).astype(np.uint8)
        lab[rs.uniform(size=(h, w)) < 0.2] = 255
        if dtype == "uint16":
            d = rs.randint(500, 3000, (h, w)).astype(np.uint16)
            d[rs.uniform(size=(h, w)) < 0.1] = 0
        else:
            d = rs.uniform(0.5, 3.0, (h, w)).astype(np.float32)
            bad = rs.uniform(size=(h, w)) < 0.1
            d[bad] = rs.choice(np.array([0.0, np.nan, np.inf, -1.5], np.float32), int(bad.sum()))
        return d, lab

    def shifted(pair):
        d, lab = pair
        step = rs.randint(-30, 100, d.shape) if dtype == "uint16" else rs.uniform(-0.03, 0.1, d.shape)
        with np.errstate(invalid="ignore"):
            moved = np.where(d > 0, d.astype(np.float64) + step, 0).astype(npdt) if dtype == "uint16" else (d.astype(np.float64) + step).astype(npdt)
        lab2 = np.where(rs.uniform(size=lab.shape) < 0.15, rs.randint(0, 4, lab.shape), lab).astype(np.uint8)
        return moved, lab2
    for h, w in ((24, 40), (17, 33), (33, 40)):
        o = random_pair(h, w)
        obs.append(o)
        pred.append((shifted(o), shifted(o)))
    n = len(obs)
    scene = np.stack([_scene4(0.5 if f < 4 else SCALE[dtype]) for f in range(n)])
    carried = rs.normal(size=(n, K, 38))
    carried[0, 2, 13:26], carried[3, 1, :13], carried[4, 0, :26], carried[5, 2, 20] = np.nan, np.nan, np.nan, np.inf
    geom, a = [], 5
    for d, _ in obs:
        geom.append((a, d.shape[0], d.shape[1], 0, 0))
        a += d.size + 3
    cap = a + 6
    od, ol, pd, pl = np.zeros(cap, npdt), np.full(cap, 255, np.uint8), np.zeros(2 * cap, npdt), np.full(2 * cap, 255, np.uint8)
    for (s, h, w, _, _), o, p in zip(geom, obs, pred):
        od[s:s + h * w], ol[s:s + h * w] = o[0].reshape(-1), o[1].reshape(-1)
        for v in range(2):
            pd[v * cap + s:v * cap + s + h * w], pl[v * cap + s:v * cap + s + h * w] = p[v][0].reshape(-1), p[v][1].reshape(-1)
    want = RP.compare(obs, pred, scene, carried)
    out = torch.full((n, K, 38 + 15), -7.0, dtype=torch.float64, device=dev)
    args = [_t(x, dev) for x in (od, ol, pd, pl, np.asarray(geom, np.int32), scene, carried)]
    first = None
    for _ in range(2):
        got = reproject_compare(*args, out=out).cpu().numpy()
        assert _bytes(got[:, :, :38], carried)
        _check_columns(got[:, :, 38:], want[:, :, 38:], dtype)
        assert first is None or _bytes(got, first)                       # the same bytes on a second call
        first = got
    c = got[:, :, 38:]
    assert c[0, 0, :4].tolist() == [2, 3, 1, 0.25] and c[0, 1, :4].tolist() == [1, 0, 0, 0.0] and np.isnan(c[0, 1, 4:8]).all()
    assert c[0, 2, :4].tolist() == [0, 2, 0, 0.0] and np.isnan(c[0, 2, 8:]).all()                       # only the prediction has part 2
    assert c[1, 0, :3].tolist() == [0, 0, 0] and np.isnan(c[1, 0, 3:8]).all()                            # the empty union
    assert c[2, 0, :8].tolist() == [1, 1, 1, 1.0, 1.0, 1.0, 1.0, 1.0] and c[2, 0, 8:].tolist() == [1, 1, 1.0, 0.0, 0.0, 0.0, 0.0]     # one pixel
    assert np.isnan(c[3, 1, 1:8]).all() and c[3, 1, 0] == 1 and np.isnan(c[4, 0]).all() and np.isnan(c[5, 2, 8:]).all()
    assert (c[5:, :, 2] > 30).all() and (c[4, 1:, 2] > 30).all() and (c[5:, :, 7] > 0).all() and (c[5:, :, 7] < c[5:, :, 4]).all()   # mixed signs, the mean behind
    # a crop the depth entries refuse counts nothing; no frame launches nothing
    bad = np.asarray(geom, np.int32).copy()
    bad[6, 0] = cap - 10
    got = reproject_compare(*args[:4], _t(bad, dev), *args[5:]).cpu().numpy()[:, :, 38:]
    assert got[6, :, :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(got[6, :, 3:8]).all() and _bytes(got[:6], c[:6])


# ---- the two bars -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dtype", [(2, "uint16"), (3, "uint16"), (3, "float32")])
def test_exact_poses_reproduce_the_frame_and_a_shifted_pose_does_not(dev, K, dtype):
    """The record replaced by the exact one: the nonlinear IoU is >= 0.99 for every part and max |d| <= one depth quantum (uint16) -- the CPU
    test holds the mirror to the same bars on the same frames, so a failure here is the kernels'.  A nonlinear pose translated by a tenth of
    the part's extent: a strictly lower IoU and a strictly larger mean |d| for every part."""
    from articulated_pose_amd.depth import reprojection_frames
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = frames_problem(K, dtype)
    rec = RP.exact_record(render, scene, rigs, nf, kin, K)
    shifted = rec.copy()
    shifted[:, :, 13 + 10] += 0.1 * 0.32 * nf[:, None]
    exact, _ = reprojection_frames(mesh, render, scene, rigs, nf, rec, frames, dtype, dev)
    moved, _ = reprojection_frames(mesh, render, scene, rigs, nf, shifted, frames, dtype, dev)
    print(exact[:, :, [0, 8, 9, 10, 11, 13]], moved[:, :, [10, 11]])
    assert np.isfinite(exact).all() and (exact[:, :, 0] > 0).all()
    assert (exact[:, :, 10] >= 0.99).all() and (exact[:, :, 3] >= 0.99).all()
    if dtype == "uint16":
        assert (exact[:, :, 13] <= SCALE[dtype] * (1 + 1e-12)).all() and (exact[:, :, 6] <= SCALE[dtype] * (1 + 1e-12)).all()
    assert _bytes(moved[:, :, :8], exact[:, :, :8])
    assert (moved[:, :, 10] < exact[:, :, 10]).all() and (moved[:, :, 11] > exact[:, :, 11]).all()


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------
def _pipe(K, dtype, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.weights import synthetic_weights
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype), **kw)
    return AncshPipeline(K, synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1), B_, N_, "cuda:0", **kw)


def _stream_batches(rs, K, dtype, kin, mesh, dev, nbatches=3):
    """Three batches of three frames (a batch_size = 4 pipeline pads each; two slots: the third batch reuses a slot): per batch (crops, norm
    factors, poses, render tables, scene tables -- the device builder's, which the posed step builds again --, rigs)."""
    from articulated_pose_amd.depth import pose_scene_tables
    out = []
    for k in range(nbatches):
        ps = poses(rs, 3)
        rt, sc = pose_scene_tables(kin, ps, dev)
        crops = [(h, w, o) for (h, w), o in zip(SIZES, crop_origins(mesh, rt))]
        out.append((crops, rs.uniform(0.7, 1.3, 3).astype(np.float32), ps, rt, sc, random_rigs(rs, 3, K, sapien=(K == 3 and k == 1))))
    return out


def _check_against_eager(got, off, batches, mesh, dtype, K, dev, observed, layouts=None):
    """Every retired batch: the 15 columns equal depth.reprojection_frames on the same tables and the streamed record's own leading columns,
    byte for byte; every earlier column and every other element of the tuple equal the pipeline built without the option; n_obs equals the
    stream's per-part pixel counts from link_counts.  layouts = the two pipelines' record_layout: the hand slices are the layout's blocks."""
    from articulated_pose_amd.depth import reprojection_frames
    from articulated_pose_amd.pose.reprojection import named_columns
    assert len(got) == len(off) == len(batches)
    seen = 0
    for k, (g, o, (crops, nf, ps, rt, sc, rigs)) in enumerate(zip(got, off, batches)):
        rec = g[2]
        W = o[2].shape[2]
        assert rec.shape == (3, K, W + 15) and g[:2] == o[:2] and len(g) == len(o)
        assert _bytes(rec[:, :, :W], o[2]), k
        if layouts is not None:
            L, Lo = layouts
            assert L.width == rec.shape[2] and Lo.width == W == L.span("reprojection").start and L.names == Lo.names + ("reprojection",)
            assert _bytes(L.block(rec, "reprojection"), rec[:, :, W:]) and all(_bytes(L.block(rec, n), Lo.block(o[2], n)) for n in Lo.names)
            assert _bytes(named_columns(L.block(rec, "reprojection"))["n_obs"], rec[:, :, W]) and L.column("reprojection", "n_obs") == W
        assert all(_bytes(a, b) for a, b in zip(g[3:], o[3:])), k
        columns, pred = reprojection_frames(mesh, rt, sc, rigs, nf, rec[:, :, :W], observed(k, crops, rt, sc, g[1]), dtype, dev)
        assert _bytes(rec[:, :, W:], columns), (k, rec[:, :, W:], columns)
        lc = g[-1]
        for f in range(3):
            parts, _ = RP.link_parts(sc[f], K)
            for j in range(K):
                if np.isfinite(rec[f, j, W]):
                    assert rec[f, j, W] == sum(int(lc[f, l]) for l in range(16) if parts[l] == j), (k, f, j)
                    seen += 1
    assert seen > 0 and any(np.isfinite(g[2][:, :, -14:]).any() for g in got)       # some fitted pose was rendered and scored


def test_posed_keyed_stream_equals_the_eager_chain_and_the_plain_pipeline(dev):
    """stream_posed_batches, K = 3, uint16, keyed, two slots, three padded batches: the step's last three ABI calls are the option's; the slot
    owns the predicted frames' tables and pixel triple."""
    from articulated_pose_amd.depth import render_depth_frames
    from test_fit_quality_gpu import _launch_names
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k, cloud_base=4 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results = []
    for on in (True, False):
        P = _pipe(K, dtype, render_mesh=mesh, kinematics=kin, keyed=True, fit_quality=True, reprojection=on)
        names = _launch_names(P.prepare())
        sl = P.slots[0]
        L = check_record_layout(P, ("pose", "fit_quality", "point_gt") + (("reprojection",) if on else ()))
        if on:
            assert names[-3:] == ["ancsh_reproject_scene_build", "ancsh_render_depth_labels", "ancsh_reproject_compare_rec"], names[-5:]
            assert sl.reproj_tables[0].shape == (2 * B_, 208) and sl.reproj_tables[1].shape == (2 * B_, 5)
            assert [tuple(t.shape) for t in sl.reproj_pix] == [(2 * CAP_,)] * 3 and sl.reproj_pix[2].dtype == torch.int64
            assert all(s.reproj_pix[0].data_ptr() != sl.reproj_pix[0].data_ptr() for s in P.slots[1:])
            assert sl.out["record"].shape == (B_, K, 26) and sl.out["record_reproj"].shape == (B_, K, 39 + 21 + 15)
            assert (L.width, L.key, L.carried("reprojection")) == (39 + 21 + 15, "record_reproj", ("record_point_gt", 39 + 21))
        else:
            assert sl.reproj_pix is None and not any("reproject" in n for n in names) and "record_reproj" not in sl.out
            assert names == results[0][1][:-3]
        results.append((list(P.stream_posed_batches(feed, articulation=True, link_counts=True)), names, L))
        del P
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(mesh, rt, crops, dtype, dev)
    _check_against_eager(results[0][0], results[1][0], batches, mesh, dtype, K, dev, observed, layouts=(results[0][2], results[1][2]))


def test_rendered_stream_with_a_sensor_compares_against_the_degraded_frame(dev):
    """stream_render_batches, K = 2, float32, a noisy sensor, not keyed: the observed side is the degraded frame -- the eager chain is fed
    depth.sensor_frames' output for the batch's seed, and n_obs equals the degraded frame's link counts."""
    from articulated_pose_amd.depth import pack_sensor, render_depth_frames, sensor_frames
    K, dtype = 2, "float32"
    rs = np.random.RandomState(43)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    table = pack_sensor(sigma=(0.002, 0.001, 0.0), z0=1.0, p_hole=0.2, p_edge=0.5, edge_rel=0.05)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(render=rt, scene=sc, rig=rigs, seed=900 + 5 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, layouts = [], []
    for on in (True, False):
        P = _pipe(K, dtype, render_mesh=mesh, sensor=table, reprojection=on)
        results.append(list(P.stream_render_batches(feed, articulation=True, link_counts=True)))
        layouts.append(check_record_layout(P, ("pose", "point_gt") + (("reprojection",) if on else ())))
        del P
    observed = lambda k, crops, rt, sc, seed: sensor_frames(render_depth_frames(mesh, rt, crops, dtype, dev), sc, table, dtype, seed=seed, device=dev)
    _check_against_eager(results[0], results[1], batches, mesh, dtype, K, dev, observed, layouts=layouts)
    clean = render_depth_frames(mesh, batches[0][3], batches[0][0], dtype, dev)
    noisy = observed(0, batches[0][0], batches[0][3], batches[0][4], results[0][0][1])
    assert sum(int((l != 255).sum()) for _, l, _ in noisy) < sum(int((l != 255).sum()) for _, l, _ in clean)


def test_library_stream_equals_the_eager_chain(dev):
    """A two-instance library through stream_render_batches (the frame's instance in its render table's value 9, which the predicted tables
    carry on): the second instance is the object at nine tenths of its size.  Built under the F16x2 range guard, whose f32 graph of the step
    carries the option too."""
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, render_depth_frames
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(47)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    lib = pack_mesh_library([mesh, pack_mesh([(0.9 * v, f) for v, f in object_links()])])
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev, nbatches=2)
    for k, b in enumerate(batches):
        b[3][:, 9] = [(k + f) % 2 for f in range(3)]
    feed = [(crops, nf, dict(render=rt, scene=sc, rig=rigs, seed=70 + k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results = []
    for on in (True, False):
        P = _pipe(K, dtype, render_mesh=lib, reprojection=on, arithmetic="f16x2", range_guard=True)
        results.append(list(P.stream_render_batches(feed, articulation=True, link_counts=True)))
        sl = P.slots[0]                                                  # the range guard's f32 graph ends with the same three calls
        assert sl.graph32 is not None and ("record_reproj" in sl.out32) == on and ("record_reproj" in sl.out) == on
        assert not on or sl.out32["record_reproj"].shape == sl.out["record_reproj"].shape == (B_, K, 26 + 21 + 15)
        assert check_record_layout(P).width == 26 + 21 + (15 if on else 0)      # the f32 graph's record too
        del P
    observed = lambda k, crops, rt, sc, seed: render_depth_frames(lib, rt, crops, dtype, dev)
    _check_against_eager(results[0], results[1], batches, lib, dtype, K, dev, observed)
