"""GPU: annotated depth frames -- ancsh_depth_annotate_stream and depth.annotate_depth_batch against the numpy float64 restatement of
tools/preprocess_data.py:259-320 and lib/dataset.py:475-485 (tests/test_depth_annotate_cpu.py), the minimum rule, and
AncshPipeline(depth_capacity=..., point_ground_truth=True, build_point_gt=True) against the xyz build_point_gt pipeline fed the operator's
rows.  The paths the option does not touch are held to bytes the parent commit streamed (tests/golden/depth_annotate_unchanged.npz)."""
import os

import numpy as np
import pytest
import torch

from redzone import Arena
from test_depth_annotate_cpu import random_scene, restate_cloud, scene_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.0
PARTS_MAP = [[0], [2, 1]]               # rank differs from the link index, and part 1 has two links
SCALE = {"uint16": 1e-4, "float32": 1.0}


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _depth(rs, h, w, dtype, holes=0.08):
    """Depths of 0.5 .. 3 units with holes: zeros, and for float32 NaN, Inf and a negative value as well."""
    if dtype == "uint16":
        d = rs.randint(5000, 30000, (h, w)).astype(np.uint16)
        d[rs.uniform(size=(h, w)) < holes] = 0
        return d
    d = rs.uniform(0.5, 3.0, (h, w)).astype(np.float32)
    u = rs.uniform(size=(h, w))
    for k, v in enumerate((0.0, np.nan, np.inf, -1.5)):
        d[(u >= holes / 4 * k) & (u < holes / 4 * (k + 1))] = v
    return d


def _background(rs, lab, share=0.1):
    """Some pixels of no link: half of them 255, half a value that is no link of a three-link scene."""
    u = rs.uniform(size=lab.shape)
    lab[u < share / 2] = 255
    lab[(u >= share / 2) & (u < share)] = 7
    return lab


def _layout(crops, labels, origins, pixel_capacity, dtype):
    """Crops back to back from pixel 0 of buffers of pixel_capacity pixels; the pixels behind them look valid (depth 1, link 0)."""
    pix = np.full(pixel_capacity, 10000 if dtype == "uint16" else 1.0, np.uint16 if dtype == "uint16" else np.float32)
    lab = np.zeros(pixel_capacity, np.uint8)
    geom = np.zeros((len(crops), 5), np.int32)
    a = 0
    for k, (c, l) in enumerate(zip(crops, labels)):
        pix[a:a + c.size], lab[a:a + c.size] = c.reshape(-1), l.reshape(-1)
        geom[k] = (a, c.shape[0], c.shape[1], origins[k][0], origins[k][1])
        a += c.size
    assert a <= pixel_capacity
    return pix, lab, geom


def _operator(dev, pix, lab, geom, scenes, extra_rows=32):
    """One call of the entry on redzone-guarded outputs -> (rows with the extra rows behind pixel_capacity, offsets, counts, link counts)."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import MAX_CHUNKS
    B, cap = geom.shape[0], pix.shape[0]
    arena = Arena()
    d_pix = torch.from_numpy(pix.view(np.int16) if pix.dtype == np.uint16 else pix).to(dev)
    d_lab, d_geom, d_scene = torch.from_numpy(lab).to(dev), torch.from_numpy(geom).to(dev), torch.from_numpy(np.ascontiguousarray(scenes)).to(dev)
    rows = arena.empty((cap + extra_rows, 7), dtype=torch.float32, device=dev)
    rows.fill_(SENTINEL)
    off = arena.empty((B + 1,), dtype=torch.int32, device=dev)
    cnt = arena.empty((B,), dtype=torch.int32, device=dev)
    lc = arena.empty((B, 16), dtype=torch.int32, device=dev)
    scratch = arena.empty((B * MAX_CHUNKS * 16,), dtype=torch.int32, device=dev)
    _lib.call("ancsh_depth_annotate_stream", B, 0 if pix.dtype == np.uint16 else 1, _lib.ptr(d_pix), _lib.ptr(d_lab), cap, _lib.ptr(d_geom),
              _lib.ptr(d_scene), _lib.ptr(rows), cap, _lib.ptr(off), _lib.ptr(cnt), _lib.ptr(lc), _lib.ptr(scratch))
    torch.cuda.synchronize()
    out = rows.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy(), lc.cpu().numpy()
    arena.check()
    return out


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def check_cloud(got, S, sc, depth, label, origin, parts_map, scale, min_px, what):
    """A cloud's rows against the restatement: order, part column and count exact; x y z bit-equal to the entry's written float64
    expression on the scene's coefficients, cast once -- and within half a float32 ulp + 1e-12 of the reference's own cloud_cam_real --;
    cx cy cz within 0.5 ulp_f32(want) + 1e-12 of the restated chain (a correctly rounded float64 value up to float64 noise: the 1e-12
    covers the host's composition of M against the reference's per-point chain of products).  -> the per-link counts."""
    lab = np.where(label < len(S["world_pos"]), label, -1)
    want, counts, pix = restate_cloud(S, depth, lab, origin, parts_map, scale, min_px)
    if want is None:
        assert got.shape == (1, 7) and np.isnan(got).all(), what
        return counts
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 6], want[:, 6].astype(np.float32)), what
    row, col = (pix[:, 0] + origin[0]).astype(np.float64), (pix[:, 1] + origin[1]).astype(np.float64)
    z = depth[pix[:, 0], pix[:, 1]].astype(np.float64) * sc[6]
    x, y = z * ((sc[0] * col + sc[1] * row) + sc[2]), z * ((sc[3] * col + sc[4] * row) + sc[5])
    written = np.stack([x, y, z], 1).astype(np.float32)
    assert _bytes(got[:, :3], written), (what, np.flatnonzero((got[:, :3] != written).any(1))[:8])
    for name, cols in (("x y z", slice(0, 3)), ("cx cy cz", slice(3, 6))):
        err = np.abs(got[:, cols].astype(np.float64) - want[:, cols])
        bound = 0.5 * _ulp32(want[:, cols]) + 1e-12
        print("%s, %s: worst error / bound = %.3f, largest |value| %.3g" % (what, name, (err / bound).max(), np.abs(want[:, cols]).max()))
        assert (err <= bound).all(), (what, name, (err / bound).max())
    assert np.abs(want[:, 3:6]).max() <= 10.0, what
    return counts


def check_batch(dev, crops, labels, origins, scenes_S, parts_map, dtype, pixel_capacity, min_px, what):
    scale = SCALE[dtype]
    tables = np.stack([scene_table(S, parts_map, scale, min_px) for S in scenes_S])
    pix, lab, geom = _layout(crops, labels, origins, pixel_capacity, dtype)
    rows, off, cnt, lc = got = _operator(dev, pix, lab, geom, tables)
    again = _operator(dev, pix, lab, geom, tables)
    assert all(_bytes(a, b) for a, b in zip(got, again)), what          # a pure function of the input
    assert off[0] == 0
    for b in range(len(crops)):
        counts = check_cloud(rows[off[b]:off[b + 1]], scenes_S[b], tables[b], crops[b], labels[b].astype(np.int64), origins[b], parts_map, scale, min_px,
                             "%s cloud %d" % (what, b))
        used = [s for g in parts_map for s in g]
        assert lc[b].tolist() == [counts[s] if s in used else 0 for s in range(len(scenes_S[b]["world_pos"]))] + [0] * (16 - len(scenes_S[b]["world_pos"])), (what, b)
        total = sum(counts[s] for s in used) if all(counts[s] >= min_px for s in used) else 0
        assert cnt[b] == total and off[b + 1] - off[b] == max(total, 1), (what, b, cnt[b], total)
    assert (rows[off[-1]:] == SENTINEL).all(), what                      # nothing behind offsets[nclouds]
    return got


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_three_frames_over_three_chunks_equal_the_restatement(dev, dtype):
    """pixel_capacity = 3 * 3 * 2048: every cloud has three chunks, so chunk and cloud boundaries are crossed; the second crop starts at an
    odd pixel of the buffer.  Crop 0 is a per-pixel checkerboard of the three links (every wave step splits three ways), crop 1 keeps
    link 1 inside its first chunk (absent from the two others), crop 2 is 1 x 9 with three pixels a link."""
    rs = np.random.RandomState(5 + len(dtype))
    shapes, origins = [(53, 37), (64, 64), (1, 9)], [(100, 200), (17, 301), (40, 44)]
    crops = [_depth(rs, h, w, dtype) for h, w in shapes]
    i, j = np.indices(shapes[0])
    lab0 = _background(rs, ((i + j) % 3).astype(np.uint8))
    i, j = np.indices(shapes[1])
    lab1 = _background(rs, np.where(i < 20, np.where(j < 40, 1, 0), np.where(j < 25, 2, 0)).astype(np.uint8))
    assert 20 * 64 < (64 * 64 + 2) // 3                                  # link 1 ends inside chunk 0 of 3
    lab2 = np.array([[0, 1, 2, 2, 1, 0, 1, 2, 0]], np.uint8)
    crops[2][:] = 20000 if dtype == "uint16" else 2.0
    scenes_S = [random_scene(rs, 3) for _ in shapes]
    rows, off, cnt, lc = check_batch(dev, crops, [lab0, lab1, lab2], origins, scenes_S, PARTS_MAP, dtype, 3 * 3 * 2048, 2, dtype)
    assert crops[0].size % 2 == 1 and cnt[2] == 9 and (lc[:, :3] > 0).all() and cnt[0] > 1500 and cnt[1] > 3000
    assert rows[off[2]:off[3], 6].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1]    # link 0 | link 2, then link 1: parts 0 | 1 1


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_one_chunk_of_several_steps_and_an_unused_link(dev, dtype):
    """Four clouds in 4 * 2048 pixels: one chunk a cloud, and the 80 x 90 crop's chunk takes 4 (uint16) / 8 (float32) steps of 256 lanes, so
    the running per-link bases cross steps.  Link 1 is in no group of the parts map: its pixels are dropped and its count reads 0."""
    rs = np.random.RandomState(17)
    shapes, origins = [(1, 9), (80, 90), (3, 5), (2, 2)], [(0, 0), (200, 150), (11, 500), (300, 300)]
    crops = [_depth(rs, h, w, dtype, holes=0.04) for h, w in shapes]
    labels = [_background(rs, rs.randint(0, 4, s).astype(np.uint8)) for s in shapes]
    scenes_S = [random_scene(rs, 4) for _ in shapes]
    rows, off, cnt, lc = check_batch(dev, crops, labels, origins, scenes_S, [[3], [0, 2]], dtype, 4 * 2048, 1, dtype + " steps")
    assert cnt[1] > 4000 and (lc[:, 1] == 0).all()


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_minimum_rule(dev, dtype):
    """tools/preprocess_data.py:279-281: a frame whose link 2 has 9 valid pixels has no rows -- count 0, one NaN row, offsets advanced by
    one --, with 10 it passes; its neighbours' rows are the same bytes either way."""
    rs = np.random.RandomState(23)
    shapes, origins = [(24, 30), (20, 21), (30, 16)], [(10, 10), (250, 250), (400, 100)]
    crops = [_depth(rs, h, w, dtype, holes=0.0) for h, w in shapes]
    labels = [rs.randint(0, 3, s).astype(np.uint8) for s in shapes]
    labels[1][labels[1] == 2] = 0
    spots = rs.permutation(20 * 21)[:11]
    labels[1].reshape(-1)[spots] = 2                                     # eleven pixels of link 2 ...
    crops[1].reshape(-1)[spots[0]] = 0                                   # ... one of them a hole: ten valid
    scenes_S = [random_scene(rs, 3) for _ in shapes]
    ten = check_batch(dev, crops, labels, origins, scenes_S, PARTS_MAP, dtype, 3 * 2048, 10, dtype + " ten")
    crops[1].reshape(-1)[spots[1]] = 0                                   # nine valid
    nine = check_batch(dev, crops, labels, origins, scenes_S, PARTS_MAP, dtype, 3 * 2048, 10, dtype + " nine")
    assert ten[3][1, 2] == 10 and ten[2][1] == 20 * 21 - 1 and nine[3][1, 2] == 9 and nine[2][1] == 0
    assert nine[1][2] - nine[1][1] == 1 and np.isnan(nine[0][nine[1][1]]).all()
    for b in (0, 2):
        assert _bytes(ten[0][ten[1][b]:ten[1][b + 1]], nine[0][nine[1][b]:nine[1][b + 1]]) and ten[2][b] == nine[2][b] > 300, b


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------
K_, B_, N_, CAP_ = 3, 2, 64, 8192
LINKS_, MAP_ = 4, [[0], [2, 1], [3]]


def _frame(rs, dtype, starve=None):
    """(depth crop, label crop, origin, scene): four links in the quadrants of a crop of about 40 x 36 pixels around the principal point, with
    background and holes; starve = a link left with five pixels."""
    h, w = int(rs.randint(34, 44)), int(rs.randint(30, 40))
    i, j = np.indices((h, w))
    lab = (2 * (i >= h // 2) + (j >= w // 2)).astype(np.uint8)
    if starve is not None:
        at = np.flatnonzero(lab.reshape(-1) == starve)
        lab.reshape(-1)[at[5:]] = (starve + 1) % LINKS_
    lab = _background(rs, lab, share=0.06 if starve is None else 0.0)
    return _depth(rs, h, w, dtype, holes=0.05 if starve is None else 0.0), lab, (int(rs.randint(200, 260)), int(rs.randint(200, 260))), random_scene(rs, LINKS_)


def _batch(rs, dtype, n, starve=None):
    """-> (frames, norm factors, scene tables, rigs, joint frames) of one batch; starve: frame 1's link 3 is below the minimum."""
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    made = [_frame(rs, dtype, starve=3 if (starve and k == 1) else None) for k in range(n)]
    tables = np.stack([scene_table(m[3], MAP_, SCALE[dtype]) for m in made])
    return [m[:3] for m in made], rs.uniform(0.9, 1.1, n).astype(np.float32), tables, np.tile(stream_rig(), (n, 1)), random_frames(rs, n)


def _weights():
    """Random weights for both networks (N_ = 64 points are too few for the passthrough problem's populated parts)."""
    from articulated_pose_amd.weights import synthetic_weights
    return dict(w_ancsh=synthetic_weights(K_, seed=0), w_npcs=synthetic_weights(K_, mixed_pred=False, early_split_nocs=False, seed=1))


def _pipes(pb, dtype, **kw):
    """(the pipeline of annotated depth frames, the xyz build_point_gt pipeline) with the same arguments otherwise."""
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True), **kw)
    mk = lambda **cap: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **cap))
    return mk(depth_capacity=CAP_, depth_dtype=dtype), mk(raw_capacity=CAP_)


def _clouds(frames, tables, dtype):
    """The operator's rows of a batch as the xyz pipeline takes them, its counts and link counts."""
    from articulated_pose_amd.depth import annotate_depth_batch
    rows, off, cnt, lc = annotate_depth_batch(frames, tables, dtype, K_)
    assert rows.shape == (off[-1], 7) and rows.dtype == np.float32 and lc.shape == (len(frames), 16)
    return [np.ascontiguousarray(rows[off[b]:off[b + 1]]) for b in range(len(frames))], cnt, lc


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_annotated_depth_stream_equals_the_xyz_build_stream(dev, dtype):
    """Three batches through two slots, the last one short: records, articulation blocks and counts of the annotated depth stream equal, byte
    for byte, those of an xyz build_point_gt pipeline fed the rows depth.annotate_depth_batch returned for the same frames -- same rigs,
    joint frames, seeds and joint_source="predicted"."""
    from articulated_pose_amd.depth import SCENE_WIDTH
    pb = _weights()
    rs = np.random.RandomState(31)
    batches = [_batch(rs, dtype, n) for n in (2, 2, 1)]
    A, X = _pipes(pb, dtype)
    sl = A.slots[0]
    assert sl.src_rows.shape == (CAP_, 7) and sl.raw_rows.shape == (CAP_, 18) and sl.h_rows is None and sl.scene.shape == sl.h_scene.shape == (B_, SCENE_WIDTH)
    assert sl.scene.dtype == torch.float64 and sl.link_counts.shape == (B_, 16) and sl.h_mask.shape == (CAP_,) and sl.rig.shape[0] == B_
    for k, (frames, nf, tables, rigs, jf) in enumerate(batches):
        clouds, cnt, lc = _clouds(frames, tables, dtype)
        for b, (d, l, org) in enumerate(frames):                         # the operator's rows are the restatement's (spot check: the order)
            assert cnt[b] == (l < LINKS_)[(d != 0) & np.isfinite(d.astype(np.float64)) & (d.astype(np.float64) > 0)].sum() and cnt[b] > 700
            assert (np.diff(clouds[b][:, 6]) >= 0).all() and set(clouds[b][:, 6]) == {0.0, 1.0, 2.0}
        A.submit_depth(frames, nf, scene=tables, rig=rigs, frame=jf)
        X.submit(clouds, nf, rig=rigs, frame=jf)
        ga, gx = A.retire(articulation=True, link_counts=True), X.retire(articulation=True)
        assert len(ga) == 6 and len(gx) == 4 and ga[:2] == gx[:2]
        assert ga[2].shape == (len(frames), K_, 26 + 21) and _bytes(ga[2], gx[2]) and _bytes(ga[3], gx[3]), k
        assert ga[4].dtype == np.int32 and np.array_equal(ga[4], cnt) and ga[5].dtype == np.int32 and np.array_equal(ga[5], lc), k
        assert np.isfinite(ga[2][:, :, 26:]).any() and np.isfinite(ga[2][:, :, :26]).any()
        n = sum(c.shape[0] for c in clouds)
        assert _bytes(A.slots[k % 2].src_rows[:n].cpu().numpy(), np.concatenate(clouds)), k
        assert _bytes(A.slots[k % 2].raw_rows[:n].cpu().numpy(), X.slots[k % 2].raw_rows[:n].cpu().numpy()), k
        for name in ("P", "perm"):                                       # the sampler drew the same rows
            assert _bytes(getattr(A.slots[k % 2], name).cpu().numpy(), getattr(X.slots[k % 2], name).cpu().numpy()), (k, name)
        assert np.isfinite(A.slots[k % 2].P.cpu().numpy()).all()
    # the generator: scenes, rigs and joint frames travel in the per-batch dict; link counts only when asked
    feed = [(f, nf, "t%d" % k, dict(scene=t, rig=r, frame=jf)) for k, (f, nf, t, r, jf) in enumerate(batches)]
    del A, X
    A, X = _pipes(pb, dtype)                                             # fresh pipelines: the default seeds start over
    got = list(A.stream_depth_batches(feed, articulation=True))
    want = list(X.stream_batches([(_clouds(f, t, dtype)[0], nf, jf, r, "t%d" % k) for k, (f, nf, t, r, jf) in enumerate(batches)], articulation=True))
    assert [len(g) for g in got] == [5, 5, 5] and [g[0] for g in got] == ["t0", "t1", "t2"] and got[2][2].shape[0] == 1
    for g, w in zip(got, want):
        assert _bytes(g[2], w[2]) and _bytes(g[3], w[3])
    assert [g[1] for g in got] == [w[1] for w in want]
    # refused before anything is enqueued, and the pipeline stays usable
    frames, nf, tables, rigs, jf = batches[0]
    for kw in (dict(scene=None), dict(rig=None), dict(cameras=[1, 0, 0, 0, 1, 0]), dict(scene=tables[:, :239]), dict(scene=np.where(np.arange(240) == 14, 17, tables)),
               dict(frames=[(d, l.astype(np.float32), o) for d, l, o in frames]), dict(frames=[(np.ones((100, 90), frames[0][0].dtype), np.zeros((100, 90), int), (0, 0))] * 2)):
        args = dict(dict(frames=frames, norm_factors=nf, scene=tables, rig=rigs, frame=jf), **kw)
        with pytest.raises(ValueError):
            A.submit_depth(**args)
    with pytest.raises(RuntimeError):
        A.retire(label_images=True)
    assert not A._inflight


def test_a_frame_below_the_minimum_poisons_its_own_record_only(dev):
    """A batch whose frame 1 leaves link 3 with five pixels: that frame streams an all-NaN record, count 0 and an all-NaN articulation row
    -- ancsh_point_gt_build turns the NaN row's NaN part into an all-NaN row, which the sampler hands on --, frame 0's record is the one of
    the same batch with frame 1 intact, byte for byte."""
    pb = _weights()
    A, _ = _pipes(pb, "uint16", slots=1)
    del _
    frames, nf, tables, rigs, jf = _batch(np.random.RandomState(41), "uint16", 2, starve=True)
    A.submit_depth(frames, nf, scene=tables, rig=rigs, frame=jf, seed=77)
    _, _, rec, art, cnt, lc = A.retire(articulation=True, link_counts=True)
    assert cnt[1] == 0 and lc[1, 3] == 5 and cnt[0] > 700 and np.isnan(rec[1]).all() and np.isfinite(rec[0, :, :26]).any()
    # on the device the row is NaN but for ancsh_point_gt_rec's two point counts (columns ld + 10, ld + 11), which retire() blanks
    on_device = A.slots[0].out["record_point_gt"].cpu().numpy()[1]
    assert np.isnan(np.delete(on_device, [36, 37], axis=1)).all() and (on_device[:, 36:38] == 0).all()
    raw = A.slots[0].raw_rows.cpu().numpy()
    assert np.isnan(raw[cnt[0], :3]).all() and raw[cnt[0], 3] == raw[cnt[0], 17] == -1 and np.isnan(raw[cnt[0], 4:17]).all()
    d, l, org = frames[1]
    relaxed = tables.copy()
    relaxed[1, 13] = 5                                                  # the same frames under a minimum the link meets
    A.submit_depth(frames, nf, scene=relaxed, rig=rigs, frame=jf, seed=77)
    _, _, rec2, art2, cnt2, _ = A.retire(articulation=True, link_counts=True)
    assert cnt2[1] > 700 and cnt2[0] == cnt[0] and np.isfinite(rec2[1, :, :26]).any()
    assert _bytes(rec2[0], rec[0]) and _bytes(art2[0], art[0])


def test_launch_budget(dev):
    """The annotated step is the xyz build_point_gt step behind ONE more ABI call (two kernel launches), in the order annotate, build, sample;
    a plain depth pipeline and the xyz build_point_gt pipeline issue none of the new calls."""
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_fit_quality_gpu import _launch_names
    pb = _weights()
    A, X = _pipes(pb, "uint16", slots=1)
    on, off = _launch_names(A.prepare()), _launch_names(X.prepare())
    assert on[:3] == ["ancsh_depth_annotate_stream", "ancsh_point_gt_build", "ancsh_input_sample_stream_xyz"] and on[1:] == off
    plain = AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", couple=True, slots=1, niter_a=64, niter_b=8, joint_source="predicted",
                          depth_capacity=CAP_)
    names = _launch_names(plain.prepare())
    assert names[:2] == ["ancsh_depth_unproject_stream", "ancsh_input_sample_stream_xyz"] and "ancsh_depth_annotate_stream" not in names + off


# ---- the paths the option does not touch --------------------------------------------------------------------------------------------------------
def unchanged_streams():
    """A plain depth stream and an xyz build_point_gt stream at small shapes, built from seeded generators only -> {name: records and
    blocks}.  tests/golden/depth_annotate_unchanged.npz holds what the commit before ancsh_depth_annotate_stream returned here."""
    from articulated_pose_amd.depth import unprojection_from_intrinsics
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_point_gt_build_gpu import stream_rig
    pb = _weights()
    kw = dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True)
    out = {}
    rs = np.random.RandomState(53)
    depth = AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", depth_capacity=CAP_, depth_dtype="uint16", **kw)
    batches = []
    for n in (2, 2, 1):
        frames = []
        for _ in range(n):
            h, w = int(rs.randint(34, 44)), int(rs.randint(30, 40))
            frames.append((_depth(rs, h, w, "uint16"), rs.uniform(size=(h, w)) < 0.8, (int(rs.randint(200, 260)), int(rs.randint(200, 260)))))
        batches.append((frames, rs.uniform(0.9, 1.1, n).astype(np.float32)))
    got = list(depth.stream_depth_batches(batches, unprojection_from_intrinsics(300.0, 310.0, 256.0, 250.0), 1e-4, articulation=True))
    out["depth_record"], out["depth_articulation"] = np.concatenate([g[2] for g in got]), np.concatenate([g[3] for g in got])
    out["depth_counts"] = np.concatenate([g[4] for g in got])
    # slot 0 still holds the last batch: the rows the depth front end unprojected and the points the sampler drew from them
    out["depth_rows"], out["depth_P"] = depth.slots[0].raw_rows[:int(got[2][4][0])].cpu().numpy(), depth.slots[0].P.cpu().numpy()
    del depth
    xyz = AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", raw_capacity=CAP_, point_ground_truth=True, build_point_gt=True, **kw)
    batches = []
    for n in (2, 2, 1):
        clouds = []
        for _ in range(n):
            m = int(rs.randint(40, 900))
            clouds.append(np.concatenate([rs.uniform(-0.5, 0.5, (m, 3)), rs.uniform(-0.3, 0.3, (m, 3)), np.sort(rs.randint(0, K_, (m, 1)), axis=0)], 1).astype(np.float32))
        batches.append((clouds, rs.uniform(0.9, 1.1, n).astype(np.float32), rs.normal(size=(n, 13)), np.tile(stream_rig(), (n, 1))))
    got = list(xyz.stream_batches(batches, articulation=True))
    out["xyz_record"], out["xyz_articulation"] = np.concatenate([g[2] for g in got]), np.concatenate([g[3] for g in got])
    out["xyz_rows"], out["xyz_P"] = xyz.slots[0].raw_rows[:batches[2][0][0].shape[0]].cpu().numpy(), xyz.slots[0].P.cpu().numpy()
    return out


def test_untouched_paths_stream_the_parent_commits_bytes(dev):
    want = np.load(os.path.join(HERE, "golden", "depth_annotate_unchanged.npz"))
    got = unchanged_streams()
    assert sorted(got) == sorted(want.files)
    for name in want.files:
        assert _bytes(got[name], want[name]), name
    assert got["depth_record"].shape == (5, K_, 26) and got["xyz_record"].shape == (5, K_, 47) and np.isfinite(got["xyz_record"][:, :, 26:]).any()
    assert got["depth_rows"].shape == (got["depth_counts"][4], 3) and got["xyz_rows"].shape[1] == 18
    assert all(np.isfinite(got[k]).all() for k in ("depth_rows", "depth_P", "xyz_rows", "xyz_P"))
