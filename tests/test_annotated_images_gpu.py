"""GPU: the predicted and ground-truth part / NOCS images of annotated frames -- ancsh_depth_annotated_images against the numpy mirror of its
contract (tests/annotated_images_mirror.py: the inverse of the annotation's stable counting sort), byte for byte over every pixel of every
crop; the round trip through the entries that write its inputs; and AncshPipeline(..., annotated_images=True) on the four annotated-frame
streams against the mirror applied to the eager operators' rows."""
import numpy as np
import pytest
import torch

import annotated_images_mirror as M
from redzone import Arena
from test_depth_annotate_cpu import random_scene, scene_table, valid_depth
from test_depth_annotate_gpu import SCALE, _bytes, _depth

pytestmark = pytest.mark.gpu
UNTOUCHED_L, UNTOUCHED_V = -7, -7.0
LINKS, PARTS_MAP = 4, [[3], [0, 2]]             # link 1 is not used (rank -1); ranks differ from the link indices
SHAPES = [(1, 7), (5, 3), (96, 90)]
STARTS, DESTS = [3, 13, 31], [5, 16, 37]        # crops and images with gaps between them, no start a multiple of 8
PIXELS = 12288


def _frames(rs, dtype):
    """Three frames: 1 x 7 with every link above its minimum of 2; 5 x 3 whose link 3 keeps one pixel under a minimum of 2 (no rows); 96 x 90,
    a per-pixel checkerboard of the four links (every wave interleaves three used links and the unused one) with background bytes (255 and 7,
    which is >= nlinks) and depth holes.  -> (depth crops, label crops, scene tables (3, 240))."""
    crops = [_depth(rs, h, w, dtype) for h, w in SHAPES]
    crops[0][:] = 20000 if dtype == "uint16" else 2.0
    lab0 = np.array([[0, 2, 3, 0, 2, 3, 3]], np.uint8)
    i, j = np.indices(SHAPES[1])
    lab1 = np.array([0, 2, 3], np.uint8)[(i + j) % 3]
    at = np.flatnonzero(lab1.reshape(-1) == 3)
    lab1.reshape(-1)[at[1:]] = 0
    crops[1].reshape(-1)[at[0]] = crops[0][0, 0]                         # link 3's one pixel is valid: one valid pixel, a minimum of two
    i, j = np.indices(SHAPES[2])
    lab2 = ((i + j) % 4).astype(np.uint8)
    u = rs.uniform(size=SHAPES[2])
    lab2[u < 0.04], lab2[(u >= 0.04) & (u < 0.08)] = 255, 7
    tables = np.stack([scene_table(random_scene(rs, LINKS), PARTS_MAP, SCALE[dtype], m) for m in (2, 2, 10)])
    return crops, [lab0, lab1, lab2], tables


def _layout(crops, labels, dtype, clouds):
    """Flat buffers of PIXELS pixels (what lies between and behind the crops looks valid: depth 1, link 0) and the geometry of `clouds` =
    [(frame, dest)]: a cloud beyond the three frames aliases its frame's pixels."""
    pix = np.full(PIXELS, 10000 if dtype == "uint16" else 1.0, np.uint16 if dtype == "uint16" else np.float32)
    lab = np.zeros(PIXELS, np.uint8)
    for c, l, a in zip(crops, labels, STARTS):
        pix[a:a + c.size], lab[a:a + c.size] = c.reshape(-1), l.reshape(-1)
    geom = np.array([(STARTS[f], SHAPES[f][0], SHAPES[f][1], 100 + f, 200 + f) for f, _ in clouds], np.int32)
    return pix, lab, geom, np.array([d for _, d in clouds], np.int32)


def _nan_payloads(rs, a, share=0.1):
    bits = a.view(np.uint32)
    junk = rs.uniform(size=bits.shape) < share
    bits[junk] = (0x7f800001 + rs.randint(0, 0x7ffffe, int(junk.sum()))).astype(np.uint32) | (rs.randint(0, 2, int(junk.sum())).astype(np.uint32) << 31)
    assert np.isnan(a[junk]).all()
    return a


def _rows(rs, cap):
    """Distinct per-row data, so that a wrong row cannot compare equal: labels = a permutation-like ramp, values and ground truth random with
    NaN payloads in a tenth of them; the part column holds integers, a few NaN and Inf."""
    labels = (np.arange(cap, dtype=np.int32) * 7 + 3) % 1000003 - 1
    values = _nan_payloads(rs, rs.normal(size=(cap, 7)).astype(np.float32))
    gt = _nan_payloads(rs, rs.normal(size=(cap, 18)).astype(np.float32))
    gt[:, 3] = rs.randint(0, 3, cap)
    gt[rs.uniform(size=cap) < 0.02, 3] = np.nan
    gt[rs.uniform(size=cap) < 0.02, 3] = np.inf
    return labels, values, gt


def _annotate(dev, pix, lab, geom, tables):
    from articulated_pose_amd.depth import MAX_CHUNKS, depth_annotate
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(pix=t(pix.view(np.int16) if pix.dtype == np.uint16 else pix), lab=t(lab), geom=t(geom), scene=t(tables),
             scratch=torch.zeros((geom.shape[0] * MAX_CHUNKS * 16,), dtype=torch.int32, device=dev))
    d["rows"], d["off"], d["cnt"], _ = depth_annotate(d["pix"], d["lab"], d["geom"], d["scene"], capacity=PIXELS + geom.shape[0], scratch=d["scratch"])
    return d


def _entry(dev, d, dest, labels, values, gt, icap):
    """One call of the entry on redzone-guarded images prefilled with the UNTOUCHED sentinels -> the four images as numpy."""
    from articulated_pose_amd import _lib
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_lab, d_val, d_gt, d_dest = t(labels), t(values), t(gt), t(dest)
    assert _bytes(d_val.cpu().numpy(), values) and _bytes(d_gt.cpu().numpy(), gt)       # the NaN payloads reached the device
    arena = Arena()
    imgs = [arena.empty(s, dtype=dt, device=dev) for s, dt in (((icap,), torch.int32), ((icap, 7), torch.float32), ((icap,), torch.int32),
                                                                ((icap, 6), torch.float32))]
    for im, fill in zip(imgs, (UNTOUCHED_L, UNTOUCHED_V, UNTOUCHED_L, UNTOUCHED_V)):
        im.fill_(fill)
    B = d["geom"].shape[0]
    _lib.call("ancsh_depth_annotated_images", B, 0 if d["pix"].dtype == torch.int16 else 1, _lib.ptr(d["pix"]), _lib.ptr(d["lab"]), PIXELS,
              _lib.ptr(d["geom"]), _lib.ptr(d["scene"]), _lib.ptr(d["off"]), _lib.ptr(d["cnt"]), _lib.ptr(d["scratch"]), _lib.ptr(d_lab),
              _lib.ptr(d_val), _lib.ptr(d_gt), gt.shape[1], labels.shape[0], _lib.ptr(d_dest), *(_lib.ptr(im) for im in imgs), icap)
    torch.cuda.synchronize()
    out = [im.cpu().numpy() for im in imgs]
    arena.check()
    return out


def _compare(got, want, what):
    for name, g, w in zip(("labels", "values", "gt_labels", "gt_values"), got, want):
        bad = np.flatnonzero((g.view(np.int32) != w.view(np.int32)).reshape(g.shape[0], -1).any(1))
        assert g.shape == w.shape and bad.size == 0, (what, name, bad[:8], g[bad[:4]], w[bad[:4]])


@pytest.mark.parametrize("chunks", [2, 1])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_operator_equals_the_mirror(dev, dtype, chunks):
    """chunks = 2: three frames and one silenced padding cloud on frame 0's pixels in 12288 pixels -- the 96 x 90 crop's chunks run several
    256-thread steps and its rows cross the chunk boundary.  chunks = 1: the same frames with three silenced clouds, 2048 pixels a cloud.  The
    row capacity ends 37 rows inside the last frame."""
    from articulated_pose_amd.depth import depth_annotated_images
    rs = np.random.RandomState(11 + len(dtype))
    crops, labs, tables = _frames(rs, dtype)
    clouds = [(0, DESTS[0]), (1, DESTS[1]), (2, DESTS[2])] + ([(0, -1)] if chunks == 2 else [(0, -1), (2, -3), (2, -1)])
    assert (PIXELS // len(clouds) + 2047) // 2048 == chunks
    pix, lab, geom, dest = _layout(crops, labs, dtype, clouds)
    scenes = tables[[f for f, _ in clouds]]
    d = _annotate(dev, pix, lab, geom, scenes)
    cnt, off, _ = M.batch_offsets(pix, lab, geom, scenes)
    assert np.array_equal(d["cnt"].cpu().numpy(), cnt) and np.array_equal(d["off"].cpu().numpy(), off)
    assert cnt[0] == 7 and cnt[1] == 0 and cnt[2] > 5000 and off[3] - off[2] == cnt[2]
    capacity = int(off[3]) - 37
    icap = DESTS[2] + 96 * 90 + 11
    labels, values, gt = _rows(rs, capacity)
    got = _entry(dev, d, dest, labels, values, gt, icap)
    again = _entry(dev, d, dest, labels, values, gt, icap)
    want = M.expected(pix, lab, geom, scenes, dest, labels, values, gt, capacity, icap, (UNTOUCHED_L, UNTOUCHED_V))
    _compare(got, want[:4], (dtype, chunks))
    _compare(again, got, (dtype, chunks, "a pure function of the input"))
    il, iv, igl, igv = got
    covered = np.zeros(icap, bool)
    for d0, (h, w) in zip(DESTS, SHAPES):
        covered[d0:d0 + h * w] = True
    assert (~covered).sum() > 20 and (il[~covered] == UNTOUCHED_L).all() and (igl[~covered] == UNTOUCHED_L).all()
    assert (iv[~covered] == UNTOUCHED_V).all() and (igv[~covered] == UNTOUCHED_V).all()
    # the frame below its minimum: background everywhere
    a, e = DESTS[1], DESTS[1] + 15
    assert (il[a:e] == -1).all() and (igl[a:e] == -1).all() and (iv[a:e].view(np.uint32) == M.NAN_BITS).all() and (igv[a:e].view(np.uint32) == M.NAN_BITS).all()
    # the rows cut at capacity: the last 37 valid pixels of the last link in rank order read background, the row in front of them does not
    big = il[DESTS[2]:DESTS[2] + 96 * 90].reshape(96, 90)
    last = np.argwhere((labs[2] == 2) & valid_depth(crops[2]))
    assert (big[last[-37:, 0], last[-37:, 1]] == -1).all() and big[last[-38, 0], last[-38, 1]] == labels[capacity - 1]
    assert (igl[covered] == -1).sum() > (il[covered] == -1).sum()        # a non-finite part reads -1
    # a cloud whose images would pass image_capacity writes nothing; the others are unaffected
    short = _entry(dev, d, dest, labels, values, gt, icap - 12)
    _compare(short, M.expected(pix, lab, geom, scenes, dest, labels, values, gt, capacity, icap - 12, (UNTOUCHED_L, UNTOUCHED_V))[:4], "image cut")
    assert (short[0][DESTS[2]:] == UNTOUCHED_L).all() and (short[0][DESTS[0]:DESTS[0] + 7] >= 0).all()
    # the host wrapper: the same images; its own prefill where no crop lies
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = depth_annotated_images(d["pix"], d["lab"], d["geom"], d["scene"], t(dest), d["off"], d["cnt"], t(labels), t(values), t(gt), scratch=d["scratch"])
    assert [tuple(o.shape) for o in out] == [(PIXELS,), (PIXELS, 7), (PIXELS,), (PIXELS, 6)]
    for o, g in zip(out, got):
        o = o.cpu().numpy()
        assert _bytes(o[:icap][covered], g[covered])
        assert (o[:icap][~covered] == -1).all() if o.dtype == np.int32 else np.isnan(o[:icap][~covered]).all()
    with pytest.raises(ValueError, match="scratch"):
        depth_annotated_images(d["pix"], d["lab"], d["geom"], d["scene"], t(dest), d["off"], d["cnt"], t(labels), t(values), t(gt))


# ---- the entries that write its inputs -------------------------------------------------------------------------------------------------------------
K_, N_ = 3, 64


def _eager_rows(dev, frames, scenes, rigs, nf, dtype, P, npcs, ancsh):
    """The eager operators on one batch of frames: depth_annotate, point_gt_build and raw_point_labels (from the sampled points P and the
    two networks' heads) -> (label crops as the device read them, scenes, per-row labels, values, 18-column rows, offsets, counts, capacity)."""
    from articulated_pose_amd import dataset, depth as D
    n = len(frames)
    depths, labels, origins, _, scenes = D.check_annotated_frames(frames, np.ones(n), scenes, dtype, K_)
    total = sum(d.size for d in depths)
    pix, lab, geom = np.zeros(total, D.DEPTH_DTYPES[dtype][0]), np.full(total, D.NOT_OBJECT, np.uint8), np.zeros((n, D.GEOM_WORDS), np.int32)
    D.pack_depth_frames(depths, labels, origins, pix, lab, geom)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cap = total + n
    rows7, off, cnt, _ = D.depth_annotate(t(pix.view(np.int16) if dtype == "uint16" else pix), t(lab), t(geom), t(scenes), capacity=cap)
    rows18 = dataset.point_gt_build(rows7, off, t(np.asarray(rigs, np.float64)), K_, torch.zeros((cap, dataset.NCHAN), dtype=torch.float32, device=dev))
    rl, rv = dataset.raw_point_labels(rows18, off, np.asarray(nf, np.float32), P, npcs, ancsh)
    return labels, scenes, rl.cpu().numpy(), rv.cpu().numpy(), rows18.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy(), cap


def _mirror_images(frames, eager):
    labels, scenes, rl, rv, rows18, off, cnt, cap = eager
    out = []
    for b, ((d, _, _), lab) in enumerate(zip(frames, labels)):
        rows, n = M.pixel_rows(np.asarray(d), lab, scenes[b])
        assert n == cnt[b], b
        out.append(M.frame_images(rows, int(off[b]), rl, rv, rows18, cap))
    return out


def _compare_frames(got, want, what):
    assert isinstance(got, list) and len(got) == len(want), (what, len(got), len(want))
    for f, (g, w) in enumerate(zip(got, want)):
        assert len(g) == 4 and [a.dtype for a in g] == [np.int32, np.float32, np.int32, np.float32], (what, f)
        for name, a, b in zip(("labels", "values", "gt_labels", "gt_values"), g, w):
            assert _bytes(a, b), (what, f, name, np.argwhere(a.view(np.int32) != b.view(np.int32))[:6])


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_round_trip_through_the_entries_that_write_its_inputs(dev, dtype):
    """depth.annotated_frame_images on the operator test's frames: the entry is fed what ancsh_depth_annotate_stream, ancsh_point_gt_build
    and ancsh_raw_point_labels wrote.  At every valid pixel the ground-truth part is the scene's part of the pixel's link label, whatever
    the row order; the ground-truth values are columns 4..9 of the pixel's row; the predictions are raw_point_labels' for that row."""
    from articulated_pose_amd.depth import annotated_frame_images
    from test_point_gt_build_gpu import stream_rig
    rs = np.random.RandomState(3)
    crops, labs, tables = _frames(rs, dtype)
    frames = [(c, l, (100 + f, 200 + f)) for f, (c, l) in enumerate(zip(crops, labs))]
    rigs, nf = np.tile(stream_rig(), (3, 1)), np.array([1.0, 0.9, 1.1], np.float32)
    P = torch.from_numpy(rs.uniform(-0.5, 0.5, (3, N_, 3)).astype(np.float32)).to(dev)
    head = lambda c: torch.from_numpy(rs.uniform(0, 1, (3, N_, c)).astype(np.float32)).to(dev)
    npcs, ancsh = dict(W=head(K_), nocs_per_point=head(3 * K_)), dict(gocs_per_point=head(3 * K_))
    got = annotated_frame_images(frames, tables, rigs, dtype, K_, nf, P, npcs, ancsh, dev)
    eager = _eager_rows(dev, frames, tables, rigs, nf, dtype, P, npcs, ancsh)
    _compare_frames(got, _mirror_images(frames, eager), dtype)
    part_of = {l: int(tables[0][M.SCENE_HEAD + M.SCENE_LINK * l + 1]) for l in M.link_order(tables[0])}
    assert part_of == {3: 0, 0: 1, 2: 1}
    for f, ((d, l, _), (il, iv, igl, igv)) in enumerate(zip(frames, got)):
        valid = np.isin(l, list(part_of)) & valid_depth(d) & (f != 1)    # frame 1 is below its minimum
        assert (igl[~valid] == -1).all() and (il[~valid] == -1).all() and (igv[~valid].view(np.uint32) == M.NAN_BITS).all()
        assert np.array_equal(igl[valid], np.array([part_of.get(v, -1) for v in l.reshape(-1)]).reshape(l.shape)[valid]), f
        assert np.isfinite(igv[valid]).all() and (il[valid] >= 0).all() and np.isfinite(iv[valid]).all(), f
    assert (got[1][2] == -1).all() and (got[2][2] >= 0).sum() > 5000
    none = annotated_frame_images(frames, tables, rigs, dtype, K_, device=dev)      # no predictions: only the ground truth
    for (il, iv, igl, igv), g in zip(none, got):
        assert (il == -1).all() and np.isnan(iv).all() and _bytes(igl, g[2]) and _bytes(igv, g[3])


# ---- the streams -----------------------------------------------------------------------------------------------------------------------------------
B_, CAP_, SIZES = 3, 3 * 64 * 64, (3, 2, 3)     # two slots: slot 0 replays batches 0 and 2, and batch 1 is short (one padding frame)


def _pipes(dtype, **kw):
    """(the pipeline with annotated_images=True, the same pipeline without it)."""
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_render_gpu import _weights
    pb = _weights()
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype), **kw)
    mk = lambda **more: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **more))
    return mk(annotated_images=True), mk()


def _depth_feed(dev, dtype, rs):
    """Annotated frames as submit_depth takes them; frame 1 of the last batch is below its minimum."""
    from test_depth_annotate_gpu import _batch
    feed, eager = [], []
    for k, n in enumerate(SIZES):
        frames, nf, tables, rigs, jf = _batch(rs, dtype, n, starve=k == 2)
        feed.append((frames, nf, "t%d" % k, dict(scene=tables, rig=rigs, frame=jf)))
        eager.append((frames, tables, rigs, nf))
    return feed, eager, {}


def _posed_feed(dev, dtype, rs, kind):
    """Frames the step renders itself: kind = "render" (tables and fixed origins travel in), "posed" (poses and centred crops) or "library"
    (posed, two instances mixed inside a batch).  The eager frames are rendered with the same tables at the origins centre_crops returns."""
    from articulated_pose_amd.depth import centre_crops, pack_mesh_library, pack_pose, pose_scene_tables, render_depth_frames
    from test_mesh_library_gpu import _stream_library
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    from test_render_cpu import object_scene
    meshes, kins, _ = _stream_library(rs, dtype)
    ninst = 2 if kind == "library" else 1
    feed, eager = [], []
    for k, n in enumerate(SIZES):
        sizes = [(int(rs.randint(50, 61)), int(rs.randint(50, 61))) for _ in range(n)]
        which = [(k + f) % ninst for f in range(n)]
        poses, rts, scs, frames, crops = [], [], [], [], []
        for f, i in enumerate(which):
            q, V = [0.0, rs.uniform(0.2, 1.1), rs.uniform(-0.03, 0.03)], object_scene(rs, 3)["viewMat"]
            poses.append(pack_pose(q, V, instance=i))
            rt, sc = pose_scene_tables(kins[i], np.stack([pack_pose(q, V)]), dev)
            origin = tuple(int(v) for v in centre_crops(meshes[i], rt, [sizes[f]], dev)[0])
            frames += render_depth_frames(meshes[i], rt, [sizes[f] + (origin,)], dtype, dev)
            crops.append(sizes[f] + (origin,))
            rts.append(rt[0]), scs.append(sc[0])
        nf, rigs, jf = rs.uniform(0.9, 1.1, n).astype(np.float32), np.tile(stream_rig(), (n, 1)), random_frames(rs, n)
        if kind == "render":
            feed.append((crops, nf, dict(render=np.stack(rts), scene=np.stack(scs), rig=rigs, frame=jf), "t%d" % k))
        else:
            feed.append(([(h, w, None) for h, w in sizes], nf, dict(pose=np.stack(poses), rig=rigs, frame=jf), "t%d" % k))
        eager.append((frames, np.stack(scs), rigs, nf))
    if kind == "library":
        return feed, eager, dict(render_mesh=pack_mesh_library(meshes[:2]), kinematics=kins[:2])
    return feed, eager, dict(render_mesh=meshes[0], **(dict(kinematics=kins[0]) if kind == "posed" else {}))


METHOD = dict(depth="stream_depth_batches", render="stream_render_batches", posed="stream_posed_batches", library="stream_posed_batches")


@pytest.mark.parametrize("kind,dtype,guard", [("depth", "uint16", False), ("depth", "float32", True), ("render", "uint16", False),
                                              ("posed", "float32", False), ("library", "uint16", False)],
                         ids=["depth", "depth-range-guard", "render", "posed", "library"])
def test_stream_images_equal_the_mirror_of_the_eager_rows(dev, kind, dtype, guard):
    """Three batches through two slots (slot 0 is replayed with other frames; batch 1 is short).  For every batch the images equal the mirror
    applied to the eager operators' rows for the same frames -- raw_point_labels fed the slot's sampled points and the step's own heads --, and
    the records, articulation blocks, counts and link counts are byte-equal to the same pipeline built without the option.  guard: cloud 0 of
    batch 1 is beyond f16's range, and its images are the f32 graph's."""
    from articulated_pose_amd.stream import unpack_results
    rs = np.random.RandomState(17 + len(kind))
    feed, eager, more = _depth_feed(dev, dtype, rs) if kind == "depth" else _posed_feed(dev, dtype, rs, kind)
    if guard:
        more = dict(more, arithmetic="f16x2", range_guard=True)
        feed[1][1][0] = 1e6
    pipe, plain = _pipes(dtype, **more)
    sl = pipe.slots[0]
    assert [tuple(t.shape) for t in sl.aimg] == [(CAP_,), (CAP_, 7), (CAP_,), (CAP_, 6)] and sl.rowlab[1].shape == (CAP_, 7) and sl.img is None
    assert all(h.is_pinned() for h in sl.outputs["annotated_images"].host) and (sl.aimg32 is not None) == guard
    assert plain.slots[0].aimg is None and plain.slots[0].rowlab is None and plain.slots[0].hdr.numel() == sl.hdr.numel() - B_
    asked = dict(flags=True, articulation=True, counts=True, link_counts=True)
    want = list(getattr(plain, METHOD[kind])(feed, flags=True, articulation=True, link_counts=True))
    seen = 0
    for k, g in enumerate(getattr(pipe, METHOD[kind])(feed, flags=True, articulation=True, link_counts=True, annotated_images=True)):
        r, w = unpack_results(g, annotated_images=True, **asked), unpack_results(want[k], **asked)
        assert len(g) == len(want[k]) + 1 == 8 and r["tag"] == w["tag"] == "t%d" % k and r["seed"] == w["seed"], k
        for name in ("record", "flags", "articulation", "counts", "link_counts"):
            assert _bytes(r[name], w[name]), (kind, k, name)
        frames, scenes, rigs, nf = eager[k]
        n = len(frames)
        assert len(r["annotated_images"]) == n == SIZES[k] and all(im[0].shape == np.shape(f[0]) for im, f in zip(r["annotated_images"], frames))
        s = pipe.slots[k % 2]                                            # still holds batch k: the other slot took batch k + 1
        expect = {}
        for f32 in ([False, True] if r["flags"].any() else [False]):
            out = s.pick("out", f32)
            heads = [{h: v[:n].contiguous() for h, v in out[net].items() if h in ("W", "nocs_per_point", "gocs_per_point")} for net in ("npcs", "ancsh")]
            rows = _eager_rows(dev, frames, scenes, rigs, feed[k][1], dtype, s.P[:n].contiguous(), heads[0], heads[1])
            assert np.array_equal(rows[6], r["counts"]), (kind, k)
            expect[f32] = _mirror_images(frames, rows)
        _compare_frames(r["annotated_images"], [expect[bool(flag)][c] for c, flag in enumerate(r["flags"])], (kind, k))
        for c, (il, iv, igl, igv) in enumerate(r["annotated_images"]):
            if r["counts"][c]:
                assert (igl >= 0).sum() == r["counts"][c] and (il >= 0).sum() > 0.9 * r["counts"][c], (kind, k, c)
            else:
                assert (igl == -1).all() and (il == -1).all() and np.isnan(r["record"][c]).all(), (kind, k, c)
        seen += 1
    assert seen == len(SIZES) and (r["counts"] > 300).any()
    if kind == "depth":
        assert (r["counts"][1] == 0) and r["link_counts"][1, 3] == 5     # the frame below its minimum came through the stream
    if guard:
        assert pipe.f32_reruns == plain.f32_reruns == 1
    # retire() without the option's keyword returns the tuple it always did; a pipeline without the option refuses the keyword
    submit = dict(depth="submit_depth", render="submit_render", posed="submit_posed", library="submit_posed")[kind]
    item = feed[0]
    args, side = (item[0], item[1]), item[3] if kind == "depth" else item[2]
    getattr(pipe, submit)(*args, **side)
    assert len(pipe.retire()) == 4
    with pytest.raises(RuntimeError, match="annotated_images=True"):
        plain.retire(annotated_images=True)


def test_launch_budget(dev):
    """The annotated_images=True step is the annotated depth step's sequence followed by ancsh_raw_point_labels, ancsh_depth_annotated_images
    and nothing else; nothing between the annotation and the new entry names the slot's scratch."""
    from test_fit_quality_gpu import _launch_names
    pipe, plain = _pipes("uint16", slots=1)
    on, off = _launch_names(pipe.prepare()), _launch_names(plain.prepare())
    assert off[0] == "ancsh_depth_annotate_stream" and "ancsh_raw_point_labels" not in off and "ancsh_depth_annotated_images" not in off
    assert on == off + ["ancsh_raw_point_labels", "ancsh_depth_annotated_images"]
