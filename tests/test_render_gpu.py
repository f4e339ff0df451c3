"""GPU: ancsh_render_depth_labels against its numpy mirror (tests/render_mirror.py, validated on its own in tests/test_render_cpu.py), byte
for byte and inside red zones; the round trip through ancsh_depth_annotate_stream back onto the boxes' surfaces; and
AncshPipeline(render_mesh=...) against the annotated depth pipeline fed the eager renderer's frames."""
import numpy as np
import pytest
import torch

import render_mirror as RM
from redzone import Arena
from test_depth_annotate_cpu import link_matrices, scene_table
from test_render_cpu import BOX_HI, BOX_LO, box_mesh, object_mesh, object_scene, pinhole_table, render_table

pytestmark = pytest.mark.gpu
DTYPES = {"uint16": np.uint16, "float32": np.float32}
FILL = {"uint16": 0x5A5A, "float32": -7.0}
LABEL_FILL = 77


def _bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _operator(dev, mesh, geom, tables, cap, dtype):
    """One call of the entry on redzone-guarded outputs prefilled with sentinels -> (depth (cap,), labels (cap,)) as numpy arrays."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import mesh_to_device
    verts, tris, tri_link, V, T = mesh_to_device(mesh, dev)
    geom, tables = np.ascontiguousarray(geom, np.int32).reshape(-1, 5), np.ascontiguousarray(tables, np.float64).reshape(-1, RM.RENDER_WIDTH)
    arena = Arena()
    depth = arena.empty((cap,), dtype=torch.int16 if dtype == "uint16" else torch.float32, device=dev)
    labels = arena.empty((cap,), dtype=torch.uint8, device=dev)
    zbuf = arena.empty((cap,), dtype=torch.int64, device=dev)
    depth.copy_(torch.from_numpy(np.full(cap, FILL[dtype], DTYPES[dtype]).view(np.int16 if dtype == "uint16" else np.float32)))
    labels.fill_(LABEL_FILL)
    d_geom, d_tables = torch.from_numpy(geom).to(dev), torch.from_numpy(tables).to(dev)
    _lib.call("ancsh_render_depth_labels", geom.shape[0], 0 if dtype == "uint16" else 1, _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(tri_link), V, T,
              _lib.ptr(d_geom), _lib.ptr(d_tables), _lib.ptr(depth), _lib.ptr(labels), _lib.ptr(zbuf), cap)
    torch.cuda.synchronize()
    out = depth.cpu().numpy().view(DTYPES[dtype]), labels.cpu().numpy()
    arena.check()
    return out


def check_against_mirror(dev, mesh, geom, tables, cap, dtype, what):
    """The entry's buffers equal the mirror's, byte for byte, twice (a pure function of its input) -> (depth, labels)."""
    want = RM.render_flat(mesh[0], mesh[1], mesh[2], geom, np.asarray(tables, np.float64).reshape(-1, RM.RENDER_WIDTH), cap, DTYPES[dtype], FILL[dtype], LABEL_FILL)
    got = _operator(dev, mesh, geom, tables, cap, dtype)
    for name, g, w in zip(("depth", "labels"), got, want):
        assert _bytes(g, w), (what, name, int((g != w).sum()), np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
    again = _operator(dev, mesh, geom, tables, cap, dtype)
    assert _bytes(again[0], got[0]) and _bytes(again[1], got[1]), what
    return got


def _posed_tables(rs, n, L, depth_scale):
    """n render tables of an L-link object under general (non-dyadic) views."""
    return np.stack([render_table(object_scene(rs, L), depth_scale) for _ in range(n)])


RAGGED = [(17, 23, (20, 18)), (1, 64, (31, 0)), (64, 1, (0, 29))]       # (h, w, (row0, col0)) inside the 64 x 64 image, each across the object


def _ragged_geom(crops, first=3, gap=5):
    """Crops at unaligned starts with gaps between them -> (geom, the pixel behind the last crop)."""
    geom, a = [], first
    for h, w, (r0, c0) in crops:
        geom.append((a, h, w, r0, c0))
        a += h * w + gap
    return np.asarray(geom, np.int32), a


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("links", [1, 2])
def test_ragged_crops_of_posed_objects_equal_the_mirror(dev, dtype, links):
    """One box (12 triangles) and the two-link object at an opened joint (24), one frame and three frames of ragged crops at unaligned
    starts with gaps: the gaps and the pixels around the crops keep their sentinels."""
    rs = np.random.RandomState(links)
    mesh = object_mesh(links)
    assert mesh[1].shape == (12 * links, 3)
    scale = 1e-3 if dtype == "uint16" else 1.0
    for crops in (RAGGED[:1], RAGGED):
        geom, end = _ragged_geom(crops)
        depth, labels = check_against_mirror(dev, mesh, geom, _posed_tables(rs, len(crops), links, scale), end + 7, dtype, (dtype, links, len(crops)))
        inside = np.zeros(end + 7, bool)
        for a, h, w, _, _ in geom:
            inside[a:a + h * w] = True
        assert (labels[~inside] == LABEL_FILL).all() and (labels[inside] != LABEL_FILL).all()
        assert set(np.unique(labels[inside])) == set(range(links)) | {255}                      # every link and the background show


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_full_image_and_a_box_across_its_border(dev, dtype):
    """A full 64 x 64 crop (two chunks of more than one block's step) of a box that reaches past the left and the upper border of the image,
    and a crop that cuts the same box: triangles partly outside the crop and partly outside the image."""
    v, f = box_mesh(BOX_LO, BOX_HI)
    mesh = (v.astype(np.float32), f.astype(np.int32), np.zeros(12, np.int32))
    c, s = np.cos(0.5), np.sin(0.5)
    R = np.array([[c, 0, s, -0.55], [0.1, 1, 0, -0.5], [-s, 0, c, 1.3]])
    rt = pinhole_table(70.3, 69.1, 31.7, 30.2, [R], 1e-3 if dtype == "uint16" else 1.0)
    geom = np.array([(0, 64, 64, 0, 0), (4096 + 11, 20, 30, 0, 0)], np.int32)
    depth, labels = check_against_mirror(dev, mesh, geom, np.stack([rt, rt]), 4096 + 11 + 600 + 5, dtype, dtype)
    img = labels[:4096].reshape(64, 64)
    assert (img[0] == 0).any() and (img[:, 0] == 0).any() and (img == 0).sum() > 100 and (img[:, 40:] == 255).all()
    assert _bytes(labels[4107:4707].reshape(20, 30), img[:20, :30]) and _bytes(depth[4107:4707].reshape(20, 30), depth[:4096].reshape(64, 64)[:20, :30])


def _special_mesh():
    """Hand-made triangles at depths 1, 2 and 100 under col = 32 x + 32, row = 32 y + 32 (both links: the identity map):
    0: a right triangle of link 0 whose hypotenuse passes exactly through sample points; 1: the same triangle, link 1 (coplanar: the lower
    index wins); 2: one vertex behind z_min (dropped whole); 3: zero area; 4: a nearer sliver of link 1 over part of triangle 0;
    5: a far triangle of link 1 (z = 100); 6: a very near one of link 0 (z = 0.0004)."""
    v = np.array([(0, 0, 1), (0.5, 0, 1), (0, 0.5, 1),                  # 0 1 2
                  (-0.5, -0.5, 1), (0, -0.5, 1), (-0.5, 0.25, -1),      # 3 4 5
                  (-0.75, -0.75, 1), (-0.5, -0.5, 1), (-0.25, -0.25, 1),      # 6 7 8
                  (0.1, 0.05, 0.5), (0.15, 0.05, 0.5), (0.1, 0.15, 0.5),      # 9 10 11
                  (-50, 10, 100), (-20, 10, 100), (-50, 60, 100),       # 12 13 14
                  (-0.0002, 0.0001, 0.0004), (-0.0001, 0.0001, 0.0004), (-0.0002, 0.0003, 0.0004)], np.float32)      # 15 16 17
    tris = np.array([(0, 1, 2), (2, 1, 0), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17)], np.int32)
    return v, tris, np.array([0, 1, 0, 0, 1, 1, 0], np.int32)


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_rules_on_hand_made_triangles(dev, dtype):
    """The edge rule, the tie rule, the drop rules, the quantisation limits, a frame whose nlinks is 0 and a crop that would pass
    pixel_capacity -- each against the mirror, and the rule itself spelled out on the mirror's pixels."""
    mesh = _special_mesh()
    I = np.eye(4)[:3]
    # depth_scale 0.001: z = 0.0004 quantises to 0 (not written), z = 100 to 100000 > 65535 (not written), z = 1 to 1000
    rt = pinhole_table(32.0, 32.0, 32.0, 32.0, [I, I], 1e-3 if dtype == "uint16" else 1.0)
    none = rt.copy()
    none[8] = 0                                                         # nlinks 0: an all-background crop
    one = rt.copy()
    one[8] = 1                                                          # link 1's triangles are dropped
    cap = 3 * 4096 + 100
    geom = np.array([(0, 64, 64, 0, 0), (4096, 64, 64, 0, 0), (8192, 64, 64, 0, 0), (cap - 50, 8, 8, 30, 30), (-1, 8, 8, 30, 30), (0, 0, 8, 30, 30)], np.int32)
    depth, labels = check_against_mirror(dev, mesh, geom, np.stack([rt, none, one, rt, rt, rt]), cap, dtype, dtype)
    img, d = labels[:4096].reshape(64, 64), depth[:4096].reshape(64, 64)
    assert all(img[32 + k, 48 - k] == 0 for k in range(17)) and img[33, 48] == 255      # on the hypotenuse: covered; one pixel beyond: not
    assert img[40, 36] == 0 and img[37, 40] == 1 and d[37, 40] == (500 if dtype == "uint16" else 0.5)      # tie: triangle 0; the nearer sliver wins
    assert (img[:32, :32] == 255).all()                                # neither the triangle with a vertex behind z_min nor the degenerate one shows
    far, near = d[32:, :32] > 99.99, (d[32:, :32] > 0) & (d[32:, :32] < 0.001)
    if dtype == "float32":                                              # float32 keeps both extremes, the near one in front
        assert far.sum() > 20 and near.sum() > 50 and (img[32:, :32][far] == 1).all() and (img[32:, :32][near] == 0).all() and near[10, 17]
    else:                                                               # uint16: one quantises to 0, the other beyond 65535
        assert (img[32:, :32] == 255).all() and (d[img == 255] == 0).all() and (d[img != 255] >= 1).all() and d.max() == 1000
    assert (labels[4096:8192] == 255).all() and (depth[4096:8192] == 0).all()
    assert (labels[8192:3 * 4096] != 1).all() and (labels[8192:3 * 4096] == 0).sum() > 100
    assert (labels[3 * 4096:] == LABEL_FILL).all()                      # the crops outside the buffers wrote nothing
    # T == 0 renders background
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0,), np.int32))
    depth, labels = check_against_mirror(dev, empty, geom[:1], rt[None], 4096, dtype, "T == 0")
    assert (labels == 255).all() and (depth == 0).all()


# ---- the round trip ---------------------------------------------------------------------------------------------------------------------------
def _surface_distance(p, lo, hi):
    """Distance of the points p (n, 3) to the surface of the box [lo, hi]."""
    out = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.minimum(p - lo, hi - p).min(1)
    return np.where(inside > 0, inside, out)


@pytest.mark.parametrize("dtype,scale", [("uint16", 1e-3), ("float32", 1.0)])
def test_round_trip_through_the_annotation_lands_on_the_boxes(dev, dtype, scale):
    """Render the two-link object, annotate the frames: link_counts is the mirror's label histogram, and every row's coordinates, taken back
    into the link's model frame, lie on its box within (depth_scale / 2) max |(s, t, 1)| over the image corners -- the quantisation of z
    along the ray (float32 frames: the same formula) -- plus 4 * 2^-24 max |c|, the float32 rounding of the row."""
    from articulated_pose_amd.depth import annotate_depth_batch, render_depth_frames
    rs = np.random.RandomState(9)
    mesh, parts_map, K = object_mesh(2), [[0], [1]], 2
    scenes_S = [object_scene(rs, 2, opening=o) for o in (0.6, 1.1, 0.2)]
    crops = [(64, 64, (0, 0)), (40, 64, (12, 0)), (64, 64, (0, 0))]
    tables = np.stack([render_table(S, scale) for S in scenes_S])
    frames = render_depth_frames(mesh, tables, crops, dtype, dev)
    assert [f[0].shape for f in frames] == [(64, 64), (40, 64), (64, 64)] and [f[2] for f in frames] == [(0, 0), (12, 0), (0, 0)]
    scenes = np.stack([scene_table(S, parts_map, scale) for S in scenes_S])
    rows, off, cnt, lc = annotate_depth_batch(frames, scenes, dtype, K)
    for b, (S, (h, w, (r0, c0))) in enumerate(zip(scenes_S, crops)):
        d, lab, _ = RM.render_crop(mesh[0], mesh[1], mesh[2], h, w, r0, c0, tables[b], DTYPES[dtype])
        assert _bytes(frames[b][0], d) and _bytes(frames[b][1], lab), b
        hist = np.bincount(lab.reshape(-1), minlength=256)
        assert lc[b].tolist() == hist[:2].tolist() + [0] * 14 and cnt[b] == hist[:2].sum() and (hist[:2] > 100).all(), (b, lc[b], hist[:2])
        got = rows[off[b]:off[b] + cnt[b]].astype(np.float64)
        sc = scenes[b]
        corners = np.array([[(sc[7] * c + sc[8] * r) + sc[9], (sc[10] * c + sc[11] * r) + sc[12], 1.0] for r in (0, 63) for c in (0, 63)])
        bound = scale / 2 * np.linalg.norm(corners, axis=1).max() + 4 * 2.0 ** -24 * np.abs(got[:, 3:6]).max()
        _, canon2urdf = link_matrices(S)
        for l in range(2):
            c = got[got[:, 6] == l, 3:6]
            model = (c - canon2urdf[l][:3, 3]) @ canon2urdf[l][:3, :3]    # canon2urdf is rigid: its inverse keeps distances
            dist = _surface_distance(model, BOX_LO.astype(np.float32).astype(np.float64), BOX_HI.astype(np.float32).astype(np.float64))
            print("%s frame %d link %d: %d rows, worst distance / bound = %.3f (bound %.3g)" % (dtype, b, l, len(c), dist.max() / bound, bound))
            assert len(c) == hist[l] and dist.max() <= bound, (dtype, b, l, dist.max(), bound)


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------
K_, B_, N_, CAP_, LINKS_ = 3, 2, 64, 8192, 3
MAP_ = [[0], [2], [1]]
SCALE = {"uint16": 1e-3, "float32": 1.0}


def _weights():
    from articulated_pose_amd.weights import synthetic_weights
    return dict(w_ancsh=synthetic_weights(K_, seed=0), w_npcs=synthetic_weights(K_, mixed_pred=False, early_split_nocs=False, seed=1))


def _batch(rs, dtype, n, starve=False):
    """-> (crops, norm factors, render tables, scene tables, rigs, joint frames) of one batch of n frames; starve: frame 0's crop leaves
    link 2 (on the left of the image) fewer pixels than the scene's minimum."""
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    S = [object_scene(rs, LINKS_) for _ in range(n)]
    crops = [(int(rs.randint(56, 65)), int(rs.randint(56, 65)), (int(rs.randint(0, 3)), int(rs.randint(0, 3)))) for _ in range(n)]
    if starve:
        crops[0] = (60, 42, (2, 22))
    return (crops, rs.uniform(0.9, 1.1, n).astype(np.float32), np.stack([render_table(s, SCALE[dtype]) for s in S]),
            np.stack([scene_table(s, MAP_, SCALE[dtype]) for s in S]), np.tile(stream_rig(), (n, 1)), random_frames(rs, n))


def _pipes(pb, dtype, mesh, **kw):
    """(the rendering pipeline, the annotated depth pipeline) with the same arguments otherwise."""
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=4, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype), **kw)
    mk = lambda **more: AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **dict(kw, **more))
    return mk(render_mesh=mesh), mk()


@pytest.mark.parametrize("dtype,slots,options", [("uint16", 1, {}), ("float32", 4, {}), ("uint16", 4, dict(ground_truth=True, build_gt_pose=True)),
                                                 ("uint16", 4, dict(keyed=True)),
                                                 ("uint16", 2, dict(range_guard=True, arithmetic="f16x2", fit_quality=True, joint_states=True,
                                                                    joint_types=["revolute", "prismatic"]))],
                         ids=["u16-1slot", "f32-4slots", "gt-pose", "keyed", "guard-quality-states-types"])
def test_rendered_stream_equals_the_annotated_depth_stream(dev, dtype, slots, options):
    """Ten batches, one of them short and one with a frame whose link 2 shows fewer pixels than the minimum (plain, with the ground-truth
    poses built in the step, keyed, and under the range guard with the wide record, joint states and a prismatic joint): records, counts and link counts
    of stream_render_batches equal, byte for byte, those of stream_depth_batches fed depth.render_depth_frames' output for the same tables.
    One graph per slot serves every batch, and no pixel staging exists on the rendering pipeline."""
    from articulated_pose_amd.depth import render_depth_frames
    from articulated_pose_amd.pose.gt_errors import pack_box_extents
    pb, mesh = _weights(), object_mesh(LINKS_)
    rs = np.random.RandomState(3)
    batches = [_batch(rs, dtype, 1 if k == 2 else 2, starve=(k == 5)) for k in range(10)]
    R, A = _pipes(pb, dtype, mesh, slots=slots, **options)
    R.prepare()
    sl = R.slots[0]
    assert sl.h_pix is None and sl.h_mask is None and sl.zbuf.shape == (CAP_,) and sl.zbuf.dtype == torch.int64 and sl.render.shape == (B_, 208)
    assert all(s.zbuf.data_ptr() != sl.zbuf.data_ptr() for s in R.slots[1:]) and R.mesh[3:] == (24, 36) and A.mesh is None
    graphs = [s.graph for s in R.slots]
    feed_r, feed_a = [], []
    for k, (crops, nf, rt, sc, rigs, jf) in enumerate(batches):
        side = dict(scene=sc, rig=rigs)
        if options.get("build_gt_pose"):
            side["gt"] = pack_box_extents([np.tile(BOX_HI - BOX_LO, (K_, 1))] * len(crops))
        else:
            side["frame"] = jf
        if options.get("keyed"):
            side["cloud_base"] = 2 * k
        feed_r.append((crops, nf, dict(side, render=rt), "t%d" % k))
        feed_a.append((render_depth_frames(mesh, rt, crops, dtype, dev), nf, "t%d" % k, side))
    got = list(R.stream_render_batches(feed_r, articulation=True, link_counts=True))
    want = list(A.stream_depth_batches(feed_a, articulation=True, link_counts=True))
    assert all(g is not None and g is s.graph for g, s in zip(graphs, R.slots))        # one graph per slot served every batch
    assert len(got) == len(want) == 10 and [g[0] for g in got] == ["t%d" % k for k in range(10)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 6 and g[:2] == w[:2], k
        for a, b in zip(g[2:], w[2:]):                                   # record, articulation block, counts, link counts
            assert _bytes(a, b), k
    assert got[2][2].shape[0] == 1 and got[0][2].shape == (2, K_, got[0][2].shape[2]) and np.isfinite(got[0][2][:, :, :26]).any()
    lc5, cnt5 = got[5][5], got[5][4]
    assert 0 < lc5[0, 2] < 10 and cnt5[0] == 0 and np.isnan(got[5][2][0]).all() and cnt5[1] > 500 and np.isfinite(got[5][2][1, :, :26]).any()
    assert all((g[4] > 500).all() for k, g in enumerate(got) if k != 5)
    # bad input: ValueError before anything is enqueued, and the pipeline stays usable
    crops, nf, rt, sc, rigs, jf = batches[0]
    good = dict(feed_r[0][2], crops=crops, norm_factors=nf)
    for kw in (dict(render=None), dict(scene=None), dict(rig=None), dict(render=rt[:, :100]), dict(render=np.where(np.arange(208) == 7, -1.0, rt)),
               dict(crops=[(64, 64, (0, 0))] * 3), dict(crops=[(100, 90, (0, 0))] * 2), dict(crops=[(64, 0, (0, 0))] * 2), dict(norm_factors=[1.0])):
        with pytest.raises(ValueError):
            R.submit_render(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="submit_render"):
        R.submit_depth(feed_a[0][0], nf, scene=sc, rig=rigs)
    with pytest.raises(RuntimeError, match="submit_depth"):
        A.submit_render(**good)
    assert not R._inflight
    R.submit_render(seed=got[0][1], **good)
    again = R.retire(articulation=True, link_counts=True)
    assert all(_bytes(a, b) for a, b in zip(again[2:], got[0][2:]))


def test_launch_budget(dev):
    """The rendering step is the annotated depth step behind ONE more ABI call, in front of ancsh_depth_annotate_stream; a pipeline without
    the option issues none."""
    from test_fit_quality_gpu import _launch_names
    pb = _weights()
    R, A = _pipes(pb, "uint16", object_mesh(LINKS_), slots=1)
    on, off = _launch_names(R.prepare()), _launch_names(A.prepare())
    assert on[:2] == ["ancsh_render_depth_labels", "ancsh_depth_annotate_stream"] and on[1:] == off and "ancsh_render_depth_labels" not in off
