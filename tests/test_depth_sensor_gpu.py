"""GPU: ancsh_depth_sensor_model / _keyed against their numpy mirror (tests/depth_sensor_mirror.py, validated on its own in
tests/test_depth_sensor_cpu.py), byte for byte and inside red zones; the identity table; and AncshPipeline(sensor=...): the identity table
changes no byte of any streamed result, and a noisy table gives what the eager chain render_depth_frames -> sensor_frames -> submit_depth
gives."""
import numpy as np
import pytest
import torch

import depth_sensor_mirror as SM
from redzone import Arena
from test_render_cpu import object_mesh
from test_render_gpu import B_, CAP_, DTYPES, FILL, K_, LABEL_FILL, LINKS_, N_, SCALE, _batch, _bytes, _weights

pytestmark = pytest.mark.gpu
EVERY_TERM = dict(sigma=(0.002, 0.001, 0.0005), z0=1.0, p_hole=0.1, p_edge=0.5, edge_rel=0.05, disparity=(35.0, 8), z_range=(0.45, 3.5))
NOISY = dict(sigma=(0.002, 0.001, 0.0), z0=1.0, p_hole=0.2, p_edge=0.5, edge_rel=0.05, disparity=(35.0, 8))


def _crop(rs, dtype, h, w):
    """A crop of two smooth surfaces with a depth step between them, a background block, sparse unusable pixels (zeros; float32: NaN, +Inf
    and negative values too) and depths on both sides of EVERY_TERM's z_range."""
    ii, jj = np.mgrid[0:h, 0:w]
    z = 0.4 + 3.4 * (ii * w + jj) / max(1, h * w - 1) + 0.01 * rs.uniform(size=(h, w)) + 0.4 * (jj > w // 2)
    d = np.rint(z * 1000).astype(np.uint16) if dtype == "uint16" else z.astype(np.float32)
    lab = ((ii + jj) // 7 % 3).astype(np.uint8)
    if h * w > 1:
        lab[h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 3)] = 255
    bad = rs.uniform(size=(h, w)) < 0.03
    d[bad] = 0 if dtype == "uint16" else rs.choice(np.array([0.0, np.nan, np.inf, -1.5], np.float32), int(bad.sum()))
    lab[rs.uniform(size=(h, w)) < 0.02] = 255
    return d, lab


def _pack(rs, dtype, shapes, first=3, gap=5):
    """Crops at unaligned starts with gaps between them -> (depth (cap,), labels (cap,), geom (n, 5), scenes (n, 240), cap)."""
    geom, a = [], first
    for h, w in shapes:
        geom.append((a, h, w, 0, 0))
        a += h * w + gap
    cap = a + 2
    depth, labels = np.zeros(cap, DTYPES[dtype]), np.full(cap, 255, np.uint8)
    for (start, h, w, _, _) in geom:
        d, l = _crop(rs, dtype, h, w)
        depth[start:start + h * w], labels[start:start + h * w] = d.reshape(-1), l.reshape(-1)
    scenes = np.zeros((len(shapes), SM.SCENE_WIDTH))
    scenes[:, 6] = SCALE[dtype]
    scenes[:, 14] = 3
    return depth, labels, np.asarray(geom, np.int32), scenes, cap


class _Call(object):
    """The entry's device arguments inside red zones, outputs prefilled with sentinels."""

    def __init__(self, dev, dtype, keyed, depth, labels, geom, scenes, table, seed, base):
        from articulated_pose_amd.dataset import seed_bits, stream_key_words
        self.dtype, self.keyed, self.n, self.cap = dtype, keyed, geom.shape[0], depth.shape[0]
        tt, view = (torch.int16, np.int16) if dtype == "uint16" else (torch.float32, np.float32)
        self.arena = arena = Arena()
        self.d_in, self.d_out = arena.empty((self.cap,), dtype=tt, device=dev), arena.empty((self.cap,), dtype=tt, device=dev)
        self.l_in, self.l_out = arena.empty((self.cap,), dtype=torch.uint8, device=dev), arena.empty((self.cap,), dtype=torch.uint8, device=dev)
        self.d_in.copy_(torch.from_numpy(depth.view(view)))
        self.l_in.copy_(torch.from_numpy(labels))
        self.geom, self.scenes = torch.from_numpy(np.ascontiguousarray(geom, np.int32).reshape(-1, 5)).to(dev), torch.from_numpy(scenes).to(dev)
        self.table = torch.from_numpy(np.asarray(table, np.float64)).to(dev)
        key = stream_key_words(seed, base) if keyed else np.array([seed_bits(seed)], np.int64)
        self.key = torch.from_numpy(key).to(dev)
        self.prefill()

    def prefill(self):
        view = np.int16 if self.dtype == "uint16" else np.float32
        self.d_out.copy_(torch.from_numpy(np.full(self.cap, FILL[self.dtype], DTYPES[self.dtype]).view(view)))
        self.l_out.fill_(LABEL_FILL)

    def args(self, **over):
        from articulated_pose_amd import _lib
        a = dict(n=self.n, kind=0 if self.dtype == "uint16" else 1, d_in=_lib.ptr(self.d_in), l_in=_lib.ptr(self.l_in), cap=self.cap,
                 geom=_lib.ptr(self.geom), scenes=_lib.ptr(self.scenes), table=_lib.ptr(self.table), key=_lib.ptr(self.key),
                 d_out=_lib.ptr(self.d_out), l_out=_lib.ptr(self.l_out))
        a.update(over)
        return [a[k] for k in ("n", "kind", "d_in", "l_in", "cap", "geom", "scenes", "table", "key", "d_out", "l_out")]

    def run(self, **over):
        from articulated_pose_amd import _lib
        _lib.call("ancsh_depth_sensor_model_keyed" if self.keyed else "ancsh_depth_sensor_model", *self.args(**over))
        return self.outputs()

    def outputs(self):
        torch.cuda.synchronize()
        return self.d_out.cpu().numpy().view(DTYPES[self.dtype]), self.l_out.cpu().numpy()      # (the guards: arena.check(), once, at the end)

    def untouched(self):
        d, l = self.outputs()
        return _bytes(d, np.full(self.cap, FILL[self.dtype], DTYPES[self.dtype])) and (l == LABEL_FILL).all()


CASES = [[(1, 1)], [(1, 7)], [(5, 1)], [(17, 64)], [(64, 65)], [(33, 40)] * 3]


@pytest.mark.parametrize("keyed", [False, True], ids=["seed", "keyed-base5"])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_entry_equals_the_mirror(dev, dtype, keyed):
    """Every term of the table on; single crops from 1 x 1 to 64 x 65 (one to three chunks) and three 33 x 40 frames in one call, at unaligned
    starts: depth and labels equal the mirror's byte for byte, pixels of no crop keep the sentinel, and a second call writes the same."""
    from articulated_pose_amd.depth import pack_sensor
    table, base, seed = pack_sensor(**EVERY_TERM), (5 if keyed else 0), 0xC0FFEE1234567
    rs = np.random.RandomState(17)
    for shapes in CASES:
        depth, labels, geom, scenes, cap = _pack(rs, dtype, shapes)
        want = SM.sensor_flat(depth, labels, geom, scenes, table, seed, base, fill=FILL[dtype], label_fill=LABEL_FILL)
        call = _Call(dev, dtype, keyed, depth, labels, geom, scenes, table, seed, base)
        got = call.run()
        for name, g, w in zip(("depth", "labels"), got, want):
            diff = g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)
            assert _bytes(g, w), (shapes, name, int(diff.any(1).sum()), np.flatnonzero(diff.any(1))[:8])
        call.prefill()
        again = call.run()
        assert _bytes(again[0], got[0]) and _bytes(again[1], got[1]), shapes
        call.arena.check()
        if len(shapes) == 3 or shapes == [(64, 65)]:                          # the table does something: drops and moved depths
            inside = want[1] != LABEL_FILL
            assert ((want[1] == 255) & (labels != 255) & inside).any() and ((want[0] != depth) & inside & (want[1] != 255)).any()


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_identity_table_and_refusals(dev, dtype):
    """The identity table copies the crops byte for byte (both entries).  nframes == 0 returns 0 and writes nothing; a refused crop writes
    nothing; overlapping buffers, a misaligned or null pointer and a bad depth_type are refused before any launch."""
    from articulated_pose_amd.depth import depth_sensor_model, pack_sensor
    rs = np.random.RandomState(23)
    depth, labels, geom, scenes, cap = _pack(rs, dtype, [(9, 31), (40, 33), (1, 5)])
    ident = pack_sensor()
    want_d, want_l = np.full(cap, FILL[dtype], DTYPES[dtype]), np.full(cap, LABEL_FILL, np.uint8)
    for start, h, w, _, _ in geom:
        want_d[start:start + h * w], want_l[start:start + h * w] = depth[start:start + h * w], labels[start:start + h * w]
    for keyed in (False, True):
        call = _Call(dev, dtype, keyed, depth, labels, geom, scenes, ident, 99, 7)
        got = call.run()
        assert _bytes(got[0], want_d) and _bytes(got[1], want_l), keyed
        call.arena.check()
    # the operator on tensors: fresh outputs read background where no crop lies
    out = depth_sensor_model(call.d_in, call.l_in, call.geom, call.scenes, call.table, call.key)
    inside = want_l != LABEL_FILL
    assert _bytes(out[0].cpu().numpy().view(DTYPES[dtype])[inside], depth[inside]) and _bytes(out[1].cpu().numpy()[inside], labels[inside])
    assert (out[1].cpu().numpy()[~inside] == 255).all() and (out[0].cpu().numpy().view(np.uint8).reshape(cap, -1)[~inside] == 0).all()
    with pytest.raises(ValueError, match="overlap"):
        depth_sensor_model(call.d_in, call.l_in, call.geom, call.scenes, call.table, call.key, out=(call.d_in, call.l_out))
    # nothing launched, nothing written
    call = _Call(dev, dtype, False, depth, labels, geom, scenes, pack_sensor(**EVERY_TERM), 99, 0)
    call.run(n=0)
    assert call.untouched()
    bad_geom = torch.tensor([(0, 0, 5, 0, 0), (0, 5, 0, 0, 0), (cap - 4, 1, 5, 0, 0), (-1, 1, 5, 0, 0)], dtype=torch.int32, device=dev)
    sc4 = torch.from_numpy(np.tile(scenes[:1], (4, 1))).to(dev)
    from articulated_pose_amd import _lib
    call.run(n=4, geom=_lib.ptr(bad_geom), scenes=_lib.ptr(sc4))
    assert call.untouched()
    a = dict(zip(("n", "kind", "d_in", "l_in", "cap", "geom", "scenes", "table", "key", "d_out", "l_out"), call.args()))
    item = 2 if dtype == "uint16" else 4
    for over, what in ((dict(d_out=a["d_in"]), "overlap"), (dict(l_out=a["l_in"]), "overlap"), (dict(d_out=a["d_in"] + 16 * item), "overlap"),
                       (dict(l_out=a["l_in"] + 8), "overlap"), (dict(d_in=a["d_in"] + item), "aligned"), (dict(d_out=a["d_out"] + item), "aligned"),
                       (dict(l_in=a["l_in"] + 4), "aligned"), (dict(l_out=a["l_out"] + 1), "aligned"), (dict(kind=2), "depth_type"),
                       (dict(kind=-1), "depth_type"), (dict(n=-1), "nframes"), (dict(n=65536), "65535"), (dict(cap=1 << 30), "pixel_capacity"),
                       (dict(table=0), "null"), (dict(key=0), "null"), (dict(d_out=0), "null")):
        with pytest.raises(ValueError, match=what):
            call.run(**over)
    assert call.untouched()
    call.arena.check()


# ---- the stream -------------------------------------------------------------------------------------------------------------------------------
def _equal(a, b):
    """Byte equality through the tuples and lists of a retired result."""
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and _bytes(a, b)
    return a == b


def _pipe(pb, dtype, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", joint_source="predicted", articulation=True,
                   point_ground_truth=True, build_point_gt=True, depth_capacity=CAP_, depth_dtype=dtype), **kw)
    return AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **kw)


def test_identity_sensor_changes_no_byte_of_the_posed_stream(dev):
    """The posed pipeline with sensor=identity and without, same seeds, three batches, one of them short: every element of every result
    tuple is equal byte for byte, the annotated images included.  The slot owns a second pixel pair; the sensor launch stands directly behind
    the renderer."""
    from articulated_pose_amd.depth import pack_sensor
    from test_fit_quality_gpu import _launch_names
    from test_point_gt_build_gpu import stream_rig
    from test_point_gt_gpu import random_frames
    from test_pose_scene_gpu import _posed_object, _poses
    pb, mesh, dtype = _weights(), object_mesh(LINKS_), "uint16"
    rs = np.random.RandomState(13)
    kin, S = _posed_object(rs, dtype)
    feed = []
    for k in range(3):
        n = 1 if k == 1 else 2
        sizes = [(int(rs.randint(56, 65)), int(rs.randint(56, 65))) for _ in range(n)]
        crops = [(h, w, None if (f + k) % 2 == 0 else (int(rs.randint(0, 3)), int(rs.randint(0, 3)))) for f, (h, w) in enumerate(sizes)]
        feed.append((crops, rs.uniform(0.9, 1.1, n).astype(np.float32),
                     dict(pose=_poses(rs, S, n), rig=np.tile(stream_rig(), (n, 1)), frame=random_frames(rs, n)), "t%d" % k))
    results = []
    for sensor in (pack_sensor(), None):
        P = _pipe(pb, dtype, render_mesh=mesh, kinematics=kin, annotated_images=True, sensor=sensor)
        names = _launch_names(P.prepare())
        sl = P.slots[0]
        if sensor is not None:
            assert P.sensor and sl.apix.shape == sl.pix.shape and sl.apix.dtype == sl.pix.dtype and sl.amask.dtype == torch.uint8
            assert sl.apix.data_ptr() != sl.pix.data_ptr() and sl.amask.data_ptr() != sl.mask.data_ptr()
            assert all(s.apix.data_ptr() != sl.apix.data_ptr() for s in P.slots[1:])
            i = names.index("ancsh_render_depth_labels")
            assert names[i + 1:i + 3] == ["ancsh_depth_sensor_model", "ancsh_depth_annotate_stream"], names[:6]
        else:
            assert not P.sensor and sl.apix is sl.pix and sl.amask is sl.mask and not any(n.startswith("ancsh_depth_sensor") for n in names)
        results.append(list(P.stream_posed_batches(feed, flags=True, articulation=True, link_counts=True, annotated_images=True)))
        del P
    on, off = results
    assert len(on) == len(off) == 3 and on[1][2].shape[0] == 1
    for k, (g, w) in enumerate(zip(on, off)):
        assert len(g) == len(w) == 8 and _equal(g, w), k
    assert all((g[-2] > 300).all() for g in on) and np.isfinite(on[0][2][:, :, :26]).any()


def _link_pixels(frames):
    return np.array([[int(((l == k) & (d > 0) & np.isfinite(d.astype(np.float64))).sum()) for k in range(LINKS_)] for d, l, _ in frames])


@pytest.mark.parametrize("dtype,slots,keyed", [("uint16", 1, True), ("float32", 2, False)], ids=["u16-keyed", "f32-2slots"])
def test_noisy_rendered_stream_equals_the_eager_chain(dev, dtype, slots, keyed):
    """Four batches, one of them short: records, articulation blocks, counts and link counts of the rendering pipeline built with a noisy
    sensor equal, byte for byte, those of the annotated depth pipeline fed depth.sensor_frames' output of depth.render_depth_frames' frames
    for the batch's seed and base -- and so do those of the annotated depth pipeline built with the sensor and fed the CLEAN frames (the
    model behind the H2D copy; its short batch copies the padding frame again).  The mirror says beforehand that every link of every frame keeps its minimum of pixels, and gives the very
    frames sensor_frames gives.  Noisy counts are <= the clean ones, somewhere smaller."""
    from articulated_pose_amd.depth import annotate_depth_batch, pack_sensor, render_depth_frames, sensor_frames
    pb, mesh, table = _weights(), object_mesh(LINKS_), pack_sensor(**NOISY)
    rs = np.random.RandomState(29)
    batches = [_batch(rs, dtype, 1 if k == 2 else 2) for k in range(4)]
    R, A = _pipe(pb, dtype, slots=slots, keyed=keyed, render_mesh=mesh, sensor=table), _pipe(pb, dtype, slots=slots, keyed=keyed)
    S = _pipe(pb, dtype, slots=slots, keyed=keyed, sensor=table)
    assert S.slots[0].h_pix is not None and S.slots[0].apix.data_ptr() != S.slots[0].pix.data_ptr() and A.slots[0].apix is A.slots[0].pix
    feed_r, feed_a, feed_s, clean_counts = [], [], [], []
    for k, (crops, nf, rt, sc, rigs, jf) in enumerate(batches):
        seed, base = 1000 + 7 * k, (3 * k if keyed else 0)
        side = dict(scene=sc, rig=rigs, frame=jf, seed=seed, **(dict(cloud_base=base) if keyed else {}))
        clean = render_depth_frames(mesh, rt, crops, dtype, dev)
        noisy = sensor_frames(clean, sc, table, dtype, seed=seed, cloud_base=base, device=dev)
        mirrored = SM.sensor_frame_list(clean, sc, table, seed, base)
        assert all(_bytes(a[0], b[0]) and _bytes(a[1], b[1]) and tuple(a[2]) == tuple(b[2]) for a, b in zip(noisy, mirrored)), k
        px, min_px = _link_pixels(mirrored), sc[:, 13]
        assert (px >= min_px[:, None]).all() and (min_px >= 1).all(), (k, px, min_px)
        _, _, cnt, lc = annotate_depth_batch(clean, sc, dtype, K_, dev)
        clean_counts.append((cnt, lc))
        feed_r.append((crops, nf, dict(side, render=rt), "t%d" % k))
        feed_a.append((noisy, nf, "t%d" % k, side))
        feed_s.append((clean, nf, "t%d" % k, side))
    got = list(R.stream_render_batches(feed_r, articulation=True, link_counts=True))
    want = list(A.stream_depth_batches(feed_a, articulation=True, link_counts=True))
    sub = list(S.stream_depth_batches(feed_s, articulation=True, link_counts=True))
    assert len(got) == len(want) == len(sub) == 4 and [g[0] for g in got] == ["t%d" % k for k in range(4)] and got[2][2].shape[0] == 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 6 and g[:2] == w[:2], k
        for a, b in zip(g[2:], w[2:]):                                   # record, articulation block, counts, link counts
            assert _bytes(a, b), k
        assert len(sub[k]) == 6 and sub[k][:2] == w[:2] and all(_bytes(a, b) for a, b in zip(sub[k][2:], w[2:])), k
    assert np.isfinite(got[0][2][:, :, :26]).any()
    less = 0
    for g, (cnt, lc) in zip(got, clean_counts):
        assert (g[4] > 0).all() and (g[4] <= cnt).all() and (g[5] <= lc).all()
        less += int((cnt - g[4]).sum())
    assert less > 0
