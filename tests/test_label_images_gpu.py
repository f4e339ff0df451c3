"""GPU: the depth front end's label / NOCS images -- ancsh_depth_label_images against the numpy statement of its contract (the inverse of
the compaction tests/depth_oracle.py restates), byte for byte, and AncshPipeline(depth_capacity=..., label_images=True) against the xyz
stream with dense=True fed the oracle's clouds."""
import numpy as np
import pytest
import torch

import depth_oracle as O
from redzone import Arena
from test_dense_gpu import _same
from test_depth_gpu import SIDE, _camera, _cams, _depth_batches, _depth_image, _layout, _scale, _xyz

pytestmark = pytest.mark.gpu
UNTOUCHED_L, UNTOUCHED_V = -7, -7.0
NAN_BITS = 0x7fc00000


def _rows(rs, cap):
    """Random per-row labels / values; a tenth of the values are NaNs with random payloads, some labels are -1."""
    labels = rs.randint(-1, 8, cap).astype(np.int32)
    values = rs.normal(size=(cap, 7)).astype(np.float32)
    bits = values.view(np.uint32)
    junk = rs.uniform(size=bits.shape) < 0.1
    bits[junk] = (0x7f800001 + rs.randint(0, 0x7ffffe, int(junk.sum()))).astype(np.uint32) | (rs.randint(0, 2, int(junk.sum())).astype(np.uint32) << 31)
    assert np.isnan(values[junk]).all()
    return labels, values


def _counts(pix, mask, geom):
    """(counts (B,) int64, offsets (B+1,) int64, unsaturated) of the depth entry, from the oracle's validity rule."""
    cnt = np.zeros(geom.shape[0], np.int64)
    for b, (start, h, w) in enumerate(geom[:, :3].tolist()):
        if start >= 0 and h >= 1 and w >= 1 and start + h * w <= pix.shape[0]:
            m = None if mask is None else mask[start:start + h * w].reshape(h, w)
            cnt[b] = O.valid_pixels(pix[start:start + h * w].reshape(h, w), m).sum()
    return cnt, np.concatenate([[0], np.cumsum(np.maximum(cnt, 1))])


def _operator(dev, pix, mask, geom, dest, labels, values, icap):
    """ancsh_depth_unproject_stream (rows for every pixel of every cloud), then ancsh_depth_label_images with capacity = the rows that
    `labels` / `values` hold, on redzone-guarded images prefilled with the UNTOUCHED sentinels -> (img_labels, img_values, offsets,
    counts) as numpy."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import MAX_CHUNKS
    B = geom.shape[0]
    kind = 0 if pix.dtype == np.uint16 else 1
    d_pix = torch.from_numpy(pix.view(np.int16) if pix.dtype == np.uint16 else pix).to(dev)
    d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
    d_geom = torch.from_numpy(geom).to(dev)
    d_cam = torch.from_numpy(_cams(np.random.RandomState(0), B)).to(dev)
    capacity = labels.shape[0]
    row_cap = max(pix.shape[0], int(np.abs(geom[:, 1].astype(np.int64) * geom[:, 2]).sum()))
    rows = torch.zeros((row_cap, 3), dtype=torch.float32, device=dev)
    off = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    scratch = torch.zeros((B * MAX_CHUNKS,), dtype=torch.int32, device=dev)
    _lib.call("ancsh_depth_unproject_stream", B, kind, _lib.ptr(d_pix), _lib.ptr(d_mask), pix.shape[0], _lib.ptr(d_geom), _lib.ptr(d_cam),
              _lib.ptr(rows), row_cap, _lib.ptr(off), _lib.ptr(cnt), _lib.ptr(scratch))
    assert values.shape == (capacity, 7)
    d_lab, d_val, d_dest = torch.from_numpy(labels).to(dev), torch.from_numpy(values).to(dev), torch.from_numpy(dest).to(dev)
    assert _same(d_val.cpu().numpy(), values)                           # the NaN payloads reached the device
    arena = Arena()
    img_l = arena.empty((icap,), dtype=torch.int32, device=dev)
    img_v = arena.empty((icap, 7), dtype=torch.float32, device=dev)
    img_l.fill_(UNTOUCHED_L)
    img_v.fill_(UNTOUCHED_V)
    _lib.call("ancsh_depth_label_images", B, kind, _lib.ptr(d_pix), _lib.ptr(d_mask), pix.shape[0], _lib.ptr(d_geom), _lib.ptr(off),
              _lib.ptr(scratch), _lib.ptr(d_lab), _lib.ptr(d_val), capacity, _lib.ptr(d_dest), _lib.ptr(img_l), _lib.ptr(img_v), icap)
    torch.cuda.synchronize()
    out = img_l.cpu().numpy(), img_v.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    arena.check()
    return out


def _expected(pix, mask, geom, dest, labels, values, capacity, icap):
    """The contract in numpy: full(-1 / NaN) images with img[valid pixels] = rows[offsets[b] : offsets[b] + counts[b]] (cut at capacity),
    at dest[b]; everything else UNTOUCHED."""
    cnt, off = _counts(pix, mask, geom)
    img_l = np.full(icap, UNTOUCHED_L, np.int32)
    img_v = np.full((icap, 7), UNTOUCHED_V, np.float32)
    for b in range(geom.shape[0]):
        start, h, w = (int(v) for v in geom[b, :3])
        d0 = int(dest[b])
        if d0 < 0 or start < 0 or h < 1 or w < 1 or start + h * w > pix.shape[0] or d0 + h * w > icap:
            continue
        m = None if mask is None else mask[start:start + h * w].reshape(h, w)
        valid = O.valid_pixels(pix[start:start + h * w].reshape(h, w), m).reshape(-1)
        assert valid.sum() == cnt[b]
        lab = np.full(h * w, -1, np.int32)
        val = np.full((h * w, 7), NAN_BITS, np.uint32).view(np.float32)
        r = off[b] + np.arange(cnt[b])
        keep = r < capacity
        idx = np.flatnonzero(valid)
        lab[idx[keep]] = labels[r[keep]]
        val[idx[keep]] = values[r[keep]]
        img_l[d0:d0 + h * w], img_v[d0:d0 + h * w] = lab, val
    return img_l, img_v, off, cnt


def _check(dev, pix, mask, geom, dest, capacity=None, icap=None, seed=0, what=""):
    capacity = pix.shape[0] if capacity is None else capacity
    icap = pix.shape[0] if icap is None else icap
    labels, values = _rows(np.random.RandomState(seed), capacity)
    dest = np.asarray(dest, np.int32)
    got = _operator(dev, pix, mask, geom, dest, labels, values, icap)
    again = _operator(dev, pix, mask, geom, dest, labels, values, icap)
    want = _expected(pix, mask, geom, dest, labels, values, capacity, icap)
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[2].astype(np.int64), np.minimum(want[2], 2 ** 31 - 1)), what
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (what, bad[:8], got[0][bad[:8]], want[0][bad[:8]])
    assert _same(got[1], want[1]), (what, np.flatnonzero((got[1].view(np.int32) != want[1].view(np.int32)).any(1))[:8])
    assert _same(got[0], again[0]) and _same(got[1], again[1]), what
    return got, want


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_ragged_crops_with_gaps(dev, dtype, with_mask):
    rs = np.random.RandomState(len(dtype) + 7 * with_mask)
    shapes = [(1, 1), (3, 7), (512, 512), (17, 300), (300, 300), (64, 1), (1, 129), (5, 5), (40, 33)]
    crops = [_depth_image(rs, h, w, dtype) for h, w in shapes]
    crops[0][:] = 1
    crops[7][:] = 0                                               # a cloud without a valid pixel: an all -1 / NaN image
    masks = [rs.randint(0, 3, c.shape).astype(np.uint8) * 100 for c in crops] if with_mask else None
    if with_mask:
        masks[0][:] = 1
        masks[8][:] = 0
    pix, mask, geom = _layout(rs, crops, masks, [(0, 0)] * len(crops))
    assert any(g[0] % 8 for g in geom) and any(g[0] % 4 for g in geom)
    # images at the crops' own starts: the gaps between them stay untouched
    (img_l, img_v, off, cnt), _ = _check(dev, pix, mask, geom, geom[:, 0], what=(dtype, with_mask))
    covered = np.zeros(pix.shape[0], bool)
    for s, h, w in geom[:, :3]:
        covered[s:s + h * w] = True
    assert (~covered).sum() >= len(crops) and (img_l[~covered] == UNTOUCHED_L).all() and (img_v[~covered] == UNTOUCHED_V).all()
    assert cnt[2] > 50000 and (img_l[geom[7, 0]:geom[7, 0] + 25] == -1).all()
    assert (img_v[geom[7, 0]:geom[7, 0] + 25].view(np.uint32) == NAN_BITS).all()
    # packed elsewhere: other gaps, in another order, in a larger image buffer
    order = rs.permutation(len(crops))
    dest, a = np.zeros(len(crops), np.int32), 3
    for b in order:
        dest[b] = a
        a += crops[b].size + int(rs.randint(0, 6))
    _check(dev, pix, mask, geom, dest, icap=a + 11, seed=1, what=(dtype, with_mask, "moved"))
    # the host wrapper: the same images from the same tensors
    from articulated_pose_amd.depth import depth_label_images, depth_unproject
    labels, values = _rows(np.random.RandomState(2), pix.shape[0])
    t = lambda x: torch.from_numpy(x).to(dev)
    d_pix = t(pix.view(np.int16) if pix.dtype == np.uint16 else pix)
    d_mask = None if mask is None else t(mask)
    scratch = torch.zeros((len(crops) * 64,), dtype=torch.int32, device=dev)
    _, d_off, _ = depth_unproject(d_pix, d_mask, t(geom), t(_cams(rs, len(crops))), scratch=scratch)
    wl, wv = depth_label_images(d_pix, d_mask, t(geom), t(geom[:, 0].copy()), d_off, t(labels), t(values), scratch=scratch)
    el, ev, _, _ = _expected(pix, mask, geom, geom[:, 0], labels, values, pix.shape[0], pix.shape[0])
    wl, wv = wl.cpu().numpy(), wv.cpu().numpy()
    assert _same(wl[covered], el[covered]) and _same(wv[covered], ev[covered])
    assert (wl[~covered] == -1).all() and np.isnan(wv[~covered]).all()           # the wrapper's own prefill
    with pytest.raises(ValueError):
        depth_label_images(d_pix, d_mask, t(geom), t(geom[:, 0].copy()), d_off, t(labels), t(values))       # no scratch


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_valid_counts_around_the_step_sizes(dev, dtype, with_mask):
    """Exactly n valid pixels for n around a wave, around 1024 and around the kernels' step (256 lanes x 16 bytes = 2048 uint16 / 1024
    float32 pixels), as runs from the crop's start and scattered; the 1 x 1 clouds bring the grid down to one chunk a cloud."""
    rs = np.random.RandomState(3)
    ns = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
    crops, masks = [], []
    for k, n in enumerate(ns + ns):
        c = _depth_image(rs, 72, 60, dtype, holes=0.0, junk=False)
        sel = np.zeros(c.size, bool)
        sel[(np.arange(n) if k < len(ns) else rs.permutation(c.size)[:n])] = True
        sel = sel.reshape(c.shape)
        if with_mask:
            masks.append(sel.astype(np.uint8))
        else:
            c[~sel] = 0
        crops.append(c)
    for _ in range(30):
        crops.append(_depth_image(rs, 1, 1, dtype, holes=0.0, junk=False))
        masks.append(np.ones((1, 1), np.uint8))
    pix, mask, geom = _layout(rs, crops, masks if with_mask else None, [(0, 0)] * len(crops))
    (_, _, _, cnt), _ = _check(dev, pix, mask, geom, geom[:, 0], what=(dtype, with_mask))
    assert cnt[:2 * len(ns)].tolist() == ns + ns and (cnt[2 * len(ns):] == 1).all()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_wide_crops_and_chunk_boundaries(dev, dtype, with_mask):
    """Three one-row crops wider than ANCSH_DEPTH_MAX_CHUNKS * 2048 pixels on the full 64-chunk grid: valid runs that end one pixel in
    front of, on and behind the first chunk boundary, one that ends behind the second, and scattered pixels."""
    from articulated_pose_amd.depth import MAX_CHUNKS
    rs = np.random.RandomState(5)
    n = MAX_CHUNKS * 2048 + 77
    per = -(-n // MAX_CHUNKS)
    runs = [per - 1, per, per + 1, 2 * per + 1, None]
    crops, masks = [], []
    for run in runs:
        c = _depth_image(rs, 1, n, dtype, holes=0.0, junk=False)
        sel = np.zeros(n, bool)
        if run is None:
            sel[:] = rs.uniform(size=n) < 0.4
        else:
            sel[:run] = True
        if with_mask:
            masks.append(sel.reshape(1, n).astype(np.uint8))
        else:
            c[0, ~sel] = 0
        crops.append(c)
    pix, mask, geom = _layout(rs, crops, masks if with_mask else None, [(0, 0)] * len(crops))
    assert (pix.shape[0] // len(crops) + 2047) // 2048 >= MAX_CHUNKS           # the grid has every chunk
    (_, _, _, cnt), _ = _check(dev, pix, mask, geom, geom[:, 0], what=(dtype, with_mask))
    assert cnt[:4].tolist() == runs[:4]


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_shared_pixels_silenced_clouds_and_capacity_cut(dev, dtype, with_mask):
    rs = np.random.RandomState(9 + with_mask)
    shapes = [(3, 7), (300, 300), (17, 300), (5, 5)]
    crops = [_depth_image(rs, h, w, dtype) for h, w in shapes]
    masks = [rs.randint(0, 2, c.shape).astype(np.uint8) for c in crops] if with_mask else None
    pix, mask, geom = _layout(rs, crops, masks, [(0, 0)] * len(crops), gaps=False)
    npx = pix.shape[0]
    # clouds 4 and 5 share cloud 1's pixels, cloud 6 cloud 2's: 4 gets an image of its own behind the crops, 5 and 6 are silenced
    geom2 = np.concatenate([geom, geom[[1, 1, 2]]])
    dest = np.concatenate([geom[:, 0], [npx + 5, -1, -3]]).astype(np.int32)
    icap = npx + 5 + 300 * 300 + 9
    cap = npx + 3 * 300 * 300
    (img_l, img_v, off, cnt), _ = _check(dev, pix, mask, geom2, dest, capacity=cap, icap=icap, what=(dtype, with_mask, "shared"))
    assert cnt[4] == cnt[1] > 1000 and (img_l[npx:npx + 5] == UNTOUCHED_L).all() and (img_l[-9:] == UNTOUCHED_L).all()
    a, e = geom[1, 0], geom[1, 0] + 300 * 300
    assert not np.array_equal(img_l[a:e], img_l[npx + 5:npx + 5 + 300 * 300])            # the same pixels, other rows
    # a cloud whose image would pass image_capacity writes nothing (one pixel short), the others are unaffected
    _check(dev, pix, mask, geom2, dest, capacity=cap, icap=icap - 10, seed=3, what=(dtype, with_mask, "image cut"))
    # a capacity that ends inside cloud 4's rows: its cut pixels read -1 / NaN, cloud 5, entirely beyond, gives an all -1 / NaN image
    wcnt, woff = _counts(pix, mask, geom2)
    cut_at = int(woff[4] + wcnt[4] // 2)
    dest3 = np.concatenate([geom[:, 0], [npx, npx + 300 * 300, -1]]).astype(np.int32)
    (img_l, img_v, off, cnt), _ = _check(dev, pix, mask, geom2, dest3, capacity=cut_at, icap=npx + 2 * 300 * 300, seed=4,
                                         what=(dtype, with_mask, "capacity cut"))
    assert woff[4] < cut_at < woff[5]
    first, second = img_l[npx:npx + 300 * 300], img_l[npx + 300 * 300:]
    assert (second == -1).all() and (img_v[npx + 300 * 300:].view(np.uint32) == NAN_BITS).all()
    valid4 = np.flatnonzero(O.valid_pixels(crops[1], None if masks is None else masks[1]).reshape(-1))
    cut = valid4[cut_at - woff[4]:]
    assert cut.size > 0 and (first[cut] == -1).all() and (img_v[npx:npx + 300 * 300][cut].view(np.uint32) == NAN_BITS).all()


# ---- the stream -----------------------------------------------------------------------------------------------------------------
def _mk(pb, K, B, N, slots, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, niter_a=64, niter_b=8, seed=100, lm_schedule="throughput", joint_source="predicted", slots=slots), **kw)
    return AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, "cuda:0", **kw)


def _check_images(imgs, frames, counts, dense, what):
    """One batch: every frame's image pair against the dense rows of its cloud (labels, values, offsets of the xyz stream)."""
    lab, val, off = dense
    assert isinstance(imgs, list) and len(imgs) == len(frames) == len(off) - 1, what
    for c, ((d, m, _), (il, iv)) in enumerate(zip(frames, imgs)):
        assert il.shape == d.shape and il.dtype == np.int32 and iv.shape == d.shape + (7,) and iv.dtype == np.float32, (what, c)
        valid = O.valid_pixels(d, m)
        assert valid.sum() == counts[c], (what, c)
        a = int(off[c])
        assert _same(il[valid], lab[a:a + counts[c]]) and _same(iv[valid], val[a:a + counts[c]]), (what, c)
        assert (il[~valid] == -1).all() and (iv[~valid].view(np.uint32) == NAN_BITS).all(), (what, c)
        if counts[c]:
            assert (il[valid] >= 0).mean() > 0.9, (what, c)


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("slots", [1, 4])
def test_label_image_stream_equals_dense_xyz_stream(dev, dtype, slots):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=1)
    batches = _depth_batches(pb, 10, B, np.random.RandomState(slots), dtype)
    d, m, org = batches[3][0][1]
    batches[3][0][1] = (d, np.zeros_like(m), org)                        # a frame without a valid pixel
    xyz, counts = _xyz(batches, dtype)
    assert counts[3][1] == 0 and len(batches[-1][0]) == B // 2
    cap = B * SIDE * SIDE
    pipe = _mk(pb, K, B, N, slots, articulation=True, depth_capacity=cap, depth_dtype=dtype, label_images=True)
    plain = _mk(pb, K, B, N, slots, articulation=True, depth_capacity=cap, depth_dtype=dtype)
    dense = _mk(pb, K, B, N, slots, articulation=True, raw_capacity=cap, dense=True)
    sl = pipe.slots[0]
    assert sl.img[0].shape == (cap,) and sl.img[1].shape == (cap, 7) and sl.h_img[1].is_pinned() and sl.rowlab[1].shape == (cap, 7)
    assert plain.slots[0].img is None and plain.slots[0].hdr.numel() == sl.hdr.numel() - B
    got, graphs = [], None
    for item in pipe.stream_depth_batches(batches, _camera(), _scale(dtype), articulation=True, label_images=True):
        got.append(item)
        graphs = graphs or [s.graph for s in pipe.slots]
    base = list(plain.stream_depth_batches(batches, _camera(), _scale(dtype), articulation=True))
    want = list(dense.stream_batches(xyz, articulation=True, dense=True))
    assert len(got) == len(base) == len(want) == 10
    for k, (g, p, w) in enumerate(zip(got, base, want)):
        assert len(g) == 6 and len(p) == 5 and g[:2] == p[:2] == w[:2], k
        assert _same(g[2], p[2]) and _same(g[3], p[3]) and _same(g[2], w[2]) and _same(g[3], w[3]), k      # records, articulation blocks
        assert g[5].dtype == np.int32 and np.array_equal(g[5], p[4]) and np.array_equal(g[5], counts[k]), k  # the counts stay last
        _check_images(g[4], batches[k][0], counts[k], w[4], (dtype, slots, k))
    assert len(got[-1][4]) == B // 2                                      # the short batch: n_valid pairs, frame 0's image its own
    il, iv = got[3][4][1]                                                 # the frame without a valid pixel
    assert (il == -1).all() and (iv.view(np.uint32) == NAN_BITS).all() and np.isnan(got[3][2][1]).all()
    # fresh host arrays: a later batch does not change what was returned
    keep = [(a.copy(), b.copy()) for a, b in got[0][4]]
    pipe.submit_depth(batches[1][0], batches[1][1], _camera(), _scale(dtype))
    assert len(pipe.retire()) == 4                                        # default: no images
    assert all(_same(a, x) and _same(b, y) for (a, b), (x, y) in zip(keep, got[0][4]))
    assert all(s.graph is not None and s.graph is g0 for s, g0 in zip(pipe.slots, graphs))       # one capture per slot served every batch
    with pytest.raises(RuntimeError, match="label_images=True"):
        next(plain.stream_depth_batches(batches[:1], _camera(), _scale(dtype), label_images=True))


@pytest.mark.parametrize("variant", ["prismatic", "keyed", "range_guard"])
def test_label_image_stream_composes(dev, variant):
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K = 4 if variant == "prismatic" else 3
    B, N = 4, 512
    pb = passthrough_pose_problem(K, 6, N, seed=2)
    kw = dict(prismatic=dict(joint_types="prismatic"), keyed=dict(keyed=True), range_guard=dict(arithmetic="f16x2", range_guard=True))[variant]
    batches = _depth_batches(pb, 5, B, np.random.RandomState(5), "uint16")
    if variant == "range_guard":
        batches[1][1][0] = 1e6                                            # cloud 0 of batch 1: beyond f16's range -> refit in f32
    xyz, counts = _xyz(batches, "uint16")
    cap = B * SIDE * SIDE
    pipe = _mk(pb, K, B, N, 2, depth_capacity=cap, depth_dtype="uint16", label_images=True, **kw)
    dense = _mk(pb, K, B, N, 2, raw_capacity=cap, dense=True, **kw)
    if variant == "range_guard":
        assert pipe.slots[0].img32[1].shape == (cap, 7) and pipe.slots[0].h_img32[0].is_pinned()
    base = 40 if variant == "keyed" else 0
    got, want = [], []
    for k, ((frames, nf), (clouds, _)) in enumerate(zip(batches, xyz)):
        cb = dict(cloud_base=base + k) if variant == "keyed" else {}
        pipe.submit_depth(frames, nf, _camera(), 1e-4, tag=k, **cb)
        dense.submit(clouds, nf, tag=k, **cb)
        got.append(pipe.retire(flags=True, label_images=True))
        want.append(dense.retire(flags=True, dense=True))
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == 6 and g[:2] == w[:2] and _same(g[2], w[2]) and np.array_equal(g[3], w[3]), (variant, k)
        assert np.array_equal(g[5], counts[k])
        _check_images(g[4], batches[k][0], counts[k], w[4], (variant, k))
    if variant == "range_guard":
        assert pipe.f32_reruns == dense.f32_reruns == 1 and got[1][3][0] != 0
    if variant == "keyed":                                                # the base matters: base 0 gives other records
        pipe.submit_depth(batches[0][0], batches[0][1], _camera(), 1e-4, seed=got[0][1], cloud_base=0)
        assert not _same(pipe.retire()[2], got[0][2])


def test_launch_budget(dev):
    """The label_images=True step is the plain depth step's sequence followed by ancsh_raw_point_labels, ancsh_depth_label_images and
    nothing else; a pipeline built without the option issues the sequence it always did."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.synthetic import passthrough_pose_problem
    K, B, N = 3, 4, 512
    pb = passthrough_pose_problem(K, 4, N, seed=2)
    batches = _depth_batches(pb, 2, B, np.random.RandomState(2), "uint16", short_last=False)
    cap = B * SIDE * SIDE
    calls = {}
    for name, extra in (("images", dict(label_images=True)), ("plain", dict())):
        pipe = _mk(pb, K, B, N, 1, use_graph=False, articulation=True, depth_capacity=cap, **extra)
        pipe.submit_depth(batches[0][0], batches[0][1], _camera(), 1e-4)
        pipe.retire()
        _lib.profile_start()
        pipe.submit_depth(batches[1][0], batches[1][1], _camera(), 1e-4)
        calls[name] = [n for n, _, _ in _lib.profile_stop()]
        pipe.retire()
    assert calls["plain"][0] == "ancsh_depth_unproject_stream" and calls["plain"][-1] == "ancsh_articulation_rec"
    assert "ancsh_raw_point_labels" not in calls["plain"] and "ancsh_depth_label_images" not in calls["plain"]
    assert calls["images"] == calls["plain"] + ["ancsh_raw_point_labels", "ancsh_depth_label_images"]
