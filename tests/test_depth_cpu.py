"""CPU tests of the depth front end (no GPU): the numpy restatement of ancsh_depth_unproject_stream (tests/depth_oracle.py) against golden
clouds computed by the reference's own statements (tests/golden/gen_depth_golden.py), the camera helpers, the symbol / ABI, the entry's
argument checks before any launch, and the host-side validation of frames and pipeline arguments."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import depth_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
P16 = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails its checks first
NAME = "ancsh_depth_unproject_stream"


def _golden():
    return np.load(os.path.join(HERE, "golden", "depth_unproject.npz"))


def test_oracle_fmaf_rounds_once():
    rs = np.random.RandomState(0)
    a, b, c = (rs.normal(size=400).astype(np.float32) * np.float32(10.0) ** rs.randint(-3, 4, 400).astype(np.float32) for _ in range(3))
    c[:100] = -(a[:100] * b[:100])                       # heavy cancellation: the product's low bits decide
    got = O.fmaf(a, b, c)
    for k in range(400):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = np.float32(float(exact))                      # float(Fraction) and float32(float64) each round to nearest: check by neighbours
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        ties = [v for v in cands if abs(Fraction(float(v)) - exact) == abs(Fraction(float(best)) - exact)]
        assert got[k] in ties, (k, a[k], b[k], c[k], got[k], best)
        if len(ties) == 2:                                 # a tie goes to the even mantissa
            assert (np.float32(got[k]).view(np.int32) & 1) == 0


@pytest.mark.parametrize("tag", ["pybullet", "general"])
def test_restatement_against_the_reference_golden(tag):
    """The f32 restatement differs from the reference's float64 cloud by the rounding of three coefficients, two fmafs, the scale product
    and the final product: at most ~7 half-ulps of m = z (|A00| col + |A01| row + |A02|) (near the principal point gx cancels, so the error
    is relative to m, not |x|).  Ceiling 8 * 2^-24 * m, every point compared.  Measured maxima, in units of 2^-24 m: 0.80 (x) / 0.56 (y) for the
    PyBullet-form matrix, 0.97 / 1.35 for the general one."""
    from articulated_pose_amd.depth import unprojection_from_projmat
    g = _golden()
    H, W = int(g["height"]), int(g["width"])
    row, col, d = g["row"], g["col"], g["depth"]
    want = g["cloud_cam_real_" + tag]
    A = unprojection_from_projmat(g["projMat_" + tag], H, W)
    assert np.all(A != 0) if tag == "general" else (A[1] == 0 and A[3] == 0)
    depth = np.zeros((H, W), np.float32)
    mask = np.zeros((H, W), np.uint8)
    depth[row, col], mask[row, col] = d, 1
    assert d.dtype == np.float32 and len(d) > 3000 and (d > 0).all()
    got = O.unproject_crop(depth, mask, (0, 0), np.concatenate([A, [1.0]]).astype(np.float32))
    assert got.shape == want.shape == (len(d), 3)          # no point left out, the reference's np.where order
    assert np.array_equal(got[:, 2], d) and np.array_equal(want[:, 2], d.astype(np.float64))      # z is float32(d) exactly
    z = d.astype(np.float64)
    worst = []
    for axis, (a0, a1, a2) in enumerate((A[:3], A[3:])):
        m = z * (abs(a0) * col + abs(a1) * row + abs(a2))
        err = np.abs(got[:, axis].astype(np.float64) - want[:, axis])
        worst.append(float((err / m).max() / 2.0 ** -24))
        print("%s axis %d: max error %.3f x 2^-24 m" % (tag, axis, worst[-1]))
        assert (err <= 8 * 2.0 ** -24 * m).all(), (tag, axis, worst[-1])
    # the same pixels as a crop with an origin: the same bytes (the origin is added to the pixel index, not folded into A02)
    r0, c0 = int(row.min()), int(col.min())
    crop = (depth[r0:row.max() + 1, c0:col.max() + 1], mask[r0:row.max() + 1, c0:col.max() + 1], (r0, c0))
    again = O.unproject_crop(*crop, np.concatenate([A, [1.0]]).astype(np.float32))
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


def test_oracle_validity_order_nan_row_and_counts():
    d = np.array([[1.0, np.nan, 0.0], [np.inf, -2.0, 3.0], [-np.inf, 4.0, -0.0]], np.float32)
    assert O.valid_pixels(d, None).tolist() == [[True, False, False], [False, False, True], [False, True, False]]
    m = np.array([[0, 1, 1], [1, 1, 7], [1, 0, 1]], np.uint8)
    assert np.argwhere(O.valid_pixels(d, m)).tolist() == [[1, 2]]
    u = np.array([[0, 1], [65535, 0]], np.uint16)
    assert O.valid_pixels(u, None).tolist() == [[False, True], [True, False]]
    cam = np.array([[0.5, 0.25, -1, 0.125, 2, 3, 0.5], [1, 0, 0, 0, 1, 0, 1], [1, 0, 0, 0, 1, 0, 1]], np.float32)
    pix = np.concatenate([d.reshape(-1), np.zeros(4, np.float32), [5.0]]).astype(np.float32)
    geom = np.array([[0, 3, 3, 10, 20], [9, 2, 2, 0, 0], [13, 1, 1, 2, 3]], np.int32)
    rows, off, cnt = O.unproject_flat(pix, None, geom, cam, fill=-7.0)
    assert cnt.tolist() == [3, 0, 1] and off.tolist() == [0, 3, 4, 5]
    z = np.float32(0.5)                                    # pixel (0, 0): row 10, col 20, d = 1
    assert rows[0].tolist() == [z * np.float32(0.5 * 20 + 0.25 * 10 - 1), z * np.float32(0.125 * 20 + 2 * 10 + 3), z]
    assert rows[1, 2] == 1.5 and rows[2, 2] == 2.0          # (1, 2) before (2, 1): row-major
    assert np.isnan(rows[3]).all() and rows[4].tolist() == [15.0, 10.0, 5.0] and (rows[5:] == -7.0).all()
    clouds, counts = O.unproject_frames([(d, None, (10, 20)), (np.zeros((2, 2), np.float32), None, (0, 0))], cam[0, :6], 0.5)
    assert counts.tolist() == [3, 0] and np.array_equal(clouds[0], rows[:3]) and np.isnan(clouds[1]).all() and clouds[1].shape == (1, 3)


def test_camera_helpers():
    from articulated_pose_amd.depth import unprojection_from_intrinsics, unprojection_from_projmat
    fx, fy, cx, cy, H, W = 610.3, 598.7, 301.25, 255.5, 480, 640
    A = unprojection_from_intrinsics(fx, fy, cx, cy)
    assert A.dtype == np.float64 and np.array_equal(A, [1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy])
    # the projMat whose reference-convention back-projection is that pinhole camera: x = -d (u + P02) / P00 with u = 2 col / W - 1
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[0, 2], P[1, 2] = -2 * fx / W, -2 * fy / H, 1 - 2 * cx / W, 1 - 2 * cy / H
    P[2, 2], P[2, 3], P[3, 2] = -1.002, -0.2002, -1.0
    B = unprojection_from_projmat(P, H, W)
    assert B.dtype == np.float64 and np.abs(B - A).max() <= 1e-12
    with pytest.raises(ValueError):
        unprojection_from_projmat(np.eye(3), H, W)


def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_14():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in declared_symbols() and NAME in exported and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME]) == 13
    assert _L().ancsh_abi_version() == 14


def test_entry_rejects_bad_arguments_before_launch():
    L = _L()

    def call(nclouds=2, kind=0, depth=P16, mask=P16, px=100, geom=P16, cam=P16, rows=P16, cap=100, off=P16, cnt=P16, scratch=P16):
        return L.ancsh_depth_unproject_stream(nclouds, kind, depth, mask, px, geom, cam, rows, cap, off, cnt, scratch, None)
    for kw, msg in ((dict(nclouds=-1), b"bad shape"), (dict(nclouds=65536), b"65535"), (dict(kind=2), b"depth_type=2"),
                    (dict(kind=-1), b"depth_type=-1"), (dict(px=-1), b"pixel_capacity=-1"), (dict(px=1 << 30, cap=1 << 30), b"pixel_capacity"),
                    (dict(px=101), b"below pixel_capacity"), (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"),
                    (dict(mask=ctypes.c_void_p(4)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for k in ("depth", "geom", "cam", "rows", "off", "cnt", "scratch"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nclouds=0, **{k: None}) == -1             # nulls are refused even for an empty batch
    assert call(nclouds=0, mask=None) == 0                    # no mask, no cloud: nothing launched, no device touched


def test_check_depth_frames():
    from articulated_pose_amd.depth import check_depth_frames, pack_depth_frames
    u = np.arange(12, dtype=np.uint16).reshape(3, 4)
    m = u % 2 == 0
    cam = [1, 0, 0, 0, 1, 0]
    d, ms, org, nf, c = check_depth_frames([(u, m, (5, 6)), (u[:, ::2], None, (0, 0))], [1.0, 2.0], cam, 0.001, "uint16", 4)
    assert [x.shape for x in d] == [(3, 4), (3, 2)] and d[1].flags.c_contiguous and ms[1] is None and ms[0].dtype == np.uint8
    assert org.tolist() == [[5, 6], [0, 0]] and c.shape == (2, 7) and c.dtype == np.float32 and c[1, 6] == np.float32(0.001)
    pix, mask, geom = np.zeros(20, np.uint16), np.zeros(20, np.uint8), np.zeros((2, 5), np.int32)
    assert pack_depth_frames(d, ms, org, pix, mask, geom) == 18
    assert geom.tolist() == [[0, 3, 4, 5, 6], [12, 3, 2, 0, 0]] and mask[:18].tolist() == [1, 0] * 6 + [1] * 6
    assert pix[12:18].tolist() == [0, 2, 4, 6, 8, 10]
    per_frame = check_depth_frames([(u, None, (0, 0))] * 2, [1, 1], [cam, cam], [0.5, 0.25], np.uint16)[4]
    assert per_frame[:, 6].tolist() == [0.5, 0.25]
    f = u.astype(np.float32)
    bad = [dict(frames=[(f, None, (0, 0))]),                                       # a wrong dtype
           dict(frames=[(u[:0], None, (0, 0))]), dict(frames=[(u[0], None, (0, 0))]),  # an empty crop, a 1-d crop
           dict(frames=[(u, m[:2], (0, 0))]), dict(frames=[(u, m.astype(np.float32), (0, 0))]),      # a mask of another shape / a float mask
           dict(frames=[(u, None, (0.5, 0))]), dict(frames=[(u, None, 3)]), dict(frames=[(u, None)]), dict(frames=[]), dict(frames=u),
           dict(frames=[(u, None, (0, 0))] * 5),                                  # more than max_clouds
           dict(cameras=[1, 0, 0, 0, 1]), dict(cameras=[1, 0, np.nan, 0, 1, 0]), dict(cameras=[cam] * 2),
           dict(depth_scale=np.inf), dict(depth_scale=[1.0, 2.0]), dict(depth_scale=1e60), dict(norm_factors=[np.nan]),
           dict(norm_factors=[1.0, 1.0]), dict(depth_dtype="float64")]
    for kw in bad:
        args = dict(dict(frames=[(u, m, (0, 0))], norm_factors=[1.0], cameras=cam, depth_scale=1.0, depth_dtype="uint16", max_clouds=4), **kw)
        with pytest.raises(ValueError):
            check_depth_frames(**args)


def test_pipelines_refuse_unsupported_depth_combinations_before_gpu_work():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from test_sharded_stream_cpu import _FakeStreamPipeline
    base = dict(depth_capacity=4096, joint_source="predicted")
    for kw, msg in ((dict(joint_source="gt"), "predicted"), (dict(couple=False), "couple=True"), (dict(dense=True), "dense"),
                    (dict(raw_capacity=100), "raw_capacity"), (dict(depth_dtype="float64"), "depth_dtype"), (dict(depth_capacity=1), "depth_capacity"),
                    (dict(depth_capacity=1 << 30), "depth_capacity")):
        with pytest.raises(ValueError, match=msg):
            AncshPipeline(3, None, None, 2, 512, "cpu", **dict(base, **kw))
    with pytest.raises(ValueError, match="depth"):
        ShardedPipeline(3, None, None, 4, 512, "cpu", pipeline_factory=_FakeStreamPipeline, **base)
