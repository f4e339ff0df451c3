"""CPU (no GPU): the sensor table's packing and its rules, the option's place in check_options, and the numpy mirror of
ancsh_depth_sensor_model (tests/depth_sensor_mirror.py) validated on its own: identity, the hole share, the noise's moments, the edge rule on
a hand-made crop, the disparity steps, and the purity of the draws in the frame's global index."""
import numpy as np
import pytest

import depth_sensor_mirror as SM

DTYPES = {"uint16": np.uint16, "float32": np.float32}
INF = float("inf")


def scenes(n, depth_scale):
    s = np.zeros((n, SM.SCENE_WIDTH))
    s[:, 6] = depth_scale
    return s


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_pack_sensor_layout_and_refusals():
    from articulated_pose_amd.depth import SENSOR_WIDTH, check_sensor, pack_sensor
    t = pack_sensor(sigma=(0.001, 0.002, 0.003), z0=0.5, p_hole=0.1, p_edge=0.6, edge_rel=0.04, disparity=(35.0, 8), z_range=(0.2, 4.0))
    assert SENSOR_WIDTH == SM.SENSOR_WIDTH == 16 and t.dtype == np.float64 and t.shape == (16,)
    assert t.tolist() == [0.001, 0.002, 0.003, 0.5, 0.1, 0.6, 0.04, 35.0, 8.0, 0.2, 4.0, 0, 0, 0, 0, 0]
    ident = pack_sensor()
    assert ident.tolist() == [0, 0, 0, 0, 0, 0, 0.05, 0, 1, 0, INF, 0, 0, 0, 0, 0]
    assert pack_sensor(z0=-1.0)[3] == -1.0 and pack_sensor(p_hole=1.0, p_edge=1.0, edge_rel=0.0)[4:7].tolist() == [1.0, 1.0, 0.0]
    assert np.array_equal(check_sensor(t), t) and check_sensor(t) is not t and np.array_equal(check_sensor(t.tolist()), t)
    for kw in (dict(p_hole=-0.01), dict(p_hole=1.01), dict(p_hole=float("nan")), dict(p_edge=-1e-9), dict(p_edge=2), dict(p_edge=float("nan")),
               dict(sigma=(-1e-6, 0, 0)), dict(sigma=(0, -1, 0)), dict(sigma=(0, 0, -1)), dict(sigma=(INF, 0, 0)), dict(sigma=(0, float("nan"), 0)),
               dict(sigma=(0, 0)), dict(sigma=None), dict(z0=INF), dict(z0=float("nan")), dict(edge_rel=-0.1), dict(edge_rel=INF),
               dict(disparity=(-1.0, 4)), dict(disparity=(INF, 4)), dict(disparity=(30.0, 0.5)), dict(disparity=(30.0, 0)), dict(disparity=(30.0, INF)),
               dict(disparity=(30.0,)), dict(z_range=(2.0, 1.0)), dict(z_range=(-INF, 1.0)), dict(z_range=(float("nan"), 1.0)),
               dict(z_range=(0.0, float("nan"))), dict(z_range=(1.0,)), dict(p_hole="much")):
        with pytest.raises(ValueError, match="sensor"):
            pack_sensor(**kw)
    for k, v in ((0, -1.0), (4, 1.5), (5, -0.5), (6, -1.0), (7, -1.0), (8, 0.0), (9, -INF), (10, -1.0), (11, 1.0), (15, 1e-300), (2, float("nan"))):
        bad = ident.copy()
        bad[k] = v
        with pytest.raises(ValueError, match="sensor"):
            check_sensor(bad)
    for bad in (np.zeros(15), np.zeros((2, 16)), None, "table"):
        with pytest.raises(ValueError, match="sensor"):
            check_sensor(bad)


def test_the_option_is_one_rule_of_check_options():
    from articulated_pose_amd.depth import pack_mesh, pack_sensor
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import OPTION_FLAGS, check_options
    from test_pose_scene_cpu import kin_table
    from test_render_cpu import box_mesh, object_scene
    assert "sensor" in OPTION_FLAGS
    table = pack_sensor(sigma=(0.01, 0, 0), p_hole=0.1)
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    S = object_scene(np.random.RandomState(0), 1)
    kin = kin_table(S, dict(parents=[-1], kinds=["fixed"], joint_xyz=[(0, 0, 0)], joint_rpy=[(0, 0, 0)], joint_axis=[(0, 0, 0)]), [[0]])
    # valid on every annotated-frame pipeline: submitted, rendered, posed; with the images, keyed, guarded; and nothing else moves
    for extra in (dict(), dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(annotated_images=True, keyed=True),
                  dict(render_mesh=mesh, ground_truth=True, build_gt_pose=True, range_guard=True, fit_quality=True, joint_states=True)):
        off, on = check_options(batch_size=2, **dict(annotated, **extra)), check_options(batch_size=2, sensor=table, **dict(annotated, **extra))
        assert on.sensor and not off.sensor and on._replace(sensor=False) == off
    # anywhere else: ValueError that names what it needs
    for kw in (dict(), dict(raw_capacity=1000), dict(depth_capacity=4096, joint_source="predicted"),
               dict(depth_capacity=4096, joint_source="predicted", label_images=True),
               dict(raw_capacity=1000, articulation=True, point_ground_truth=True, build_point_gt=True)):
        with pytest.raises(ValueError, match="sensor .* depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True"):
            check_options(sensor=table, **kw)
        with pytest.raises(ValueError, match="sensor"):
            AncshPipeline(3, None, None, 2, 64, "cpu", sensor=table, **kw)
    # a table that is not one: refused with the table's own message
    for bad in (table[:15], np.where(np.arange(16) == 4, 1.5, table), "noisy"):
        with pytest.raises(ValueError, match="sensor"):
            check_options(sensor=bad, **annotated)


def test_entries_refuse_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device (no pointer is read on the host), so they are testable without a GPU.  Every call
    here has nframes == 0, which launches nothing -- after all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    cap = 4096
    good = dict(n=0, kind=0, d_in=0x10000, l_in=0x20000, cap=cap, geom=0x30000, scene=0x40000, sensor=0x50000, seed=0x60000, d_out=0x70000,
                l_out=0x80000)
    order = ("n", "kind", "d_in", "l_in", "cap", "geom", "scene", "sensor", "seed", "d_out", "l_out")
    for name in ("ancsh_depth_sensor_model", "ancsh_depth_sensor_model_keyed"):
        fn = getattr(L, name)
        call = lambda **over: fn(*[dict(good, **over)[k] for k in order], None)
        assert call() == 0
        for over, what in ((dict(n=-1), b"nframes"), (dict(n=65536), b"65535"), (dict(kind=2), b"depth_type"), (dict(cap=-1), b"pixel_capacity"),
                           (dict(cap=1 << 30), b"pixel_capacity"), (dict(d_in=None), b"null"), (dict(l_in=None), b"null"), (dict(geom=None), b"null"),
                           (dict(scene=None), b"null"), (dict(sensor=None), b"null"), (dict(seed=None), b"null"), (dict(d_out=None), b"null"),
                           (dict(l_out=None), b"null"), (dict(d_in=0x10008), b"aligned"), (dict(d_out=0x70002), b"aligned"),
                           (dict(l_in=0x20004), b"aligned"), (dict(l_out=0x80001), b"aligned"), (dict(scene=0x40004), b"aligned"),
                           (dict(sensor=0x50004), b"aligned"), (dict(seed=0x60004), b"aligned"),
                           (dict(d_out=0x10000), b"overlap"), (dict(d_out=0x10000 + 2 * cap - 16), b"overlap"), (dict(l_out=0x20000), b"overlap"),
                           (dict(l_out=0x20000 + cap - 8), b"overlap"), (dict(l_out=0x10000 + 2 * cap - 8), b"overlap"),
                           (dict(d_out=0x20000 - 16), b"overlap"), (dict(d_out=0x80000 - 16), b"overlap")):
            assert call(**over) == -1 and what in L.ancsh_last_error() and name[6:].encode() in L.ancsh_last_error(), (name, over, L.ancsh_last_error())
        # float32 pixels are 4 bytes wide: buffers that are apart as uint16 overlap
        assert call(kind=1, d_out=0x10000 + 2 * cap) == -1 and b"overlap" in L.ancsh_last_error()
        assert call(d_out=0x10000 + 2 * cap) == 0


# ---- the mirror -----------------------------------------------------------------------------------------------------------------------------
def _mixed_crop(rs, dtype, h, w):
    """A crop with surface, background and unusable pixels (zeros; float32: NaN, +Inf and negative values too)."""
    if dtype == "uint16":
        d = rs.randint(500, 3000, (h, w)).astype(np.uint16)
    else:
        d = rs.uniform(0.5, 3.0, (h, w)).astype(np.float32)
    lab = rs.randint(0, 3, (h, w)).astype(np.uint8)
    lab[rs.uniform(size=(h, w)) < 0.2] = 255
    bad = rs.uniform(size=(h, w)) < 0.15
    d[bad] = 0 if dtype == "uint16" else rs.choice(np.array([0.0, np.nan, np.inf, -1.5], np.float32), int(bad.sum()))
    return d, lab


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_identity_table_copies_every_byte(dtype):
    from articulated_pose_amd.depth import pack_sensor
    rs = np.random.RandomState(1)
    d, lab = _mixed_crop(rs, dtype, 9, 13)
    ident = pack_sensor()
    assert (ident[:6] == 0).all() and ident[10] == INF
    for scale in (1e-3, 1.0, 0.37):
        od, ol = SM.sensor_crop(d, lab, scale, ident, 12345, 3)
        assert od.tobytes() == d.tobytes() and ol.tobytes() == lab.tobytes()
    zero = np.zeros(16)
    zero[10] = INF                           # the all-zero table with z_far = +Inf, steps and edge_rel included
    od, ol = SM.sensor_crop(d, lab, 1e-3, zero, 7, 0)
    assert od.tobytes() == d.tobytes() and ol.tobytes() == lab.tobytes()


def _flat_crop(dtype, z=1.5, n=200):
    d = np.full((n, n), 1500 if dtype == "uint16" else z, DTYPES[dtype])
    return d, np.zeros((n, n), np.uint8), (1e-3 if dtype == "uint16" else 1.0)


def test_hole_share_of_a_flat_crop():
    from articulated_pose_amd.depth import pack_sensor
    d, lab, scale = _flat_crop("uint16")
    od, ol = SM.sensor_crop(d, lab, scale, pack_sensor(p_hole=0.25), 2024, 0)
    dropped = ol == 255
    assert ((od == 0) == dropped).all() and (od[~dropped] == 1500).all() and (ol[~dropped] == 0).all()
    share, tol = dropped.mean(), 4 * np.sqrt(0.25 * 0.75 / 40000)
    print("hole share", share, "+-", tol)
    assert abs(share - 0.25) <= tol


def test_noise_moments_of_a_flat_crop():
    from articulated_pose_amd.depth import pack_sensor
    d, lab, scale = _flat_crop("float32")
    od, ol = SM.sensor_crop(d, lab, scale, pack_sensor(sigma=(0.01, 0, 0)), 99, 1)
    assert (ol == 0).all() and od.dtype == np.float32
    e = (od.astype(np.float64) - 1.5) / 0.01
    print("noise mean", e.mean(), "variance", e.var())
    assert abs(e.mean()) <= 4 / np.sqrt(40000) and abs(e.var() - 1.0) <= 0.05
    assert np.abs(e).max() <= 2 * np.sqrt(3.0) + 1e-3        # Irwin-Hall of four: bounded


def test_edges_of_a_hand_made_crop():
    """A 6 x 6 crop: columns 0..2 at depth 1.0, columns 3..5 at 1.5 (a step far above edge_rel), the corner (0, 0) background.  With p_edge =
    1 exactly the pixels beside the step and beside the corner drop; the crop's border alone makes no edge."""
    from articulated_pose_amd.depth import pack_sensor
    d = np.full((6, 6), 1.0, np.float32)
    d[:, 3:] = 1.5
    lab = np.zeros((6, 6), np.uint8)
    lab[0, 0], d[0, 0] = 255, 0.0
    want = np.zeros((6, 6), bool)
    want[:, 2:4] = True                      # both sides of the step
    want[0, 1] = want[1, 0] = True           # the corner's neighbours
    od, ol = SM.sensor_crop(d, lab, 1.0, pack_sensor(p_edge=1.0, edge_rel=0.05), 5, 2)
    dropped = (ol == 255) & (lab != 255)
    assert np.array_equal(dropped, want), dropped.astype(int)
    assert ol[0, 0] == 255 and od[0, 0] == 0 and (od[~want] == d[~want]).all() and (od[want] == 0).all()
    for i, j in ((0, 5), (5, 0), (5, 5), (3, 0), (0, 4), (5, 1)):       # on the border, no discontinuity inside the crop: kept
        assert ol[i, j] == 0 and od[i, j] == d[i, j]
    # a step below edge_rel is no edge; p_edge = 0 evaluates nothing
    od2, ol2 = SM.sensor_crop(d, lab, 1.0, pack_sensor(p_edge=1.0, edge_rel=0.6), 5, 2)
    assert int(((ol2 == 255) & (lab != 255)).sum()) == 2
    od3, ol3 = SM.sensor_crop(d, lab, 1.0, pack_sensor(p_edge=0.0), 5, 2)
    assert od3.tobytes() == d.tobytes() and ol3.tobytes() == lab.tobytes()
    # an unusable depth under an object label is no surface either
    d4 = d.copy()
    d4[4, 5] = np.nan
    _, ol4 = SM.sensor_crop(d4, lab, 1.0, pack_sensor(p_edge=1.0), 5, 2)
    assert ol4[3, 5] == 255 and ol4[5, 5] == 255 and ol4[4, 5] == 0       # the neighbours drop; the pixel itself is copied verbatim


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_disparity_steps(dtype):
    from articulated_pose_amd.depth import pack_sensor
    rs = np.random.RandomState(4)
    qd, steps = 35.0, 8.0
    if dtype == "uint16":
        d, scale = rs.randint(400, 4000, (20, 20)).astype(np.uint16), 1e-3
    else:
        d, scale = rs.uniform(0.4, 4.0, (20, 20)).astype(np.float32), 1.0
    lab = np.zeros((20, 20), np.uint8)
    table = pack_sensor(disparity=(qd, steps))
    # z2 itself, before it is stored: the float64 value the mirror's step 7 gives
    z = d.astype(np.float64) * scale
    z2 = qd / (np.rint((qd / z) * steps) / steps)
    assert np.abs(qd / z2 * steps - np.rint(qd / z2 * steps)).max() <= 1e-9
    od, ol = SM.sensor_crop(d, lab, scale, table, 8, 0)
    assert (ol == 0).all()
    want = np.rint(z2 / scale).astype(np.uint16) if dtype == "uint16" else (z2 / scale).astype(np.float32)
    same = z2.view(np.int64) == z.view(np.int64)
    assert np.array_equal(np.where(same, d, want), od) and (od != d).any()
    # quantised depths are a fixed point: a second pass changes nothing that float32 / uint16 storage did not move
    if dtype == "float32":
        steps_out = qd / od.astype(np.float64) * steps
        assert np.abs(steps_out - np.rint(steps_out)).max() <= 1e-4    # float32 storage of z2: relative 6e-8 of up to ~700 steps
    # a depth beyond the last disparity step drops
    far = np.full((1, 1), 60000, np.uint16)
    assert SM.sensor_crop(far, lab[:1, :1], 1.0, pack_sensor(disparity=(1000.0, 1)), 0, 0)[1][0, 0] == 255


def test_z_range_and_store_range():
    from articulated_pose_amd.depth import pack_sensor
    d = np.array([[500, 1000, 2000, 3000]], np.uint16)
    lab = np.zeros((1, 4), np.uint8)
    od, ol = SM.sensor_crop(d, lab, 1e-3, pack_sensor(z_range=(1.0, 2.0)), 3, 0)
    assert od.tolist() == [[0, 1000, 2000, 0]] and ol.tolist() == [[255, 0, 0, 255]]
    # noise that carries a uint16 value out of 1..65535 drops the pixel
    big = np.full((8, 8), 65535, np.uint16)
    od, ol = SM.sensor_crop(big, np.zeros((8, 8), np.uint8), 1.0, pack_sensor(sigma=(5.0, 0, 0)), 3, 0)
    assert ((ol == 255) == (od == 0)).all() and (ol == 255).any() and (ol == 0).any()


def test_draws_follow_the_global_frame_index():
    from articulated_pose_amd.depth import pack_sensor
    rs = np.random.RandomState(6)
    table = pack_sensor(sigma=(0.002, 0.001, 0), z0=1.0, p_hole=0.2, p_edge=0.5, disparity=(35.0, 8))
    crops = [_mixed_crop(rs, "uint16", 7, 9) for _ in range(3)]
    cap = 3 * 63 + 11
    pix, lab = np.zeros(cap, np.uint16), np.full(cap, 255, np.uint8)
    geom = np.array([(2 + 66 * k, 7, 9, 0, 0) for k in range(3)], np.int32)
    for (d, l), g in zip(crops, geom):
        pix[g[0]:g[0] + 63], lab[g[0]:g[0] + 63] = d.reshape(-1), l.reshape(-1)
    sc = scenes(3, 1e-3)
    whole = SM.sensor_flat(pix, lab, geom, sc, table, 77, 0, fill=0x5A5A, label_fill=77)
    part = SM.sensor_flat(pix, lab, geom[1:], sc[1:], table, 77, 1, fill=0x5A5A, label_fill=77)
    lo = geom[1, 0]
    assert whole[0][lo:].tobytes() == part[0][lo:].tobytes() and whole[1][lo:].tobytes() == part[1][lo:].tobytes()
    assert (part[0][:lo] == 0x5A5A).all() and (whole[0][:2] == 0x5A5A).all() and (whole[1][65:68] == 77).all()     # pixels of no crop
    other = SM.sensor_flat(pix, lab, geom[1:], sc[1:], table, 77, 0, fill=0x5A5A, label_fill=77)
    assert other[0][lo:].tobytes() != part[0][lo:].tobytes()                                                         # another index, other draws
    frames = SM.sensor_frame_list([(d, l, (0, 0)) for d, l in crops], sc, table, 77, 0)
    assert all(np.array_equal(f[0].reshape(-1), whole[0][g[0]:g[0] + 63]) for f, g in zip(frames, geom))
    # refused crops write nothing
    none = SM.sensor_flat(pix, lab, np.array([(0, 0, 9, 0, 0), (0, 7, 0, 0, 0), (cap - 62, 7, 9, 0, 0), (-1, 7, 9, 0, 0)], np.int32), scenes(4, 1e-3),
                          table, 77, 0, fill=0x5A5A, label_fill=77)
    assert (none[0] == 0x5A5A).all() and (none[1] == 77).all()


def test_splitmix64_is_the_generator_of_the_pose_fit():
    """The published test vector of splitmix64 (seed 0: the first outputs of the reference implementation's stream are the function at 0 and
    at the golden-ratio increments)."""
    assert SM.splitmix64(0) == 0xE220A8397B1DCDAF
    assert SM.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    r = SM.draw(1, 2, 3, 0)
    assert r == SM.splitmix64(1 ^ SM.splitmix64(0xE000000000000000 | (2 << 36) | (3 << 4))) and 0 <= SM.uniform(r) < 1
