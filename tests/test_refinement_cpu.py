"""CPU (no GPU): render-and-compare ICP's place in the ABI and in check_options, the entries' argument checks before any launch, pack_refine's
checks, and the numpy mirror (tests/refinement_mirror.py) validated on its own on test_reprojection_cpu's frames: the exact record costs what
depth quantisation costs, perturbed poses come back to a strictly lower cost for every part, and the edge cases follow the header's rules.  The
perturbation and the table here are the GPU tests' too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refinement_mirror as RF
import reprojection_mirror as RP
from test_reprojection_cpu import DTYPES, SCALE, frames_problem, posed_object
from test_render_cpu import box_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = (("ancsh_refine_pass", 27), ("ancsh_refine_rec", 7))
P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first or has no frame


# ---- the table and the perturbation (shared with the GPU tests) ------------------------------------------------------------------------------
# Chosen so that the mirror alone brings EVERY part of these frames to a strictly lower cost (checked below, on the CPU): the frames are 64 x
# 64, a pixel is about 0.01 of the cloud's unit and a part about 30 pixels wide, so the truncation distance is 0.01 -- with the default 0.1 one
# pixel of lost silhouette costs more than the whole depth residual of a part -- and the poses are moved by 0.009 along the part's viewing ray
# (three hundredths of the object's extent, 0.32) and turned by 2 degrees about an axis in the image plane through the part's observed centroid.
# A larger shift, or a shift across the ray, makes the one-faced box slide along its face further than its silhouette forgives.
MAX_DIST, SHIFT, TILT_DEG, AXIS_PHASE = 0.01, 0.009, 2.0, 0.3


def refine_table(**over):
    from articulated_pose_amd.pose.refinement import pack_refine
    return pack_refine(**dict(dict(iters=3, max_dist=MAX_DIST), **over))


def centroids(scene, nf, frames, K):
    """Per (frame, part): the mean observed point in the scaled cloud's space; NaN for a part without a pixel."""
    out = np.full((len(frames), K, 3), np.nan)
    for f, (d, l, (r0, c0)) in enumerate(frames):
        sc = scene[f]
        img = RP.part_image(d, l, RP.link_parts(sc, K)[0])
        for j in range(K):
            ii, jj = np.nonzero(img == j)
            if len(ii):
                row, col = r0 + ii.astype(np.float64), c0 + jj.astype(np.float64)
                z = d[ii, jj].astype(np.float64) * sc[6]
                pts = np.stack([z * (sc[7] * col + sc[8] * row + sc[9]), -z * (sc[10] * col + sc[11] * row + sc[12]), z], 1)
                out[f, j] = np.float64(np.float32(nf[f])) * pts.mean(0)
    return out


def perturbed_record(rec, cen, shift=SHIFT, deg=TILT_DEG, phase=AXIS_PHASE):
    """Every pose of the record turned by `deg` about an axis in the image plane through its part's centroid (a different axis per frame, part
    and pose) and moved by `shift` along the centroid's ray: away from the camera for the baseline pose, towards it for the nonlinear one."""
    out = rec.copy()
    for f in range(rec.shape[0]):
        for j in range(rec.shape[1]):
            for v in range(2):
                p, c = rec[f, j, 13 * v:13 * v + 13], cen[f, j]
                if not (np.isfinite(p).all() and np.isfinite(c).all()):
                    continue
                ray = c / np.linalg.norm(c)
                e = np.cross(ray, [0.0, 1.0, 0.0])
                e /= np.linalg.norm(e)
                th = phase + 1.3 * (2 * j + v) + 0.7 * f
                ax = np.cos(th) * e + np.sin(th) * np.cross(ray, e)
                a = np.radians(deg)
                Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
                dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
                out[f, j, 13 * v:13 * v + 9] = (dR @ p[:9].reshape(3, 3)).reshape(9)
                out[f, j, 13 * v + 10:13 * v + 13] = dR @ (p[10:13] - c) + c + (shift if v == 0 else -shift) * ray
    return out


def refine_problem(K, dtype, sapien=False):
    """frames_problem and its exact and perturbed records: (problem tuple, exact (3, K, 26), perturbed (3, K, 26))."""
    prob = frames_problem(K, dtype, sapien=sapien)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    rec = RP.exact_record(render, scene, rigs, nf, kin, K)
    return prob, rec, perturbed_record(rec, centroids(scene, nf, frames, K))


def mirror(prob, rec, dtype, table, frames=None):
    mesh, kin, render, scene, rigs, nf, geom, cap, own = prob
    return RF.refine(mesh, render, scene, rigs, nf, rec, geom, own if frames is None else frames, dtype, table)


def behavioural_bars(columns, strict):
    """cost_best <= cost_start always, by construction; strict: < for every part and pose.  columns (n, K, 36)."""
    from articulated_pose_amd.pose.refinement import named_columns
    c = named_columns(columns)
    for v in ("baseline_", "nonlinear_"):
        start, best = c[v + "cost_start"], c[v + "cost_best"]
        assert np.isfinite(start).all() and (best <= start).all(), (v, start, best)
        assert ((c[v + "best_pass"] == 0) | (best < start)).all()
        if strict:
            assert (best < start).all() and (c[v + "best_pass"] >= 1).all(), (v, start, best)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose import refinement as R
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name, nargs in NAMES:
        assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.lib().ancsh_abi_version() == 14
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    for name, value in (("WIDTH", R.REFINE_WIDTH), ("SUMS", R.REFINE_SUMS), ("PARAMS", R.REFINE_PARAMS), ("MAX_ITERS", R.MAX_ITERS)):
        assert "#define ANCSH_REFINE_%s %d\n" % (name, value) in header
    assert R.REFINE_WIDTH == RF.WIDTH == 36 == len(R.COLUMN_NAMES) and R.REFINE_SUMS == RF.SUMS == 32 and R.BEST_WIDTH == RF.BEST == 18
    assert R.COLUMN_NAMES[R.COL_BASELINE] == "baseline_R00" and R.COLUMN_NAMES[R.COL_NONLINEAR + 13] == "nonlinear_cost_start"
    assert R.COLUMN_NAMES[17] == "baseline_passes_solved" and R.COLUMN_NAMES[R.COL_NONLINEAR + 9] == "nonlinear_s"
    rec = np.arange(2 * 3 * 77.0).reshape(2, 3, 77)
    named = R.named_columns(rec)
    assert named["baseline_R00"][1, 2] == 77 * 5 + 41 and named["nonlinear_passes_solved"][0, 0] == 76
    with pytest.raises(ValueError, match="36"):
        R.named_columns(np.zeros((2, 35)))
    got = R.refined_record(rec)
    assert got.shape == (2, 3, 26) and got[1, 2].tolist() == list(range(77 * 5 + 41, 77 * 5 + 54)) + list(range(77 * 5 + 59, 77 * 5 + 72))
    with pytest.raises(ValueError, match="62"):
        R.refined_record(np.zeros((2, 61)))
    src = open(os.path.join(os.path.dirname(HERE), "articulated-pose_amd", "csrc", "Makefile")).read()
    assert "refinement.hip" in src


def test_entries_refuse_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device (no pointer is read on the host); an accepted call here has nframes == 0, which launches
    nothing -- after all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    ptrs = ("verts", "tris", "tri_link", "od", "ol", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params", "pin", "pout", "best", "sums")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, kind=0, V=10, T=12, cap=4096, p=0, last=0, ld=26, pout=ctypes.c_void_p(32))
    order = ("n", "K", "kind", "verts", "tris", "tri_link", "V", "T", "od", "ol", "cap", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params",
             "p", "last", "pin", "ld", "pout", "best", "sums")
    run = lambda **over: L.ancsh_refine_pass(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(kind=1, p=8, last=1, ld=77, K=8, V=0, T=0) == 0
    odd = lambda a: ctypes.c_void_p(a)
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(kind=-1), b"depth_type=-1"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"),
                       (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T="), (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V="), (dict(p=-1), b"pass=-1"),
                       (dict(p=9), b"pass=9"), (dict(last=2), b"is_last=2"), (dict(ld=25), b"ld_in=25"), (dict(od=odd(17)), b"aligned"),
                       (dict(kind=1, pd=odd(18)), b"aligned"), (dict(verts=odd(18)), b"aligned"), (dict(tris=odd(18)), b"aligned"),
                       (dict(tri_link=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(nf=odd(18)), b"aligned"),
                       (dict(zb=odd(20)), b"aligned"), (dict(scene=odd(20)), b"aligned"), (dict(rt=odd(20)), b"aligned"),
                       (dict(params=odd(20)), b"aligned"), (dict(pin=odd(20)), b"aligned"), (dict(pout=odd(20)), b"aligned"),
                       (dict(best=odd(20)), b"aligned"), (dict(sums=odd(20)), b"aligned"), (dict(pout=P16), b"overlap")):
        assert run(**over) == -1 and what in L.ancsh_last_error() and b"refine_pass" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs:
        assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    good = dict(n=0, K=3, best=P16, carried=P16, ld=26, wide=ctypes.c_void_p(64))
    order = ("n", "K", "best", "carried", "ld", "wide")
    rec = lambda **over: L.ancsh_refine_rec(*[dict(good, **over)[k] for k in order], None)
    assert rec() == 0 and rec(K=8, ld=4096) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(ld=25), b"ld=25"),
                       (dict(ld=4097), b"ld=4097"), (dict(best=odd(4)), b"aligned"), (dict(carried=odd(4)), b"aligned"), (dict(wide=odd(4)), b"aligned"),
                       (dict(wide=P16), b"overlap")):
        assert rec(**over) == -1 and what in L.ancsh_last_error() and b"refine_rec" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ("best", "carried", "wide"):
        assert rec(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k


# ---- the table and the option ----------------------------------------------------------------------------------------------------------------
def test_pack_refine_checks_its_values():
    from articulated_pose_amd.pose.refinement import check_refine_table, pack_refine
    t = pack_refine()
    assert t.shape == (8,) and t.dtype == np.float64 and t[:4].tolist() == [3.0, 0.1, 0.1, 1e-3] and t[4] == np.radians(10.0) and t[5:].tolist() == [32.0, 0, 0]
    assert pack_refine(iters=8, max_dist=0.5, min_cos=0.0, damping=0.0, max_angle_deg=90.0, min_pixels=1)[0] == 8
    for kw, what in ((dict(iters=0), "iters"), (dict(iters=9), "iters"), (dict(iters=2.5), "iters"), (dict(iters=float("nan")), "iters"),
                     (dict(max_dist=0.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
                     (dict(min_cos=-0.1), "min_cos"), (dict(min_cos=1.5), "min_cos"), (dict(min_cos=float("nan")), "min_cos"),
                     (dict(damping=-1.0), "damping"), (dict(damping=float("inf")), "damping"), (dict(max_angle_deg=0.0), "max_angle_deg"),
                     (dict(max_angle_deg=91.0), "max_angle_deg"), (dict(max_angle_deg=float("nan")), "max_angle_deg"), (dict(min_pixels=0), "min_pixels"),
                     (dict(min_pixels=3.5), "min_pixels"), (dict(iters="many"), "numbers"), (dict(max_dist=None), "numbers")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            pack_refine(**kw)
    for bad in (np.zeros(7), np.zeros((2, 8)), "table", None):
        with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table"):
            check_refine_table(bad)
    reserved = pack_refine()
    reserved[7] = 1.0
    with pytest.raises(ValueError, match="reserved"):
        check_refine_table(reserved)


def test_the_option_is_one_rule_of_check_options():
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, pack_sensor
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.refinement import pack_refine
    from articulated_pose_amd.stream import RESULT_NAMES, Options, check_options
    assert Options._fields[-1] == "refine" and "record_refined" not in RESULT_NAMES and "refine" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    table = pack_refine()
    # valid on every pipeline that holds a mesh -- and nothing else moves
    for extra in (dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(render_mesh=pack_mesh_library([mesh, mesh])),
                  dict(render_mesh=mesh, sensor=pack_sensor(p_hole=0.1), annotated_images=True, keyed=True),
                  dict(render_mesh=mesh, ground_truth=True, build_gt_pose=True, range_guard=True, fit_quality=True, joint_states=True),
                  dict(render_mesh=mesh, reprojection=True)):
        off, on = check_options(batch_size=2, **dict(annotated, **extra)), check_options(batch_size=2, refine=table, **dict(annotated, **extra))
        assert on.refine is True and off.refine is False and on.record_key == "record_refined" and on.record_width == off.record_width + 36
        assert on._replace(refine=False, record_key=off.record_key, record_width=off.record_width) == off
    for fq in (False, True):
        for rp in (False, True):
            o = check_options(batch_size=2, render_mesh=mesh, refine=table, fit_quality=fq, reprojection=rp, **annotated)
            assert o.record_width == (39 if fq else 26) + 21 + (15 if rp else 0) + 36 and o.record_key == "record_refined", (fq, rp)
    # anywhere else: ValueError that names what is missing; a bad table is refused where it is given
    for kw in (dict(), dict(raw_capacity=1000), dict(depth_capacity=4096, joint_source="predicted"), annotated,
               dict(annotated, sensor=pack_sensor(p_hole=0.1)), dict(raw_capacity=1000, articulation=True, point_ground_truth=True, build_point_gt=True)):
        with pytest.raises(ValueError, match="refine=.* render_mesh"):
            check_options(refine=table, **kw)
        with pytest.raises(ValueError, match="render_mesh"):
            AncshPipeline(3, None, None, 2, 64, "cpu", refine=table, **kw)
    with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table"):
        check_options(batch_size=2, render_mesh=mesh, refine=np.zeros(5), **annotated)
    with pytest.raises(ValueError, match="refine: iters"):
        check_options(batch_size=2, render_mesh=mesh, refine=np.zeros(8), **annotated)
    with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, refine=table)
    with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", refine=table)


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_exact_poses_cost_what_depth_quantisation_costs(K, dtype):
    """With the exact record the two points of a pixel lie on one ray, |p - q| = nf |z_p - z_o| |(u, w, 1)|, and z_o is z_p through the
    frame's depth format: at most half a quantum for uint16 (plus the float32 rounding of z_p), two float32 roundings for float32.  So the
    quadratic part of the cost, sum r^2 / n_obs, is at most that distance squared.  The truncated part counts the observed pixels the pose
    does not explain: test_reprojection_cpu holds the exact record to an IoU >= 0.99, and min_cos = 0.1 drops only faces seen at under six
    degrees, which cover few pixels: at least nine in ten observed pixels are used.  The refinement keeps the pose or lowers the cost."""
    prob, rec, _ = refine_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    cols, sums, bounds, poses = mirror(prob, rec, dtype, table)
    behavioural_bars(cols, strict=False)
    for f, (d, l, (r0, c0)) in enumerate(frames):
        sc = scene[f]
        rows, cs = r0 + np.arange(d.shape[0])[:, None], c0 + np.arange(d.shape[1])[None, :]
        ray = np.sqrt((sc[7] * cs + sc[8] * rows + sc[9]) ** 2 + (sc[10] * cs + sc[11] * rows + sc[12]) ** 2 + 1.0).max()
        zmax = float(d.max()) * sc[6]
        dz = 0.5 * SCALE[dtype] + zmax * 2.0 ** -23 if dtype == "uint16" else 2 * zmax * 2.0 ** -23
        quantum = float(nf[f]) * dz * ray
        s0 = sums[0, f]                                                  # (K, 2, 32)
        print(f, "sum r^2 / n_obs", (s0[:, :, 27] / s0[:, :, 29]).ravel(), "allowed", quantum ** 2, "used / observed", (s0[:, :, 28] / s0[:, :, 29]).ravel())
        assert (s0[:, :, 29] > 0).all() and (s0[:, :, 27] / s0[:, :, 29] <= quantum ** 2).all()
        assert (s0[:, :, 28] >= 0.9 * s0[:, :, 29]).all()
        assert (cols[f].reshape(K, 2, 18)[:, :, 13] <= quantum ** 2 + MAX_DIST ** 2 * 0.1).all()


@pytest.mark.parametrize("K,dtype,sapien", [(2, "uint16", False), (2, "float32", False), (3, "uint16", False), (3, "float32", False), (3, "uint16", True)],
                         ids=["K2-uint16", "K2-float32", "K3-uint16", "K3-float32", "K3-sapien-rotation"])
def test_perturbed_poses_come_back_to_a_strictly_lower_cost(K, dtype, sapien):
    """The two behavioural bars of the GPU test, met by the mirror alone with MAX_DIST, SHIFT, TILT_DEG and AXIS_PHASE above: cost_best <
    cost_start for every part and pose, and cost_best <= cost_start by construction.  No bar on the pose error per degree of freedom: a part
    that shows only flat faces has unobservable directions."""
    from articulated_pose_amd.pose.refinement import named_columns
    prob, rec, per = refine_problem(K, dtype, sapien)
    assert np.isfinite(per).all() and (np.abs(per - rec).max(axis=(0, 1))[[10, 11, 12, 23, 24, 25]] > 0).all()
    cols, sums, bounds, poses = mirror(prob, per, dtype, refine_table())
    c = named_columns(cols)
    print("start", c["baseline_cost_start"].ravel(), c["nonlinear_cost_start"].ravel(), "\nbest ", c["baseline_cost_best"].ravel(),
          c["nonlinear_cost_best"].ravel(), "\npass ", c["baseline_best_pass"].ravel(), c["nonlinear_best_pass"].ravel())
    behavioural_bars(cols, strict=True)
    assert (c["baseline_passes_solved"] == 3).all() and (c["baseline_s"] == per[:, :, 9]).all() and (c["nonlinear_s"] == per[:, :, 22]).all()
    # the best row is one of the evaluated poses, its cost that pass's cost, and the columns are the best block
    for f in range(3):
        for j in range(K):
            for v in range(2):
                b = cols[f, j, 18 * v:18 * v + 18]
                p = int(b[16])
                assert b[:13].tobytes() == poses[p, f, j, 13 * v:13 * v + 13].tobytes() and b[14] == sums[p, f, j, v, 30] and b[15] == sums[p, f, j, v, 28]
                assert b[13] == sums[0, f, j, v, 30] and b[14] == np.nanmin(sums[:, f, j, v, 30])
                R = b[:9].reshape(3, 3)                                  # the quaternion update keeps R a rotation to rounding
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-13


def test_edge_cases_follow_the_headers_rules():
    """A part with no observed pixel, a prediction that misses the crop, n_used just below and just at min_pixels, a NaN pose, a zero norm
    factor, and the link in no part."""
    K, dtype = 3, "uint16"
    prob, rec, per = refine_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = refine_table()
    parts, _ = RP.link_parts(scene[0], K)
    # the link in no part: its pixels are observed by no part
    d2, l2 = frames[2][0], frames[2][1]
    assert parts[3] == -1 and (l2 == 3).sum() > 0
    base = mirror(prob, per, dtype, table)
    for j in range(K):
        img = RP.part_image(d2, l2, parts) == j
        assert base[1][0, 2, j, 0, 29] == img.sum() and not (img & (l2 == 3)).any()
    # frame 0: part 1's pixels are erased from the observation; frame 1, part 0, nonlinear: the prediction misses the crop; frame 1, part 2,
    # baseline: a NaN pose; frame 2: a zero norm factor
    obs = [list(fr) for fr in frames]
    lab0 = obs[0][1].copy()
    lab0[np.isin(lab0, np.nonzero(parts == 1)[0])] = 255
    obs[0][1] = lab0
    bad = per.copy()
    bad[1, 0, 13 + 10] += 10.0
    bad[1, 2, 4] = np.nan
    nf2 = nf.copy()
    nf2[2] = 0.0
    cols, sums, bounds, poses = RF.refine(mesh, render, scene, rigs, nf2, bad, geom, [tuple(o) for o in obs], dtype, table)
    b = cols.reshape(3, K, 2, 18)
    for v in range(2):                                                   # no observed pixel: C = NaN, nothing to solve, the pose as it came
        assert (sums[:, 0, 1, v, 29] == 0).all() and np.isnan(sums[:, 0, 1, v, 30]).all() and (sums[:, 0, 1, v, 31] == 0).all()
        assert b[0, 1, v, :13].tobytes() == bad[0, 1, 13 * v:13 * v + 13].tobytes() and np.isnan(b[0, 1, v, 13:15]).all()
        assert b[0, 1, v, 15:].tolist() == [0, 0, 0]
    assert (sums[:, 1, 0, 1, 28] == 0).all() and (sums[:, 1, 0, 1, 29] > 0).all()      # the prediction misses the crop: every observed pixel is missed
    assert b[1, 0, 1, :13].tobytes() == bad[1, 0, 13:26].tobytes() and b[1, 0, 1, 13:].tolist() == [sums[0, 1, 0, 1, 30]] * 2 + [0, 0, 0]
    assert abs(b[1, 0, 1, 13] - table[1] * table[1]) <= 1e-18 and (poses[:, 1, 0, 13:26] == bad[1, 0, 13:26]).all()
    assert np.isnan(b[1, 2, 0]).all() and np.isnan(sums[:, 1, 2, 0, :31]).all() and (sums[:, 1, 2, 0, 31] == 0).all()      # the NaN pose
    assert np.array_equal(poses[-1, 1, 2, :13], bad[1, 2, :13], equal_nan=True) and np.isfinite(b[1, 2, 1]).all()
    assert np.isnan(b[2]).all() and poses[-1, 2].tobytes() == bad[2].tobytes()                                                # the zero norm factor
    assert np.isfinite(b[0, 0]).all() and np.isfinite(b[0, 2]).all() and np.isfinite(b[1, 1]).all()                          # the neighbours are untouched
    assert b[0, 0].tobytes() == base[0].reshape(3, K, 2, 18)[0, 0].tobytes()
    # min_pixels: with the threshold at the first pass's n_used the pass solves, one above it the pose passes through
    n0 = base[1][0, 0, 0, 0, 28]
    at, above = (mirror(prob, per, dtype, refine_table(iters=1, min_pixels=n)) for n in (n0, n0 + 1))
    assert at[1][0, 0, 0, 0, 31] == 1 and at[0][0, 0, 17] == 1 and at[3][1, 0, 0, :13].tobytes() != per[0, 0, :13].tobytes()
    assert above[1][0, 0, 0, 0, 31] == 0 and above[0][0, 0, 17] == 0 and above[3][1, 0, 0, :13].tobytes() == per[0, 0, :13].tobytes()
    assert above[0][0, 0, 16] == 0 and above[0][0, 0, 13] == above[0][0, 0, 14] == at[0][0, 0, 13]


def test_solve_matches_a_float64_solver_and_the_update_is_a_rigid_motion():
    """The mirror's Cholesky against numpy's solver on a pass's own system, and the update applied to points: c' = dR (c - centre) + centre + dt."""
    K, dtype = 2, "uint16"
    prob, rec, per = refine_problem(K, dtype)
    table = refine_table(max_angle_deg=90.0, max_dist=MAX_DIST)
    cols, sums, bounds, poses = mirror(prob, per, dtype, table)
    S, pose = sums[0, 0, 1, 0], per[0, 1, :13]
    ok, out = RF.solve_update(S, pose, table)
    assert ok and sums[0, 0, 1, 0, 31] == 1 and out.tobytes() == poses[1, 0, 1, :13].tobytes()
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[:21]
    A = A + np.triu(A, 1).T
    xi = np.linalg.solve(A + np.diag(table[3] * np.diag(A) + 1e-12), -S[21:27])
    dn = np.linalg.norm(xi[3:])
    xi = xi * min(1.0, table[1] / dn)
    c = np.array(RF.centre(pose))
    R0, R1, s = pose[:9].reshape(3, 3), out[:9].reshape(3, 3), pose[9]
    dR = R1 @ R0.T
    w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2
    assert np.abs(dR @ dR.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(dR) - 1) < 1e-15
    assert np.abs(w - xi[:3]).max() <= 1e-9 + np.linalg.norm(xi[:3]) ** 3          # the quaternion is the exponential map to second order
    x = np.random.RandomState(0).uniform(0, 1, (5, 3))
    before, after = s * x @ R0.T + pose[10:13], s * x @ R1.T + out[10:13]
    assert np.abs(after - ((before - c) @ dR.T + c + xi[3:])).max() < 1e-12
