"""CPU (no GPU): the silhouette term of render-and-compare ICP.  Its two entries' place in the ABI and their argument checks before any launch,
pack_refine(silhouette=...) and the option table, and the mirror (tests/silhouette_mirror.py) validated on its own on test_reprojection_cpu's
frames: the field against an independent brute force, the exact record (no far pixel, the cost of today within what boundary pixels can cost,
best-of), the behavioural bar -- poses shifted across the ray come back, which the plain loop does not do -- and the existing perturbation,
which must still end strictly lower for every part.  The table and the perturbation here are the GPU tests' too."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import refinement_mirror as RF
import reprojection_mirror as RP
import silhouette_mirror as SM
from test_refinement_cpu import MAX_DIST, behavioural_bars, centroids, mirror, refine_problem, refine_table
from test_reprojection_cpu import posed_object
from test_render_cpu import box_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = (("ancsh_silhouette_field", 10), ("ancsh_refine_pass_sil", 28))
P16 = ctypes.c_void_p(16)     # a non-null, aligned pointer that is never dereferenced: every call below fails its checks first or has no frame

# ---- the table (shared with the GPU tests) ----------------------------------------------------------------------------------------------------
# test_refinement_cpu's truncation distance (a pixel is about 0.01 of the cloud's unit) with six passes, because a step's translation is
# clamped to max_dist and the larger shift is four of them; weight 1 (an overhang pixel's miss counts like a depth pixel's); dist = 0.1, ten
# pixels, well beyond both shifts, so no pixel is far; slack = 0: these frames come from the renderer that draws the predictions, so there is
# no raster disagreement to forgive, and with slack = 1 a part is left hanging over by up to a pixel -- half of the smaller shift; min_pixels =
# 12, because a part of 80 pixels that has slid off its observation by four pixels keeps fewer than 32 rows of either kind.
WEIGHT, DIST, SLACK, ITERS, MIN_PIXELS = 1.0, 0.1, 0.0, 6, 12
SHIFTS = (0.02, 0.04)
CASES = [(K, dtype, shift) for K in (2, 3) for dtype in ("uint16", "float32") for shift in SHIFTS]
IDS = ["K%d-%s-shift%g" % c for c in CASES]


def silhouette_table(**over):
    from articulated_pose_amd.pose.refinement import pack_refine
    kw = dict(dict(iters=ITERS, max_dist=MAX_DIST, min_pixels=MIN_PIXELS, silhouette=dict(weight=WEIGHT, dist=DIST, slack=SLACK)), **over)
    return pack_refine(**kw)


@functools.lru_cache(maxsize=None)
def problem(K, dtype, sapien=False):
    """refine_problem and the observed centroids, computed once and shared (nobody writes to them)."""
    prob, rec, per = refine_problem(K, dtype, sapien)
    return prob, rec, per, centroids(prob[3], prob[5], prob[8], K)


def refined(cols):
    return np.concatenate([cols[..., :13], cols[..., 18:31]], -1)


def sil_mirror(prob, rec, dtype, table):
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    return SM.refine(mesh, render, scene, rigs, nf, rec, geom, frames, dtype, table)


def lateral_bar(ratios_sil, ratios_plain):
    """The bar of the issue on the (n, K, 2) ratios lateral error / shift: the median at most 0.5, and no more triples above 1.0 than the
    plain loop leaves."""
    s, p = ratios_sil.ravel(), ratios_plain.ravel()
    print("silhouette: median %.3f, at or below 0.5: %d, above 1.0: %d (worst %.2f);  plain: median %.3f, above 1.0: %d (worst %.2f);  of %d"
          % (np.median(s), (s <= 0.5).sum(), (s > 1.0).sum(), s.max(), np.median(p), (p > 1.0).sum(), p.max(), s.size))
    assert np.isfinite(s).all() and np.median(s) <= 0.5, np.sort(s)
    assert (s > 1.0).sum() <= (p > 1.0).sum(), (np.sort(s), np.sort(p))


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
    assert _lib.lib().ancsh_abi_version() == 14 and len(_lib.SIGNATURES["ancsh_refine_pass"]) == 27
    header = open(os.path.join(os.path.dirname(HERE), "include", "ancsh_hip.h")).read()
    for name, value in (("SIL_SUMS", R.REFINE_SIL_SUMS), ("SIL_PARAMS", R.REFINE_SIL_PARAMS), ("SUMS", R.REFINE_SUMS), ("PARAMS", R.REFINE_PARAMS)):
        assert "#define ANCSH_REFINE_%s %d\n" % (name, value) in header
    assert R.REFINE_SIL_SUMS == SM.SUMS == 36 and R.REFINE_SIL_PARAMS == SM.PARAMS == 16 and R.FIELD_SENTINEL == SM.SENTINEL == -32768
    assert R.SIL_SUMS_COLUMNS["n_sil"] == 33 and R.SIL_SUMS_COLUMNS["n_far"] == 34 and R.SIL_SUMS_COLUMNS["mm"] == 32


def test_entries_refuse_bad_arguments_before_any_launch():
    """EINVAL paths return before touching the device (no pointer is read on the host); an accepted call here has nframes == 0, which launches
    nothing -- after all the checks, so a call that is wrongly accepted returns 0 and fails the test."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    odd = lambda a: ctypes.c_void_p(a)
    ptrs = ("verts", "tris", "tri_link", "od", "ol", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params", "field", "pin", "pout", "best", "sums")
    good = dict({k: P16 for k in ptrs}, n=0, K=3, kind=0, V=10, T=12, cap=4096, p=0, last=0, ld=26, pout=ctypes.c_void_p(32))
    order = ("n", "K", "kind", "verts", "tris", "tri_link", "V", "T", "od", "ol", "cap", "zb", "pd", "pl", "geom", "scene", "rt", "nf", "params",
             "field", "p", "last", "pin", "ld", "pout", "best", "sums")
    run = lambda **over: L.ancsh_refine_pass_sil(*[dict(good, **over)[k] for k in order], None)
    assert run() == 0 and run(kind=1, p=8, last=1, ld=77, K=8, V=0, T=0) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(kind=-1), b"depth_type=-1"), (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"),
                       (dict(T=-1), b"T=-1"), (dict(T=1 << 24), b"T="), (dict(V=-1), b"V=-1"), (dict(V=1 << 24), b"V="), (dict(p=-1), b"pass=-1"),
                       (dict(p=9), b"pass=9"), (dict(last=2), b"is_last=2"), (dict(ld=25), b"ld_in=25"), (dict(od=odd(17)), b"aligned"),
                       (dict(kind=1, pd=odd(18)), b"aligned"), (dict(verts=odd(18)), b"aligned"), (dict(tris=odd(18)), b"aligned"),
                       (dict(tri_link=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(nf=odd(18)), b"aligned"),
                       (dict(field=odd(18)), b"aligned"), (dict(zb=odd(20)), b"aligned"), (dict(scene=odd(20)), b"aligned"),
                       (dict(rt=odd(20)), b"aligned"), (dict(params=odd(20)), b"aligned"), (dict(pin=odd(20)), b"aligned"),
                       (dict(pout=odd(20)), b"aligned"), (dict(best=odd(20)), b"aligned"), (dict(sums=odd(20)), b"aligned"), (dict(pout=P16), b"overlap")):
        assert run(**over) == -1 and what in L.ancsh_last_error() and b"refine_pass_sil" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ptrs:
        assert run(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    good = dict(n=0, K=3, kind=0, od=P16, ol=P16, cap=4096, geom=P16, scene=P16, field=P16)
    order = ("n", "K", "kind", "od", "ol", "cap", "geom", "scene", "field")
    fld = lambda **over: L.ancsh_silhouette_field(*[dict(good, **over)[k] for k in order], None)
    assert fld() == 0 and fld(K=8, kind=1, cap=0) == 0 and fld(K=1, ol=odd(17)) == 0
    for over, what in ((dict(n=-1), b"nframes"), (dict(n=32768), b"32767"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"), (dict(kind=2), b"depth_type=2"),
                       (dict(cap=-1), b"pixel_capacity"), (dict(cap=1 << 29), b"pixel_capacity"), (dict(od=odd(17)), b"aligned"),
                       (dict(kind=1, od=odd(18)), b"aligned"), (dict(geom=odd(18)), b"aligned"), (dict(field=odd(18)), b"aligned"),
                       (dict(scene=odd(20)), b"aligned")):
        assert fld(**over) == -1 and what in L.ancsh_last_error() and b"silhouette_field" in L.ancsh_last_error(), (over, L.ancsh_last_error())
    for k in ("od", "ol", "geom", "scene", "field"):
        assert fld(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k


# ---- the table and the option ----------------------------------------------------------------------------------------------------------------
def test_pack_refine_checks_the_silhouette_values_and_passes_plain_tables_through():
    from articulated_pose_amd.pose.refinement import check_refine_table, pack_refine
    plain = pack_refine(iters=5, max_dist=0.02)
    assert pack_refine(iters=5, max_dist=0.02, silhouette=None).tobytes() == plain.tobytes() and plain.shape == (8,)
    assert check_refine_table(plain).tobytes() == plain.tobytes() and check_refine_table(plain) is not plain
    t = pack_refine(iters=5, max_dist=0.02, silhouette=dict(weight=2.0, dist=0.05, slack=0.5))
    assert t.shape == (16,) and t.dtype == np.float64 and t[:8].tobytes() == plain.tobytes() and t[8:].tolist() == [2.0, 0.05, 0.5, 0, 0, 0, 0, 0]
    assert pack_refine(silhouette=dict(dist=0.05))[8:11].tolist() == [1.0, 0.05, 1.0] and pack_refine(silhouette=(3.0, 0.2))[8:11].tolist() == [3.0, 0.2, 1.0]
    assert pack_refine(silhouette=dict(dist=1e-3, slack=0))[10] == 0 and check_refine_table(t).tobytes() == t.tobytes()
    for sil, what in ((dict(weight=0.0, dist=0.1), "weight"), (dict(weight=-1.0, dist=0.1), "weight"), (dict(weight=float("nan"), dist=0.1), "weight"),
                      (dict(weight=float("inf"), dist=0.1), "weight"), (dict(dist=0.0), "dist"), (dict(dist=float("inf")), "dist"),
                      (dict(dist=float("nan")), "dist"), (dict(dist=0.1, slack=-0.5), "slack"), (dict(dist=0.1, slack=float("nan")), "slack"),
                      (dict(weight=1.0), "dist"), (dict(dist=0.1, reach=2), "silhouette takes"), ((1.0, 0.0), "dist"), ((0.0, 0.1), "weight"),
                      (dict(dist="far"), "silhouette"), (5.0, "silhouette")):
        with pytest.raises(ValueError, match="refine: .*" + what):
            pack_refine(silhouette=sil)
    with pytest.raises(ValueError, match="refine: iters"):
        pack_refine(iters=0, silhouette=(1.0, 0.1))
    for bad in (np.zeros(7), np.zeros(15), np.zeros(17), np.zeros((2, 16))):
        with pytest.raises(ValueError, match=r"refine: one \(8,\) float64 table"):
            check_refine_table(bad)
    for at in (6, 7, 11, 15):
        reserved = t.copy()
        reserved[at] = 1.0
        with pytest.raises(ValueError, match="reserved"):
            check_refine_table(reserved)


def test_the_term_is_one_more_value_of_the_refine_option():
    from articulated_pose_amd.depth import pack_mesh, pack_sensor
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pose.refinement import pack_refine
    from articulated_pose_amd.stream import RESULT_NAMES, Options, check_options
    assert Options._fields[-2:] == ("silhouette", "refine") and "silhouette" not in RESULT_NAMES
    annotated = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)
    mesh = pack_mesh([box_mesh([0, 0, 0], [1, 1, 1])])
    kin, _ = posed_object(np.random.RandomState(0), 3, "uint16")
    plain, sil = pack_refine(), silhouette_table()
    for extra in (dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin), dict(render_mesh=mesh, reprojection=True),
                  dict(render_mesh=mesh, sensor=pack_sensor(p_hole=0.1), annotated_images=True, keyed=True),
                  dict(render_mesh=mesh, ground_truth=True, build_gt_pose=True, range_guard=True, fit_quality=True, joint_states=True)):
        off, on = check_options(batch_size=2, refine=plain, **dict(annotated, **extra)), check_options(batch_size=2, refine=sil, **dict(annotated, **extra))
        assert on.silhouette is True and off.silhouette is False and on.refine is True and on._replace(silhouette=False) == off
        assert check_options(batch_size=2, **dict(annotated, **extra)).silhouette is False
    with pytest.raises(ValueError, match="refine=.* render_mesh"):
        check_options(refine=sil, **annotated)
    with pytest.raises(ValueError, match="refine: silhouette weight"):
        check_options(batch_size=2, render_mesh=mesh, refine=np.r_[plain, np.zeros(8)], **annotated)
    with pytest.raises(ValueError, match="ShardedPipeline .* refine=.* render_mesh"):
        ShardedPipeline(3, None, None, 4, 64, "cpu", raw_capacity=1000, refine=sil)


# ---- the mirror: the field --------------------------------------------------------------------------------------------------------------------
def brute_field(mask):
    """The definition, pixel by pixel: the observed pixel of least (squared distance, row, column)."""
    h, w = mask.shape
    seen = [(int(r), int(c)) for r, c in zip(*np.nonzero(mask))]
    out = np.full((h, w, 2), SM.SENTINEL, np.int16)
    for i in range(h):
        for jj in range(w):
            if seen:
                _, r, c = min(((r - i) ** 2 + (c - jj) ** 2, r, c) for r, c in seen)
                out[i, jj] = r - i, c - jj
    return out


def test_the_field_is_the_nearest_observed_pixel_under_the_tie_rule():
    """The mirror's vectorised search against the definition, on hand-made masks where ties abound and on a frame's own parts."""
    rs = np.random.RandomState(3)
    masks = [np.zeros((5, 7), bool), np.ones((4, 3), bool), np.indices((6, 9)).sum(0) % 2 == 0, rs.rand(9, 11) < 0.15, np.zeros((1, 1), bool), np.ones((1, 6), bool)]
    corner = np.zeros((7, 5), bool)
    corner[6, 4] = True
    prob, rec, per, cen = problem(3, "uint16")
    img = RP.part_image(prob[8][1][0], prob[8][1][1], RP.link_parts(prob[3][1], 3)[0])
    for m in masks + [corner] + [img == j for j in range(3)]:
        got = SM.field_of_mask(m)
        assert got.dtype == np.int16 and got.tobytes() == brute_field(m).tobytes(), m.shape
    chk = SM.field_of_mask(masks[2])
    assert chk[0, 1].tolist() == [0, -1] and chk[1, 0].tolist() == [-1, 0] and chk[1, 2].tolist() == [-1, 0] and chk[0, 0].tolist() == [0, 0]
    assert (SM.field_of_mask(masks[0]) == SM.SENTINEL).all() and (SM.field_of_mask(masks[1]) == 0).all()
    flat = SM.field_flat(prob[8], prob[3], prob[6], 3, prob[7], fill=-7)
    s, h, w = (int(v) for v in prob[6][1][:3])
    assert flat.shape == (3, prob[7]) and (flat[:, :3] == -7).all() and (flat[:, s - 1] == -7).all()
    word = int(flat[2, s + 5 * w + 9])
    assert [np.int16(word & 0xffff), np.int16((word >> 16) & 0xffff)] == SM.field_of_mask(img == 2)[5, 9].tolist()


# ---- the mirror: the loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_exact_poses_cost_what_they_cost_today_plus_what_boundary_pixels_can_cost(K, dtype):
    """With the exact record no pixel is far, and the cost exceeds today's by at most weight^2 (share of boundary pixels) (pixel footprint)^2:
    an exact pose's prediction can leave the observed part only through raster disagreement, one pixel at the part's boundary, so at most as
    many overhang pixels as the part has boundary pixels (observed pixels with a 4-neighbour that is not the part's), each at most one pixel
    diagonal from an observed pixel: m <= nf z_max sqrt(2) pitch, pitch the larger of the camera matrix's column and row steps.  Best-of holds."""
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    table = silhouette_table()
    cols, sums, bounds, poses = sil_mirror(prob, rec, dtype, table)
    plain = mirror(prob, rec, dtype, refine_table(iters=ITERS))[1]
    behavioural_bars(cols, strict=False)
    assert (sums[..., 34] == 0).all() and sums.shape == (ITERS + 1, 3, K, 2, 36) and (sums[..., 35] == 0).all()
    for f, (d, l, _) in enumerate(frames):
        sc = scene[f]
        img = RP.part_image(d, l, RP.link_parts(sc, K)[0])
        pitch = max(np.hypot(sc[7], sc[10]), np.hypot(sc[8], sc[11]))
        foot = float(nf[f]) * float(d.max()) * sc[6] * np.sqrt(2.0) * pitch
        for j in range(K):
            m = np.pad(img == j, 1)
            inner = m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
            share = ((img == j) & ~inner).sum() / (img == j).sum()
            extra = sums[0, f, j, :, 30] - plain[0, f, j, :, 30]
            print(f, j, "extra cost", extra, "allowed", WEIGHT ** 2 * share * foot ** 2, "n_sil", sums[0, f, j, :, 33])
            assert (extra >= 0).all() and (extra <= WEIGHT ** 2 * share * foot ** 2).all()
            assert (sums[0, f, j, :, 33] <= ((img == j) & ~inner).sum()).all()
    assert sums[0, ..., :30].tobytes() == plain[0, ..., :30].tobytes() or (sums[0, ..., 33] > 0).any()      # no overhang row: today's sums


@pytest.mark.parametrize("K,dtype,shift", CASES, ids=IDS)
def test_poses_shifted_across_the_ray_come_back(K, dtype, shift):
    """The behavioural bar.  Every pose of the exact record is moved by `shift` (2 and 4 pixels) perpendicular to its part's centroid ray, no
    tilt.  The lateral error of a refined pose is how far it carries the part's observed centroid from where the exact pose has it, across the
    ray.  With the term: the median over (frame, part, pose) of error / shift is at most 0.5 and no more triples end above 1.0 than with the
    plain loop.  The plain loop with test_refinement_cpu's table does not meet the median bar: it cannot see the error it is asked to correct."""
    prob, rec, per, cen = problem(K, dtype)
    lat = SM.lateral_record(rec, cen, shift)
    assert np.abs(SM.lateral_errors(rec, lat, cen) / shift - 1.0).max() < 1e-9
    cols = sil_mirror(prob, lat, dtype, silhouette_table())[0]
    p_cols = mirror(prob, lat, dtype, refine_table())[0]
    behavioural_bars(cols, strict=False)
    r_sil, r_plain = SM.lateral_errors(rec, refined(cols), cen) / shift, SM.lateral_errors(rec, refined(p_cols), cen) / shift
    lateral_bar(r_sil, r_plain)
    assert not np.median(r_plain) <= 0.5, np.sort(r_plain.ravel())


@pytest.mark.parametrize("K,dtype,sapien", [(2, "uint16", False), (2, "float32", False), (3, "uint16", False), (3, "float32", False), (3, "uint16", True)],
                         ids=["K2-uint16", "K2-float32", "K3-uint16", "K3-float32", "K3-sapien-rotation"])
def test_the_existing_perturbation_still_ends_strictly_lower(K, dtype, sapien):
    """test_refinement_cpu's perturbation (along the ray, tilted) with the term on: cost_best < cost_start for every part and pose, on the
    new measure; the best row is one of the evaluated poses and its cost that pass's."""
    prob, rec, per, cen = problem(K, dtype, sapien)
    cols, sums, bounds, poses = sil_mirror(prob, per, dtype, silhouette_table())
    behavioural_bars(cols, strict=True)
    for f in range(3):
        for j in range(K):
            for v in range(2):
                b = cols[f, j, 18 * v:18 * v + 18]
                p = int(b[16])
                assert b[:13].tobytes() == poses[p, f, j, 13 * v:13 * v + 13].tobytes() and b[14] == sums[p, f, j, v, 30] and b[15] == sums[p, f, j, v, 28]
                assert b[13] == sums[0, f, j, v, 30] and b[14] == np.nanmin(sums[:, f, j, v, 30])
                assert sums[p, f, j, v, 30] == SM.cost(sums[p, f, j, v], silhouette_table())


def test_overhang_rules_far_pixels_occlusion_and_the_solve_threshold():
    """A prediction entirely beside the observed part: every predicted pixel over background is far (dist below the gap), gives no row and is
    charged dist^2; with dist above the gap the same pixels give rows and the pass solves on them alone (no depth row: n_used = 0, min_pixels
    met only through n_sil).  Another part observed in front of the prediction is an occlusion and gives nothing."""
    K, dtype = 3, "uint16"
    prob, rec, per, cen = problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    side = SM.lateral_record(rec, cen, 0.6)                              # sixty pixels: beside the object wherever it still hits the crop
    near, wide = silhouette_table(iters=1, silhouette=dict(weight=WEIGHT, dist=0.05, slack=0.0)), silhouette_table(iters=1, max_dist=2.0, min_pixels=8, silhouette=dict(weight=WEIGHT, dist=5.0, slack=0.0))
    s_near = sil_mirror(prob, side, dtype, near)[1]
    s_wide = sil_mirror(prob, side, dtype, wide)[1]
    seen = s_near[0, ..., 34] > 0
    assert seen.any() and (s_near[0, ..., 33][seen] == 0).all() and (s_near[0, ..., 28][seen] == 0).all() and (s_near[0, ..., 31][seen] == 0).all()
    want = (MAX_DIST ** 2 * s_near[0, ..., 29] + WEIGHT ** 2 * 0.05 ** 2 * s_near[0, ..., 34]) / s_near[0, ..., 29]
    assert np.abs(s_near[0, ..., 30] - want)[seen].max() <= 1e-15
    rows = seen & (s_wide[0, ..., 33] >= 8)
    assert rows.any() and (s_wide[0, ..., 33][seen] == s_near[0, ..., 34][seen]).all() and (s_wide[0, ..., 34] == 0).all()
    assert (s_wide[0, ..., 28][rows] == 0).all() and (s_wide[0, ..., 31][rows] == 1).all()
    obs, hidden = occluded_frames(prob)
    assert hidden > 0
    ray = cen[0, 0] / np.linalg.norm(cen[0, 0])
    for sign, more in ((+1.0, False), (-1.0, True)):                     # behind the other part: an occlusion; in front of it: an overhang
        moved = rec.copy()
        moved[0, 0, 10:13] += sign * 0.05 * ray
        S1, _ = SM.evaluate(mesh, render, scene, rigs, nf, moved, geom, obs, silhouette_table())
        S0, _ = SM.evaluate(mesh, render, scene, rigs, nf, moved, geom, frames, silhouette_table())
        n1, n0 = S1[0, 0, 0, 33] + S1[0, 0, 0, 34], S0[0, 0, 0, 33] + S0[0, 0, 0, 34]
        assert S1[0, 0, 0, 29] == S0[0, 0, 0, 29] - hidden and ((n1 > n0) if more else (n1 == n0)), (sign, n1, n0)
    obs2 = [tuple(fr) for fr in frames]
    parts, _ = RP.link_parts(scene[0], K)
    lab = obs2[0][1].copy()
    lab[np.isin(lab, np.nonzero(parts == 0)[0])] = 255                   # part 0 has no observed pixel: the sentinel, nothing to pull towards
    obs2[0] = (obs2[0][0], lab, obs2[0][2])
    S, _ = SM.evaluate(mesh, render, scene, rigs, nf, rec, geom, obs2, silhouette_table())
    assert S[0, 0, 0, 29] == 0 and S[0, 0, 0, 33] + S[0, 0, 0, 34] == 0 and np.isnan(S[0, 0, 0, 30])


def occluded_frames(prob, K=3):
    """frames_problem's frames with the upper half of part 0's pixels in frame 0 relabelled as a link of part 1, at their own depth: another
    part observed where part 0 is predicted -> (frames, how many pixels)."""
    frames, scene = prob[8], prob[3]
    parts, _ = RP.link_parts(scene[0], K)
    d, l, origin = frames[0]
    img = RP.part_image(d, l, parts)
    rows = np.nonzero((img == 0).any(1))[0]
    upper = (img == 0) & (np.arange(img.shape[0])[:, None] < (rows[0] + rows[-1] + 1) // 2)
    lab = l.copy()
    lab[upper] = int(np.nonzero(parts == 1)[0][0])
    return [(d, lab, origin)] + [tuple(fr) for fr in frames[1:]], int(upper.sum())
