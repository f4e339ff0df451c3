"""CPU tests of the annotated frames' images (no GPU): the symbol / ABI of ancsh_depth_annotated_images, its argument checks before any
launch, the annotated_images option in stream.check_options and the pipeline's guards, the result tuple's naming, and the numpy mirror
(tests/annotated_images_mirror.py) against the restatement of the annotation the CPU suite already uses."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import annotated_images_mirror as M
from test_depth_annotate_cpu import random_scene, restate_cloud, scene_table

NAME = "ancsh_depth_annotated_images"
P16 = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails its checks first
ANNOTATED = dict(depth_capacity=4096, joint_source="predicted", articulation=True, point_ground_truth=True, build_point_gt=True)


def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_14():
    from articulated_pose_amd import _lib
    from articulated_pose_amd import depth as D
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in declared_symbols() and NAME in exported and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME]) == 22
    assert _L().ancsh_abi_version() == 14
    assert (D.LABEL_VALUES, D.GT_IMAGE_VALUES, D.LABEL_NAN_BITS) == (7, 6, M.NAN_BITS)
    assert (M.SCENE_HEAD, M.SCENE_LINK, M.MAX_LINKS) == (D.SCENE_HEAD, D.SCENE_LINK, D.SCENE_MAX_LINKS)


def test_entry_rejects_bad_arguments_before_launch():
    L = _L()
    pointers = ("depth", "link", "geom", "scene", "off", "cnt", "scratch", "labels", "values", "gt", "dest", "il", "iv", "igl", "igv")

    def call(nclouds=2, kind=0, px=100, nchan=18, cap=100, icap=100, **p):
        p = dict({k: P16 for k in pointers}, **p)
        return L.ancsh_depth_annotated_images(nclouds, kind, p["depth"], p["link"], px, p["geom"], p["scene"], p["off"], p["cnt"], p["scratch"],
                                              p["labels"], p["values"], p["gt"], nchan, cap, p["dest"], p["il"], p["iv"], p["igl"], p["igv"],
                                              icap, None)
    for kw, msg in ((dict(nclouds=-1), b"bad shape"), (dict(nclouds=65536), b"65535"), (dict(kind=2), b"depth_type=2"),
                    (dict(kind=-1), b"depth_type=-1"), (dict(px=-1), b"pixel_capacity=-1"), (dict(px=1 << 30), b"pixel_capacity"),
                    (dict(cap=-1), b"capacity=-1 rows"), (dict(cap=1 << 30), b"capacity=1073741824 rows"),
                    (dict(nchan=9), b"gt_nchan=9"), (dict(icap=-1), b"image_capacity=-1"), (dict(icap=1 << 30), b"image_capacity=1073741824"),
                    (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(link=ctypes.c_void_p(4)), b"8-byte aligned"),
                    (dict(scene=ctypes.c_void_p(4)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        assert msg in L.ancsh_last_error() and b"depth_annotated_images" in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for k in pointers:
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nclouds=0, **{k: None}) == -1             # nulls are refused even for an empty batch
    for kind in (0, 1):
        assert call(nclouds=0, kind=kind) == 0                # both depth types; no cloud: nothing launched, no device touched
    assert call(nclouds=0, nchan=10, cap=0, icap=0, px=0) == 0


def test_check_options_accepts_the_option_exactly_on_annotated_frames():
    from articulated_pose_amd.stream import OPTION_FLAGS, RENDERED, check_options
    assert "annotated_images" in OPTION_FLAGS
    mesh, kin = (np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), np.zeros(1, np.int32)), np.zeros(672)
    for extra in (dict(), dict(keyed=True), dict(fit_quality=True, ground_truth=True, build_gt_pose=True), dict(range_guard=True),
                  dict(render_mesh=mesh), dict(render_mesh=mesh, kinematics=kin)):
        o = check_options(batch_size=2, annotated_images=True, **dict(ANNOTATED, **extra))
        assert o.annotated_images and o.link_counts and not o.label_images and not o.dense
        off = check_options(batch_size=2, **dict(ANNOTATED, **extra))
        assert not off.annotated_images and o._replace(annotated_images=False) == off       # nothing else moves
    assert RENDERED.startswith("depth_capacity")
    depth = dict(depth_capacity=4096, joint_source="predicted")
    for kw, missing in ((dict(), "depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True"),
                        (depth, "point_ground_truth=True, build_point_gt=True"), (dict(depth, label_images=True), "point_ground_truth=True, build_point_gt=True"),
                        (dict(raw_capacity=4096, articulation=True, point_ground_truth=True, build_point_gt=True), "depth_capacity=<pixels>$"),
                        (dict(raw_capacity=4096, dense=True), "depth_capacity=<pixels>, point_ground_truth=True, build_point_gt=True")):
        with pytest.raises(ValueError, match="annotated_images=True .* it needs " + missing):
            check_options(annotated_images=True, **kw)
    # label_images stays refused on annotated frames, with or without the new option
    for extra in (dict(), dict(annotated_images=True)):
        with pytest.raises(ValueError, match="label_images=True carries rows back to pixels in pixel order; the rows of annotated depth frames"):
            check_options(label_images=True, **dict(ANNOTATED, **extra))


def test_pipeline_refuses_the_option_before_gpu_work_and_the_output_on_a_pipeline_without_it():
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    with pytest.raises(ValueError, match="annotated_images=True .* it needs point_ground_truth=True, build_point_gt=True"):
        AncshPipeline(3, None, None, 2, 64, "cpu", depth_capacity=4096, joint_source="predicted", annotated_images=True)
    with pytest.raises(ValueError, match="label_images"):
        AncshPipeline(3, None, None, 2, 64, "cpu", label_images=True, annotated_images=True, **ANNOTATED)
    pipe = AncshPipeline.__new__(AncshPipeline)
    for opts in (check_options(batch_size=2, **ANNOTATED), check_options(batch_size=2, depth_capacity=4096, joint_source="predicted", label_images=True),
                 check_options(raw_capacity=100)):
        pipe.opts, pipe.B, pipe.K = opts, 2, 3
        with pytest.raises(RuntimeError) as e:
            pipe.retire(annotated_images=True)
        assert str(e.value) == ("retire(annotated_images=True) needs AncshPipeline(..., depth_capacity=<pixels>, point_ground_truth=True, "
                                "build_point_gt=True, annotated_images=True)")
        for method in ("stream_depth_batches", "stream_render_batches", "stream_posed_batches"):
            with pytest.raises(RuntimeError, match=r"%s\(annotated_images=True\) needs AncshPipeline" % method):
                next(getattr(pipe, method)([], annotated_images=True))


def test_results_name_the_images_behind_label_images():
    from articulated_pose_amd.stream import RESULT_NAMES, RESULT_ORDER, pack_results, result_names, unpack_results
    at = RESULT_NAMES.index("annotated_images")
    assert RESULT_NAMES[at - 1] == "label_images" and RESULT_NAMES[:at] + RESULT_NAMES[at + 1:] == RESULT_ORDER
    named = {k: k.upper() for k in RESULT_NAMES}
    assert result_names(annotated_images=True, counts=True, link_counts=True) == ["tag", "seed", "record", "annotated_images", "counts", "link_counts"]
    asked = dict(flags=True, articulation=True, annotated_images=True, counts=True, link_counts=True)
    got = pack_results(named, **asked)
    assert got == ("TAG", "SEED", "RECORD", "FLAGS", "ARTICULATION", "ANNOTATED_IMAGES", "COUNTS", "LINK_COUNTS")
    assert unpack_results(got, **asked)["annotated_images"] == "ANNOTATED_IMAGES"
    assert pack_results(named, counts=True) == ("TAG", "SEED", "RECORD", "COUNTS")          # not asked for: the tuple it always was


def test_cutter_returns_fresh_four_tuples():
    from articulated_pose_amd.depth import cut_annotated_images
    n = 3 + 2 * 5 + 4
    il, igl = np.arange(n, dtype=np.int32), -np.arange(n, dtype=np.int32)
    iv, igv = np.arange(n * 7, dtype=np.float32).reshape(n, 7), np.arange(n * 6, dtype=np.float32).reshape(n, 6)
    out = cut_annotated_images(il, iv, igl, igv, [(2, 5), (1, 4)], first=3)
    assert [tuple(a.shape for a in f) for f in out] == [((2, 5), (2, 5, 7), (2, 5), (2, 5, 6)), ((1, 4), (1, 4, 7), (1, 4), (1, 4, 6))]
    assert out[0][0][1, 2] == 3 + 7 and out[1][2][0, 1] == -(13 + 1) and out[1][3][0, 3, 5] == (16 * 6 + 5) and out[0][1][0, 0, 6] == 3 * 7 + 6
    out[0][0][:] = 99
    assert il[3] == 3                                                    # fresh arrays
    for bad in (dict(shapes=[(2, 5), (2, 4)]), dict(igl=igl[:-1]), dict(igv=igv[:, :5]), dict(igl=igl.astype(np.int64))):
        args = dict(dict(il=il, iv=iv, igl=igl, igv=igv, shapes=[(2, 5), (1, 4)]), **bad)
        with pytest.raises(ValueError):
            cut_annotated_images(args["il"], args["iv"], args["igl"], args["igv"], args["shapes"], first=3)


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_mirror_inverts_the_row_order_of_the_annotation_restatement(dtype):
    """arange(rows) scattered as the labels: the image then holds, at every valid pixel, the index of that pixel's row in the order
    dataset.pack_annotated_cloud gives the restated frame (lib/dataset.py:475-485), and -1 elsewhere."""
    from articulated_pose_amd.dataset import pack_annotated_cloud
    from test_depth_annotate_cpu import restate_frame, valid_depth
    rs = np.random.RandomState(7)
    parts_map, L = [[3], [0, 2]], 4                                      # link 1 is not used; ranks differ from the link indices
    for h, w, min_px in ((23, 31, 1), (5, 3, 1), (1, 7, 0), (12, 9, 40)):
        S = random_scene(rs, L)
        depth = rs.randint(1, 30000, (h, w)).astype(np.uint16) if dtype == "uint16" else rs.uniform(0.5, 3.0, (h, w)).astype(np.float32)
        depth[rs.uniform(size=(h, w)) < 0.1] = 0
        label = rs.randint(0, 6, (h, w)).astype(np.uint8)                # 4 and 5 are no links of the scene
        label[0, 0] = 255
        sc = scene_table(S, parts_map, min_link_pixels=min_px)
        assert M.link_order(sc) == [3, 0, 2]
        rows, n = M.pixel_rows(depth, label, sc)
        lab = np.where(label < L, label, -1).astype(np.int64)
        want, counts, pix = restate_cloud(S, depth, lab, (10, 20), parts_map, 1.0, min_px)
        if want is None:
            assert n == 0 and (rows == -1).all() and min_px == 40
            continue
        per = restate_frame(S, depth, lab, (10, 20))
        packed = pack_annotated_cloud({s: per[s][0] for s in per}, {s: per[s][1] for s in per}, parts_map)
        assert n == len(want) == len(packed) and np.array_equal(packed[:, :3], want[:, :3].astype(np.float32))
        gt = np.zeros((n, 18), np.float32)
        gt[:, 3], gt[:, 4:10] = packed[:, 6], packed[:, :6]
        il, iv, igl, igv = M.frame_images(rows, 0, np.arange(n, dtype=np.int32), np.zeros((n, 7), np.float32), gt, n)
        assert np.array_equal(il[pix[:, 0], pix[:, 1]], np.arange(n))   # row k of the packed cloud came from pixel pix[k]
        used = np.isin(label, [3, 0, 2]) & valid_depth(depth)
        assert used.sum() == n and (il[~used] == -1).all() and (igl[~used] == -1).all()
        assert (iv[~used].view(np.uint32) == M.NAN_BITS).all() and (igv[~used].view(np.uint32) == M.NAN_BITS).all()
        assert np.array_equal(igl[pix[:, 0], pix[:, 1]], packed[:, 6].astype(np.int32)) and np.array_equal(igv[pix[:, 0], pix[:, 1]], packed[:, :6])
        # rows at and beyond a capacity are cut
        if n <= 5:
            continue
        cut = M.frame_images(rows, 5, np.arange(n + 5, dtype=np.int32), np.zeros((n + 5, 7), np.float32), np.zeros((n + 5, 18), np.float32), n)[0]
        assert (cut[pix[-5:, 0], pix[-5:, 1]] == -1).all() and np.array_equal(cut[pix[:-5, 0], pix[:-5, 1]], 5 + np.arange(n - 5))
