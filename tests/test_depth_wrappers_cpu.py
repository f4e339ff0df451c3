"""What the device wrappers of the depth front end (depth.py, pose/reprojection.py) refuse and what they pass on: _lib.call is replaced by a
recorder and torch.Tensor.is_cuda, for the duration of a test, by a property that is true unless the tensor carries the marker below, so
nothing is launched and no GPU is needed.  The first tests make one good call per wrapper and variant: the entry, the scalars and which
tensor's pointer stands where.  BAD holds one bad argument (or two, to pin which is reported) per `raise` of each wrapper, WANT the exception
and message of each.  WANT is written out, not derived from the code under test: it is what the wrappers raised while each of them still
spelled its checks out itself."""
import numpy as np
import pytest
import torch

from articulated_pose_amd import _lib, dataset, depth
from articulated_pose_amd.pose import reprojection

MARK = "_test_on_host"          # a tensor with this attribute set reads is_cuda = False under the `calls` fixture
B, PIXELS, ROWS, K = 2, 31, 33, 2       # crops of 4 x 4 and 3 x 5 in a 31-pixel buffer: ragged, the second start non-zero
GEOM = [[0, 4, 4, 0, 0], [16, 3, 5, 2, 1]]
TRIANGLE = (np.eye(3), np.array([[0, 1, 2]]))
NO_CPU = "articulated-pose_amd ops run on the MI355X only (no CPU fallback in the product path)"
CPU_TENSOR = "articulated-pose_amd ops run on the MI355X only: got a CPU tensor (no CPU fallback in the product path)"


@pytest.fixture()
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda t: not getattr(t, MARK, False)))
    return rec


def inputs(kind="uint16"):
    """Fresh tensors for every wrapper's arguments, by the wrappers' own argument names."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype)
    pix = torch.int16 if kind == "uint16" else torch.float32
    return dict(
        depth=z((PIXELS,), pix), mask=torch.ones((PIXELS,), dtype=torch.uint8), labels=z((PIXELS,), torch.uint8),
        geom=torch.tensor(GEOM, dtype=torch.int32), cam=z((B, 7), torch.float32), scene=z((B, 240), torch.float64),
        render=z((B, 208), torch.float64), dest=z((B,), torch.int32), offsets=z((B + 1,), torch.int32), counts=z((B,), torch.int32),
        row_labels=z((ROWS,), torch.int32), row_values=z((ROWS, 7), torch.float32), gt_rows=z((ROWS, 18), torch.float32),
        small_scratch=z((B * 64,), torch.int32), link_scratch=z((B * 64 * 16,), torch.int32), zbuf=z((PIXELS,), torch.int64),
        bounds=z((B, 4), torch.int32), sensor=z((16,), torch.float64), seed=z((1,), torch.int64), key=z((4,), torch.int32),
        mesh=depth.mesh_to_device(depth.pack_mesh([TRIANGLE]), "cpu"),
        library=depth.mesh_to_device(depth.pack_mesh_library([[TRIANGLE], [TRIANGLE, TRIANGLE]]), "cpu"),
        kin=z((672,), torch.float64), kin_stack=z((2, 672), torch.float64), pose=z((B, 32), torch.float64),
        rig=z((B, dataset.RIG_WIDTH(K)), torch.float64), norm_factor=z((B,), torch.float32), record=z((B, K, 26), torch.float64),
        pred_depth=z((2 * PIXELS,), pix), pred_labels=z((2 * PIXELS,), torch.uint8))


# wrapper -> (function, the names in inputs() of its positional arguments, keyword arguments {keyword: name in inputs()})
WRAPPERS = {
    "unproject": (depth.depth_unproject, ("depth", "mask", "geom", "cam"), dict(scratch="small_scratch")),
    "label_images": (depth.depth_label_images, ("depth", "mask", "geom", "dest", "offsets", "row_labels", "row_values"),
                     dict(scratch="small_scratch")),
    "annotate": (depth.depth_annotate, ("depth", "labels", "geom", "scene"), dict(scratch="link_scratch")),
    "sensor": (depth.depth_sensor_model, ("depth", "labels", "geom", "scene", "sensor", "seed"), {}),
    "sensor_keyed": (depth.depth_sensor_model, ("depth", "labels", "geom", "scene", "sensor", "key"), {}),
    "annotated_images": (depth.depth_annotated_images, ("depth", "labels", "geom", "scene", "dest", "offsets", "counts", "row_labels",
                                                        "row_values", "gt_rows"), dict(scratch="link_scratch")),
    "render": (depth.render_depth, ("mesh", "geom", "render", "dtype"), dict(scratch="zbuf", pixel_capacity="pixels")),
    "render_lib": (depth.render_depth, ("library", "geom", "render", "dtype"), dict(scratch="zbuf", pixel_capacity="pixels")),
    "pose_scene": (depth.pose_scene_build, ("kin", "pose"), {}),
    "pose_scene_lib": (depth.pose_scene_build, ("kin_stack", "pose"), {}),
    "centre": (depth.centre_crop_origins, ("mesh", "geom", "render"), dict(scratch="bounds")),
    "centre_lib": (depth.centre_crop_origins, ("library", "geom", "render"), dict(scratch="bounds")),
    "reproject_build": (reprojection.reproject_scene_build, ("render", "scene", "rig", "norm_factor", "record", "geom", "pixels"), {}),
    "reproject_compare": (reprojection.reproject_compare, ("depth", "labels", "pred_depth", "pred_labels", "geom", "scene", "record"), {}),
}


def run(wrapper, kind="uint16", mutate=None):
    """Call `wrapper` on inputs(kind), after mutate(them) -> (them, what it returned)."""
    fn, names, kw = WRAPPERS[wrapper]
    t = inputs(kind)
    t.update(dtype=kind, pixels=PIXELS)
    if mutate is not None:
        mutate(t)
    return t, fn(*(t[n] for n in names), **{k: t[n] for k, n in kw.items() if n in t})


def ptrs(*tensors):
    return tuple(t.data_ptr() for t in tensors)


def filled(t, shape, dtype, value):
    same = torch.isnan(t).all() if value != value else (t == value).all()
    return tuple(t.shape) == shape and t.dtype == dtype and bool(same)


# ---- one good call per wrapper and variant --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_unproject(calls, kind):
    t, (rows, offsets, counts) = run("unproject", kind)
    (name, args), = calls
    assert name == "ancsh_depth_unproject_stream" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, int(kind == "float32")) + ptrs(t["depth"], t["mask"]) + (PIXELS,) + ptrs(t["geom"], t["cam"], rows) + (PIXELS,) \
        + ptrs(offsets, counts, t["small_scratch"])
    assert filled(rows, (PIXELS, 3), torch.float32, 0) and filled(offsets, (B + 1,), torch.int32, 0) and filled(counts, (B,), torch.int32, 0)


def test_unproject_without_mask_and_with_capacity(calls):
    t, (rows, _, _) = run("unproject", mutate=lambda t: t.update(mask=None))
    assert calls[0][1][3] == 0 and calls[0][1][8] == PIXELS
    calls.clear()
    rows = depth.depth_unproject(t["depth"], None, t["geom"], t["cam"], capacity=7)[0]
    assert calls[0][1][8] == 7 and tuple(rows.shape) == (7, 3)


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_label_images(calls, kind):
    t, (img_labels, img_values) = run("label_images", kind)
    (name, args), = calls
    assert name == "ancsh_depth_label_images" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, int(kind == "float32")) + ptrs(t["depth"], t["mask"]) + (PIXELS,) \
        + ptrs(t["geom"], t["offsets"], t["small_scratch"], t["row_labels"], t["row_values"]) + (ROWS,) \
        + ptrs(t["dest"], img_labels, img_values) + (PIXELS,)
    assert filled(img_labels, (PIXELS,), torch.int32, -1) and filled(img_values, (PIXELS, 7), torch.float32, float("nan"))


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_annotate(calls, kind):
    t, (rows, offsets, counts, link_counts) = run("annotate", kind)
    (name, args), = calls
    assert name == "ancsh_depth_annotate_stream" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, int(kind == "float32")) + ptrs(t["depth"], t["labels"]) + (PIXELS,) + ptrs(t["geom"], t["scene"], rows) + (PIXELS,) \
        + ptrs(offsets, counts, link_counts, t["link_scratch"])
    assert filled(rows, (PIXELS, 7), torch.float32, 0) and filled(offsets, (B + 1,), torch.int32, 0)
    assert filled(counts, (B,), torch.int32, 0) and filled(link_counts, (B, 16), torch.int32, 0)
    calls.clear()
    rows = depth.depth_annotate(t["depth"], t["labels"], t["geom"], t["scene"], capacity=ROWS)[0]
    assert calls[0][1][8] == ROWS and tuple(rows.shape) == (ROWS, 7)


@pytest.mark.parametrize("wrapper, kind, entry", [("sensor", "uint16", "ancsh_depth_sensor_model"),
                                                  ("sensor_keyed", "float32", "ancsh_depth_sensor_model_keyed")])
def test_sensor_model(calls, wrapper, kind, entry):
    t, (depth_out, labels_out) = run(wrapper, kind)
    (name, args), = calls
    assert name == entry and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, int(kind == "float32")) + ptrs(t["depth"], t["labels"]) + (PIXELS,) \
        + ptrs(t["geom"], t["scene"], t["sensor"], t["key" if wrapper == "sensor_keyed" else "seed"], depth_out, labels_out)
    assert filled(depth_out, (PIXELS,), t["depth"].dtype, 0) and filled(labels_out, (PIXELS,), torch.uint8, 255)
    assert depth_out.data_ptr() != t["depth"].data_ptr() and labels_out.data_ptr() != t["labels"].data_ptr()


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_annotated_images(calls, kind):
    t, out = run("annotated_images", kind)
    (name, args), = calls
    assert name == "ancsh_depth_annotated_images" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, int(kind == "float32")) + ptrs(t["depth"], t["labels"]) + (PIXELS,) \
        + ptrs(t["geom"], t["scene"], t["offsets"], t["counts"], t["link_scratch"], t["row_labels"], t["row_values"], t["gt_rows"]) \
        + (18, ROWS) + ptrs(t["dest"], *out) + (PIXELS,)
    assert filled(out[0], (PIXELS,), torch.int32, -1) and filled(out[1], (PIXELS, 7), torch.float32, float("nan"))
    assert filled(out[2], (PIXELS,), torch.int32, -1) and filled(out[3], (PIXELS, 6), torch.float32, float("nan"))


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_render_mesh(calls, kind):
    t, (d, lab) = run("render", kind)
    (name, args), = calls
    assert name == "ancsh_render_depth_labels" and len(args) == len(_lib.SIGNATURES[name]) - 1
    verts, tris, tri_link, V, T = t["mesh"]
    assert (V, T) == (3, 1)
    assert args == (B, int(kind == "float32")) + ptrs(verts, tris, tri_link) + (3, 1) + ptrs(t["geom"], t["render"], d, lab, t["zbuf"]) + (PIXELS,)
    assert filled(d, (PIXELS,), t["depth"].dtype, 0) and filled(lab, (PIXELS,), torch.uint8, 255)


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_render_library(calls, kind):
    t, (d, lab) = run("render_lib", kind)
    (name, args), = calls
    assert name == "ancsh_render_depth_labels_lib" and len(args) == len(_lib.SIGNATURES[name]) - 1
    lib = t["library"]
    verts, tris, tri_link, V, T = lib
    assert (V, T, lib.ninst, lib.Tmax) == (9, 3, 2, 2)            # instances of one and two triangles: ninst = 2, Tmax = 2
    assert args == (B, int(kind == "float32")) + ptrs(verts, tris, tri_link) + (9, 3) + ptrs(lib.tri_off) + (2, 2) \
        + ptrs(t["geom"], t["render"], d, lab, t["zbuf"]) + (PIXELS,)
    assert filled(d, (PIXELS,), t["depth"].dtype, 0) and filled(lab, (PIXELS,), torch.uint8, 255)


def test_render_into_out(calls):
    t = inputs("float32")
    got = depth.render_depth(t["mesh"], t["geom"], t["render"], "float32", out=(t["depth"], t["labels"]))
    assert ptrs(*got) == ptrs(t["depth"], t["labels"]) == calls[0][1][9:11] and calls[0][1][12] == PIXELS


def test_pose_scene_build(calls):
    t, (render, scene) = run("pose_scene")
    (name, args), = calls
    assert name == "ancsh_pose_scene_build" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B,) + ptrs(t["kin"], t["pose"], render, scene)
    assert (tuple(render.shape), tuple(scene.shape), render.dtype, scene.dtype) == ((B, 208), (B, 240), torch.float64, torch.float64)


def test_pose_scene_build_library(calls):
    t, (render, scene) = run("pose_scene_lib")
    (name, args), = calls
    assert name == "ancsh_pose_scene_build_lib" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B,) + ptrs(t["kin_stack"]) + (2,) + ptrs(t["pose"], render, scene)
    assert (tuple(render.shape), tuple(scene.shape), render.dtype, scene.dtype) == ((B, 208), (B, 240), torch.float64, torch.float64)


def test_centre_crop_origins(calls):
    t, geom = run("centre")
    (name, args), = calls
    assert name == "ancsh_render_centre_crops" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B,) + ptrs(*t["mesh"][:3]) + (3, 1) + ptrs(t["render"], t["geom"], t["bounds"]) and geom is t["geom"]


def test_centre_crop_origins_library(calls):
    t, geom = run("centre_lib")
    (name, args), = calls
    assert name == "ancsh_render_centre_crops_lib" and len(args) == len(_lib.SIGNATURES[name]) - 1
    lib = t["library"]
    assert args == (B,) + ptrs(*lib[:3]) + (9, 3) + ptrs(lib.tri_off) + (2,) + ptrs(t["render"], t["geom"], t["bounds"]) and geom is t["geom"]


def test_reproject_scene_build(calls):
    t, (render_out, geom_out) = run("reproject_build")
    (name, args), = calls
    assert name == "ancsh_reproject_scene_build" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, K) + ptrs(t["render"], t["scene"], t["rig"]) + (dataset.RIG_WIDTH(K),) + ptrs(t["norm_factor"], t["record"]) + (26,) \
        + ptrs(t["geom"]) + (PIXELS,) + ptrs(render_out, geom_out)
    assert filled(render_out, (2 * B, 208), torch.float64, 0) and filled(geom_out, (2 * B, 5), torch.int32, 0)


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_reproject_compare(calls, kind):
    t, wide = run("reproject_compare", kind)
    (name, args), = calls
    assert name == "ancsh_reproject_compare_rec" and len(args) == len(_lib.SIGNATURES[name]) - 1
    assert args == (B, K, int(kind == "float32")) + ptrs(t["depth"], t["labels"]) + (PIXELS,) \
        + ptrs(t["pred_depth"], t["pred_labels"], t["geom"], t["scene"], t["record"]) + (26,) + ptrs(wide)
    assert (tuple(wide.shape), wide.dtype) == ((B, K, 26 + 15), torch.float64)


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------------------
def on_host(*names):
    """The named tensors are not on the device (a mesh: its vertices -- the tensor that names the mesh's device --, or by index)."""
    def mutate(t):
        for n in names:
            n, i = n if isinstance(n, tuple) else (n, 0)
            setattr(t[n][i] if isinstance(t[n], tuple) else t[n], MARK, True)
    return mutate


def to(name, fn, *more):
    """The named argument replaced by fn(it); more = further (name, fn) pairs, flat."""
    def mutate(t):
        for n, f in zip((name,) + more[0::2], (fn,) + more[1::2]):
            t[n] = f(t[n])
    return mutate


def mesh_with(i, fn):
    """A mesh's i-th tensor replaced, its class and attributes kept."""
    def change(m):
        new = depth.DeviceMesh(m[:i] + (fn(m[i]),) + m[i + 1:])
        new.tri_off, new.host_tri_off, new.ninst, new.Tmax = m.tri_off, m.host_tri_off, m.ninst, m.Tmax
        return new
    return change


def lib_with_tri_off(fn):
    def change(m):
        new = mesh_with(0, lambda v: v)(m)
        new.tri_off = fn(m.tri_off)
        return new
    return change


none = lambda t: None
wide = lambda t: t.double() if t.dtype != torch.float64 else t.float()       # another dtype
longer = lambda t: torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype)
strided = lambda t: torch.zeros((t.shape[0], 2) + tuple(t.shape[1:]), dtype=t.dtype)[:, 0]      # the same shape, not contiguous
matrix = lambda t: t.reshape(1, -1)
short = lambda t: t[:-1]
out_as = lambda *outs: (lambda t: t.update(out=outs))

BAD = {
    # depth_unproject: no check of out or scratch, and no device check behind the first tensor
    "unproject-host": ("unproject", on_host("depth")),
    "unproject-depth-dtype": ("unproject", to("depth", wide)),
    "unproject-depth-2d": ("unproject", to("depth", matrix)),
    "unproject-depth-strided": ("unproject", to("depth", strided)),
    "unproject-mask-dtype": ("unproject", to("mask", wide)),
    "unproject-mask-length": ("unproject", to("mask", longer)),
    "unproject-geom-dtype": ("unproject", to("geom", wide)),
    "unproject-geom-width": ("unproject", to("geom", lambda g: g[:, :4].contiguous())),
    "unproject-cam-frames": ("unproject", to("cam", longer)),
    "unproject-cam-strided": ("unproject", to("cam", strided)),
    "unproject-depth-and-mask": ("unproject", to("depth", wide, "mask", wide)),
    "unproject-mask-and-cam": ("unproject", to("mask", longer, "cam", wide)),
    "unproject-host-and-depth": ("unproject", lambda t: (to("depth", matrix)(t), on_host("depth")(t))),
    "unproject-mask-host-passes": ("unproject", on_host("mask", "geom", "cam")),
    # depth_label_images
    "label_images-host": ("label_images", on_host("depth")),
    "label_images-depth": ("label_images", to("depth", wide)),
    "label_images-mask": ("label_images", to("mask", short)),
    "label_images-geom": ("label_images", to("geom", strided)),
    "label_images-dest": ("label_images", to("dest", longer)),
    "label_images-offsets": ("label_images", to("offsets", short)),
    "label_images-dest-and-offsets": ("label_images", to("dest", wide, "offsets", wide)),
    "label_images-labels-2d": ("label_images", to("row_labels", matrix)),
    "label_images-values-width": ("label_images", to("row_values", lambda v: v[:, :6].contiguous())),
    "label_images-values-rows": ("label_images", to("row_values", longer)),
    "label_images-scratch-none": ("label_images", to("small_scratch", none)),
    "label_images-scratch-short": ("label_images", to("small_scratch", short)),
    "label_images-scratch-dtype": ("label_images", to("small_scratch", lambda s: s.long())),
    "label_images-out-dtype": ("label_images", out_as(torch.zeros(5), torch.zeros((5, 7)))),
    "label_images-out-rows": ("label_images", out_as(torch.zeros(5, dtype=torch.int32), torch.zeros((6, 7)))),
    "label_images-values-and-scratch": ("label_images", to("row_values", longer, "small_scratch", none)),
    "label_images-later-host": ("label_images", on_host("row_values")),
    "label_images-mask-host": ("label_images", on_host("mask")),
    "label_images-scratch-and-host": ("label_images", lambda t: (to("small_scratch", short)(t), on_host("geom")(t))),
    # depth_annotate
    "annotate-host": ("annotate", on_host("depth")),
    "annotate-depth": ("annotate", to("depth", strided)),
    "annotate-labels-none": ("annotate", to("labels", none)),
    "annotate-labels-dtype": ("annotate", to("labels", wide)),
    "annotate-geom": ("annotate", to("geom", longer)),
    "annotate-scene-dtype": ("annotate", to("scene", wide)),
    "annotate-scene-width": ("annotate", to("scene", lambda s: s[:, :208].contiguous())),
    "annotate-rows": ("annotate", out_as(torch.zeros((9, 3)), torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                         torch.zeros((2, 16), dtype=torch.int32))),
    "annotate-link_counts": ("annotate", out_as(torch.zeros((9, 7)), torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                                torch.zeros((2, 8), dtype=torch.int32))),
    "annotate-scratch-short": ("annotate", to("link_scratch", short)),
    "annotate-scratch-dtype": ("annotate", to("link_scratch", lambda s: s.long())),
    "annotate-labels-and-scene": ("annotate", to("labels", short, "scene", wide)),
    "annotate-later-host": ("annotate", on_host("scene")),
    "annotate-scratch-and-host": ("annotate", lambda t: (to("link_scratch", short)(t), on_host("labels")(t))),
    # depth_sensor_model
    "sensor-host": ("sensor", on_host("depth")),
    "sensor-depth": ("sensor", to("depth", wide)),
    "sensor-labels": ("sensor", to("labels", none)),
    "sensor-geom-scene": ("sensor", to("scene", longer)),
    "sensor-table-dtype": ("sensor", to("sensor", wide)),
    "sensor-table-length": ("sensor", to("sensor", short)),
    "sensor-seed-length": ("sensor", to("seed", longer)),
    "sensor-seed-dtype": ("sensor", to("seed", lambda s: s.double())),
    "sensor-key-length": ("sensor_keyed", to("key", short)),
    "sensor-key-strided": ("sensor_keyed", to("key", strided)),
    "sensor-out-dtype": ("sensor", out_as(torch.zeros(PIXELS), torch.zeros(PIXELS, dtype=torch.uint8))),
    "sensor-out-length": ("sensor", out_as(torch.zeros(PIXELS, dtype=torch.int16), torch.zeros(PIXELS + 1, dtype=torch.uint8))),
    "sensor-table-and-seed": ("sensor", to("sensor", short, "seed", longer)),
    "sensor-later-host": ("sensor_keyed", on_host("key")),
    "sensor-out-and-host": ("sensor", lambda t: (out_as(torch.zeros(PIXELS), torch.zeros(PIXELS))(t), on_host("sensor")(t))),
    # depth_annotated_images
    "annotated_images-host": ("annotated_images", on_host("depth")),
    "annotated_images-depth": ("annotated_images", to("depth", matrix)),
    "annotated_images-labels": ("annotated_images", to("labels", longer)),
    "annotated_images-geom-scene": ("annotated_images", to("geom", wide)),
    "annotated_images-dest": ("annotated_images", to("dest", wide)),
    "annotated_images-offsets": ("annotated_images", to("offsets", longer)),
    "annotated_images-counts": ("annotated_images", to("counts", strided)),
    "annotated_images-offsets-and-counts": ("annotated_images", to("offsets", short, "counts", short)),
    "annotated_images-row-pair": ("annotated_images", to("row_labels", wide)),
    "annotated_images-gt-rows-narrow": ("annotated_images", to("gt_rows", lambda g: g[:, :9].contiguous())),
    "annotated_images-gt-rows-count": ("annotated_images", to("gt_rows", longer)),
    "annotated_images-scratch-none": ("annotated_images", to("link_scratch", none)),
    "annotated_images-scratch-short": ("annotated_images", to("link_scratch", short)),
    "annotated_images-out": ("annotated_images", lambda t: t.update(out=depth.annotated_image_buffers(5, "cpu")[:3] + (torch.zeros((5, 7)),))),
    "annotated_images-out-rows": ("annotated_images", lambda t: t.update(out=depth.annotated_image_buffers(5, "cpu")[:2]
                                                                          + depth.annotated_image_buffers(6, "cpu")[2:])),
    "annotated_images-gt-rows-and-scratch": ("annotated_images", to("gt_rows", wide, "link_scratch", none)),
    "annotated_images-later-host": ("annotated_images", on_host("gt_rows")),
    # render_depth
    "render-dtype-name": ("render", lambda t: t.update(dtype="float16")),
    "render-host": ("render", on_host("mesh")),
    "render-mesh-dtype": ("render", to("mesh", mesh_with(1, lambda x: x.long()))),
    "render-mesh-short": ("render", to("mesh", mesh_with(0, lambda v: v[:2].contiguous()))),
    "render-tri_off-dtype": ("render_lib", to("library", lib_with_tri_off(lambda o: o.long()))),
    "render-tri_off-length": ("render_lib", to("library", lib_with_tri_off(longer))),
    "render-tri_off-host": ("render_lib", lambda t: setattr(t["library"].tri_off, MARK, True)),
    "render-geom": ("render", to("geom", strided)),
    "render-table-width": ("render", to("render", lambda r: torch.zeros((B, 240), dtype=torch.float64))),
    "render-needs-out": ("render", lambda t: t.pop("pixels")),
    "render-depth-kind": ("render", out_as(torch.zeros(PIXELS), torch.zeros(PIXELS, dtype=torch.uint8))),
    "render-depth-kind-float32": ("render", lambda t: (t.update(dtype="float32"),
                                                       out_as(torch.zeros(PIXELS, dtype=torch.int16), torch.zeros(PIXELS, dtype=torch.uint8))(t))),
    "render-depth-2d": ("render", out_as(torch.zeros((1, PIXELS), dtype=torch.int16), torch.zeros(PIXELS, dtype=torch.uint8))),
    "render-labels": ("render", out_as(torch.zeros(PIXELS, dtype=torch.int16), torch.zeros(PIXELS, dtype=torch.int8))),
    "render-labels-none": ("render", out_as(torch.zeros(PIXELS, dtype=torch.int16), None)),      # not looked for: it falls over None.dtype
    "render-scratch-dtype": ("render", to("zbuf", lambda z: z.int())),
    "render-scratch-short": ("render", to("zbuf", short)),
    "render-mesh-and-geom": ("render", to("mesh", mesh_with(2, wide), "geom", wide)),
    "render-geom-and-labels": ("render", lambda t: (to("geom", wide)(t), out_as(torch.zeros(PIXELS, dtype=torch.int16), torch.zeros(3))(t))),
    "render-later-host": ("render", on_host(("mesh", 1))),
    "render-scratch-and-host": ("render", lambda t: (to("zbuf", short)(t), on_host("render")(t))),
    # pose_scene_build
    "pose_scene-host": ("pose_scene", on_host("kin")),
    "pose_scene-kin-dtype": ("pose_scene", to("kin", wide)),
    "pose_scene-kin-length": ("pose_scene", to("kin", short)),
    "pose_scene-stack-width": ("pose_scene_lib", to("kin_stack", lambda k: k[:, :671].contiguous())),
    "pose_scene-stack-empty": ("pose_scene_lib", to("kin_stack", lambda k: k[:0])),
    "pose_scene-pose-width": ("pose_scene", to("pose", lambda p: p[:, :31].contiguous())),
    "pose_scene-pose-strided": ("pose_scene", to("pose", strided)),
    "pose_scene-out-shape": ("pose_scene", out_as(torch.zeros((B, 240), dtype=torch.float64), torch.zeros((B, 208), dtype=torch.float64))),
    "pose_scene-out-dtype": ("pose_scene", out_as(torch.zeros((B, 208)), torch.zeros((B, 240)))),
    "pose_scene-later-host": ("pose_scene_lib", on_host("pose")),
    "pose_scene-kin-and-host": ("pose_scene", lambda t: (to("kin", short)(t), on_host("kin")(t))),
    # centre_crop_origins
    "centre-host": ("centre", on_host("mesh")),
    "centre-mesh": ("centre", to("mesh", mesh_with(2, wide))),
    "centre-tri_off": ("centre_lib", to("library", lib_with_tri_off(short))),
    "centre-geom-render": ("centre", to("render", wide)),
    "centre-scratch-short": ("centre", to("bounds", short)),
    "centre-scratch-strided": ("centre_lib", to("bounds", strided)),
    "centre-render-and-scratch": ("centre", to("render", longer, "bounds", wide)),
    "centre-later-host": ("centre_lib", on_host("bounds")),
    # reprojection.reproject_scene_build
    "reproject_build-host": ("reproject_build", on_host("record")),
    "reproject_build-render": ("reproject_build", to("render", wide)),
    "reproject_build-scene": ("reproject_build", to("scene", longer)),
    "reproject_build-rig": ("reproject_build", to("rig", lambda r: r[:, :-1].contiguous())),
    "reproject_build-norm_factor": ("reproject_build", to("norm_factor", wide)),
    "reproject_build-geom": ("reproject_build", to("geom", strided)),
    "reproject_build-record-narrow": ("reproject_build", to("record", lambda r: r[:, :, :25].contiguous())),
    "reproject_build-record-2d": ("reproject_build", to("record", lambda r: r[0])),
    "reproject_build-out": ("reproject_build", out_as(torch.zeros((2 * B, 208), dtype=torch.float64), torch.zeros((B, 5), dtype=torch.int32))),
    "reproject_build-scene-and-rig": ("reproject_build", to("scene", wide, "rig", wide)),
    "reproject_build-later-host": ("reproject_build", on_host("rig")),
    # reprojection.reproject_compare
    "reproject_compare-host": ("reproject_compare", on_host("record")),
    "reproject_compare-depth": ("reproject_compare", to("depth", wide)),
    "reproject_compare-labels": ("reproject_compare", to("labels", short)),
    "reproject_compare-labels-none": ("reproject_compare", to("labels", none)),
    "reproject_compare-pred-dtype": ("reproject_compare", to("pred_depth", wide)),
    "reproject_compare-pred-length": ("reproject_compare", to("pred_labels", short)),
    "reproject_compare-scene": ("reproject_compare", to("scene", wide)),
    "reproject_compare-geom": ("reproject_compare", to("geom", wide)),
    "reproject_compare-record": ("reproject_compare", to("record", strided)),
    "reproject_compare-out": ("reproject_compare", lambda t: t.update(out=torch.zeros((B, K, 26), dtype=torch.float64))),
    "reproject_compare-labels-and-pred": ("reproject_compare", to("labels", wide, "pred_depth", short)),
    "reproject_compare-later-host": ("reproject_compare", on_host("depth")),
}

WANT = {
    'unproject-host': (RuntimeError, NO_CPU),
    'unproject-depth-dtype': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'unproject-depth-2d': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'unproject-depth-strided': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'unproject-mask-dtype': (ValueError, 'mask must be a contiguous (31,) uint8 tensor'),
    'unproject-mask-length': (ValueError, 'mask must be a contiguous (31,) uint8 tensor'),
    'unproject-geom-dtype': (ValueError, 'geom must be (B, 5) int32 and cam (B, 7) float32, contiguous'),
    'unproject-geom-width': (ValueError, 'geom must be (B, 5) int32 and cam (B, 7) float32, contiguous'),
    'unproject-cam-frames': (ValueError, 'geom must be (B, 5) int32 and cam (B, 7) float32, contiguous'),
    'unproject-cam-strided': (ValueError, 'geom must be (B, 5) int32 and cam (B, 7) float32, contiguous'),
    'unproject-depth-and-mask': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'unproject-mask-and-cam': (ValueError, 'mask must be a contiguous (31,) uint8 tensor'),
    'unproject-host-and-depth': (RuntimeError, NO_CPU),
    'unproject-mask-host-passes': (None, None),            # depth_unproject checks no tensor's device but its first
    'label_images-host': (RuntimeError, NO_CPU),
    'label_images-depth': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'label_images-mask': (ValueError, 'mask must be a contiguous (31,) uint8 tensor'),
    'label_images-geom': (ValueError, 'geom must be (B, 5) int32, contiguous'),
    'label_images-dest': (ValueError, 'dest must be a contiguous (2,) int32 tensor'),
    'label_images-offsets': (ValueError, 'offsets must be a contiguous (3,) int32 tensor'),
    'label_images-dest-and-offsets': (ValueError, 'dest must be a contiguous (2,) int32 tensor'),
    'label_images-labels-2d': (ValueError, 'labels must be (capacity,) int32 and values (capacity, 7) float32, contiguous'),
    'label_images-values-width': (ValueError, 'labels must be (capacity,) int32 and values (capacity, 7) float32, contiguous'),
    'label_images-values-rows': (ValueError, 'labels must be (capacity,) int32 and values (capacity, 7) float32, contiguous'),
    'label_images-scratch-none': (ValueError, 'scratch must be the (>= 128,) int32 tensor depth_unproject() was given'),
    'label_images-scratch-short': (ValueError, 'scratch must be the (>= 128,) int32 tensor depth_unproject() was given'),
    'label_images-scratch-dtype': (ValueError, 'scratch must be the (>= 128,) int32 tensor depth_unproject() was given'),
    'label_images-out-dtype': (ValueError, 'out must be contiguous (img_labels (n,) int32, img_values (n, 7) float32)'),
    'label_images-out-rows': (ValueError, 'out must be contiguous (img_labels (n,) int32, img_values (n, 7) float32)'),
    'label_images-values-and-scratch': (ValueError, 'labels must be (capacity,) int32 and values (capacity, 7) float32, contiguous'),
    'label_images-later-host': (RuntimeError, NO_CPU),
    'label_images-mask-host': (RuntimeError, NO_CPU),
    'label_images-scratch-and-host': (ValueError, 'scratch must be the (>= 128,) int32 tensor depth_unproject() was given'),
    'annotate-host': (RuntimeError, NO_CPU),
    'annotate-depth': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'annotate-labels-none': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'annotate-labels-dtype': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'annotate-geom': (ValueError, 'geom must be (B, 5) int32 and scene (B, 240) float64, contiguous'),
    'annotate-scene-dtype': (ValueError, 'geom must be (B, 5) int32 and scene (B, 240) float64, contiguous'),
    'annotate-scene-width': (ValueError, 'geom must be (B, 5) int32 and scene (B, 240) float64, contiguous'),
    'annotate-rows': (ValueError, 'rows must be a contiguous (capacity, 7) float32 tensor'),
    'annotate-link_counts': (ValueError, 'link_counts must be a contiguous (B, 16) int32 tensor'),
    'annotate-scratch-short': (ValueError, 'scratch must be a contiguous int32 tensor of >= 2048 elements'),
    'annotate-scratch-dtype': (ValueError, 'scratch must be a contiguous int32 tensor of >= 2048 elements'),
    'annotate-labels-and-scene': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'annotate-later-host': (RuntimeError, CPU_TENSOR),
    'annotate-scratch-and-host': (ValueError, 'scratch must be a contiguous int32 tensor of >= 2048 elements'),
    'sensor-host': (RuntimeError, NO_CPU),
    'sensor-depth': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'sensor-labels': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'sensor-geom-scene': (ValueError, 'geom must be (B, 5) int32 and scene (B, 240) float64, contiguous'),
    'sensor-table-dtype': (ValueError, "sensor must be a contiguous (16,) float64 tensor (depth.pack_sensor's table)"),
    'sensor-table-length': (ValueError, "sensor must be a contiguous (16,) float64 tensor (depth.pack_sensor's table)"),
    'sensor-seed-length': (ValueError, 'seed_or_key must be the device seed (1,) int64 or the key block (4,) int32'),
    'sensor-seed-dtype': (ValueError, 'seed_or_key must be the device seed (1,) int64 or the key block (4,) int32'),
    'sensor-key-length': (ValueError, 'seed_or_key must be the device seed (1,) int64 or the key block (4,) int32'),
    'sensor-key-strided': (ValueError, 'seed_or_key must be the device seed (1,) int64 or the key block (4,) int32'),
    'sensor-out-dtype': (ValueError, "out must be contiguous (depth (31,) of the input's dtype, labels (31,) uint8)"),
    'sensor-out-length': (ValueError, "out must be contiguous (depth (31,) of the input's dtype, labels (31,) uint8)"),
    'sensor-table-and-seed': (ValueError, "sensor must be a contiguous (16,) float64 tensor (depth.pack_sensor's table)"),
    'sensor-later-host': (RuntimeError, CPU_TENSOR),
    'sensor-out-and-host': (ValueError, "out must be contiguous (depth (31,) of the input's dtype, labels (31,) uint8)"),
    'annotated_images-host': (RuntimeError, NO_CPU),
    'annotated_images-depth': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'annotated_images-labels': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'annotated_images-geom-scene': (ValueError, 'geom must be (B, 5) int32 and scene (B, 240) float64, contiguous'),
    'annotated_images-dest': (ValueError, 'dest must be a contiguous (2,) int32 tensor'),
    'annotated_images-offsets': (ValueError, 'offsets must be a contiguous (3,) int32 tensor'),
    'annotated_images-counts': (ValueError, 'counts must be a contiguous (2,) int32 tensor'),
    'annotated_images-offsets-and-counts': (ValueError, 'offsets must be a contiguous (3,) int32 tensor'),
    'annotated_images-row-pair': (ValueError, 'row_labels must be (capacity,) int32 and row_values (capacity, 7) float32, contiguous'),
    'annotated_images-gt-rows-narrow': (ValueError, "gt_rows must be a contiguous (33, >= 10) float32 tensor (dataset.point_gt_build's rows)"),
    'annotated_images-gt-rows-count': (ValueError, "gt_rows must be a contiguous (33, >= 10) float32 tensor (dataset.point_gt_build's rows)"),
    'annotated_images-scratch-none': (ValueError, 'scratch must be the (>= 2048,) int32 tensor depth_annotate() was given'),
    'annotated_images-scratch-short': (ValueError, 'scratch must be the (>= 2048,) int32 tensor depth_annotate() was given'),
    'annotated_images-out': (ValueError, 'out must be contiguous (img_labels (n,) int32, img_values (n, 7) float32, img_gt_labels (n,) int32, img_gt_values (n, 6) float32)'),
    'annotated_images-out-rows': (ValueError, 'out must be contiguous (img_labels (n,) int32, img_values (n, 7) float32, img_gt_labels (n,) int32, img_gt_values (n, 6) float32)'),
    'annotated_images-gt-rows-and-scratch': (ValueError, "gt_rows must be a contiguous (33, >= 10) float32 tensor (dataset.point_gt_build's rows)"),
    'annotated_images-later-host': (RuntimeError, CPU_TENSOR),
    'render-dtype-name': (ValueError, "depth_dtype must be 'uint16' or 'float32', got 'float16'"),
    'render-host': (RuntimeError, NO_CPU),
    'render-mesh-dtype': (ValueError, "mesh must be depth.mesh_to_device's (verts float32, tris int32, tri_link int32, V, T), contiguous"),
    'render-mesh-short': (ValueError, "mesh must be depth.mesh_to_device's (verts float32, tris int32, tri_link int32, V, T), contiguous"),
    'render-tri_off-dtype': (ValueError, "a mesh library's tri_off must be depth.mesh_to_device's (ninst + 1,) int32 device tensor"),
    'render-tri_off-length': (ValueError, "a mesh library's tri_off must be depth.mesh_to_device's (ninst + 1,) int32 device tensor"),
    'render-tri_off-host': (ValueError, "a mesh library's tri_off must be depth.mesh_to_device's (ninst + 1,) int32 device tensor"),
    'render-geom': (ValueError, 'geom must be (B, 5) int32 and render (B, 208) float64, contiguous'),
    'render-table-width': (ValueError, 'geom must be (B, 5) int32 and render (B, 208) float64, contiguous'),
    'render-needs-out': (ValueError, 'render_depth needs out=(depth, labels) or pixel_capacity'),
    'render-depth-kind': (ValueError, 'depth must be a contiguous 1-d uint16 tensor'),
    'render-depth-kind-float32': (ValueError, 'depth must be a contiguous 1-d float32 tensor'),
    'render-depth-2d': (ValueError, 'depth must be a contiguous 1-d uint16 tensor'),
    'render-labels': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'render-labels-none': (AttributeError, "'NoneType' object has no attribute 'dtype'"),
    'render-scratch-dtype': (ValueError, 'scratch must be a contiguous int64 tensor of >= 31 elements'),
    'render-scratch-short': (ValueError, 'scratch must be a contiguous int64 tensor of >= 31 elements'),
    'render-mesh-and-geom': (ValueError, "mesh must be depth.mesh_to_device's (verts float32, tris int32, tri_link int32, V, T), contiguous"),
    'render-geom-and-labels': (ValueError, 'geom must be (B, 5) int32 and render (B, 208) float64, contiguous'),
    'render-later-host': (RuntimeError, CPU_TENSOR),
    'render-scratch-and-host': (ValueError, 'scratch must be a contiguous int64 tensor of >= 31 elements'),
    'pose_scene-host': (RuntimeError, NO_CPU),
    'pose_scene-kin-dtype': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-kin-length': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-stack-width': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-stack-empty': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-pose-width': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-pose-strided': (ValueError, 'kin must be (672,) float64 -- a library: (ninst, 672) -- and pose (B, 32) float64, contiguous'),
    'pose_scene-out-shape': (ValueError, 'out must be (render (B, 208), scene (B, 240)) float64, contiguous'),
    'pose_scene-out-dtype': (ValueError, 'out must be (render (B, 208), scene (B, 240)) float64, contiguous'),
    'pose_scene-later-host': (RuntimeError, CPU_TENSOR),
    'pose_scene-kin-and-host': (RuntimeError, NO_CPU),
    'centre-host': (RuntimeError, NO_CPU),
    'centre-mesh': (ValueError, "mesh must be depth.mesh_to_device's (verts float32, tris int32, tri_link int32, V, T), contiguous"),
    'centre-tri_off': (ValueError, "a mesh library's tri_off must be depth.mesh_to_device's (ninst + 1,) int32 device tensor"),
    'centre-geom-render': (ValueError, 'geom must be (B, 5) int32 and render (B, 208) float64, contiguous'),
    'centre-scratch-short': (ValueError, 'scratch must be a contiguous int32 tensor of >= 8 elements'),
    'centre-scratch-strided': (ValueError, 'scratch must be a contiguous int32 tensor of >= 8 elements'),
    'centre-render-and-scratch': (ValueError, 'geom must be (B, 5) int32 and render (B, 208) float64, contiguous'),
    'centre-later-host': (RuntimeError, CPU_TENSOR),
    'reproject_build-host': (RuntimeError, NO_CPU),
    'reproject_build-render': (ValueError, 'render must be a contiguous (2, 208) float64 tensor'),
    'reproject_build-scene': (ValueError, 'scene must be a contiguous (2, 240) float64 tensor'),
    'reproject_build-rig': (ValueError, 'rig must be a contiguous (2, 88) float64 tensor'),
    'reproject_build-norm_factor': (ValueError, 'norm_factor must be a contiguous (2,) float32 tensor'),
    'reproject_build-geom': (ValueError, 'geom must be a contiguous (2, 5) int32 tensor'),
    'reproject_build-record-narrow': (ValueError, 'record must be a contiguous (2, 2, >= 26) float64 tensor'),
    'reproject_build-record-2d': (ValueError, 'a rig holds 1..8 parts, got K=0'),
    'reproject_build-out': (ValueError, 'out must be contiguous (render (4, 208) float64, geom (4, 5) int32)'),
    'reproject_build-scene-and-rig': (ValueError, 'scene must be a contiguous (2, 240) float64 tensor'),
    'reproject_build-later-host': (RuntimeError, CPU_TENSOR),
    'reproject_compare-host': (RuntimeError, NO_CPU),
    'reproject_compare-depth': (ValueError, 'depth must be a contiguous 1-d uint16 or float32 tensor'),
    'reproject_compare-labels': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'reproject_compare-labels-none': (AttributeError, "'NoneType' object has no attribute 'dtype'"),
    'reproject_compare-pred-dtype': (ValueError, 'the predicted pair must be contiguous (depth (62,) of the observed dtype, labels (62,) uint8)'),
    'reproject_compare-pred-length': (ValueError, 'the predicted pair must be contiguous (depth (62,) of the observed dtype, labels (62,) uint8)'),
    'reproject_compare-scene': (ValueError, 'scene must be a contiguous (2, 240) float64 tensor'),
    'reproject_compare-geom': (ValueError, 'geom must be a contiguous (2, 5) int32 tensor'),
    'reproject_compare-record': (ValueError, 'record must be a contiguous (2, 2, >= 26) float64 tensor'),
    'reproject_compare-out': (ValueError, 'out must be a contiguous (2, 2, 41) float64 tensor'),
    'reproject_compare-labels-and-pred': (ValueError, 'labels must be a contiguous (31,) uint8 tensor'),
    'reproject_compare-later-host': (RuntimeError, CPU_TENSOR),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_argument(calls, case):
    wrapper, mutate = BAD[case]
    fn, names, kw = WRAPPERS[wrapper]
    t = inputs()
    t.update(dtype="uint16", pixels=PIXELS)
    mutate(t)
    kwargs = {k: t[n] for k, n in kw.items() if n in t}
    if "out" in t:
        kwargs["out"] = t["out"]
    exc, message = WANT[case]
    if exc is None:                    # nothing is refused: the call goes through
        fn(*(t[n] for n in names), **kwargs)
        assert len(calls) == 1
        return
    with pytest.raises(exc) as raised:
        fn(*(t[n] for n in names), **kwargs)
    assert type(raised.value) is exc and str(raised.value) == message
    assert calls == []


def test_every_wrapper_is_covered():
    assert {w for w, _ in BAD.values()} == set(WRAPPERS)
    assert set(WANT) == set(BAD)
