"""CPU tests of the depth front end's label / NOCS images (no GPU): the symbol and its binding, ancsh_depth_label_images' argument checks
before any launch, the constructor / retire rules of AncshPipeline(label_images=True), and the numpy frame-cutting helper."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

P16 = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails its checks first
NAME = "ancsh_depth_label_images"


def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_14():
    from articulated_pose_amd import _lib
    from articulated_pose_amd.depth import LABEL_NAN_BITS
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in declared_symbols() and NAME in exported and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME]) == 16
    assert _L().ancsh_abi_version() == 14
    # the header fixes the NaN of a pixel without a row: numpy's quiet NaN, which is what raw_point_labels_kernel's NAN is
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "ancsh_hip.h")).read()
    assert "#define ANCSH_LABEL_NAN_BITS 0x7fc00000u" in header and LABEL_NAN_BITS == 0x7fc00000
    assert np.array([np.nan], np.float32).view(np.uint32)[0] == LABEL_NAN_BITS


def test_entry_rejects_bad_arguments_before_launch():
    L = _L()

    def call(nclouds=2, kind=0, depth=P16, mask=P16, px=100, geom=P16, off=P16, scratch=P16, labels=P16, values=P16, cap=100, dest=P16,
             img_labels=P16, img_values=P16, icap=100):
        return L.ancsh_depth_label_images(nclouds, kind, depth, mask, px, geom, off, scratch, labels, values, cap, dest, img_labels,
                                          img_values, icap, None)
    for kw, msg in ((dict(nclouds=-1), b"bad shape"), (dict(nclouds=65536), b"65535"), (dict(kind=2), b"depth_type=2"),
                    (dict(kind=-1), b"depth_type=-1"), (dict(px=-1), b"pixel_capacity=-1"), (dict(px=1 << 30), b"pixel_capacity"),
                    (dict(cap=-1), b"capacity=-1 rows"), (dict(cap=1 << 30), b"rows out of range"),
                    (dict(icap=-1), b"image_capacity=-1"), (dict(icap=1 << 30), b"image_capacity"),
                    (dict(depth=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(mask=ctypes.c_void_p(4)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        err = L.ancsh_last_error()
        assert msg in err and err.startswith(b"depth_label_images:"), (kw, err)
    for k in ("depth", "geom", "off", "scratch", "labels", "values", "dest", "img_labels", "img_values"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
        assert call(nclouds=0, **{k: None}) == -1             # nulls are refused even for an empty batch
    assert call(nclouds=0, mask=None) == 0                    # no mask, no cloud: nothing launched, no device touched
    assert call(nclouds=0, cap=0, icap=0, px=0) == 0


def test_constructor_and_retire_rules_before_gpu_work():
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    base = dict(joint_source="predicted")
    with pytest.raises(ValueError, match="label_images=True .* depth_capacity"):
        AncshPipeline(3, None, None, 2, 512, "cpu", label_images=True, **base)
    with pytest.raises(ValueError, match="label_images=True .* depth_capacity"):
        AncshPipeline(3, None, None, 2, 512, "cpu", raw_capacity=4096, label_images=True, **base)
    # dense with the depth front end still raises, and now names the option that serves depth frames
    for extra in (dict(), dict(label_images=True)):
        with pytest.raises(ValueError, match="dense.*label_images=True"):
            AncshPipeline(3, None, None, 2, 512, "cpu", depth_capacity=4096, dense=True, **dict(base, **extra))
    # a pipeline built without the option refuses to return images, before it looks at its (empty) in-flight window
    pipe = AncshPipeline.__new__(AncshPipeline)
    pipe.opts = check_options(raw_capacity=4096)
    pipe._inflight = []
    with pytest.raises(RuntimeError, match="label_images=True"):
        pipe.retire(label_images=True)
    with pytest.raises(RuntimeError, match="label_images=True"):
        next(pipe.stream_depth_batches([], None, label_images=True))
    with pytest.raises(RuntimeError, match="no batch in flight"):
        pipe.retire()


def test_cut_label_images_on_ragged_shapes():
    from articulated_pose_amd.depth import LABEL_VALUES, cut_label_images
    assert LABEL_VALUES == 7
    shapes = [(3, 4), (1, 1), (2, 5), (7, 1), (1, 6)]
    n = sum(h * w for h, w in shapes)
    first = 5
    labels = np.arange(first + n + 3, dtype=np.int32) * 3 - 7
    values = np.arange((first + n + 3) * 7, dtype=np.float32).reshape(-1, 7)
    values[first + 12] = np.nan                                    # the 1 x 1 frame
    got = cut_label_images(labels, values, shapes, first=first)
    assert len(got) == len(shapes)
    a = first
    for (h, w), (lab, val) in zip(shapes, got):
        assert lab.shape == (h, w) and lab.dtype == np.int32 and val.shape == (h, w, 7) and val.dtype == np.float32
        assert lab.flags.c_contiguous and val.flags.c_contiguous
        for i in range(h):
            for j in range(w):
                q = a + i * w + j
                assert lab[i, j] == labels[q] and np.array_equal(val[i, j].view(np.int32), values[q].view(np.int32))
        a += h * w
    assert got[1][0].shape == (1, 1) and np.isnan(got[1][1]).all()
    # fresh arrays: the staging may be rewritten afterwards
    before = got[0][0].copy()
    labels[:] = 0
    values[:] = 0
    assert np.array_equal(got[0][0], before) and got[2][1][0, 0, 0] != 0
    assert cut_label_images(labels[:0], values[:0], []) == []
    with pytest.raises(ValueError):
        cut_label_images(labels[:n - 1], values[:n - 1], shapes)          # the buffers end inside the last frame
    with pytest.raises(ValueError):
        cut_label_images(labels, values, [(0, 3)])
    with pytest.raises(ValueError):
        cut_label_images(labels.astype(np.int64), values, shapes)
    with pytest.raises(ValueError):
        cut_label_images(labels, values[:, :6], shapes)
