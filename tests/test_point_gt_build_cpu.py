"""CPU (no GPU): the per-point ground-truth builder's host side.  dataset.pack_joint_rig against the reference's own joint_params_gt, the
float64 mirror of ancsh_point_gt_build (tests/point_gt_build_mirror.py) on the packed rig against every column the reference's
create_data_shape2motion / create_data_mobility / create_unit_data_from_hdf5 produced (tests/golden/point_gt_build.npz), the entry's
declaration, export, binding and argument checks, and the ValueErrors of the host functions and of both pipelines, raised before a device
is touched."""
import ctypes
import functools
import os

import numpy as np
import pytest

from point_gt_build_mirror import build_rows, frame_of, load_case, rig_width

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_gt_build.npz")
CASES = ("a", "b", "c", "d", "e")
P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """-> (case dict, src (n, 7) float32, rig, joint_params, K) of a golden case, packed by the product's host functions."""
    from articulated_pose_amd.dataset import pack_annotated_cloud, pack_joint_rig
    with np.load(GOLDEN) as z:
        c = load_case(z, name)
    f, joints = frame_of(c)
    src = pack_annotated_cloud(f["gt_points"], f["gt_coords"], c["parts_map"])
    rig, jp = pack_joint_rig(c["corners"], c["factors"], joints, c["parts_map"], c["dataset"], c["target_order"], 0.2)
    return c, src, rig, jp, len(c["parts_map"])


def within_one_ulp(got, want):
    """Every element of got within one float32 ulp of the reference's float32 value (np.spacing); -> the worst distance in ulps."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return float(d.max()) if d.size else 0.0


def check_rows(got, want, what):
    """The bars of the issue: x y z, cls and joint_cls bit-exact, every other column within one float32 ulp of the reference's value."""
    exact = [0, 1, 2, 3, 17]
    assert np.array_equal(got[:, exact].view(np.uint32), want[:, exact].view(np.uint32)), what
    worst = within_one_ulp(got[:, 4:17], want[:, 4:17])
    print("%s: worst column difference %.3g ulp" % (what, worst))
    assert worst <= 1.0, (what, worst)


def test_fixture_covers_the_cases_and_sizes():
    sizes = set()
    for name in CASES:
        c, src, rig, jp, K = golden_case(name)
        assert src.shape == (sum(c["link_sizes"]), 7) and src.dtype == np.float32 and rig.shape == (rig_width(K),) and jp.shape == (K, 7)
        sizes.update(np.bincount(src[:, 6].astype(int), minlength=K).tolist())
    assert {1, 67, 300} <= sizes
    assert os.path.getsize(GOLDEN) < (1 << 20)
    c = golden_case("c")[0]
    assert c["parts_map"] == [[0, 3, 4], [1, 2]] and golden_case("d")[0]["target_order"] == [3, 0, 1, 2]


@pytest.mark.parametrize("name", CASES)
def test_joint_params_equal_the_reference(name):
    c, _, _, jp, K = golden_case(name)
    want = c["joint_params"]
    assert jp.dtype == np.float64 and want.shape == (K, 7)
    np.testing.assert_allclose(jp, want, rtol=1e-12, atol=0)
    assert np.abs(want[1:]).max() > 0


@pytest.mark.parametrize("name", CASES)
def test_mirror_on_the_packed_rig_reproduces_every_golden_column(name):
    c, src, rig, _, K = golden_case(name)
    check_rows(build_rows(src, rig, K), c["rows"], "mirror, case " + name)
    if name == "b":            # the overwrite order: points inside both tubes carry the LATER joint's label
        got, hs = build_rows(src, rig, K, return_h=True)
        h0, h1 = [h for idx, k, kind, h in hs if idx[0] == 0]
        both = (h0 < 0.2) & (h1 < 0.2)
        assert both.sum() >= 5 and (c["rows"][:300][both, 17] == 2).all() and (c["rows"][:300][(h0 < 0.2) & ~both, 17] == 1).any()
    if name == "d":            # relabelled by target_order, every point selected by a constant entry, rotated
        assert (c["rows"][:130, 3] == 1).all() and (c["rows"][-300:, 3] == 0).all() and (c["rows"][:, 17] == c["rows"][:, 3]).all()
        assert (c["rows"][:, 10] > 0).all()


def test_rig_layout_and_width():
    from articulated_pose_amd import dataset as D
    assert [D.RIG_WIDTH(K) for K in range(1, 9)] == [rig_width(K) for K in range(1, 9)] and D.RIG_WIDTH(8) == 718
    for K in (0, 9):
        with pytest.raises(ValueError, match="1..8 parts"):
            D.RIG_WIDTH(K)
    rig = D.identity_rig(3)
    src = np.random.RandomState(0).uniform(-1, 1, (50, 7)).astype(np.float32)
    src[:, 6] = np.arange(50) % 3
    rows = build_rows(src, rig, 3)
    assert np.array_equal(rows[:, 3], src[:, 6]) and (rows[:, 10:] == 0).all() and np.abs(rows[:, 4:7] - src[:, 3:6]).max() < 1e-6
    # the header's macros say the same
    txt = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "ancsh_hip.h")).read()
    for line in ("#define ANCSH_RIG_ROT 4", "#define ANCSH_RIG_GMAP 13", "#define ANCSH_RIG_HEAD 22", "#define ANCSH_RIG_ENTRY 9",
                 "#define ANCSH_RIG_PART(K) (15 + ANCSH_RIG_ENTRY * (K))"):
        assert line in txt, line


def test_entry_is_declared_exported_and_bound_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    L = _lib.lib()
    assert "ancsh_point_gt_build" in declared_symbols() and hasattr(L, "ancsh_point_gt_build")
    assert len(_lib.SIGNATURES["ancsh_point_gt_build"]) == 9
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()

    def call(nclouds=1, K=3, src=P8, cap=100, off=P8, rig=P8, rig_ld=None, rows=P8):
        return L.ancsh_point_gt_build(nclouds, K, src, cap, off, rig, rig_width(K) if rig_ld is None and 1 <= K <= 8 else (rig_ld or 0), rows, None)
    for kw, word in ((dict(nclouds=-1), b"nclouds=-1"), (dict(nclouds=65536), b"nclouds=65536"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"),
                     (dict(rig_ld=147), b"rig_ld=147"), (dict(K=2, rig_ld=rig_width(3)), b"rig_ld=148"), (dict(cap=-1), b"capacity=-1"),
                     (dict(cap=1 << 30), b"capacity="), (dict(src=None), b"null pointer"), (dict(off=None), b"null pointer"),
                     (dict(rig=None), b"null pointer"), (dict(rows=None), b"null pointer")):
        assert call(**kw) == -1 and word in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for K in range(1, 9):                                              # nothing to do: nothing enqueued, whatever the pointers
        assert L.ancsh_point_gt_build(0, K, None, 0, None, None, rig_width(K), None, None) == 0


def test_pack_functions_refuse_bad_input():
    from articulated_pose_amd import dataset as D
    c, src, rig, _, K = golden_case("d")
    f, joints = frame_of(c)
    with pytest.raises(ValueError, match="target_order"):
        D.pack_joint_rig(c["corners"], c["factors"], joints, c["parts_map"], "sapien")
    with pytest.raises(ValueError, match="dataset must be"):
        D.pack_joint_rig(c["corners"], c["factors"], joints, c["parts_map"], "BMVC15")
    with pytest.raises(ValueError, match="1..8 parts"):
        D.pack_joint_rig(c["corners"], c["factors"], joints, [], "shape2motion")
    with pytest.raises(ValueError, match="1..8 parts"):
        D.pack_joint_rig(c["corners"], c["factors"], joints, [[j] for j in range(9)], "shape2motion")
    with pytest.raises(ValueError, match="need 5 entries"):
        D.pack_joint_rig(c["corners"][:4], c["factors"], joints, c["parts_map"], "sapien", c["target_order"])
    ragged = [c["corners"][0], c["corners"][1][:1]] + list(c["corners"][2:])
    with pytest.raises(ValueError, match=r"norm_corners\[1\]"):
        D.pack_joint_rig(ragged, c["factors"], joints, c["parts_map"], "sapien", c["target_order"])
    with pytest.raises(ValueError, match=r"norm_factors\[2\]"):
        D.pack_joint_rig(c["corners"], [1.0, 1.0, [1.0, 2.0], 1.0, 1.0], joints, c["parts_map"], "sapien", c["target_order"])
    with pytest.raises(ValueError, match="must name parts in"):
        D.pack_joint_rig(c["corners"], c["factors"], joints, c["parts_map"], "sapien", [4, 0, 1, 2])
    # a part measured against more joints than the rig holds: K = 1, the parent joint (link 1 leads the group) and a child
    one = {"link": {"xyz": [[0, 0, 0]] * 3}, "joint": {"axis": [[0, 0, 1.0]] * 3, "parent": [-1, 2, 2]}}
    with pytest.raises(ValueError, match="measured against 3 joints"):
        D.pack_joint_rig(c["corners"][:2], c["factors"][:2], one, [[1, 2]], "shape2motion")
    # the groups are concatenated in parts_map order, dicts keyed like the .h5 groups or plain sequences
    a = golden_case("c")[0]
    f, _ = frame_of(a)
    rows = D.pack_annotated_cloud(f["gt_points"], [f["gt_coords"][str(i)] for i in range(5)], a["parts_map"])
    order = np.concatenate([np.arange(*np.cumsum([0] + a["link_sizes"])[[i, i + 1]]) for i in (0, 3, 4, 1, 2)])
    assert np.array_equal(rows[:, :3], a["points"][order]) and np.array_equal(rows[:, 3:6], a["coords"][order])
    assert np.array_equal(rows[:, 6], np.repeat([0.0, 1.0], [67, 67]).astype(np.float32))
    with pytest.raises(ValueError, match="points but"):
        D.pack_annotated_cloud(f["gt_points"], dict(f["gt_coords"], **{"0": f["gt_coords"]["0"][:-1]}), a["parts_map"])
    # the eager wrapper's and the stream's cloud check
    for bad, word in ((src[:, :6], r"\(n_raw, 7\)"), (np.where(np.arange(7) == 6, 0.5, src), "integers in"),
                      (np.where(np.arange(7) == 6, float(K), src), "integers in"), (np.where(np.arange(7) == 6, np.nan, src), "integers in"),
                      (src[:0], r"\(n_raw, 7\)")):
        with pytest.raises(ValueError, match=word):
            D.check_annotated_clouds([bad], [1.0], K, 4)
    with pytest.raises(ValueError, match=r"rig must be \(1, %d\)" % rig_width(K)):
        D.check_rigs(np.zeros((1, rig_width(K) + 1)), 1, K)
    with pytest.raises(ValueError, match=r"rig must be \(2, "):
        D.check_rigs(rig[None], 2, K)
    with pytest.raises(RuntimeError, match="MI355X only"):
        D.build_point_gt_rows([src], [rig], "cpu")


def test_pipelines_refuse_before_a_device_is_touched():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.stream import check_options
    # the constructors check before they build a network or touch a device ("cpu" never reaches a kernel)
    with pytest.raises(ValueError, match="build_point_gt=True .* needs point_ground_truth=True"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, articulation=True, build_point_gt=True)
    with pytest.raises(ValueError, match="build_point_gt=True .* needs point_ground_truth=True"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1000, articulation=True, build_point_gt=True)
    _, src, rig, _, K = golden_case("b")
    pipe = AncshPipeline.__new__(AncshPipeline)
    built = dict(raw_capacity=1000, articulation=True, point_ground_truth=True)
    pipe.opts, pipe.B, pipe.K = check_options(build_point_gt=True, **built), 2, K
    with pytest.raises(ValueError, match="rig=.* needs one dataset.pack_joint_rig table per cloud"):
        pipe.submit([src], [1.0])
    with pytest.raises(ValueError, match=r"\(n_raw, 7\).*x y z \| cx cy cz \| part.*\(5, 18\)"):
        pipe.submit([np.zeros((5, 18), np.float32)], [1.0], rig=rig[None])
    with pytest.raises(ValueError, match=r"rig must be \(1, %d\)" % rig_width(K)):
        pipe.submit([src], [1.0], rig=np.stack([rig, rig]))
    with pytest.raises(ValueError, match="integers in"):
        pipe.submit([np.where(np.arange(7) == 6, 0.5, src).astype(np.float32)], [1.0], rig=rig[None])
    # a pipeline built without the option refuses rig=
    pipe.opts = check_options(**built)
    with pytest.raises(ValueError, match="rig needs AncshPipeline"):
        pipe.submit([np.zeros((5, 18), np.float32)], [1.0], rig=rig[None])
    sp = ShardedPipeline.__new__(ShardedPipeline)
    sp.raw_capacity, sp.opts = 1000, check_options(**built)
    with pytest.raises(ValueError, match="rig needs ShardedPipeline"):
        sp.submit([np.zeros((5, 18), np.float32)], [1.0], rig=rig[None])
    sp.opts = check_options(build_point_gt=True, **built)
    with pytest.raises(ValueError, match="needs one dataset.pack_joint_rig table per cloud"):
        sp.submit([src], [1.0])
