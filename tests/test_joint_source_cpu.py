"""CPU tests of the predicted joint association (no GPU): the ABI 13 entries (ancsh_pose_joint_direction_pred,
ancsh_pose_poison_records_pred, ancsh_input_sample_stream_xyz / _xyz_keyed) are declared, exported and bound and refuse bad arguments
before any launch; check_raw_clouds' xyz rule; the pipelines and the solver refuse a bad or missing joint association before any GPU
work; pose_multi_process.py --joint_source parses."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_sharded_stream_cpu import CAP, _FakeStreamPipeline

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first
NEW = ("ancsh_pose_joint_direction_pred", "ancsh_pose_poison_records_pred", "ancsh_input_sample_stream_xyz",
       "ancsh_input_sample_stream_xyz_keyed")


def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def test_new_entries_are_declared_exported_and_bound():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name in NEW:
        assert name in declared_symbols() and name in exported and name in _lib.SIGNATURES, name
    assert _L().ancsh_abi_version() >= 13


def _direction(L, b=2, n=512, K=3, jc=3, null=None):
    p = dict(axis=P8, index=P8, out=P8)
    if null:
        p[null] = None
    return L.ancsh_pose_joint_direction_pred(b, n, K, jc, p["axis"], p["index"], p["out"], None)


def test_direction_entry_rejects_bad_arguments_before_launch():
    L = _L()
    for kw, msg in ((dict(K=1), b"K >= 2"), (dict(K=0), b"bad shape"), (dict(b=-1), b"bad shape"), (dict(n=0), b"bad shape"),
                    (dict(n=8193), b"8192"), (dict(jc=0), b"joint_channels"), (dict(jc=65), b"joint_channels"),
                    (dict(K=17), b"bad shape")):
        assert _direction(L, **kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for name in ("axis", "index", "out"):
        assert _direction(L, null=name) == -1 and b"null pointer" in L.ancsh_last_error(), name
    assert _direction(L, b=0, null="out") == -1                      # nulls are refused even for an empty batch


def _poison(L, b=2, n=512, K=3, jc=3, null=None):
    p = dict(P=P8, nocs=P8, W=P8, axis=P8, index=P8, record=P8)
    if null:
        p[null] = None
    return L.ancsh_pose_poison_records_pred(b, n, K, p["P"], p["nocs"], p["W"], p["axis"], jc, p["index"], p["record"], None)


def test_poison_entry_rejects_bad_arguments_before_launch():
    L = _L()
    for kw, msg in ((dict(jc=0), b"joint_channels"), (dict(jc=-3), b"joint_channels"), (dict(K=0), b"bad shape"),
                    (dict(n=0), b"bad shape"), (dict(b=-1), b"bad shape")):
        assert _poison(L, **kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for name in ("P", "nocs", "W", "index", "record"):
        assert _poison(L, null=name) == -1 and b"null pointer" in L.ancsh_last_error(), name


@pytest.mark.parametrize("keyed", [False, True])
def test_xyz_sampler_entries_reject_bad_arguments_before_launch(keyed):
    L = _L()
    fn = L.ancsh_input_sample_stream_xyz_keyed if keyed else L.ancsh_input_sample_stream_xyz

    def call(nclouds=2, nchan=3, cap=100, seed=P8, rows=P8, off=P8, nf=P8, P=P8):
        return fn(nclouds, 16, nchan, rows, cap, off, nf, seed, P, None, None)
    for nchan in (2, 0, -1):
        assert call(nchan=nchan) == -1 and b"nchan=%d" % nchan in L.ancsh_last_error()
    assert call(seed=None) == -1 and (b"null key" if keyed else b"null seed") in L.ancsh_last_error()
    assert call(nclouds=65536) == -1 and b"65535" in L.ancsh_last_error()
    assert call(cap=-1) == -1 and b"capacity" in L.ancsh_last_error()
    for k in ("rows", "off", "nf", "P"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.ancsh_last_error(), k
    # the 4-column entries keep refusing 3-column rows and a joint-class column below 3
    old = L.ancsh_input_sample_stream_keyed if keyed else L.ancsh_input_sample_stream
    assert old(2, 16, 3, P8, 100, P8, P8, 3, P8, P8, P8, None, None) == -1
    assert old(2, 16, 4, P8, 100, P8, P8, 2, P8, P8, P8, None, None) == -1


def test_check_raw_clouds_xyz_rule():
    from articulated_pose_amd.dataset import check_raw_clouds
    rs = np.random.RandomState(0)
    c3, c4 = rs.uniform(-1, 1, (10, 3)), rs.uniform(-1, 1, (7, 4)).astype(np.float32)
    clouds, nf = check_raw_clouds([c3, c4], [1.0, 2.0], xyz_only=True)
    assert [c.shape for c in clouds] == [(10, 3), (7, 3)] and all(c.dtype == np.float32 and c.flags.c_contiguous for c in clouds)
    assert np.array_equal(clouds[0], c3.astype(np.float32)) and np.array_equal(clouds[1], c4[:, :3])
    for bad in (np.zeros((0, 3), np.float32), np.zeros((5, 2), np.float32), np.zeros((5, 5), np.float32), np.zeros(5, np.float32)):
        with pytest.raises(ValueError):
            check_raw_clouds([bad], [1.0], xyz_only=True)
    with pytest.raises(ValueError):
        check_raw_clouds([c3], [float("nan")], xyz_only=True)
    with pytest.raises(ValueError):
        check_raw_clouds([c3], [1.0])                               # the default still refuses 3-column clouds
    assert check_raw_clouds([c4], [1.0])[0][0].shape == (7, 4)


def test_pipelines_refuse_a_bad_joint_source_before_gpu_work():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    for bad in ("GT", "pred", None, 1):
        with pytest.raises(ValueError, match="joint_source"):
            AncshPipeline(3, None, None, 2, 512, "cpu", joint_source=bad)
        with pytest.raises(ValueError, match="joint_source"):
            ShardedPipeline(3, None, None, 4, 512, "cpu", joint_source=bad, pipeline_factory=_FakeStreamPipeline)


def test_predicted_without_coupling_needs_the_index_head():
    from articulated_pose_amd.pipeline import check_joint_inputs
    pred = {"nocs_per_point": 0, "instance_per_point": 0, "joint_axis_per_point": 0}
    with pytest.raises(ValueError, match="index_per_point"):
        check_joint_inputs("predicted", False, None, pred)
    with pytest.raises(ValueError, match="index_per_point"):
        check_joint_inputs("predicted", False, None, None)
    check_joint_inputs("predicted", False, None, dict(pred, index_per_point=np.zeros((1, 1, 3))))
    check_joint_inputs("predicted", True, None, None)               # coupled: the step's own index head
    with pytest.raises(ValueError, match="joint_cls"):
        check_joint_inputs("gt", True, None, None)
    check_joint_inputs("gt", True, np.zeros((1, 1), np.int32), None)


class _FakePredictedPipeline(_FakeStreamPipeline):
    """The stand-in stream built with joint_source="predicted": records what load_inputs receives."""

    def __init__(self, *a, joint_source="gt", couple=True, **kw):
        assert joint_source == "predicted" and not couple
        super().__init__(*a, **kw)
        self.loaded = None

    def load_inputs(self, P, joint_cls=None, pred=None, slot=None):
        self.loaded = (P, joint_cls, pred)


def test_sharded_pipeline_passes_the_joint_source_and_checks_inputs():
    from articulated_pose_amd.dist import ShardedPipeline
    sp = ShardedPipeline(3, None, None, 4, 8, "cpu", slots=2, pipeline_factory=_FakePredictedPipeline, raw_capacity=CAP,
                         joint_source="predicted", couple=False)
    pred = {"nocs_per_point": np.zeros((4, 8, 9)), "instance_per_point": np.zeros((4, 8, 3)), "joint_axis_per_point": np.zeros((4, 8, 3))}
    with pytest.raises(ValueError, match="index_per_point"):
        sp.load_inputs(np.zeros((4, 8, 3)), None, pred)
    assert sp.pipe.loaded is None                                   # refused before the rank's pipeline saw anything
    sp.load_inputs(np.zeros((4, 8, 3)), None, dict(pred, index_per_point=np.ones((4, 8, 3))))
    P, jc, got = sp.pipe.loaded
    assert jc is None and got["index_per_point"].shape == (4, 8, 3)
    # the default is not passed on: a stand-in that predates joint_source still builds
    ShardedPipeline(3, None, None, 4, 8, "cpu", slots=2, pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP)


def test_solver_needs_exactly_one_association():
    from articulated_pose_amd.pose import PoseSolver
    s = PoseSolver(3, 0.1, 10, 2, "cuda:0")
    z = np.zeros((1, 4, 3), np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        s.solve(z, np.zeros((1, 4, 9), np.float32), z, z)
    with pytest.raises(ValueError, match="exactly one"):
        s.solve(z, np.zeros((1, 4, 9), np.float32), z, z, np.zeros((1, 4), np.int32), joint_index=z)
    with pytest.raises(ValueError, match="exactly one"):
        s.solve_stage_b({}, z)


def test_pose_multi_process_joint_source_parses():
    from articulated_pose_amd.pose_multi_process import build_parser
    assert build_parser().parse_args([]).joint_source == "gt"
    assert build_parser().parse_args(["--joint_source", "predicted"]).joint_source == "predicted"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--joint_source", "labels"])


def test_offline_solver_refuses_a_bad_joint_source():
    from articulated_pose_amd.pose import solver_ransac_nonlinear
    with pytest.raises(ValueError, match="joint_source"):
        solver_ransac_nonlinear(0, 0, "e", "b", 0.1, 3, [], [], None, "/nonexistent/x.pkl", joint_source="labels")
