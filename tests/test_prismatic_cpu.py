"""CPU side of the prismatic joint fit: the restated oracle against the committed fixtures (which the reference's own code produced:
tests/golden/gen_prismatic_golden.py), joint_types validation before any GPU call, the category table, and the ABI 14 symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import prismatic_oracle as PR
from oracle import pose_oracle as PO

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)


def load(name):
    with np.load(os.path.join(G, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["small", "full"])
def test_oracle_reproduces_hypothesis_fixture(tag):
    g = load(f"pose_ransacB_prismatic_{tag}.npz")
    niter = len(g["draws"])
    ds = dict(source0=g["source0"], target0=g["target0"], source1=g["source1"], target1=g["target1"], nsource0=len(g["source0"]),
              nsource1=len(g["source1"]), joint_direction=g["joint_direction"])
    stream = PO.SampleStream([d for row in g["draws"] for d in (row[:3], row[3:])])
    info, log = {}, []
    m, inl = PO.ransac(ds, PR.estimator_for("prismatic", log), PO.joint_transformation_verifier, float(g["th"]), niter, stream, info)
    for k in ("rotation0", "scale0", "translation0", "rotation1", "scale1", "translation1"):
        assert np.array_equal(np.asarray(m[k]), g[k]), k
        assert np.array_equal(np.asarray(info["hyp_model"][k]), g["hyp_" + k]), k
    assert np.array_equal(inl[0], g["inliers0"]) and np.array_equal(inl[1], g["inliers1"])
    assert info["best_iter"] == int(g["best_iter"]) and info["best_score"] == float(g["best_score"])
    assert len(log) == niter + 1
    assert [l["nfev"] for l in log] == g["lm_nfev"].tolist() and [l["status"] for l in log] == g["lm_status"].tolist()
    assert np.array_equal(np.stack([l["x0"] for l in log]), g["lm_x0"]) and np.array_equal(np.stack([l["x"] for l in log]), g["lm_x"])
    # the cap the GPU parity test relies on is a property of the fixture's own draws
    n_ill = sum(PR.ill_posed(d, g["source0"], g["target0"], g["source1"], g["target1"]) for d in g["draws"])
    assert n_ill == int(g["n_ill_posed"]) and n_ill <= 0.10 * niter


@pytest.mark.parametrize("name,types", [("pose_cloud_prismatic_K4_N2048.npz", ["prismatic"] * 3),
                                        ("pose_cloud_mixed_K3_N1024.npz", ["revolute", "prismatic"])])
def test_oracle_reproduces_cloud_fixture(name, types):
    """Stage B of the whole-cloud fixtures (stage A is the frozen oracle's, pinned by its own fixtures); the mixed object's revolute
    joint is also the frozen oracle's own answer for that joint."""
    g = load(name)
    K, nb = int(g["K"]), int(g["niter_b"])
    assert g["joint_kind"].tolist() == [int(t == "prismatic") for t in types]
    sb = [PO.SampleStream([d for row in g["draws_b"][j] for d in (row[:3], row[3:])]) for j in range(K - 1)]
    logs = {}
    got = PR.solve_cloud(g["P"], g["nocs_per_point"], g["instance_per_point"], g["joint_axis_per_point"], g["joint_cls_gt"], K, None, sb,
                         types, float(g["th"]), int(g["niter_a"]), nb, lm_logs=logs)
    for j in range(K):
        R, s, t = got["nonlinear"][j]
        assert np.array_equal(R, g["nonlinear_R"][j]) and float(s) == g["nonlinear_s"][j] and np.array_equal(t, g["nonlinear_t"][j]), j
    for j in range(1, K):
        assert [l["nfev"] for l in logs[j]] == g["lm_nfev"][j - 1].tolist()
    if "revolute" in types:
        j = types.index("revolute") + 1
        lab = np.argmax(g["instance_per_point"], 1)
        p0, pj = np.where(lab == 0)[0], np.where(lab == j)[0]
        ds = dict(source0=g["nocs_per_point"][p0, :3], target0=g["P"][p0, :3], source1=g["nocs_per_point"][pj, 3 * j:3 * j + 3],
                  target1=g["P"][pj, :3], nsource0=len(p0), nsource1=len(pj),
                  joint_direction=np.median(g["joint_axis_per_point"][np.where(g["joint_cls_gt"] == j)[0], :], 0))
        sb[j - 1].pos = 0
        m, _ = PO.ransac(ds, PO.joint_transformation_estimator, PO.joint_transformation_verifier, float(g["th"]), nb, sb[j - 1])
        assert np.array_equal(m["rotation1"], g["nonlinear_R"][j]) and np.array_equal(m["translation1"], g["nonlinear_t"][j])


def test_prismatic_objective_rows():
    x = np.array([0.1, -0.2, 0.3, 0.4, 0.5, -0.6])
    pts = np.random.RandomState(0).randn(5, 3)
    r = PR.objective_eval_r(x, pts[:3], pts[:3], pts[3:], pts[3:], np.full((2, 3), np.nan), False)
    assert r.shape == (3 * 5 + 3,) and np.isfinite(r).all()                # the joint direction does not enter
    assert np.array_equal(r[-3:], x[:3] - x[3:])


BAD_TYPES = [(["prismatic"], 3, "2 joints"), (["revolute", "prismatic", "revolute"], 3, "2 joints"), ("slider", 3, "slider"),
             (["revolute", "hinge"], 3, r"joint_types\[1\]"), (7, 3, "sequence"), ([0, 1], 3, r"joint_types\[0\]")]


@pytest.mark.parametrize("types,K,msg", BAD_TYPES)
def test_joint_types_validation_before_any_gpu_call(types, K, msg):
    """Every public entry refuses a bad joint_types with a ValueError naming the entry, before a device, a weight or a file is touched
    (device 'cuda:99' does not exist; the weights are None)."""
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose import PoseSolver, solver_ransac_nonlinear
    with pytest.raises(ValueError, match=msg):
        PoseSolver(K, device="cuda:99", joint_types=types)
    with pytest.raises(ValueError, match=msg):
        AncshPipeline(K, None, None, 4, 512, "cuda:99", joint_types=types)
    with pytest.raises(ValueError, match=msg):
        ShardedPipeline(K, None, None, 4, 512, "cuda:99", joint_types=types)
    with pytest.raises(ValueError, match=msg):
        solver_ransac_nonlinear(0, 0, "x", "y", 0.1, K, [], [], None, "/nonexistent/out.pkl", joint_types=types)


def test_joint_types_accepted_forms():
    from articulated_pose_amd.pose.parallel_ancsh_pose import check_joint_types
    assert check_joint_types(None, 4) is None
    assert check_joint_types("prismatic", 4) == (1, 1, 1) and check_joint_types("revolute", 2) == (0,)
    assert check_joint_types(("revolute", "prismatic"), 3) == (0, 1)
    assert check_joint_types([], 1) == ()


def test_pose_multi_process_joint_types_flag():
    from articulated_pose_amd import pose_multi_process as M
    from articulated_pose_amd.global_info import global_info
    infos = global_info("/nonexistent")
    assert M.build_parser().parse_args([]).joint_types == "revolute"
    assert M.resolve_joint_types("revolute", "drawer", infos) is None        # the default: today's pickles
    assert M.resolve_joint_types("category", "drawer", infos) == ["prismatic"] * 3
    assert M.resolve_joint_types("category", "laptop", infos) == ["revolute"]
    assert M.resolve_joint_types("prismatic", "eyeglasses", infos) == "prismatic"
    with pytest.raises(ValueError, match="joint_types"):
        M.resolve_joint_types("screw", "drawer", infos)
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["--joint_types", "screw"])


def test_global_info_joint_types_table():
    from articulated_pose_amd.global_info import global_info
    infos = global_info("/nonexistent")
    assert set(infos.joint_types) == set(infos.datasets)
    for name, d in infos.datasets.items():
        want = "prismatic" if name == "drawer" else "revolute"
        assert infos.joint_types[name] == (want,) * (d.num_parts - 1), name


def test_abi_14_symbols():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    assert L.ancsh_abi_version() == 14
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "ancsh_hip.h")).read()
    for base in ("ancsh_ransac_joint_rec", "ancsh_ransac_joint_rec_dseed", "ancsh_ransac_joint_rec_dkey"):
        name = base + "_kind"
        assert re.search(r"\b%s\b" % name, exported) and hasattr(L, name), name
        assert len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[base]) + 1 == 25      # one more argument: joint_kind, before the stream
        assert _lib.SIGNATURES[name][:-2] == _lib.SIGNATURES[base][:-1]
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        args = [a.strip() for a in decl.split(",")]
        assert len(args) == 25 and args[-2] == "const int *joint_kind" and args[-1] == "void *stream", name
    assert "#define ANCSH_JOINT_PRISMATIC 1" in header and "#define ANCSH_JOINT_REVOLUTE 0" in header
