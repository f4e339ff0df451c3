#!/usr/bin/env python
"""Generates the golden vectors of the PRISMATIC joint fit by IMPORTING the reference's own Python code, the way gen_pose_golden.py
does for the revolute fit (whose import_reference() shims are reused by import).

Run in the build container only (it needs the reference tree):
    python tests/golden/gen_prismatic_golden.py

The reference's ransac() never forwards joint_type, so its estimator is handed over as
functools.partial(pose.joint_transformation_estimator, joint_type='prismatic'): the keyword survives both call shapes of ransac()
(:26 and :32).  np.random.seed + the replayed draws are those of gen_pose_golden.py sections 3 and 4, and every LM call's x0 / x /
nfev / status is recorded by wrapping the module global `least_squares` of the imported solver.  On the way it asserts that
tests/prismatic_oracle.py reproduces the imported reference bit for bit on every fixture -- that is what pins that file.

Writes (arrays only):
    pose_ransacB_prismatic_{small,full}.npz   one joint, 8 / 200 hypotheses, the keys of pose_ransacB_* + n_ill_posed
    pose_cloud_prismatic_K4_N2048.npz         a drawer: K = 4, all joints prismatic, budgets 10000 / 200
    pose_cloud_mixed_K3_N1024.npz             joint 1 revolute, joint 2 prismatic, budgets 10000 / 200
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE), HERE]
sys.dont_write_bytecode = True

from gen_pose_golden import import_reference, quiet  # noqa: E402

MAX_ILL_POSED = 0.10      # of the hypotheses: the cap on the hypotheses the GPU parity test may exempt (see test_prismatic_gpu.py)


def make_mixed_cloud(cloud_id, N, joint_types):
    """synthetic.make_cloud's construction with a kind per joint: part j > 0 turns about the joint axis against part 0 when joint j
    is revolute and only slides along it when it is prismatic."""
    from articulated_pose_amd.synthetic import _axis_rot, _box_surface, _rand_rot
    K = len(joint_types) + 1
    rng = np.random.RandomState(4321 + cloud_id)
    frac = rng.dirichlet([2.0] * K)
    n = np.maximum(64, np.round(frac * N).astype(int))
    while n.sum() != N:
        n[np.argmax(n)] += np.sign(N - n.sum())
    R0 = _rand_rot(rng)
    u = rng.randn(3)
    u /= np.linalg.norm(u)
    s = rng.uniform(0.6, 1.2, K)
    t0 = rng.uniform(-0.2, 0.2, 3)
    P, nocs, cls, Rs, ts = [], [], [], [], []
    for j in range(K):
        x = _box_surface(rng, n[j], rng.uniform(0.3, 1.0, 3))
        if j == 0:
            Rj, tj = R0, t0
        elif joint_types[j - 1] == 'revolute':
            Rj, tj = R0 @ _axis_rot(u, rng.uniform(-1.2, 1.2)), t0 + rng.uniform(-0.3, 0.3, 3)
        else:
            Rj, tj = R0, t0 + rng.uniform(-0.6, 0.6) * (R0 @ u) + rng.uniform(-0.3, 0.3, 3)
        P.append(s[j] * x @ Rj.T + tj); nocs.append(x); cls.append(np.full(n[j], j)); Rs.append(Rj); ts.append(tj)
    P = np.concatenate(P)
    ctr = 0.5 * (P.max(0) + P.min(0))
    g = 1.0 / np.linalg.norm(P.max(0) - P.min(0))
    perm = rng.permutation(N)
    return dict(P=((P - ctr) * g)[perm].astype(np.float32), nocs_gt=np.concatenate(nocs)[perm].astype(np.float32),
                cls_gt=np.concatenate(cls)[perm].astype(np.int64), joint_axis=u.astype(np.float32), R=np.stack(Rs), s=s * g,
                t=np.stack([(ts[j] - ctr) * g for j in range(K)]), n_parts=n)


def main():
    d3, pose, aligning = import_reference()
    from oracle import pose_oracle as PO
    import prismatic_oracle as PR
    import articulated_pose_amd  # noqa: F401
    from articulated_pose_amd.synthetic import make_cloud, make_predictions

    calls = []
    real_ls = pose.least_squares

    def logged_ls(fun, x0, *a, **kw):
        res = real_ls(fun, x0, *a, **kw)
        calls.append(dict(x0=np.array(x0, np.float64), x=res.x.copy(), nfev=res.nfev, status=res.status, fun=fun.__name__))
        return res
    pose.least_squares = logged_ls
    prismatic = functools.partial(pose.joint_transformation_estimator, joint_type='prismatic')

    def save(name, **arrays):
        np.savez_compressed(os.path.join(HERE, name), **arrays)
        print(name, os.path.getsize(os.path.join(HERE, name)))

    # ---- one joint, per-hypothesis LM records (gen_pose_golden.py section 3 with the prismatic estimator) ----
    for tag, niter, first_cid, first_seed in (("small", 8, 107, 121), ("full", 200, 109, 122)):
        # the first (cloud id, seed) whose draws hold <= 10 % ill-posed samples: a property of the draws alone, checked before any fit
        found = False
        for cid in range(first_cid, first_cid + 40):
            c = make_cloud(cid, N=512, K=2, joint_type="prismatic")
            pr = make_predictions(c, 2, seed=cid)
            lab = np.argmax(pr["instance_per_point"], 1)
            p0, p1 = np.where(lab == 0)[0], np.where(lab == 1)[0]
            ds = dict(source0=pr["nocs_per_point"][p0, :3], target0=c["P"][p0], source1=pr["nocs_per_point"][p1, 3:6], target1=c["P"][p1])
            ds["nsource0"], ds["nsource1"] = len(p0), len(p1)
            ds["joint_direction"] = np.median(pr["joint_axis_per_point"][np.where(pr["joint_cls_gt"] == 1)[0]], 0)
            for seed in range(first_seed, first_seed + 3):
                rs = np.random.RandomState(seed)
                draws = np.stack([np.concatenate([rs.randint(len(p0), size=3), rs.randint(len(p1), size=3)]) for _ in range(niter)])
                n_ill = sum(PR.ill_posed(d, ds["source0"], ds["target0"], ds["source1"], ds["target1"]) for d in draws)
                if n_ill <= MAX_ILL_POSED * niter:
                    found = True
                    break
            if found:
                break
        if not found:
            raise SystemExit("no (cloud id, seed) with <= 10 % ill-posed draws")
        del calls[:]
        np.random.seed(seed)
        with quiet():
            model, inl = pose.ransac(ds, prismatic, pose.joint_transformation_verifier, 0.1, niter)
        assert len(calls) == niter + 1 and all(cl["fun"] == "objective_eval_r" for cl in calls)
        stream = PO.SampleStream([d for row in draws for d in (row[:3], row[3:])])
        info, lm_log = {}, []
        m2, inl2 = PO.ransac(ds, PR.estimator_for("prismatic", lm_log), PO.joint_transformation_verifier, 0.1, niter, stream, info)
        for k in model:
            assert np.array_equal(np.asarray(model[k]), np.asarray(m2[k])), k
        assert np.array_equal(inl[0], inl2[0]) and np.array_equal(inl[1], inl2[1])
        for a, b in zip(calls, lm_log):
            assert np.array_equal(a["x0"], b["x0"]) and np.array_equal(a["x"], b["x"]) and a["nfev"] == b["nfev"] and a["status"] == b["status"]
        out = dict(joint_direction=ds["joint_direction"], th=np.float64(0.1), draws=draws.astype(np.int32), inliers0=inl[0], inliers1=inl[1],
                   best_iter=np.asarray(info["best_iter"]), best_score=np.asarray(info["best_score"]),
                   lm_x0=np.stack([l["x0"] for l in calls]), lm_x=np.stack([l["x"] for l in calls]),
                   lm_nfev=np.asarray([l["nfev"] for l in calls]), lm_status=np.asarray([l["status"] for l in calls]),
                   n_ill_posed=np.asarray(n_ill), cloud_id=np.asarray(cid), seed=np.asarray(seed))
        for k in ("source0", "target0", "source1", "target1"):
            out[k] = ds[k]
        for k in model:
            out[k] = np.asarray(model[k])
            out["hyp_" + k] = np.asarray(info["hyp_model"][k])
        save(f"pose_ransacB_prismatic_{tag}.npz", **out)
        print(f"  cloud {cid} seed {seed}: {n_ill} of {niter} draws ill-posed; nfev mean {np.mean(out['lm_nfev'][:niter]):.1f} max {out['lm_nfev'][:niter].max()}")

    # ---- whole clouds (gen_pose_golden.py section 4): a drawer, and a mixed object ----
    for name, K, types, c, cid, seed in (
            ("pose_cloud_prismatic_K4_N2048.npz", 4, ["prismatic"] * 3, make_cloud(136, N=2048, K=4, joint_type="prismatic"), 136, 146),
            ("pose_cloud_mixed_K3_N1024.npz", 3, ["revolute", "prismatic"], make_mixed_cloud(137, 1024, ["revolute", "prismatic"]), 137, 147)):
        na, nb = 10000, 200
        pr = make_predictions(c, K, seed=cid)
        lab = np.argmax(pr["instance_per_point"], 1)
        counts = [int((lab == j).sum()) for j in range(K)]
        plan = []
        for j in range(K):
            plan += PO.stage_a_plan(counts[j], na)
        for j in range(1, K):
            plan += PO.stage_b_plan(counts[0], counts[j], nb)
        rs = np.random.RandomState(seed)
        all_draws = [rs.randint(n, size=3) for n in plan]
        np.random.seed(seed)
        ref = dict(baseline=[], nonlinear=[None] * K)
        partidx = [np.where(lab == j)[0] for j in range(K)]
        nfev = []
        with quiet():
            for j in range(K):
                ds = dict(source=pr["nocs_per_point"][partidx[j], 3 * j:3 * j + 3], target=c["P"][partidx[j], :3])
                ds["nsource"] = ds["source"].shape[0]
                m, _ = pose.ransac(ds, pose.single_transformation_estimator, pose.single_transformation_verifier, 0.1, na)
                ref["baseline"].append((m["rotation"], m["scale"], m["translation"]))
            for j in range(1, K):
                ds = dict(source0=pr["nocs_per_point"][partidx[0], :3], target0=c["P"][partidx[0], :3],
                          source1=pr["nocs_per_point"][partidx[j], 3 * j:3 * j + 3], target1=c["P"][partidx[j], :3])
                ds["nsource0"], ds["nsource1"] = len(partidx[0]), len(partidx[j])
                ds["joint_direction"] = np.median(pr["joint_axis_per_point"][np.where(pr["joint_cls_gt"] == j)[0], :], 0)
                del calls[:]
                est = prismatic if types[j - 1] == "prismatic" else pose.joint_transformation_estimator
                m, _ = pose.ransac(ds, est, pose.joint_transformation_verifier, 0.1, nb)
                assert all(cl["fun"] == ("objective_eval_r" if types[j - 1] == "prismatic" else "objective_eval") for cl in calls)
                nfev.append([cl["nfev"] for cl in calls])
                if j == 1:
                    ref["nonlinear"][0] = (m["rotation0"], m["scale0"], m["translation0"])
                ref["nonlinear"][j] = (m["rotation1"], m["scale1"], m["translation1"])
        pos = 0
        sa, sb = [], []
        for j in range(K):
            sa.append(PO.SampleStream(all_draws[pos:pos + na])); pos += na
        for j in range(1, K):
            sb.append(PO.SampleStream(all_draws[pos:pos + 2 * nb])); pos += 2 * nb
        logs = {}
        got = PR.solve_cloud(c["P"], pr["nocs_per_point"], pr["instance_per_point"], pr["joint_axis_per_point"], pr["joint_cls_gt"], K,
                             sa, sb, types, 0.1, na, nb, lm_logs=logs)
        for kind in ("baseline", "nonlinear"):
            for j in range(K):
                for a, b in zip(ref[kind][j], got[kind][j]):
                    assert np.array_equal(np.asarray(a), np.asarray(b)), (name, kind, j)
        for j in range(1, K):
            assert [l["nfev"] for l in logs[j]] == nfev[j - 1], (name, j)
        # a revolute joint of a mixed object: the frozen oracle's answer for that joint (same draws)
        for s in sa + sb:
            s.pos = 0
        old = PO.solve_cloud(c["P"], pr["nocs_per_point"], pr["instance_per_point"], pr["joint_axis_per_point"], pr["joint_cls_gt"], K,
                             sa, sb, 0.1, na, nb)
        for j in range(1, K):
            if types[j - 1] == "revolute":
                for jj in ((0, j) if j == 1 else (j,)):
                    for a, b in zip(ref["nonlinear"][jj], old["nonlinear"][jj]):
                        assert np.array_equal(np.asarray(a), np.asarray(b)), (name, "revolute joint", j)
        out = dict(P=c["P"], K=np.asarray(K), niter_a=np.asarray(na), niter_b=np.asarray(nb), th=np.float64(0.1),
                   draws_a=np.stack([np.stack(s.draws) for s in sa]).astype(np.int32),
                   draws_b=np.stack([np.stack(s.draws).reshape(nb, 6) for s in sb]).astype(np.int32),
                   joint_kind=np.asarray([int(t == "prismatic") for t in types], np.int32), lm_nfev=np.asarray(nfev, np.int32),
                   R_gt=c["R"], s_gt=c["s"], t_gt=c["t"], **pr)
        for kind in ("baseline", "nonlinear"):
            out[kind + "_R"] = np.stack([np.asarray(ref[kind][j][0], np.float64) for j in range(K)])
            out[kind + "_s"] = np.asarray([float(ref[kind][j][1]) for j in range(K)])
            out[kind + "_t"] = np.stack([np.asarray(ref[kind][j][2], np.float64) for j in range(K)])
        save(name, **out)


if __name__ == "__main__":
    main()
