"""CPU restatement of the reference's PRISMATIC joint fit (test infrastructure; never imported by the product).

oracle/pose_oracle.py restates joint_transformation_estimator for joint_type='revolute' only.  The other branch of the same function
is restated here, function by function, on top of that oracle's pieces (imported, not copied):

    evaluation/parallel_ancsh_pose.py:70-81     objective_eval_r
    evaluation/parallel_ancsh_pose.py:106-184   joint_transformation_estimator(..., joint_type)   (:150-152 the prismatic call)
    evaluation/parallel_ancsh_pose.py:238-341   per-cloud body with a joint type per joint -> solve_cloud

As in the oracle, the 3-point samples come from an explicit SampleStream instead of the global numpy RNG.  What pins this file:
tests/golden/gen_prismatic_golden.py asserts that it reproduces the imported reference bit for bit on every fixture it writes, and
tests/test_prismatic_cpu.py re-checks it against the committed fixtures.
"""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation as srot

from oracle import pose_oracle as PO

JOINT_TYPES = ("revolute", "prismatic")


def objective_eval_r(params, x0, y0, x1, y1, joints, isweight=True, joint_type='prismatic'):    # :70-81
    rotvec0 = params[:3].reshape((1, 3))
    rotvec1 = params[3:].reshape((1, 3))
    res0 = y0 - PO.rotate_points_with_rotvec(x0, rotvec0)
    res1 = y1 - PO.rotate_points_with_rotvec(x1, rotvec1)
    res_R = rotvec0 - rotvec1                                       # `joints` is unused
    if isweight:
        res0 /= x0.shape[0]
        res1 /= x1.shape[0]
    return np.concatenate((res0, res1, res_R), 0).ravel()


def joint_transformation_estimator(dataset, best_inliers=None, stream=None, lm_log=None, joint_type='revolute'):   # :106-184
    if joint_type not in JOINT_TYPES:
        raise ValueError(joint_type)
    if best_inliers is None:
        sample_idx0 = stream.next(dataset['nsource0'])               # :110-111
        sample_idx1 = stream.next(dataset['nsource1'])
    else:
        sample_idx0 = best_inliers[0]
        sample_idx1 = best_inliers[1]
    source0 = dataset['source0'][sample_idx0, :]
    target0 = dataset['target0'][sample_idx0, :]
    source1 = dataset['source1'][sample_idx1, :]
    target1 = dataset['target1'][sample_idx1, :]
    scale0 = PO.scale_pts(source0, target0)                          # :121-124
    scale1 = PO.scale_pts(source1, target1)
    scale0_inv = PO.scale_pts(target0, source0)
    scale1_inv = PO.scale_pts(target1, source1)

    target0_scaled_centered = scale0_inv * target0                   # :126-132
    target0_scaled_centered -= np.mean(target0_scaled_centered, 0, keepdims=True)
    source0_centered = source0 - np.mean(source0, 0, keepdims=True)
    target1_scaled_centered = scale1_inv * target1
    target1_scaled_centered -= np.mean(target1_scaled_centered, 0, keepdims=True)
    source1_centered = source1 - np.mean(source1, 0, keepdims=True)

    nj = np.min((source0.shape[0], source1.shape[0]))                # :134
    joint_points0 = np.ones_like(np.linspace(0, 1, num=nj + 1)[1:].reshape((-1, 1))) * dataset['joint_direction'].reshape((1, 3))

    R0 = PO.rotate_pts(source0_centered, target0_scaled_centered)    # :138-139
    R1 = PO.rotate_pts(source1_centered, target1_scaled_centered)
    rotvec0 = srot.from_matrix(R0).as_rotvec()                       # reference: from_dcm (:147)
    rotvec1 = srot.from_matrix(R1).as_rotvec()
    x0 = np.hstack((rotvec0, rotvec1))
    fun = objective_eval_r if joint_type == 'prismatic' else PO.objective_eval      # :150-155
    res = least_squares(fun, x0, verbose=0, ftol=1e-4, method='lm',
                        args=(source0_centered, target0_scaled_centered, source1_centered, target1_scaled_centered,
                              joint_points0, False))
    if lm_log is not None:
        lm_log.append(dict(x0=x0, x=res.x.copy(), nfev=res.nfev, status=res.status, cost=res.cost))
    R0 = srot.from_rotvec(res.x[:3]).as_matrix()                     # reference: as_dcm (:156)
    R1 = srot.from_rotvec(res.x[3:]).as_matrix()
    translation0 = np.mean(target0.T - scale0 * np.matmul(R0, source0.T), 1)       # :174-175
    translation1 = np.mean(target1.T - scale1 * np.matmul(R1, source1.T), 1)
    return dict(rotation0=R0, scale0=scale0, translation0=translation0,
                rotation1=R1, scale1=scale1, translation1=translation1)


def estimator_for(joint_type, lm_log=None):
    """A model_estimator for PO.ransac (which calls it as f(dataset, stream=...) and f(dataset, best_inliers))."""
    def est(dataset, best_inliers=None, stream=None):
        return joint_transformation_estimator(dataset, best_inliers, stream, lm_log, joint_type)
    return est


def ill_posed(draw, source0, target0, source1, target1):
    """The rule of tests/test_pose_gpu.py::test_ransac_joint_golden for a hypothesis whose LM trajectory may differ: a repeated index in
    either 3-point sample, or a sample triangle whose second singular value is below 0.1 of the first."""
    if len(set(draw[:3].tolist())) < 3 or len(set(draw[3:].tolist())) < 3:
        return True
    for pts in (source0[draw[:3]], target0[draw[:3]], source1[draw[3:]], target1[draw[3:]]):
        sv = np.linalg.svd((pts - pts.mean(0)).astype(np.float64), compute_uv=False)
        if sv[1] < 0.1 * sv[0]:
            return True
    return False


def solve_cloud(P, nocs_pred, mask_pred, joint_axis_per_point, joint_cls_gt, num_parts, streams_a, streams_b, joint_types,
                inlier_th=0.1, niter_a=10000, niter_b=200, lm_logs=None):
    """PO.solve_cloud (:238-341) with joint_types[j - 1] the kind of joint j.  streams_a None: stage B only ('baseline' is then empty).
    A part or joint without points gives None entries instead of the reference's exception."""
    cls_per_pt_pred = np.argmax(mask_pred, axis=1)
    partidx = [np.where(cls_per_pt_pred == j)[0] for j in range(num_parts)]
    out = dict(baseline=[], nonlinear=[None] * num_parts, inliers_b=[], info_b=[])
    if streams_a is not None:
        for j in range(num_parts):
            dataset = dict(source=nocs_pred[partidx[j], 3 * j:3 * (j + 1)], target=P[partidx[j], :3])
            dataset['nsource'] = dataset['source'].shape[0]
            m, _ = PO.ransac(dataset, PO.single_transformation_estimator, PO.single_transformation_verifier, inlier_th, niter_a,
                             streams_a[j])
            out['baseline'].append((m['rotation'], m['scale'], m['translation']))
    for j in range(1, num_parts):
        dataset = dict(source0=nocs_pred[partidx[0], :3], target0=P[partidx[0], :3],
                       source1=nocs_pred[partidx[j], 3 * j:3 * (j + 1)], target1=P[partidx[j], :3])
        dataset['nsource0'] = dataset['source0'].shape[0]
        dataset['nsource1'] = dataset['source1'].shape[0]
        sel = np.where(joint_cls_gt == j)[0]
        dataset['joint_direction'] = np.median(joint_axis_per_point[sel, :], 0) if len(sel) else np.full(3, np.nan)   # :295
        if dataset['nsource0'] == 0 or dataset['nsource1'] == 0:
            out['inliers_b'].append(None)
            out['info_b'].append({})
            continue
        log = None if lm_logs is None else lm_logs.setdefault(j, [])
        inf = {}
        m, inl = PO.ransac(dataset, estimator_for(joint_types[j - 1], log), PO.joint_transformation_verifier, inlier_th, niter_b,
                           streams_b[j - 1], inf)
        if j == 1:
            out['nonlinear'][0] = (m['rotation0'], m['scale0'], m['translation0'])
        out['nonlinear'][j] = (m['rotation1'], m['scale1'], m['translation1'])
        out['inliers_b'].append(inl)
        out['info_b'].append(inf)
    return out
