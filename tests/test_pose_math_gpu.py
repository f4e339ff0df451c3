"""The closed-form device functions of csrc/pose_math.h, called with chosen arguments through the test-only probe
(oracle/pose_math_probe.hip -> oracle/_build/libancsh_pose_probe.so, loaded by oracle/pose_probe.py) and held to 50-digit
references (tests/golden/pose_math.npz, written by tests/golden/gen_pose_math_golden.py; numpy is all this module needs).

Bars.  For each family the generator records the largest error that the usual float64 implementation of the same operation shows
against mpmath on the same arguments; the bar is 64 x that figure, floor 64 eps = 1.42e-14: one order of magnitude for a different
algorithm (Jacobi sweeps, or Newton + adjugate with contracted FMAs and Newton reciprocals, against backward-stable LAPACK), the
rest for a maximum over more draws than were measured.  fast_rcp / fast_rsqrt: 2 ulp, the header's own claim.  What the device showed
never sets a bar.

    family                       float64 reference           its error   bar         device (MI355X)
    horn  optimality gap / s1    numpy SVD-Kabsch            1.64e-15    1.05e-13    horn_quat 5.8e-16; horn_quat_fast 1.5e-14 (rank 1), 1.2e-15 otherwise
    horn  max|R - R*| (well)     numpy SVD-Kabsch            1.03e-14    6.58e-13    horn_quat 3.1e-15; horn_quat_fast 1.3e-14
    quat_to_mat                  scipy Rotation              3.00e-16    1.92e-14    5.6e-16
    quat_to_rotvec               scipy Rotation              8.52e-16    5.45e-14    8.9e-16
    rotvec_to_mat                scipy Rotation              4.25e-16    2.72e-14    6.7e-16
    rotvec round trip            scipy Rotation              4.44e-16    2.84e-14    4.4e-16
    rod_prepare + rod_apply      numpy Rodrigues (oracle)    2.44e-15    1.56e-13    4.3e-15
    sincos_compact  absolute     libm sin, cos               5.57e-17    1.42e-14    1.1e-16
    sincos_compact  relative     libm sin, cos (|x| <= pi)   1.05e-16    1.42e-14    2.0e-16 (5.8e-11 at fl(pi/2) with the two-term reduction)
    chol6 + chol6_solve          numpy.linalg.solve          5.63e-07    3.60e-05    6.9e-08 (6.3e-15 at condition <= 1e3)
    fast_rcp, fast_rsqrt         correctly rounded           --          2 ulp       1.17 / 1.47 ulp
    lmpar6 (properties)          --                          --          0.1 delta   | |z| - delta | <= 0.098 delta, residual 1.8e-16
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_math.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def probe(dev):
    from oracle import pose_probe
    pose_probe.lib()                      # a missing library is a failure that names the make command, not a skip
    return pose_probe.call


def quat_mat(q):
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def mat_quat(R):
    """Shepperd's method, (w, x, y, z) with w >= 0 -- the host step of the round trip"""
    out = np.empty((len(R), 4))
    for i, m in enumerate(R):
        t = np.array([m[0, 0] + m[1, 1] + m[2, 2], m[0, 0], m[1, 1], m[2, 2]])
        k = int(np.argmax(t))
        if k == 0:
            q = np.array([1 + t[0], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
        else:
            a, b, c = k - 1, k % 3, (k + 1) % 3
            q = np.empty(4)
            q[0] = m[c, b] - m[b, c]
            q[1 + a] = 1 + 2 * m[a, a] - t[0]
            q[1 + b] = m[b, a] + m[a, b]
            q[1 + c] = m[c, a] + m[a, c]
        q /= np.linalg.norm(q)
        out[i] = q if q[0] >= 0 else -q
    return out


@pytest.mark.parametrize("name", ["horn_quat", "horn_quat_fast"])
def test_horn_is_optimal_on_every_case(g, probe, name):
    """unit quaternion, w >= 0, proper R, and tr(R^T M) within the bar of the optimum s1 + s2 +- s3 on EVERY case: full rank,
    reflections, rank 2, exact rank 1 in every sign pattern and position of the largest entry, a = -b, M = 0, M x 1e-12 and 1e+12.
    A rank-1 arc of the wrong sign has gap 2."""
    M, kind = g["horn_M"], g["horn_kind"]
    q = probe(name, M)
    assert np.isfinite(q).all()
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 4 * EPS and (q[:, 0] >= 0).all()
    R = quat_mat(q)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 32 * EPS and np.abs(np.linalg.det(R) - 1).max() <= 32 * EPS   # |q| = 1 to 4 eps -> R R^T = |q|^4 I
    s1 = np.where(g["horn_sigma"][:, 0] > 0, g["horn_sigma"][:, 0], 1.0)
    gap = (g["horn_opt"] - np.einsum("nab,nab->n", R, M.reshape(-1, 3, 3))) / s1
    for k in np.unique(kind):
        print(f"{name} {k:10s} cases {int((kind == k).sum()):4d}  max gap {gap[kind == k].max():.3e}  (bar {float(g['horn_gap_bar']):.3e})")
    well = g["horn_well"]
    dR = np.abs(R.reshape(-1, 9) - g["horn_R"]).max(1)
    print(f"{name} max|R - R*| over {int(well.sum())} well-conditioned cases {dR[well].max():.3e}  (bar {float(g['horn_dR_bar']):.3e})")
    worst = int(np.argmax(gap))
    assert gap.max() <= g["horn_gap_bar"], (kind[worst], M[worst].tolist(), float(gap[worst]))
    assert dR[well].max() <= g["horn_dR_bar"]


def test_rotation_conversions(g, probe):
    """quat_to_mat, quat_to_rotvec, rotvec_to_mat at angles 0, 1e-300, 1e-12, 1e-3 -+ one ulp (both sides of the series switch), 1,
    pi - 1e-9 and pi, and the round trip rotvec -> matrix -> (host) quaternion -> rotvec"""
    e_q_R = np.abs(probe("quat_to_mat", g["rot_q"]) - g["rot_q_R"]).max()
    e_q_rv = np.abs(probe("quat_to_rotvec", g["rot_q"]) - g["rot_q_rv"]).max()
    R = probe("rotvec_to_mat", g["rot_rv"])
    e_rv_R = np.abs(R - g["rot_rv_R"]).max()
    trip = g["rot_trip"]
    back = probe("quat_to_rotvec", mat_quat(R.reshape(-1, 3, 3)[trip]))
    e_trip = np.abs(back - g["rot_rv"][trip]).max()
    print(f"quat_to_mat {e_q_R:.3e} (bar {float(g['rot_q_R_bar']):.3e})  quat_to_rotvec {e_q_rv:.3e} (bar {float(g['rot_q_rv_bar']):.3e})  "
          f"rotvec_to_mat {e_rv_R:.3e} (bar {float(g['rot_rv_R_bar']):.3e})  round trip {e_trip:.3e} (bar {float(g['rot_trip_bar']):.3e})")
    assert e_q_R <= g["rot_q_R_bar"] and e_q_rv <= g["rot_q_rv_bar"] and e_rv_R <= g["rot_rv_R_bar"] and e_trip <= g["rot_trip_bar"]


def test_rodrigues_prepare_and_apply(g, probe):
    """|rv| in {0, 1e-300, 1e-160 (the squares underflow: the th == 0 path), 1e-8, 1, 3, 50}: finite and within the bar everywhere"""
    got = probe("rodrigues", g["rod_in"])
    assert np.isfinite(got).all()
    e = np.abs(got - g["rod_out"]).max(1)
    print(f"rodrigues max error {e.max():.3e} (bar {float(g['rod_bar']):.3e}), by |rv| block {[f'{v:.1e}' for v in e.reshape(7, -1).max(1)]}")
    assert e.max() <= g["rod_bar"]


def test_sincos_compact(g, probe):
    """|x| <= 1e4, fl(k pi/2) up to k = 6366 included: absolute error; |x| <= pi: relative error too"""
    x = g["sincos_x"]
    got = probe("sincos", x)
    assert np.isfinite(got).all()
    want = np.stack([g["sincos_s"], g["sincos_c"]], 1)
    e_abs = np.abs(got - want)
    small = g["sincos_small"]
    with np.errstate(divide="ignore", invalid="ignore"):
        e_rel = np.where(want != 0, e_abs / np.abs(want), np.where(got == 0, 0.0, np.inf))[small]
    i = int(np.argmax(e_rel.max(1)))
    print(f"sincos abs {e_abs.max():.3e} (bar {float(g['sincos_abs_bar']):.3e})  rel on |x| <= pi {e_rel.max():.3e} at x = {x[small][i]!r} "
          f"(bar {float(g['sincos_rel_bar']):.3e})")
    assert e_abs.max() <= g["sincos_abs_bar"]
    assert e_rel.max() <= g["sincos_rel_bar"], (x[small][i], got[small][i].tolist(), want[small][i].tolist())


def test_fast_reciprocals_within_two_ulp(g, probe):
    """1e-290 .. 1e+290, both signs for rcp: error in ulps against the correctly rounded value"""
    worst = {}
    for name in ("rcp", "rsqrt"):
        y, frac = g[name + "_y"], g[name + "_frac"]
        got = probe(name, g[name + "_x"])[:, 0]
        assert np.isfinite(got).all()
        worst[name] = np.abs((got - y) / np.spacing(np.abs(y)) - frac).max()
    print(f"fast_rcp {worst['rcp']:.2f} ulp, fast_rsqrt {worst['rsqrt']:.2f} ulp (bar {float(g['recip_ulp_bar'])})")
    assert max(worst.values()) <= g["recip_ulp_bar"]


def test_chol6_solves_and_rejects(g, probe):
    """random SPD 6 x 6, condition 1 .. 1e10, par in {0, 1e-3, 1}: x against mpmath's solve; an indefinite matrix is not ok"""
    got = probe("chol_solve", g["chol_in"])
    assert (got[:, 6] == 1.0).all()
    want = g["chol_x"]
    e = np.abs(got[:, :6] - want).max(1) / np.abs(want).max(1)
    print(f"chol6 max relative error {e.max():.3e} (bar {float(g['chol_bar']):.3e}); at condition <= 1e3: {e[g['chol_cond'] <= 1e3].max():.3e}")
    assert e.max() <= g["chol_bar"]
    assert (probe("chol_solve", g["chol_indefinite"])[:, 6] == 0.0).all()


def test_lmpar6_properties(g, probe):
    """|A^-1 g| <= 1.1 delta: par == 0 and z is the Gauss-Newton step; otherwise | |z| - delta | <= 0.1 delta, par > 0 and
    (A + par I) z = g to the solve's bar (normwise residual)"""
    cases, inside = g["lmpar_in"], g["lmpar_inside"]
    assert len(cases) >= 0.9 * int(g["lmpar_drawn"])
    got = probe("lmpar", cases)
    assert np.isfinite(got).all()
    par, z = got[:, 0], got[:, 1:]
    delta = cases[:, 27]
    A = np.zeros((len(cases), 6, 6))
    il = np.tril_indices(6)
    A[:, il[0], il[1]] = cases[:, :21]
    A[:, il[1], il[0]] = cases[:, :21]
    gvec = cases[:, 21:27]
    assert (par[inside] == 0.0).all()
    e_gn = (np.abs(z - g["lmpar_gn"]).max(1) / np.abs(g["lmpar_gn"]).max(1))[inside].max()
    out = ~inside
    assert (par[out] > 0.0).all()
    off = np.abs(np.linalg.norm(z, axis=1) - delta)[out] / delta[out]
    Ap = A + par[:, None, None] * np.eye(6)
    res = np.linalg.norm(np.einsum("nab,nb->na", Ap, z) - gvec, axis=1) / (np.linalg.norm(Ap, axis=(1, 2)) * np.linalg.norm(z, axis=1)
                                                                           + np.linalg.norm(gvec, axis=1))
    print(f"lmpar6: Gauss-Newton step error {e_gn:.3e}, max | |z| - delta | / delta {off.max():.3f}, residual {res.max():.3e} "
          f"(bar {float(g['chol_bar']):.3e})")
    assert e_gn <= g["chol_bar"] and off.max() <= 0.1 and res.max() <= g["chol_bar"]
