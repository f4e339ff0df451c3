"""Generates tests/golden/pose_math.npz: arguments for the closed-form device functions of csrc/pose_math.h, their values at 50
digits (mpmath), and -- per family -- the largest error that the usual float64 implementation of the same operation (numpy/LAPACK
SVD-Kabsch, numpy.linalg.solve, libm sin/cos, scipy Rotation, the oracle's Rodrigues) shows against mpmath ON THE SAME ARGUMENTS.
tests/test_pose_math_gpu.py holds the device functions to 64 x that figure (floor: 64 eps); the device's own errors never enter here.

    python tests/golden/gen_pose_math_golden.py [out.npz]

CPU only, seeded, a few seconds.  tests/test_pose_math_golden_cpu.py regenerates the file and compares it with the committed one."""
import os
import sys

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

mp.mp.dps = 50
EPS = 2.0 ** -52
BAR_FACTOR = 64.0


def bar(ref_err):
    return BAR_FACTOR * max(float(ref_err), EPS)


def mpm(a):
    a = np.asarray(a, np.float64)
    return mp.matrix(a.tolist()) if a.ndim == 2 else mp.matrix([[mp.mpf(float(x))] for x in a])


def to_np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def maxabs(m):
    return max(abs(m[i, j]) for i in range(m.rows) for j in range(m.cols))


def unit(v):
    return v / np.linalg.norm(v)


# ------------------------------------------------------------------------------------------------ Horn / Kabsch
def kabsch_mp(M):
    """-> sigma (descending), optimum of tr(R^T M) over proper rotations, the maximiser R* = U diag(1, 1, d) V^T"""
    A = mpm(M)
    U, S, Vh = mp.svd_r(A)
    order = sorted(range(3), key=lambda i: -S[i])
    U = mp.matrix([[U[r, c] for c in order] for r in range(3)])
    Vh = mp.matrix([[Vh[r, c] for c in range(3)] for r in order])
    s = [S[i] for i in order]
    d = mp.sign(mp.det(U) * mp.det(Vh))
    d = d if d != 0 else mp.mpf(1)
    R = U * mp.diag([1, 1, d]) * Vh
    opt = s[0] + s[1] + d * s[2]
    tr = sum(R[i, j] * A[i, j] for i in range(3) for j in range(3))
    assert abs(tr - opt) <= mp.mpf(10) ** -40 * (s[0] if s[0] > 0 else 1), (tr, opt)
    assert maxabs(R * R.T - mp.eye(3)) < mp.mpf(10) ** -40 and abs(mp.det(R) - 1) < mp.mpf(10) ** -40
    return s, opt, R, A


def kabsch_numpy(M):
    """lib/d3_utils.py rotate_pts on the moment matrix"""
    U, D, Vh = np.linalg.svd(M)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0.0:
        U[:, -1] = -U[:, -1]
    return U @ Vh


def horn_cases(rng):
    Ms, kinds = [], []

    def add(M, kind):
        Ms.append(np.asarray(M, np.float64).reshape(3, 3)); kinds.append(kind)

    def moment(n, mirror=False):
        src = rng.randn(n, 3)
        tgt = rng.uniform(0.6, 1.6) * src @ Rotation.random(random_state=rng).as_matrix().T + 0.05 * rng.randn(n, 3)
        if mirror:
            tgt = tgt * np.array([1.0, 1.0, -1.0])
        src, tgt = src - src.mean(0), tgt - tgt.mean(0)
        return tgt.T @ src

    for n in range(4, 51):                                              # full rank, 4..50 noisy pairs (n = 3 is the rank-2 family below)
        add(moment(n), "full")
        add(moment(n), "full")
    for n in range(4, 44):
        add(moment(n, mirror=True), "reflection")
    for _ in range(40):
        add(moment(3), "rank2")                                         # three distinct points: centred, rank 2
    mags = {0: (3, 1, 2), 1: (1, 3, 2), 2: (2, 1, 3)}
    for bi in range(3):                                                 # exact a b^T: every position of the largest entry, every sign pattern
        for bj in range(3):
            for sa in range(8):
                for sb in range(8):
                    a = np.array(mags[bi], float) * [(-1) ** (sa >> k & 1) for k in range(3)]
                    b = np.array(mags[bj], float) * [(-1) ** (sb >> k & 1) for k in range(3)]
                    add(np.outer(a, b), "rank1")
    for i in range(9):                                                  # a single entry, either sign
        for sg in (1.0, -1.0):
            M = np.zeros(9); M[i] = sg * (1 + i)
            add(M, "rank1")
    for _ in range(12):                                                 # a zero component in a or b
        a, b = rng.randint(-3, 4, 3).astype(float), rng.randint(-3, 4, 3).astype(float)
        a[rng.randint(3)] = 0.0
        if np.any(a) and np.any(b):
            add(np.outer(a, b), "rank1")
    for b in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [3, 1, 0], [1, 2, 3], [-2, 1, 2], [1, -3, 1], [2, 2, -1], [0, -1, 3], [3, 3, 3], [-1, -2, -3]):
        b = np.array(b, float)
        add(np.outer(-b, b), "halfturn")                                # a = -b
    add(np.zeros(9), "zero")
    base = [Ms[i] for i in range(0, 20)] + [Ms[kinds.index("rank1") + 7 * i] for i in range(10)] + [Ms[kinds.index("rank2") + i] for i in range(4)]
    for f in (1e-12, 1e12):
        for M in base:
            add(M * f, "scaled")
    return np.array(Ms), np.array(kinds)


def gen_horn(rng, out):
    Ms, kinds = horn_cases(rng)
    n = len(Ms)
    sig, opt, Rs, gap_ref, dR_ref = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3, 3)), np.zeros(n), np.zeros(n)
    for i, M in enumerate(Ms):
        s, o, R, A = kabsch_mp(M)
        sig[i], opt[i], Rs[i] = [float(x) for x in s], float(o), to_np(R)
        Rn = mpm(kabsch_numpy(M))
        tr = sum(Rn[r, c] * A[r, c] for r in range(3) for c in range(3))
        gap_ref[i] = float(abs(o - tr) / s[0]) if s[0] > 0 else 0.0
        dR_ref[i] = float(maxabs(Rn - R))
    well = (sig[:, 1] + sig[:, 2]) >= 0.05 * sig[:, 0]
    well &= sig[:, 0] > 0
    out.update(horn_M=Ms.reshape(n, 9), horn_kind=kinds, horn_sigma=sig, horn_opt=opt, horn_R=Rs.reshape(n, 9), horn_well=well,
               horn_gap_ref=gap_ref.max(), horn_dR_ref=dR_ref[well].max(), horn_gap_bar=bar(gap_ref.max()), horn_dR_bar=bar(dR_ref[well].max()))


# ------------------------------------------------------------------------------------------------ rotations
ANGLES = [0.0, 1e-300, 1e-12, np.nextafter(1e-3, 0.0), 1e-3, np.nextafter(1e-3, 1.0), 1.0, np.pi - 1e-9, np.pi]


def axes(rng, k=9):
    return [np.array(a, float) for a in ([1, 0, 0], [0, 1, 0], [0, 0, -1])] + [unit(rng.randn(3)) for _ in range(k)]


def rodrigues_mp(rv):
    v = [mp.mpf(float(x)) for x in rv]
    th = mp.sqrt(sum(x * x for x in v))
    if th == 0:
        return mp.eye(3)
    k = [x / th for x in v]
    K = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return mp.eye(3) + mp.sin(th) * K + (1 - mp.cos(th)) * K * K


def quat_mat_mp(q):
    """rotation of the quaternion q / |q| (w, x, y, z)"""
    w, x, y, z = [mp.mpf(float(c)) for c in q]
    n2 = w * w + x * x + y * y + z * z
    return mp.matrix([[w * w + x * x - y * y - z * z, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]]) / n2


def quat_rotvec_mp(q):
    w, x, y, z = [mp.mpf(float(c)) for c in q]
    sn = mp.sqrt(x * x + y * y + z * z)
    if sn == 0:
        return mp.matrix([0, 0, 0])
    ang = 2 * mp.atan2(sn, w)
    return mp.matrix([ang * x / sn, ang * y / sn, ang * z / sn])


def gen_rot(rng, out):
    rvs, qs = [], []
    for ang in ANGLES:
        for ax in axes(rng):
            rvs.append(ang * ax)
            qs.append(np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * ax]))
    for _ in range(24):                                                 # general quaternions (w >= 0) and rotation vectors
        q = unit(rng.randn(4))
        qs.append(q if q[0] >= 0 else -q)
        rvs.append(unit(rng.randn(3)) * rng.uniform(0, np.pi))
    rvs, qs = np.array(rvs), np.array(qs)
    Rrv = np.array([to_np(rodrigues_mp(rv)) for rv in rvs])
    e_rv = max(float(maxabs(mpm(Rotation.from_rotvec(rv).as_matrix()) - rodrigues_mp(rv))) for rv in rvs)
    Rq = np.array([to_np(quat_mat_mp(q)) for q in qs])
    e_q = max(float(maxabs(mpm(Rotation.from_quat(q[[1, 2, 3, 0]]).as_matrix()) - quat_mat_mp(q))) for q in qs)
    rvq = np.array([[float(c) for c in quat_rotvec_mp(q)] for q in qs])
    e_qrv = max(float(maxabs(mpm(Rotation.from_quat(q[[1, 2, 3, 0]]).as_rotvec()) - quat_rotvec_mp(q))) for q in qs)
    # round trip rotvec -> matrix -> quaternion -> rotvec, all in scipy; angle pi itself is left out (the axis' sign is not recoverable there)
    trip = np.array([np.linalg.norm(rv) < np.pi - 5e-10 for rv in rvs])
    e_trip = max(float(np.abs(Rotation.from_matrix(Rotation.from_rotvec(rv).as_matrix()).as_rotvec() - rv).max()) for rv in rvs[trip])
    out.update(rot_rv=rvs, rot_rv_R=Rrv.reshape(-1, 9), rot_q=qs, rot_q_R=Rq.reshape(-1, 9), rot_q_rv=rvq, rot_trip=trip,
               rot_rv_R_ref=e_rv, rot_q_R_ref=e_q, rot_q_rv_ref=e_qrv, rot_trip_ref=e_trip,
               rot_rv_R_bar=bar(e_rv), rot_q_R_bar=bar(e_q), rot_q_rv_bar=bar(e_qrv), rot_trip_bar=bar(e_trip))


def gen_rod(rng, out):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from oracle import pose_oracle as PO
    cases = []
    for th in (0.0, 1e-300, 1e-160, 1e-8, 1.0, 3.0, 50.0):
        for ax in axes(rng):
            cases.append(np.concatenate([th * ax, rng.uniform(-1, 1, 3)]))
    cases = np.array(cases)
    want = np.array([[float(c) for c in rodrigues_mp(c6[:3]) * mpm(c6[3:])] for c6 in cases])
    with np.errstate(all="ignore"):
        ref = PO.rotate_points_with_rotvec(cases[:, 3:], cases[:, :3])
    # |rv| = 1e-300 and 1e-160: the squares underflow, theta is 0 and rv / theta is inf there -- the float64 reference returns NaN on most of those
    # rows, which then do not enter its error figure (the device function is still held to the bar on them)
    fin = np.isfinite(ref).all(1)
    assert fin[:12].all() and fin[36:].all()
    e = max(float(maxabs(mpm(r) - rodrigues_mp(c6[:3]) * mpm(c6[3:]))) for r, c6 in zip(ref[fin], cases[fin]))
    out.update(rod_in=cases, rod_out=want, rod_ref=e, rod_bar=bar(e))


# ------------------------------------------------------------------------------------------------ scalar functions
def gen_sincos(rng, out):
    ks = sorted(set(list(range(1, 33)) + [int(k) for k in np.unique(np.round(np.logspace(np.log10(33), np.log10(6366), 120)))] + [6365, 6366]))
    x = [0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-10, -1e-10, 1e4, -1e4]
    x += [k * (np.pi / 2) for k in ks] + [-(k * (np.pi / 2)) for k in ks[::3]]
    x += list(rng.uniform(-np.pi, np.pi, 100)) + list(rng.uniform(-1e4, 1e4, 100))
    x = np.array(x)
    assert np.abs(x).max() <= 1e4
    s = [mp.sin(mp.mpf(float(v))) for v in x]
    c = [mp.cos(mp.mpf(float(v))) for v in x]
    small = np.abs(x) <= np.pi
    e_abs = max(max(abs(mp.mpf(float(np.sin(v))) - a), abs(mp.mpf(float(np.cos(v))) - b)) for v, a, b in zip(x, s, c))
    e_rel = max(max(abs(mp.mpf(float(np.sin(v))) - a) / abs(a) if a != 0 else 0, abs(mp.mpf(float(np.cos(v))) - b) / abs(b))
                for v, a, b in zip(x[small], np.array(s, object)[small], np.array(c, object)[small]))
    out.update(sincos_x=x, sincos_s=np.array([float(v) for v in s]), sincos_c=np.array([float(v) for v in c]), sincos_small=small,
               sincos_abs_ref=float(e_abs), sincos_rel_ref=float(e_rel), sincos_abs_bar=bar(e_abs), sincos_rel_bar=bar(e_rel))


def rounded_with_rest(exact):
    """-> (y, frac): y the double nearest to the mpmath value, frac = (exact - y) / ulp(y) in [-0.5, 0.5]"""
    y = float(exact)
    return y, float((exact - mp.mpf(y)) / mp.mpf(float(np.spacing(abs(y)))))


def gen_recip(rng, out):
    mag = 10.0 ** np.linspace(-290, 290, 291) * rng.uniform(1.0, 9.9, 291)
    x = np.concatenate([mag, -mag[::2], [1.0, 2.0, 3.0, 0.5]])
    r = [rounded_with_rest(1 / mp.mpf(float(v))) for v in x]
    xs = np.concatenate([mag, [1.0, 2.0, 3.0, 4.0, 0.25]])
    q = [rounded_with_rest(1 / mp.sqrt(mp.mpf(float(v)))) for v in xs]
    out.update(rcp_x=x, rcp_y=np.array([a for a, _ in r]), rcp_frac=np.array([b for _, b in r]),
               rsqrt_x=xs, rsqrt_y=np.array([a for a, _ in q]), rsqrt_frac=np.array([b for _, b in q]), recip_ulp_bar=2.0)


# ------------------------------------------------------------------------------------------------ 6x6 solves
TRIL = np.tril_indices(6)               # row by row: (0,0) (1,0) (1,1) (2,0) ... = the header's packed order


def spd6(rng, cond, negative=False):
    Q, _ = np.linalg.qr(rng.randn(6, 6))
    ev = np.logspace(0, -np.log10(cond), 6) * rng.uniform(0.5, 2.0)
    if negative:
        ev[rng.randint(6)] *= -1.0
    A = (Q * ev) @ Q.T
    return 0.5 * (A + A.T)


def gen_chol(rng, out):
    rows, want, e, conds = [], [], 0.0, []
    for cond in np.logspace(0, 10, 34):
        for _ in range(3):
            A, b = spd6(rng, cond), rng.randn(6)
            for par in (0.0, 1e-3, 1.0):
                Ap = mpm(A) + mp.mpf(par) * mp.eye(6)
                x = mp.lu_solve(Ap, mpm(b))
                xn = np.linalg.solve(A + par * np.eye(6), b)
                nx = max(abs(v) for v in x)
                e = max(e, float(max(abs(mp.mpf(float(xn[i])) - x[i]) for i in range(6)) / nx))
                rows.append(np.concatenate([A[TRIL], [par], b]))
                want.append([float(v) for v in x])
                conds.append(cond)
    bad = np.array([np.concatenate([spd6(rng, 10.0, negative=True)[TRIL], [0.0], rng.randn(6)]) for _ in range(12)])
    out.update(chol_in=np.array(rows), chol_x=np.array(want), chol_cond=np.array(conds), chol_indefinite=bad, chol_ref=e, chol_bar=bar(e))


def gen_lmpar(rng, out):
    """properties only; kept are the cases on which a plain Newton iteration on par (More's update, as MINPACK's lmpar) meets
    | |z| - delta | <= 0.1 delta in fewer than 10 steps"""
    rows, inside, gn, drawn = [], [], [], 0
    for cond in np.logspace(0, 6, 25):
        for factor in (4.0, 1.0, 0.5, 0.1, 1e-2, 1e-3):                 # delta = factor * |A^-1 g|: the bound |A^-1 g| <= 1.1 delta holds for the first two
            for _ in range(2):
                drawn += 1
                A, g = spd6(rng, cond), rng.randn(6)
                z0 = np.linalg.solve(A, g)
                delta = factor * np.linalg.norm(z0)
                if factor < 1.0:
                    w = z0 / np.linalg.norm(z0)
                    par = ((np.linalg.norm(z0) - delta) / delta) / (w @ np.linalg.solve(A, w))
                    for step in range(10):
                        z = np.linalg.solve(A + par * np.eye(6), g)
                        fp = np.linalg.norm(z) - delta
                        if abs(fp) <= 0.1 * delta:
                            break
                        w = z / np.linalg.norm(z)
                        par = max(par + (fp / delta) / (w @ np.linalg.solve(A + par * np.eye(6), w)), 0.0)
                    else:
                        continue
                rows.append(np.concatenate([A[TRIL], g, [delta]]))
                inside.append(factor >= 1.0)
                gn.append(z0)
    assert len(rows) >= 0.9 * drawn, (len(rows), drawn)
    out.update(lmpar_in=np.array(rows), lmpar_inside=np.array(inside), lmpar_gn=np.array(gn), lmpar_drawn=drawn)


def generate():
    out = {}
    gen_horn(np.random.RandomState(101), out)
    gen_rot(np.random.RandomState(102), out)
    gen_rod(np.random.RandomState(103), out)
    gen_sincos(np.random.RandomState(104), out)
    gen_recip(np.random.RandomState(105), out)
    gen_chol(np.random.RandomState(106), out)
    gen_lmpar(np.random.RandomState(107), out)
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_math.npz")
    data = generate()
    np.savez_compressed(path, **data)
    for k in sorted(data):
        if k.endswith("_ref") or k.endswith("_bar"):
            print(f"{k:18s} {float(data[k]):.3e}")
    print(path, os.path.getsize(path), "bytes;", {k: len(data[k]) for k in ("horn_M", "rot_rv", "rod_in", "sincos_x", "rcp_x", "chol_in", "lmpar_in")})
