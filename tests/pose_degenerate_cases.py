"""Inputs and float64 bounds of the stage-A degenerate-sample tests (test_pose_degenerate_cpu.py holds the reference arithmetic
to them, test_pose_degenerate_gpu.py the kernels).  numpy only; nothing here restates the code under test: the bounds are geometry
(a line is mapped exactly by every optimal rotation of a sample on it; a point at distance d from a fixed line moves by at most
2 s d under a spin about it) or a float64 SVD-Kabsch model evaluated with a window of +-1e-4 about the threshold.

Every builder is cached: the arrays are shared between tests and must be left unchanged."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

TH = 0.1
N_SMALL = 24


def _similarity(rng):
    R = Rotation.random(random_state=rng).as_matrix()
    s = rng.uniform(0.6, 1.6)
    t = rng.uniform(-0.3, 0.3, 3)
    return R, s, t


def _apply(src32, R, s, t):
    """the exact similarity in float64, then the cast"""
    return (s * src32.astype(np.float64) @ R.T + t).astype(np.float32)


def repeated_index_triples(n):
    """all 3 n (n-1) triples with exactly one repeated index"""
    return np.array([p for i in range(n) for j in range(n) if i != j for p in ((i, i, j), (i, j, i), (j, i, i))], np.int32)


def _batch(problems):
    """problems: list of dicts with src, tgt (n,3) float32 and draws (niter,3) -> off, src, tgt, draws of ransac_single_batch"""
    off = np.concatenate([[0], np.cumsum([len(p["src"]) for p in problems])]).astype(np.int32)
    return dict(off=off, src=np.concatenate([p["src"] for p in problems]), tgt=np.concatenate([p["tgt"] for p in problems]),
                draws=np.stack([p["draws"] for p in problems]).astype(np.int32), problems=problems)


# ---------------------------------------------------------------------------------------------- 1a: collinear parts
@functools.lru_cache(maxsize=None)
def collinear_batch():
    """16 parts of 24 points on a line, lambda_k = -0.6 + 0.05 k + U[0, 0.01): gaps of 0.04..0.06 (closer pairs make scale_pts' +1e-6
    shrink the scale until the reference itself loses inliers), under an exact similarity.  Draws: the 1656 repeated-index triples + 392 random triples with >= 2 distinct indices.
    `same` holds the 24 triples (i,i,i) of a second run."""
    rng = np.random.RandomState(11)
    n = N_SMALL
    rep = repeated_index_triples(n)
    out = []
    for _ in range(16):
        R, s, t = _similarity(rng)
        u = rng.randn(3)
        u /= np.linalg.norm(u)
        lam = -0.6 + 0.05 * np.arange(n) + rng.uniform(0, 0.01, n)
        src = (rng.uniform(-0.2, 0.2, 3) + lam[:, None] * u).astype(np.float32)
        extra = []
        while len(extra) < 392:
            d = rng.randint(n, size=3)
            if len(set(d.tolist())) > 1:
                extra.append(d)
        draws = np.concatenate([rep, np.array(extra, np.int32)])
        assert draws.shape == (2048, 3)
        out.append(dict(src=src, tgt=_apply(src, R, s, t), draws=draws, R=R, s=s, t=t, u=u))
    b = _batch(out)
    b["same"] = np.tile(np.repeat(np.arange(n, dtype=np.int32), 3).reshape(1, n, 3), (16, 1, 1))
    return b


def same_index_window(tgt32, w=1e-4):
    """a sample (i,i,i): the reference fits R = I, scale 0, t = tgt_i, so hypothesis i scores #{k: |tgt_k - tgt_i| < th}.
    -> (lo, hi): that count at th - w and th + w, in float64"""
    T = tgt32.astype(np.float64)
    d = np.linalg.norm(T[None, :, :] - T[:, None, :], axis=2)          # d[i, k]
    return (d < TH - w).sum(1), (d < TH + w).sum(1)


# ---------------------------------------------------------------------------------------------- 1b: general parts, repeated-index samples
@functools.lru_cache(maxsize=None)
def general_batch():
    """8 parts of 24 points in [-0.5, 0.5]^3, every pair >= 0.05 apart, exact similarity; draws: the 1656 repeated-index triples.
    `lower` (8, 1656): #{k: 2 s d_k < th - 1e-3}, d_k the distance of src_k from the line through the two sample points."""
    rng = np.random.RandomState(12)
    n = N_SMALL
    rep = repeated_index_triples(n)
    out = []
    for _ in range(8):
        R, s, t = _similarity(rng)
        while True:
            src = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
            d = np.linalg.norm(src[:, None].astype(np.float64) - src[None].astype(np.float64), axis=2)
            if d[np.triu_indices(n, 1)].min() >= 0.05:
                break
        out.append(dict(src=src, tgt=_apply(src, R, s, t), draws=rep, R=R, s=s, t=t))
    b = _batch(out)
    b["lower"] = np.stack([spin_lower_bound(p["src"], p["draws"], p["s"]) for p in out])
    assert b["lower"].min() >= 2                                          # the two sample points themselves
    return b


def spin_lower_bound(src32, draws, s, w=1e-3):
    S = src32.astype(np.float64)
    lo = np.empty(len(draws), np.int64)
    for h, d in enumerate(draws):
        i, j = sorted(set(d.tolist()))
        e = (S[j] - S[i]) / np.linalg.norm(S[j] - S[i])
        dist = np.linalg.norm(np.cross(S - S[i], e), axis=1)
        lo[h] = np.count_nonzero(2.0 * s * dist < TH - w)
    return lo


# ---------------------------------------------------------------------------------------------- 1c: well-conditioned samples
@functools.lru_cache(maxsize=None)
def noisy_batch():
    """6 parts of 64 points, noise 0.02 on the target, 30 % of the targets replaced by uniform outliers, 500 random triples each.
    `use` (6, 500) bool: three distinct indices and sigma2/sigma1 >= 0.05 for the centred source AND target sample;
    `lo`, `hi` (6, 500): inlier counts of the float64 SVD-Kabsch model at th - 1e-4 and th + 1e-4 (valid where `use`)."""
    rng = np.random.RandomState(21)
    n, w = 64, 1e-4
    out, use, lo, hi = [], [], [], []
    for _ in range(6):
        R, s, t = _similarity(rng)
        src = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
        tgt = s * src.astype(np.float64) @ R.T + t + 0.02 * rng.randn(n, 3)
        bad = rng.rand(n) < 0.3
        tgt[bad] = rng.uniform(-1, 1, (int(bad.sum()), 3))
        tgt = tgt.astype(np.float32)
        draws = rng.randint(n, size=(500, 3)).astype(np.int32)
        out.append(dict(src=src, tgt=tgt, draws=draws, R=R, s=s, t=t))
        u, l, h = zip(*[kabsch_window(src, tgt, d, w) for d in draws])
        use.append(u); lo.append(l); hi.append(h)
    b = _batch(out)
    b.update(use=np.array(use, bool), lo=np.array(lo), hi=np.array(hi))
    return b


def kabsch_window(src32, tgt32, d, w):
    """-> (usable, lo, hi) of one hypothesis: transform_pts of the sample in float64 (SVD-Kabsch rotation, pairwise scale with the
    reference's +1e-6, mean translation), residuals of all points in float64, counts at th - w and th + w"""
    if len(set(d.tolist())) < 3:
        return False, 0, 0
    S, T = src32[d].astype(np.float64), tgt32[d].astype(np.float64)
    Sc, Tc = S - S.mean(0), T - T.mean(0)
    sv_s, sv_t = np.linalg.svd(Sc, compute_uv=False), np.linalg.svd(Tc, compute_uv=False)
    if min(sv_s[1] / sv_s[0], sv_t[1] / sv_t[0]) < 0.05:
        return False, 0, 0
    U, _, Vt = np.linalg.svd(Tc.T @ Sc)
    Rk = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))]) @ Vt
    A = np.sqrt(((Sc[:, None] - Sc[None]) ** 2).sum(2)).ravel()
    B = np.sqrt(((Tc[:, None] - Tc[None]) ** 2).sum(2)).ravel()
    sc = A @ B / (A @ A + 1e-6)
    tr = (T.T - sc * Rk @ S.T).mean(1)
    res = np.linalg.norm(tgt32.astype(np.float64) - sc * src32.astype(np.float64) @ Rk.T - tr, axis=1)
    return True, int((res < TH - w).sum()), int((res < TH + w).sum())
