"""Case builder and float64 reference for the evaluation kernels of csrc/metrics.hip (ancsh_joint_params, ancsh_articulation_rec,
ancsh_part_extents) -- test infrastructure, plain numpy, imports without a GPU.

make_case(seed) builds one batch in the record's layout (float32 arrays) whose joint votes are PLACED, not drawn: the vote count of
every (cloud, joint) comes from COUNT_LIST (the edges of the ordered compaction's 64-lane waves and 256-point chunks and of the bitonic
sort's power-of-two padding) and the votes sit in one of four LAYOUTS.  reference(case) restates the documented definitions of
csrc/metrics.hip, csrc/part_stats.h and include/ancsh_hip.h with numpy: np.argmax labels (first maximum, or first NaN), np.median of the
float32 vote columns, two-pass float64 std of the float32 row means, float64 everywhere else.  Nothing here shares code with the kernels
or with oracle/joint_params_oracle.py."""
import warnings

import numpy as np

F = np.float32
N_LIST = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 2048, 4095, 4096)
K_LIST = (1, 2, 3, 5, 8)
COUNT_LIST = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, -1)      # -1: the whole cloud (n)
LAYOUTS = ("permutation", "run64", "straddle256", "tail")
MIN_ROW_MEAN_STD = 0.02


def shape_of(seed):
    """the shape parameters cycle through their lists: every value occurs within any 40 consecutive seeds"""
    K = K_LIST[seed % 5]
    return dict(n=N_LIST[seed % 13], K=K, B=1 + (seed + seed // 5) % 5, G=3 if (seed // 3) % 2 == 0 else 3 * K,
                JC=int(np.clip((1, K - 1, K, 8)[(seed // 2) % 4], 1, 8)))


def row_mean(a):
    """np.mean(a, axis=1) of an (m, 3) float32 array as numpy evaluates it: ((a + b) + c) / 3 in float32"""
    return ((a[:, 0] + a[:, 1]) + a[:, 2]) / F(3)


def std64(v):
    """two-pass float64 std of float32 values"""
    v = v.astype(np.float64)
    return np.sqrt(np.mean((v - np.mean(v)) ** 2)) if len(v) else np.nan


def labels_of(mask):
    return np.argmax(mask, axis=-1)                     # the first maximum, or the first NaN


def _labels(rng, n, K, empty, one, two):
    parts = [j for j in range(K) if j != empty]
    special = [j for j in (one, two) if j is not None and j in parts]
    others = [j for j in parts if j not in special]
    pos = rng.permutation(n)
    lab = np.empty(n, np.int64)
    if others and n >= 3 + len(others):
        cur = 0
        for j, m in zip((one, two), (1, 2)):
            if j in special:
                lab[pos[cur:cur + m]] = j
                cur += m
        lab[pos[cur:]] = np.asarray(others)[np.arange(n - cur) % len(others)]
    else:
        lab[pos] = np.asarray(parts)[np.arange(n) % len(parts)]
    return lab


def _mask(rng, lab, K):
    n = len(lab)
    mask = (rng.rand(n, K) * 0.4).astype(F)
    mask[np.arange(n), lab] = (0.6 + 0.4 * rng.rand(n)).astype(F)
    for i in range(0, n, 7):                            # ties at 0.5: np.argmax takes the first maximum
        mask[i, lab[i]] = 0.5
        if lab[i] < K - 1:
            mask[i, rng.randint(lab[i] + 1, K)] = 0.5
    return mask


def _place(rng, n, counts, layouts):
    """-> cls (n,) with the votes of joint q + 1 placed, and [(joint, count, layout actually used, idx)]"""
    free = np.ones(n, bool)
    cls = np.zeros(n, np.int64)
    out = []
    for q in sorted(range(len(counts)), key=lambda q: -LAYOUTS.index(layouts[q])):      # the constrained layouts choose first
        cnt, lay, idx = int(min(counts[q], free.sum())), layouts[q], None
        if cnt == 0:
            out.append((q + 1, 0, lay, np.zeros(0, np.int64)))
            continue
        if lay == "tail" and free[n - cnt:].all():
            idx = np.arange(n - cnt, n)
        elif lay == "straddle256" and cnt >= 2:
            for k in rng.permutation(np.arange(1, (n - 1) // 256 + 1)):
                s = 256 * int(k) - int(rng.randint(1, cnt))
                if s >= 0 and s + cnt <= n and free[s:s + cnt].all():
                    idx = np.arange(s, s + cnt)
                    break
        elif lay == "run64":
            starts = [s for s in range(0, n - cnt + 1, 64) if free[s:s + cnt].all()]
            if starts:
                s = starts[rng.randint(len(starts))]
                idx = np.arange(s, s + cnt)
        if idx is None:
            lay, idx = "permutation", np.sort(rng.choice(np.where(free)[0], cnt, replace=False))
        free[idx] = False
        cls[idx] = q + 1
        out.append((q + 1, cnt, lay, idx))
    return cls, sorted(out, key=lambda v: v[0])


def _draw_x(rng, shape, quantised):
    return (np.round(rng.rand(*shape) * 8) / 8).astype(F) if quantised else rng.rand(*shape).astype(F)


def badly_conditioned(case):
    """[(cloud, part)]: parts of at least 2 points whose row means (global or part NOCS) have a float64 std below MIN_ROW_MEAN_STD"""
    K, G, bad = case["K"], case["G"], []
    lab = labels_of(case["mask"])
    for b in range(case["B"]):
        for j in range(K):
            idx = np.where(lab[b] == j)[0]
            if len(idx) < 2:
                continue
            x = case["gocs"][b, idx, :3] if G == 3 else case["gocs"][b, idx, 3 * j:3 * j + 3]
            y = case["nocs"][b, idx, 3 * j:3 * j + 3]
            if not (std64(row_mean(x)) >= MIN_ROW_MEAN_STD and std64(row_mean(y)) >= MIN_ROW_MEAN_STD):
                bad.append((b, j))
    return bad


def make_case(seed, n=None, K=None, B=None, G=None, JC=None, counts=None, layouts=None):
    """One batch.  The keyword arguments override the seed's shape (G / JC follow an overridden K unless given); counts (B, K-1) and
    layouts (B, K-1) override the drawn vote counts / layouts of joints 1..K-1 (joints >= JC never get votes).  The builder refuses a
    seed in which more than 1 part in 20 (at least one) needs a fresh draw to be well conditioned: none of seeds 0..39, three of the
    first 1000 (41, 495, 690: two tiny parts each), which a long fuzz reports as the builder's AssertionError, not as a kernel's."""
    sh = shape_of(seed)
    if K is not None and K != sh["K"]:
        sh.update(K=K, G=3 if sh["G"] == 3 else 3 * K, JC=int(np.clip(sh["JC"], 1, 8)))
    for k, v in (("n", n), ("B", B), ("G", G), ("JC", JC)):
        if v is not None:
            sh[k] = v
    n, K, B, G, JC = sh["n"], sh["K"], sh["B"], sh["G"], sh["JC"]
    assert G in (3, 3 * K) and 1 <= JC <= 8
    rng = np.random.RandomState(7000 + seed)
    quantised = seed % 3 == 0
    case = dict(seed=seed, n=n, K=K, B=B, G=G, JC=JC, quantised=quantised, votes=[])
    # ---- part labels of both networks
    mask, npcs_mask = np.empty((B, n, K), F), np.empty((B, n, K), F)
    tiny = 1 if B > 1 else 0
    for b in range(B):
        empty = K - 1 if (b == 0 and K > 1) else None
        one, two = (1, 2) if (b == tiny and K >= 3) else (None, None)
        mask[b] = _mask(rng, _labels(rng, n, K, empty, one, two), K)
        npcs_mask[b] = _mask(rng, _labels(rng, n, K, None if empty is None else 0, two, one), K)
    lab = labels_of(mask)
    # ---- the joint classes: placed
    J = min(K, JC) - 1                                   # joints 1..J can have votes
    cls = np.zeros((B, n), np.int64)
    for b in range(B):
        want = [COUNT_LIST[rng.randint(len(COUNT_LIST))] for _ in range(J)] if counts is None else [int(c) for c in counts[b][:J]]
        want = [n if c < 0 else c for c in want]
        lays = [LAYOUTS[rng.randint(4)] for _ in range(J)] if layouts is None else list(layouts[b][:J])
        cls[b], placed = _place(rng, n, want, lays)
        for j, cnt, lay, idx in placed:
            case["votes"].append(dict(cloud=b, joint=j, count=cnt, layout=lay, idx=idx))
        for j in range(J + 1, K):
            case["votes"].append(dict(cloud=b, joint=j, count=0, layout="none", idx=np.zeros(0, np.int64)))
    if JC > K:                                           # some points outside every joint carry a class past the last joint
        for b in range(B):
            spare = np.where(cls[b] == 0)[0][::9]
            cls[b, spare] = rng.randint(K, JC, len(spare))
    index = (rng.rand(B, n, JC) * 0.4).astype(F)
    for b in range(B):
        index[b, np.arange(n), cls[b]] = 0.9
        for i in range(0, n, 5):                         # ties: the first argmax is the placed class
            if cls[b, i] < JC - 1:
                index[b, i, rng.randint(cls[b, i] + 1, JC)] = 0.9
    joint_cls = cls.astype(np.int32)
    for b in range(1, B, 2):                             # odd clouds: labels outside 1..K-1 on points that vote for nothing
        spare = np.where(cls[b] == 0)[0][:6]
        joint_cls[b, spare] = np.asarray([-1, 0, K], np.int32)[np.arange(len(spare)) % 3]
    # ---- the heads
    gocs = _draw_x(rng, (B, n, G), quantised)
    nocs = rng.rand(B, n, 3 * K).astype(F)
    if quantised:                                        # every vote a multiple of 1/8: 0.625 k * 0.2f is exactly k / 8 in float32
        heatmap = rng.randint(0, 2, (B, n)).astype(F)
        unitvec = (0.625 * rng.randint(-3, 4, (B, n, 3))).astype(F)
        joint_axis = (np.round(rng.randn(B, n, 3) * 4) / 8).astype(F)
    else:
        heatmap = rng.rand(B, n).astype(F)
        unitvec = rng.randn(B, n, 3).astype(F)
        joint_axis = rng.randn(B, n, 3).astype(F)
    b = B - 1                                            # the last cloud: signed zeros among the votes
    for v in case["votes"]:
        if v["cloud"] == b and v["count"] > 0:
            for r, i in enumerate(v["idx"][::3]):
                z = F(-0.0) if r % 2 else F(0.0)
                joint_axis[b, i] = z
                unitvec[b, i] = z
                gocs[b, i] = z
    case.update(gocs=gocs, nocs=nocs, mask=mask, heatmap=heatmap, unitvec=unitvec, joint_axis=joint_axis, index=index, joint_cls=joint_cls,
                npcs_nocs=rng.rand(B, n, 3 * K).astype(F), npcs_mask=npcs_mask, P=rng.randn(B, n, 3).astype(F))
    # ---- every part of at least 2 points is well conditioned: std of the row means >= 0.02 on both sides (else the scale is a ratio of
    # two cancellations and no ulp bound holds); a part that is not gets a fresh draw, and that must stay rare
    redrawn = set()
    for _ in range(50):
        bad = badly_conditioned(case)
        if not bad:
            break
        for (b, j) in bad:
            redrawn.add((b, j))
            idx = np.where(lab[b] == j)[0]
            nocs[b, idx, 3 * j:3 * j + 3] = rng.rand(len(idx), 3).astype(F)
            sl = slice(0, 3) if G == 3 else slice(3 * j, 3 * j + 3)
            gocs[b, idx, sl] = _draw_x(rng, (len(idx), 3), quantised)
    assert not badly_conditioned(case), "seed %d: a part stays badly conditioned" % seed
    assert len(redrawn) <= max(1, (B * K) // 20), "seed %d: %d of %d parts needed a redraw" % (seed, len(redrawn), B * K)
    case["redrawn"] = sorted(redrawn)
    # ---- the pose record: proper rotations, s in [0.5, 2], t ~ N(0, 1) in the baseline (0..12) and nonlinear (13..25) halves
    record = np.empty((B, K, 26))
    for b in range(B):
        for j in range(K):
            for o in (0, 13):
                q, r = np.linalg.qr(rng.randn(3, 3))
                q = q * np.sign(np.diag(r))
                if np.linalg.det(q) < 0:
                    q[:, 0] = -q[:, 0]
                record[b, j, o:o + 9] = q.reshape(9)
                record[b, j, o + 9] = rng.uniform(0.5, 2.0)
                record[b, j, o + 10:o + 13] = rng.randn(3)
    case["record"] = record
    return case


def describe(case, cloud=None, joint=None):
    s = "seed=%d n=%d K=%d G=%d JC=%d B=%d" % (case["seed"], case["n"], case["K"], case["G"], case["JC"], case["B"])
    if cloud is not None:
        s += " cloud=%d" % cloud
    if joint is not None:
        v = [v for v in case["votes"] if v["cloud"] == cloud and v["joint"] == joint][0]
        s += " joint=%d count=%d layout=%s" % (joint, v["count"], v["layout"])
    return s


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _median(cols):
    """np.median of the float32 columns of an (m, c) array: NaN for a column with a NaN, NaN without rows, the float32 mean of the
    middle two for an even count (inf + -inf -> NaN)"""
    if cols.shape[0] == 0:
        return np.full(cols.shape[1], np.nan, F)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.median(cols, axis=0).astype(F)


def votes_of(g3, heatmap, unitvec):
    """nocs_g + unitvec * (1 - heatmap) * 0.2 in float32, in that order"""
    with np.errstate(all="ignore"):
        return g3 + (unitvec * (F(1) - heatmap)[:, None]) * F(0.2)


def translation(case, scale):
    """(B, K, 3): the float64 mean of the float32 elements y - float32(scale) * x over each part (NaN for an empty part)"""
    K, G = case["K"], case["G"]
    lab = labels_of(case["mask"])
    out = np.full((case["B"], K, 3), np.nan)
    for b in range(case["B"]):
        for j in range(K):
            idx = np.where(lab[b] == j)[0]
            if len(idx) == 0:
                continue
            x = case["gocs"][b, idx, :3] if G == 3 else case["gocs"][b, idx, 3 * j:3 * j + 3]
            y = case["nocs"][b, idx, 3 * j:3 * j + 3]
            with np.errstate(all="ignore"):
                out[b, j] = (y - F(scale[b, j]) * x).astype(np.float64).sum(0) / len(idx)
    return out


def part_extents(nocs, mask, P, R0, t0):
    """ancsh_part_extents as tests/test_eval_scripts_gpu.py::test_part_extents_kernel computes it -> extent (B,K,3) float32, dynam (B,K),
    count (B,K)"""
    B, n, K = mask.shape
    C = nocs.shape[2]
    lab = labels_of(mask)
    ext, dyn, cnt = np.full((B, K, 3), np.nan, F), np.full((B, K), np.nan), np.zeros((B, K), np.int32)
    for b in range(B):
        R32, t32 = R0[b].astype(F).astype(np.float64), t0[b].astype(F).astype(np.float64)
        m30 = float(F(-((t32[0] * R32[0, 0] + t32[1] * R32[1, 0]) + t32[2] * R32[2, 0])))
        for j in range(K):
            idx = np.where(lab[b] == j)[0]
            cnt[b, j] = len(idx)
            if len(idx) == 0:
                continue
            cen = nocs[b, idx, :3] if C == 3 else nocs[b, idx, 3 * j:3 * j + 3]
            with np.errstate(all="ignore"):
                ext[b, j] = F(2) * np.max(np.abs(cen - F(0.5)), axis=0)
            x = P[b, idx, :3].astype(np.float64)
            dyn[b, j] = np.min(((x[:, 0] * R32[0, 0] + x[:, 1] * R32[1, 0]) + x[:, 2] * R32[2, 0]) + m30)
    return ext, dyn, cnt


def articulation(case, ref, st0=None):
    """The (B, K, 12) block, float64, evaluated as articulation_kernel writes it.  st0 (B, 4): part 0's similarity to go through (the
    reference's own by default; a test passes the kernel's, which it has bounded separately, so that the 1e-12 bar on the pivot is not
    spent on the scale's float32 ulps)."""
    B, K, rec = case["B"], case["K"], case["record"]
    if st0 is None:
        st0 = np.concatenate([ref["scale"][:, :1], ref["translation"][:, 0]], 1)
    art = np.full((B, K, 12), np.nan)
    with np.errstate(all="ignore"):
        for b in range(B):
            if np.isnan(rec[b, 0, 13:26]).any():
                continue                                 # a poisoned record: the whole block NaN
            r0, s0, t0 = rec[b, 0, 13:22], rec[b, 0, 22], rec[b, 0, 23:26]
            s2, t2 = st0[b, 0], st0[b, 1:]
            for j in range(K):
                r, s, t = rec[b, j, 13:22], rec[b, j, 22], rec[b, j, 23:26]
                if ref["npcs_count"][b, j] > 0:
                    for k in range(3):
                        art[b, j, k] = s * float(ref["npcs_extent"][b, j, k])
                        art[b, j, 3 + k] = s * ((r[3 * k] * 0.5 + r[3 * k + 1] * 0.5) + r[3 * k + 2] * 0.5) + t[k]
                if j == 0:
                    continue
                pt, ax = ref["joint_pt"][b, j - 1].astype(np.float64), ref["joint_axis"][b, j - 1].astype(np.float64)
                pp = [s0 * (pt[k] * s2 + t2[k]) for k in range(3)]
                for k in range(3):
                    rk = r0[3 * k:3 * k + 3]
                    art[b, j, 6 + k] = ((pp[0] * rk[0] + pp[1] * rk[1]) + pp[2] * rk[2]) + t0[k]
                    art[b, j, 9 + k] = (ax[0] * rk[0] + ax[1] * rk[1]) + ax[2] * rk[2]
    return art


def reference(case):
    B, n, K, G = case["B"], case["n"], case["K"], case["G"]
    lab = labels_of(case["mask"])
    jc_pred = np.argmax(case["index"], axis=2)
    ref = dict(labels=lab, scale=np.full((B, K), np.nan), joint_pt=np.full((B, K - 1, 3), np.nan, F), joint_axis=np.full((B, K - 1, 3), np.nan, F),
               gt_joint_pt=np.full((B, K - 1, 3), np.nan, F), gt_joint_axis=np.full((B, K - 1, 3), np.nan, F))
    for b in range(B):
        for j in range(K):                               # similarity global NOCS -> part NOCS
            idx = np.where(lab[b] == j)[0]
            if len(idx) == 0:
                continue
            x = case["gocs"][b, idx, :3] if G == 3 else case["gocs"][b, idx, 3 * j:3 * j + 3]
            y = case["nocs"][b, idx, 3 * j:3 * j + 3]
            with np.errstate(all="ignore"):
                ref["scale"][b, j] = F(std64(row_mean(y))) / F(std64(row_mean(x)))      # a float32 division
        # votes: a point reads its predicted part's global-NOCS triple when G = 3K
        g3 = case["gocs"][b, :, :3] if G == 3 else np.take_along_axis(case["gocs"][b].reshape(n, K, 3), lab[b][:, None, None], 1)[:, 0]
        v = votes_of(g3, case["heatmap"][b], case["unitvec"][b])
        vg = votes_of(case["gocs"][b, :, :3], case["heatmap"][b], case["unitvec"][b])     # the ground-truth variant: 3 channels, no mask
        for j in range(1, K):
            idx = np.where(jc_pred[b] == j)[0]
            ref["joint_pt"][b, j - 1], ref["joint_axis"][b, j - 1] = _median(v[idx]), _median(case["joint_axis"][b, idx])
            idx = np.where(case["joint_cls"][b] == j)[0]
            ref["gt_joint_pt"][b, j - 1] = _median(vg[idx])
            if len(idx):                                 # float32 running sum row by row, then / count
                with np.errstate(all="ignore"):
                    ref["gt_joint_axis"][b, j - 1] = np.add.accumulate(case["joint_axis"][b, idx], axis=0, dtype=F)[-1] / F(len(idx))
    ref["translation"] = translation(case, ref["scale"])
    R0, t0 = case["record"][:, 0, 13:22].reshape(B, 3, 3), case["record"][:, 0, 23:26]
    ref["npcs_extent"], ref["npcs_dynam"], ref["npcs_count"] = part_extents(case["npcs_nocs"], case["npcs_mask"], case["P"], R0, t0)
    ref["g_extent"], ref["g_dynam"], ref["g_count"] = part_extents(case["gocs"], case["mask"], case["P"], R0, t0)
    ref["art"] = articulation(case, ref)
    return ref


def ulps(a, b):
    """distance in float32 ulps between two arrays of finite float32 values (as float64: how many float32 values lie between)"""
    def key(v):
        i = np.asarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
