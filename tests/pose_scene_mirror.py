"""numpy statement of ancsh_pose_scene_build and ancsh_render_centre_crops (include/ancsh_hip.h): the table builder, from `kin` and `pose`
in the written order, one scalar operation at a time, and the crop centring in Python integers on render_mirror's vertex transform.
Validated on its own, against depth.pack_render_scene / depth.pack_frame_scene and hand-made cases, in tests/test_pose_scene_cpu.py.  Test
infrastructure only."""
import numpy as np

import render_mirror as RM

KIN_WIDTH, KIN_HEAD, KIN_LINK, POSE_WIDTH = 672, 32, 40, 32
RENDER_WIDTH, RENDER_HEAD, RENDER_LINK = 208, 16, 12
SCENE_WIDTH, SCENE_HEAD, SCENE_LINK, MAX_LINKS = 240, 16, 14, 16
CROP_CENTRE = -(1 << 31)
f64 = np.float64


def compose(A, B):
    """C = A o B of 3 x 4 maps: C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], + A[i][3] for j = 3."""
    C = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            v = f64(f64(f64(A[i, 0] * B[0, j]) + f64(A[i, 1] * B[1, j])) + f64(A[i, 2] * B[2, j]))
            C[i, j] = f64(v + A[i, 3]) if j == 3 else v
    return C


def link_map(kin, l, q):
    """X_l = T_l o J_l(q)."""
    k = kin[KIN_HEAD + KIN_LINK * l:KIN_HEAD + KIN_LINK * (l + 1)]
    kind = 0 if l == 0 else int(k[3])
    a = k[16:19]
    J = np.eye(4)[:3].copy()
    if kind == 1:
        s, c = f64(np.sin(q)), f64(np.cos(q))
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        u = f64(1.0 - c)
        for i in range(3):
            for j in range(3):
                J[i, j] = f64(f64(f64(c * (1.0 if i == j else 0.0)) + f64(s * K[i, j])) + f64(f64(u * a[i]) * a[j]))
    elif kind == 2:
        for i in range(3):
            J[i, 3] = f64(q * a[i])
    return compose(k[4:16].reshape(3, 4), J)


def world_pose(kin, pose, l):
    """W_l (3, 4), composed from the leaf upwards."""
    W, cur = link_map(kin, l, pose[l]), l
    p = int(kin[KIN_HEAD + KIN_LINK * l + 2])
    while 0 <= p < cur:
        W = compose(link_map(kin, p, pose[p]), W)
        cur, p = p, int(kin[KIN_HEAD + KIN_LINK * p + 2])
    return W


def build_tables(kin, poses):
    """(kin (672,), poses (n, 32)) -> (render (n, 208), scene (n, 240)) float64, as the entry writes them."""
    kin, poses = np.asarray(kin, f64), np.asarray(poses, f64).reshape(-1, POSE_WIDTH)
    n = poses.shape[0]
    render, scene = np.zeros((n, RENDER_WIDTH)), np.zeros((n, SCENE_WIDTH))
    nl = int(kin[14]) if 1.0 <= kin[14] <= MAX_LINKS else 0
    for f, pose in enumerate(poses):
        scene[f, :16] = kin[:16]
        render[f, 0:6], render[f, 6], render[f, 7], render[f, 8] = kin[16:22], kin[6], kin[22], kin[14]
        V = pose[16:28].reshape(3, 4)
        for l in range(nl):
            k = kin[KIN_HEAD + KIN_LINK * l:KIN_HEAD + KIN_LINK * (l + 1)]
            A = compose(V, world_pose(kin, pose, l))
            render[f, RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)] = (-A).reshape(12)
            Rc, off = k[19:28].reshape(3, 3), k[28:31]
            S = scene[f, SCENE_HEAD + SCENE_LINK * l:SCENE_HEAD + SCENE_LINK * (l + 1)]
            S[0], S[1] = k[0], k[1]
            for i in range(3):
                m = [-f64(f64(f64(Rc[i, 0] * A[j, 0]) + f64(Rc[i, 1] * A[j, 1])) + f64(Rc[i, 2] * A[j, 2])) for j in range(3)]
                S[2 + 4 * i:5 + 4 * i] = m
                S[5 + 4 * i] = f64(f64(f64(f64(m[0] * A[0, 3]) + f64(m[1] * A[1, 3])) + f64(m[2] * A[2, 3])) + off[i])
    return render, scene


def sincos_free(kin, poses):
    """(n, 16) bool: link l of frame f passes no revolute joint's sincos on its way to the root -- its entries are bit-equal on any device.
    (A revolute joint at q = 0 exactly counts as free: sincos(0) = (0, 1) exactly.)"""
    kin, poses = np.asarray(kin, f64), np.asarray(poses, f64).reshape(-1, POSE_WIDTH)
    nl = int(kin[14])
    free = np.ones((poses.shape[0], MAX_LINKS), bool)
    for f, pose in enumerate(poses):
        for l in range(nl):
            p = l
            while p > 0:
                if int(kin[KIN_HEAD + KIN_LINK * p + 3]) == 1 and pose[p] != 0.0:
                    free[f, l] = False
                p = int(kin[KIN_HEAD + KIN_LINK * p + 2])
    return free


def centre_origins(verts, tris, tri_link, V, geom, render):
    """ancsh_render_centre_crops on its own arguments -> geom (n, 5) int32 after the call (a copy), in Python integers."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris, tri_link = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(tri_link, np.int64).reshape(-1)
    out = np.array(geom, np.int32).reshape(-1, 5).copy()
    for f, g in enumerate(out):
        if not (int(g[3]) == CROP_CENTRE and int(g[4]) == CROP_CENTRE):
            continue
        rt = np.asarray(render[f], f64)
        nl = RM.frame_links(rt)
        xs, ys = [], []
        for idx, l in zip(tris, tri_link):
            if not 0 <= l < nl:
                continue
            R = rt[RENDER_HEAD + RENDER_LINK * l:RENDER_HEAD + RENDER_LINK * (l + 1)].reshape(3, 4)
            for i in idx:
                if not 0 <= i < V:
                    continue
                X, Y, _, ok = RM.project(verts[i], R, rt)
                if ok[0]:
                    xs.append(int(X[0]))
                    ys.append(int(Y[0]))
        row0 = col0 = 0
        if xs:
            col0 = ((min(xs) + max(xs)) >> 9) - (int(g[2]) >> 1)         # Python's >> floors, like the device's arithmetic shift
            row0 = ((min(ys) + max(ys)) >> 9) - (int(g[1]) >> 1)
        out[f, 3], out[f, 4] = row0, col0
    return out
